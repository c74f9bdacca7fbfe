"""CPU: the one split behind both dense propagations (ekf_dense_split.hpp: DenseSplit, make_split, big_tile_of,
small_tile_origin, xcd_remap, dense_tile_map), walked by tests/cpp/dense_split_dump.cpp for float (256 x 128 main tiles) and
double (128 x 128) at every ld = 128 k, k = 1 .. 80.  Every 128 x 128 block of the result has exactly one owner, the main
kernel runs whole rounds of 512 or the whole list, the tail's count is the number of blocks it owns, and the numbers the GPU
tests pin (test_gpu_dense.py, test_gpu_dense64.py) come out of the header on a CPU.  The grouped walk is restated here in
Python, so the order of the tiles -- which block falls to the tail -- is held too."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LDS = [128 * k for k in range(1, 81)]
MAIN_ROWS = {"f32": 256, "f64": 128}
SLOTS = 512          # resident workgroups of the main kernel: 2 on each of 256 CUs
GROUP_M = 8


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """{(dtype, ld): {"split": [...], "owners": [t][t], "map": [t][t]}} as the C++ header computes it"""
    exe = str(tmp_path_factory.mktemp("split") / "dense_split_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "cpp", "dense_split_dump.cpp")], check=True)
    out = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        dtype, ld, what, *rest = line.split()
        rec = out.setdefault((dtype, int(ld)), {})
        assert what not in rec and what != "outside", line   # no tile reaches outside C
        if what == "split":
            rec[what] = dict(zip(("tiles_m", "tiles_n", "n_big", "rem_big", "bottom", "n_small", "perm"), map(int, rest)))
        else:
            t = int(ld) // 128
            rec[what] = np.frombuffer(bytes.fromhex(rest[0]), dtype=np.uint8).reshape(t, t)
    assert sorted(out) == sorted((d, ld) for d in MAIN_ROWS for ld in LDS)
    return out


def _tile_of(i, tiles_m, tiles_n):
    """the grouped walk: groups of 8 tile rows, inside a group down the rows first"""
    g, in_g = divmod(i, GROUP_M * tiles_n)
    gm = min(GROUP_M, tiles_m - g * GROUP_M)
    return g * GROUP_M + in_g % gm, in_g // gm


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_block_has_one_owner(dumped, dtype):
    per = MAIN_ROWS[dtype] // 128
    for ld in LDS:
        rec, t = dumped[dtype, ld], ld // 128
        sp, own = rec["split"], rec["owners"]
        assert (sp["tiles_m"], sp["tiles_n"], sp["bottom"]) == (ld // MAIN_ROWS[dtype], t, int(ld % MAIN_ROWS[dtype] != 0)), (ld, sp)
        total = sp["tiles_m"] * sp["tiles_n"]
        assert sp["n_big"] + sp["rem_big"] == total
        assert sp["n_big"] == total or (sp["n_big"] % SLOTS == 0 and 0 < sp["n_big"] and sp["rem_big"] < SLOTS), (ld, sp)
        assert sp["perm"] == 1, ld                                            # the XCD remap loses and doubles no tile
        main, tail = own >> 4, own & 15
        assert np.array_equal(main + tail, np.ones((t, t), dtype=np.uint8)), (ld, np.argwhere(main + tail != 1)[:4].tolist())
        assert sp["n_small"] == int(tail.sum()) == per * sp["rem_big"] + sp["bottom"] * t, (ld, sp)
        assert per * sp["n_big"] == int(main.sum())
        assert np.array_equal(rec["map"], tail), ld                           # what ekf_dense*_tile_map reports
        # which blocks: the first n_big tiles of the grouped walk on the main kernel, the bottom strip on the tail
        want = np.ones((t, t), dtype=np.uint8)
        for i in range(sp["n_big"]):
            tm, tn = _tile_of(i, sp["tiles_m"], sp["tiles_n"])
            want[per * tm:per * (tm + 1), tn] = 0
        assert np.array_equal(tail, want), ld
        if dtype == "f64":
            assert sp["bottom"] == 0 and sp["tiles_m"] == t


@pytest.mark.parametrize("dtype,ld,tiles,n_big,n_small", [("f32", 4736, 37, 512, 345), ("f32", 10112, 79, 3072, 97),
                                                        ("f64", 2944, 23, 512, 17), ("f64", 10112, 79, 6144, 97)])
def test_the_values_the_gpu_tests_pin(dumped, dtype, ld, tiles, n_big, n_small):
    sp = dumped[dtype, ld]["split"]
    assert (sp["tiles_n"], sp["n_big"], sp["n_small"]) == (tiles, n_big, n_small), sp
    tail = dumped[dtype, ld]["map"].astype(bool)
    assert tail.sum() == n_small
    if dtype == "f32":
        assert tail[tiles - 1].all()                 # ld is an odd multiple of 128: the bottom strip
        if ld == 4736:
            assert not tail[0, :8].any()
    elif ld == 2944:
        assert tail[22].any() and not tail[:16].any()
    else:
        assert tail[78].any()
