"""No GPU: where the operands of the fp64 dense handle sit in their device buffers (ekf_slam_ml_amd/csrc/ekf_dense64_layout.hpp),
printed by tests/cpp/dense64_layout_dump.cpp, a plain C++17 program.  Every offset and size equals the formula the host code
used before the layouts had a header of their own (restated here, in doubles, the one place they are written twice); within
a buffer the regions one call uses do not overlap and lie inside the buffer; every region of doubles starts on a multiple of
8 and every region of the sparse scoring buffer on a multiple of 16 (the kernels read Hc and nu of it as 16-byte pairs)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LDS = (128, 256, 10112)
SPS_CASES = ((1, 1, 1, 1, 0), (1, 2, 5, 1, 1), (3, 2, 5, 0, 1), (70, 3, 7, 0, 0), (5000, 2, 5, 1, 0))
MAX_M = MAX_R = MAX_S = MAX_P = 64
SCORE_ROWS, READ_MAX = 2048, 65536
D, I = 8, 4   # sizeof(double), sizeof(int)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """{name: {key: bytes}} as the C++ header computes it"""
    exe = str(tmp_path_factory.mktemp("layout") / "dense64_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "cpp", "dense64_layout_dump.cpp")], check=True)
    out = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        name, key, value = line.split()
        assert key not in out.setdefault(name, {}), line
        out[name][key] = int(value)
    return out


def _up16(b):
    return (b + 15) // 16 * 16


def _sps_name(case):
    return "sps@" + ",".join(str(v) for v in case)


def expected():
    """the offsets of the host code before the header: {name: {key: bytes}}; the formulas are in doubles where it had them so"""
    want = {}
    for ld in LDS:
        oHt = MAX_M * ld                                   # dense64_correct: oHt, oR = 2 oHt, oNu = oR + 64 * 64
        oR, total = 2 * oHt, 2 * MAX_M * ld + MAX_M * MAX_M + MAX_M   # corr_in_doubles(ld)
        want[f"corr_in@{ld}"] = {"H": 0, "Ht": D * oHt, "R": D * oR, "nu": D * (oR + MAX_M * MAX_M), "bytes": D * total}
        cs_R = 2 * MAX_M * ld                              # kCsCols = 64 * 64, cs_R(ld), cs_nu(ld) = cs_R + 64 * 64
        want[f"corr_sparse@{ld}"] = {"Hc": 0, "cols": D * MAX_M * MAX_S, "R": D * cs_R, "nu": D * (cs_R + MAX_M * MAX_M),
                                     "bytes": D * total}
        pend_T = MAX_P * ld                                # pend_T(ld), pend_zero(ld) = 2 pend_T, allocated with 2 more doubles
        want[f"pend@{ld}"] = {"K": 0, "T": D * pend_T, "zero": D * 2 * pend_T, "bytes": D * (2 * pend_T + 2)}
    want["corr_out"] = {"nis": 0, "verdict": D, "bytes": 2 * D}   # nis | verdict in the second double
    kScNu = SCORE_ROWS * MAX_M
    kScNis = kScNu + SCORE_ROWS
    kScS = kScNis + SCORE_ROWS
    kScFlag = kScS + SCORE_ROWS * MAX_M
    want["sc_small"] = {"R": 0, "nu": D * kScNu, "nis": D * kScNis, "S": D * kScS, "flag": D * kScFlag,
                        "bytes": D * (kScFlag + SCORE_ROWS // 2)}
    kBlkQ = MAX_R * MAX_R
    want["blk_in"] = {"Fr": 0, "Qr": D * kBlkQ, "dx": D * 2 * kBlkQ, "bytes": D * (2 * kBlkQ + MAX_R)}
    kIniW = MAX_R * MAX_S
    kIniXb = kIniW + MAX_R * MAX_R
    kIniCols = kIniXb + MAX_R
    want["ini_in"] = {"G": 0, "W": D * kIniW, "xb": D * kIniXb, "cols": D * kIniCols, "bytes": D * (kIniCols + MAX_S // 2)}
    kRdCols = READ_MAX + READ_MAX // 2
    want["rd_buf"] = {"out": 0, "rows": D * READ_MAX, "cols": D * kRdCols, "bytes": D * (kRdCols + READ_MAX // 2)}
    for case in SPS_CASES:                                 # sps_layout: bytes, every piece rounded up to 16
        J, m, s, r_shared, want_S = case
        mm = m * m
        oR = _up16(D * J * m * s)
        oNu = oR + _up16(D * (mm if r_shared else J * mm))
        oNis = oNu + _up16(D * J * m)
        oS = oNis + _up16(D * J)
        oCols = oS + (_up16(D * J * mm) if want_S else 0)
        oFlag = oCols + _up16(I * J * s)
        want[_sps_name(case)] = {"Hc": 0, "R": oR, "nu": oNu, "nis": oNis, "S": oS, "cols": oCols, "flag": oFlag,
                                 "bytes": oFlag + _up16(I * J)}
    return want


def regions(name):
    """{key: (element size, largest number of bytes a call puts there)} for the regions one call uses together"""
    base = name.split("@")[0]
    ld = int(name.split("@")[1]) if base in ("corr_in", "corr_sparse", "pend") else 0
    fixed = {
        "corr_in": {"H": (D, D * MAX_M * ld), "Ht": (D, D * ld * MAX_M), "R": (D, D * MAX_M * MAX_M), "nu": (D, D * MAX_M)},
        "corr_sparse": {"Hc": (D, D * MAX_M * MAX_S), "cols": (I, I * MAX_S), "R": (D, D * MAX_M * MAX_M), "nu": (D, D * MAX_M)},
        "pend": {"K": (D, D * MAX_P * ld), "T": (D, D * MAX_P * ld), "zero": (I, I)},
        "corr_out": {"nis": (D, D), "verdict": (I, I)},
        "sc_small": {"R": (D, D * SCORE_ROWS * MAX_M), "nu": (D, D * SCORE_ROWS), "nis": (D, D * SCORE_ROWS),
                     "S": (D, D * SCORE_ROWS * MAX_M), "flag": (I, I * SCORE_ROWS)},
        "blk_in": {"Fr": (D, D * MAX_R * MAX_R), "Qr": (D, D * MAX_R * MAX_R), "dx": (D, D * MAX_R)},
        "ini_in": {"G": (D, D * MAX_R * MAX_S), "W": (D, D * MAX_R * MAX_R), "xb": (D, D * MAX_R), "cols": (I, I * MAX_S)},
        "rd_buf": {"out": (D, D * READ_MAX), "rows": (I, I * READ_MAX), "cols": (I, I * READ_MAX)},
    }
    if base != "sps":
        return fixed[base]
    J, m, s, r_shared, want_S = (int(v) for v in name.split("@")[1].split(","))
    mm = m * m
    return {"Hc": (D, D * J * m * s), "R": (D, D * (mm if r_shared else J * mm)), "nu": (D, D * J * m), "nis": (D, D * J),
            "S": (D, D * J * mm if want_S else 0), "cols": (I, I * J * s), "flag": (I, I * J)}


def test_every_layout_is_printed(dumped):
    want = expected()
    assert set(dumped) == set(want)
    assert {_sps_name(c) for c in SPS_CASES} <= set(dumped) and {f"pend@{ld}" for ld in LDS} <= set(dumped)


def test_offsets_equal_the_formulas_before_the_header(dumped):
    want = expected()
    for name in want:
        assert dumped[name] == want[name], name


def test_regions_do_not_overlap_and_lie_inside(dumped):
    for name, got in dumped.items():
        reg = regions(name)
        assert set(reg) | {"bytes"} == set(got), name
        spans = sorted((got[k], got[k] + size, k) for k, (_, size) in reg.items() if size)
        for (a0, a1, ka), (b0, _, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, (name, ka, kb)
        assert spans[0][0] >= 0 and spans[-1][1] <= got["bytes"], name


def test_sparse_correction_fits_where_the_dense_one_keeps_h(dumped):
    """Hc ends before cols begins, cols ends before R begins: 64 * 64 doubles + 64 ints <= 2 * 64 * ld doubles from ld = 128
    up; R, nu and the size are the dense correction's, so a buffer serves both"""
    for ld in LDS:
        cs, cd = dumped[f"corr_sparse@{ld}"], dumped[f"corr_in@{ld}"]
        assert cs["Hc"] + D * MAX_M * MAX_S <= cs["cols"]
        assert cs["cols"] + I * MAX_S <= cs["R"]
        assert D * MAX_M * MAX_S + I * MAX_S <= D * 2 * MAX_M * ld
        assert (cs["R"], cs["nu"], cs["bytes"]) == (cd["R"], cd["nu"], cd["bytes"])


def test_alignment(dumped):
    for name, got in dumped.items():
        for key, (elem, _) in regions(name).items():
            assert got[key] % elem == 0, (name, key)                 # doubles on 8, ints on 4
            if name.startswith("sps@"):
                assert got[key] % 16 == 0, (name, key)               # Hc and nu, and every other region of it
        if name.startswith("sps@"):
            assert got["bytes"] % 16 == 0, name
