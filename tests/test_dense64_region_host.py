"""No GPU: the algebra of a local region of the dense fp64 handle (ekf_dense64_region_begin .. ekf_dense64_region_end) on the
numpy model of tests/dense_region_cases.py, against the plain full-width numpy sequence, on a COUPLED tail.
  * exact chains (symmetric integer Sigma, gains exact because S is a power of two; every product refused by
    cc.exact_product unless it is exact in float64 in any order): the region and the full-width sequence are EQUAL.  The
    proof that a chain is of this kind is its construction: dense_region_cases._build_exact raises otherwise.
  * general SPD chains with every (m, s) of dense_live_cases.PAIRS that fits: within parity.FP64_TOL, the maximum printed.
  * the chains of dense_live_cases.live_chain, whose corner is NOT symmetric: the corner of the region equals the filter of
    dimension Na (the live contract), and outside it the two differ by more than rounding -- the Gamma / Phi^T note.
  * the plan arithmetic of ekf_dense64_region.hpp through the library, the symbols and the refusals that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dense_live_cases as lc
import dense_region_cases as rc
from parity import FP64_TOL, worst

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("N,Na", [(65, 3), (65, 5), (65, 63), (65, 64), (66, 64), (200, 65), (200, 127), (200, 129), (200, 191)])
def test_region_equals_full_width_on_exact_chains(N, Na):
    ch = rc.exact_chain(N, Na)
    assert np.count_nonzero(ch["Sigma0"][:Na, Na:]) > 0 and np.array_equal(ch["Sigma0"], ch["Sigma0"].T)
    x, S = ch["region"]
    assert np.array_equal(S, ch["Sigma"]) and np.array_equal(x, ch["x"])
    assert not np.array_equal(S[Na:, Na:], ch["Sigma0"][Na:, Na:])     # the tail really owed something
    # and without the exactness checks (plain matmul) the same numbers: nothing in them depends on the order of summation
    x2, S2 = rc.run_region(ch["Sigma0"], ch["x0"], Na, ch["ops"])
    x3, S3 = rc.run_full(ch["Sigma0"], ch["x0"], ch["ops"])
    assert np.array_equal(S2, S) and np.array_equal(S3, S) and np.array_equal(x2, x) and np.array_equal(x3, x)


@pytest.mark.parametrize("N,Na", [(65, 3), (65, 64), (200, 129), (403, 191)])
def test_region_agrees_with_full_width_on_general_chains(N, Na):
    ch = rc.float_chain(N, Na)
    assert {op["op"] for op in ch["ops"]} >= {"eager", "propagate"}
    x, S = rc.run_region(ch["Sigma0"], ch["x0"], Na, ch["ops"])
    xf, Sf = rc.run_full(ch["Sigma0"], ch["x0"], ch["ops"])
    w, e = worst(x, S, xf, Sf)
    print(f"region model against the full-width sequence, N = {N}, Na = {Na}: worst per-block relative error {w:.3e}")
    assert w <= FP64_TOL, e


def test_on_a_corner_that_is_not_symmetric_only_the_corner_is_the_same():
    Na, N = 17, 40
    chain = lc.live_chain(Na, "scattered", 2, 5)
    assert not np.array_equal(chain["Sigma0"], chain["Sigma0"].T)
    S0, x0 = rc.coupled(chain["Sigma0"], chain["x0"], N, 5, integer=True)
    x, S = rc.run_region(S0, x0, Na, chain["ops"])
    xf, Sf = rc.run_full(S0, x0, chain["ops"])
    small = lc.run_model(chain, False)[-1]
    assert np.array_equal(S[:Na, :Na], small["Sigma_cur"]) and np.array_equal(x[:Na], small["state"])
    assert np.allclose(S[:Na, :Na], Sf[:Na, :Na], rtol=1e-9, atol=1e-9) and np.allclose(S[:Na, Na:], Sf[:Na, Na:], rtol=1e-9, atol=1e-9)
    assert not np.allclose(S[Na:, :Na], Sf[Na:, :Na], rtol=1e-6, atol=1e-6)   # Sigma_ba Phi^T against Sigma_ba Gamma


def test_an_empty_region_and_a_region_of_maps_only():
    ch = rc.exact_chain(65, 5)
    x, S = rc.run_region(ch["Sigma0"], ch["x0"], 5, [])
    assert np.array_equal(S, ch["Sigma0"]) and np.array_equal(x, ch["x0"])
    maps = [op for op in ch["ops"] if op["op"] in ("propagate", "init")]
    x, S = rc.run_region(ch["Sigma0"], ch["x0"], 5, maps, exact=True)
    xf, Sf = rc.run_full(ch["Sigma0"], ch["x0"], maps, exact=True)
    assert np.array_equal(S, Sf) and np.array_equal(x, xf) and np.array_equal(S[5:, 5:], ch["Sigma0"][5:, 5:])


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """ekf_dense64_region.hpp is free of HIP: a plain C++17 program prints its plans"""
    d = tmp_path_factory.mktemp("region")
    src, exe = str(d / "dump.cpp"), str(d / "dump")
    with open(src, "w") as f:
        f.write('#include <cstdio>\n#include "ekf_dense64_region.hpp"\nint main() {\n'
                '  const int c[][3] = {{3, 65, 128}, {64, 65, 128}, {65, 200, 256}, {127, 200, 256}, {128, 200, 256},\n'
                '                      {129, 403, 512}, {191, 403, 512}, {403, 10003, 10112}};\n'
                '  for (auto& q : c) { const ekf::Dense64RegionPlan p = ekf::dense64_region_plan(q[0], q[1], q[2]);\n'
                '    std::printf("%d %d %d %d %d %d %d %zu %zu %zu %d %d\\n", q[0], q[1], q[2], p.pitch, p.upd_tiles_r * p.upd_tiles_c,\n'
                '                p.gemm_tiles * p.gemm_tiles, p.gemm_k, p.acc_bytes, p.scratch_bytes, p.group_bytes,\n'
                '                (int)ekf::dense64_region_masked(p, q[0] - 1, q[0] - 1), (int)ekf::dense64_region_masked(p, q[0] - 1, q[0])); }\n'
                '  return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                    "-o", exe, src], check=True)
    return [[int(v) for v in line.split()] for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]


def test_plan_arithmetic(dumped):
    assert len(dumped) == 8
    for Na, N, ld, pitch, upd, gemm, k, acc, scratch, group, in_mask, edge_mask in dumped:
        want = rc.plan(Na, N, ld)
        assert (pitch, upd, gemm, k, acc, scratch, group) == tuple(want[n] for n in (
            "pitch", "update_tiles", "gemm_tiles", "gemm_k", "acc_bytes", "scratch_bytes", "group_bytes")), (Na, N)
        assert pitch % 128 == 0 and pitch >= Na and k % 16 == 0 and Na <= k < Na + 16
        assert in_mask == 0 and edge_mask == 1                        # the mask sits at Na exactly, not at a tile's edge
        assert scratch == 16 * Na * ld                                # 2 x Na x ld doubles
    assert dumped[-1][5] == 76 * 76                                   # N = 10003, Na = 403: tiles 3 .. 78 of Sigma's 79


def test_symbols_and_refusals_without_a_device():
    from ekf_slam_ml_amd import capi
    lib = capi.load()
    for name in ("ekf_dense64_region_begin", "ekf_dense64_region_end", "ekf_dense64_region_info", "ekf_dense64_region_launch_info"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    for name in ("region_begin", "region_end", "region_info", "region", "region_launch_info"):
        assert callable(getattr(capi.DensePropagator64, name))
    assert callable(capi.DenseEKFSLAM.local_region)
    ms, active = ctypes.c_double(7.0), ctypes.c_int(7)
    assert lib.ekf_dense64_region_begin(None, 5, ctypes.byref(ms)) == 1 and ms.value == 7.0   # EKF_ERR_INVALID
    assert lib.ekf_dense64_region_end(None, None, ctypes.byref(ms)) == 1 and ms.value == 7.0
    assert lib.ekf_dense64_region_info(None, ctypes.byref(active), None, None, None, None) == 1 and active.value == 7
    assert lib.ekf_dense64_region_launch_info(None, 5, *([None] * 8)) == 1


def test_the_regions_memory_is_one_group_or_nothing(tmp_path):
    """ekf_dense64_region_begin's reservation (ekf_dense64_region_mem.hpp) on a fake memory policy that fails the first or the
    second member of the group, out of memory or another error: the status is EKF_ERR_NOMEM / EKF_ERR_HIP, the API's error is
    cleared once, and the buffers, their byte count and the ledger's table are exactly as they were -- empty on a fresh
    handle, the smaller region's buffers when those were held.  region_begin returns on that status before it touches the
    live dimension or opens the region."""
    exe = str(tmp_path / "region_mem_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "cpp", "region_mem_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 12 and all(line.startswith("ok ") for line in out), out
