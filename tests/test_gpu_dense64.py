"""-m gpu: dense general-F covariance propagation Sigma <- F Sigma F^T + Q in fp64 on the matrix cores
(ekf_dense64_*; the double instantiation of ekf_dense_gemm.hpp) -- the fp64 twin of test_gpu_dense.py, held to the library's fp64 contract:
integer operands bit-exact, random operands within 1e-12 per block of numpy fp64, the reference's motion model
within FP64_TOL of the checker's prediction()."""
import ctypes

import numpy as np
import pytest

from parity import FP64_TOL, cov_err

pytestmark = pytest.mark.gpu
TOL = 1e-12   # three orders below FP64_TOL: what fp64 accumulation of these sizes leaves


def _ref(F, S, Q, iters=1):
    for _ in range(iters):
        S = F @ S @ F.T + Q
    return S


def _ints(rng, lo, hi, N):
    return rng.integers(lo, hi, size=(N, N)).astype(np.float64)


@pytest.mark.parametrize("N", [1, 2, 43, 128, 129, 300])
def test_dense64_operand_layouts_exact(hip, N):
    """Small integers make every fp64 product and sum exact in any order: pins the transposes, the C/D map of
    v_mfma_f64_16x16x4_f64 and the edges of the zero padding (all three operands asymmetric)."""
    rng = np.random.default_rng(100 + N)
    B = _ints(rng, -3, 4, N)
    I = np.eye(N)
    Z = np.zeros((N, N))
    d = hip.DensePropagator64(N)
    d.set(I, B, Z); d.propagate(1)
    assert np.array_equal(d.sigma, B)                       # I B I^T
    d.set(B, I, Z); d.propagate(1)
    assert np.array_equal(d.sigma, B @ B.T)                 # B I B^T
    C = _ints(rng, -2, 3, N)
    Q = _ints(rng, -5, 6, N)
    d.set(B, C, Q); d.propagate(1)
    assert np.array_equal(d.sigma, B @ C @ B.T + Q)         # B C B^T + Q
    d.close()


def test_dense64_tail_path_exact(hip):
    """N = 2850: ld = 2944 = 23 x 128 -> 529 tiles of 128 x 128 = 512 (one round of resident workgroups) + 17 tail
    tiles as 64 x 64 quarters, some in the last block row (whose lower quarters hold padding rows only and are
    skipped).  Integer operands: every element bit-exact, which pins the tile -> (row, col) maps of BOTH kernels."""
    N = 2850
    d = hip.DensePropagator64(N)
    info = d.launch_info()
    assert info == {"ld": 2944, "tiles": 23, "n_big": 512, "n_tail": 17}, info   # both kernels at work
    mask = d.tile_map()
    assert mask.sum() == 17 and mask[22].any() and not mask[:16].any()

    rng = np.random.default_rng(31)
    B = _ints(rng, -1, 2, N)
    Cm = _ints(rng, -1, 2, N)
    Q = _ints(rng, -5, 6, N)
    want = B @ Cm @ B.T + Q
    d.set(B, Cm, Q)
    d.propagate(1)
    got = d.sigma
    bad = got != want
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{bad.sum()} wrong elements, first at ({r},{c}) tile ({r // 128},{c // 128}) "
                             f"tail={mask[r // 128, c // 128]}: got {got[r, c]} want {want[r, c]}")
    # a second application feeds the result back: I Sigma I^T + 0 = Sigma
    d.set(np.eye(N), got, np.zeros((N, N)))
    d.propagate(1)
    assert np.array_equal(d.sigma, got)
    d.close()


@pytest.mark.parametrize("N", [43, 300, 403, 2003])
def test_dense64_random_F_vs_fp64(hip, N):
    rng = np.random.default_rng(N)
    F = np.eye(N) + rng.normal(size=(N, N)) / np.sqrt(N)      # dense, asymmetric
    A = rng.normal(size=(N, N))
    S = A @ A.T / N + np.eye(N)                               # SPD covariance
    Q = np.diag(rng.uniform(1e-4, 1e-2, size=N))
    d = hip.DensePropagator64(N)
    d.set(F, S, Q)
    d.propagate(1)
    want = _ref(F, S, Q)
    err = max(cov_err(d.sigma, want).values())
    assert err <= TOL, err
    d.propagate(2)   # the result feeds back as the next Sigma
    err = max(cov_err(d.sigma, _ref(F, want, Q, 2)).values())
    assert err <= TOL, err
    d.close()


def test_dense64_reproduces_the_structured_prediction(hip, oracle):
    """F = At = I + A of the reference's motion model (ekf_slam.cpp:85-101): the dense fp64 path agrees with the
    checker's prediction() within the library's contract (the fp32 twin is held to 1e-4)."""
    n = 200
    o = oracle.OracleEKF(n, oracle.STRUCTURED)
    rng = np.random.default_rng(7)
    N = o.N
    A = rng.normal(size=(N, N))
    S0 = A @ A.T / N + np.eye(N)
    st = np.zeros(N); st[0] = 0.3
    o.state, o.cov = st, S0
    dth, dx = 0.05, 0.02
    o.prediction(dth, dx)
    th = 0.3
    At = np.eye(N)
    At[1, 0] += -(dx / dth) * np.cos(th) + (dx / dth) * np.cos(th + dth)
    At[2, 0] += -(dx / dth) * np.sin(th) + (dx / dth) * np.sin(th + dth)
    Q = np.zeros((N, N)); Q[0, 0] = Q[1, 1] = Q[2, 2] = 1e-4
    d = hip.DensePropagator64(N)
    d.set(At, S0, Q)
    d.propagate(1)
    assert max(cov_err(d.sigma, o.cov).values()) <= FP64_TOL
    d.close()


def test_dense64_full_size_n10003_rows_in_tail_tiles(hip):
    """N = 10003 (ld = 10112 = 79 x 128: 6241 tiles = 12 rounds of 512 on the main kernel + 97 tail tiles): rows
    sampled INSIDE tail tiles (and a few outside), once with integer operands (bit-exact on those rows) and once
    with random operands (1e-12 per block on those rows)."""
    N = 10003
    d = hip.DensePropagator64(N)
    info = d.launch_info()
    assert info == {"ld": 10112, "tiles": 79, "n_big": 6144, "n_tail": 97}, info
    mask = d.tile_map()
    assert mask.sum() == 97 and mask[78].any()
    rng = np.random.default_rng(5)
    rows = [min(N - 1, int(tm) * 128 + int(rng.integers(0, 128))) for tm in np.unique(np.argwhere(mask)[:, 0])]
    rows += [0, 2, 5000, int(rng.integers(0, 9000)), N - 1]
    rows = np.array(sorted(set(rows)))
    # every tail tile is crossed by some sampled row
    hit = {(r // 128, int(tn)) for r in rows for tn in np.nonzero(mask[r // 128])[0]}
    assert len(hit) >= len(np.unique(np.argwhere(mask)[:, 0]))

    B = rng.integers(-1, 2, size=(N, N)).astype(np.float64)
    Cm = rng.integers(-1, 2, size=(N, N)).astype(np.float64)
    d.set(B, Cm, np.zeros((N, N)))
    d.propagate(1)
    got = d.sigma
    want = (B[rows] @ Cm) @ B.T                               # |entries| <= N^2 << 2^53: exact in any order
    assert np.array_equal(got[rows], want), f"{(got[rows] != want).sum()} wrong elements on the sampled rows"
    del B, Cm, got

    F = np.eye(N) + rng.standard_normal((N, N)) * (0.05 / np.sqrt(N))
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    Q = np.zeros((N, N)); Q[0, 0] = Q[1, 1] = Q[2, 2] = 1e-4
    d.set(F, S, Q)
    d.propagate(1)
    got = d.sigma[rows]
    want = (F[rows] @ S) @ F.T + Q[rows]
    err = np.abs(got - want) / np.abs(want).max()
    assert err.max() <= TOL, f"rel err {err.max():.2e}"
    for k, r in enumerate(rows):   # tile by tile inside the tail, so a wrong tail tile cannot hide in a row maximum
        for tn in np.nonzero(mask[r // 128])[0]:
            c0 = int(tn) * 128
            assert err[k, c0:min(N, c0 + 128)].max() <= TOL, (r, tn)
    d.close()


def test_dense64_handle_semantics(hip):
    N = 77
    d = hip.DensePropagator64(N)
    assert not d.sigma.any()                                  # a new handle is all zero
    rng = np.random.default_rng(3)
    F, S, Q = (_ints(rng, -2, 3, N) for _ in range(3))
    d.set(F, S, Q)
    d.set(None, None, None)                                   # None keeps the device contents
    d.propagate(0)                                            # iterations = 0 leaves Sigma alone
    assert np.array_equal(d.sigma, S)
    d.set(Sigma=np.eye(N))                                    # only Sigma replaced: F and Q kept
    d.propagate(1)
    assert np.array_equal(d.sigma, F @ F.T + Q)

    for bad in (0, -5):
        with pytest.raises(hip.EkfError) as e:
            hip.DensePropagator64(bad)
        assert e.value.status == 1                            # EKF_ERR_INVALID
    lib = hip.load()
    h = ctypes.c_void_p()
    assert lib.ekf_dense64_create(N, -1, None) == 1
    assert lib.ekf_dense64_destroy(None) == 0                 # destroying NULL is fine
    assert lib.ekf_dense64_create(N, -1, ctypes.byref(h)) == 0 and lib.ekf_dense64_destroy(h) == 0

    # an fp32 and an fp64 handle used in turn on one device do not disturb each other
    d32 = hip.DensePropagator(N)
    B = _ints(rng, -2, 3, N)
    d32.set(B, np.eye(N, dtype=np.float32), np.zeros((N, N), dtype=np.float32))
    d.set(np.eye(N), B, np.eye(N))
    d32.propagate(1)
    d.propagate(1)
    d32.propagate(1)
    assert np.array_equal(d32.sigma.astype(np.float64), B @ B @ B.T @ B.T)
    assert np.array_equal(d.sigma, B + np.eye(N))
    d32.close()
    d.close()
