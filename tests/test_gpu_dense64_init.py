"""-m gpu: the (re)initialisation of a block of states of the fp64 dense handle (ekf_dense64_init_block,
ekf_dense64_init.hip), its block readout and state slices.  Sigma[b, :] <- G Sigma[cols, :], Sigma[:, b] <- Sigma[:, cols] G^T,
Sigma[b, b] <- (G Sigma[cols, cols]) G^T + W, state[b] <- xb: integer operands bit-exact against numpy, nothing outside the
block's rows and columns written and nothing outside rows cols / columns cols read, random operands within 1e-12 per
region of numpy and of the dense propagate with the embedded F, the corner bit for bit the S of score_sparse, position
independence and run-to-run determinism, failure paths, the readouts, the reference's own data_association() from an
all-unknown map (live through oracle.RefEKF), a slot recycled with a correlated re-initialisation, and N = 10003 with the
time condition against correct_sparse(2, 5) timed in the same test.

Worst values seen on the MI355X (printed by test_zz_report): random operands 8.0e-16 per region against numpy and 9.2e-16
against the dense propagate with the embedded F; the reference's data_association() live, 20 ticks from an all-unknown
map, 3.5e-14 per block of state and Sigma at n = 20 and n = 200, with init_block from a different prior and with
set_state_block alone; the slot-recycling cycle 5.5e-16 per block against numpy, the correlated corner 0 against
G Sigma_pp G^T + W; N = 10003 sampled rows, columns and corner 0 / 0 / 2.2e-16 for (r, s) = (2, 0) / (2, 3) / (64, 64).
Times at N = 10003: init_block 6.5 / 6.4 / 76.0 us for (2, 0) / (2, 3) / (64, 64) against 344.6 us for
correct_sparse(2, 5) (54x and 4.5x); propagate_block 6.4 us at r = 2 (ratio 0.99) and 38.0 us at r = 64 (init_block
takes 2.00x that: the weak point); the dense propagate 61.24 ms (806x init_block(64, 64))."""
import ctypes
import os

import numpy as np
import pytest

import dense_block_cases as bc
import dense_init_cases as ic
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst
from test_gpu_dense64 import TOL   # what tests/test_gpu_dense64.py holds propagate to against numpy

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {}
R_GRID = (1, 2, 3, 16, 17, 63, 64)
S_GRID = (0, 1, 3, 5, 16, 17, 64)


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _firsts(N, r):
    mid = ((N - r) // 2) | 1                     # an odd middle offset
    return sorted({f for f in (0, 1, mid, N - r) if 0 <= f <= N - r})


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi, size=shape).astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _block_err(got, want, first, r):
    """worst relative error per region (rows, columns, corner, rest), each against its own max-abs"""
    b = np.zeros(len(want), dtype=bool)
    b[first:first + r] = True
    out = 0.0
    for rows, cols in ((b, ~b), (~b, b), (b, b), (~b, ~b)):
        w, g = want[np.ix_(rows, cols)], got[np.ix_(rows, cols)]
        if w.size:
            out = max(out, float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-3)))
    return out


# ---- 1. integers, bit-exact --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 3, 5, 43, 127, 128, 129, 300, 403])
def test_init_integers_exact(hip, N):
    """every sum exact in fp64, so any order gives the same bits: pins rows vs columns (Sigma is unsymmetric), G vs G^T,
    the strip edges, the block's neighbours in the list and the padding.  Each case is followed by one dense propagation
    with an integer F, whose result is again exact: anything written into the padding shows there."""
    rng = np.random.default_rng(1100 + N)
    d = hip.DensePropagator64(N)
    F0, Q0 = _ints(rng, -2, 3, (N, N)), _ints(rng, -5, 6, (N, N))
    d.set(F=F0, Q=Q0)
    count = 0
    for r in sorted({r for r in R_GRID if r <= N} | ({N} if N <= 64 else set())):   # r = N where N <= 64
        for s in S_GRID:
            if s > N - r:
                continue
            firsts = _firsts(N, r)
            if N > 100 and len(firsts) > 2:          # two per (r, s), in rotation: every r meets all four over its s
                firsts = [firsts[(count // 2 + k) % len(firsts)] for k in (0, 2)]
            for first in firsts:
                order = ("asc", "desc", "scattered")[count % 3]
                Sigma = _ints(rng, -3, 4, (N, N))
                x = _ints(rng, -9, 10, N)
                cols = ic.block_list(N, first, r, s, order, rng) if s else None
                G = _ints(rng, -2, 3, (r, s)) if s else None
                W = _ints(rng, -5, 6, (r, r)) if count % 4 != 3 else None
                xb = _ints(rng, -4, 5, r) if count % 3 != 2 else None
                wx, wS = ic.np_init_block(x, Sigma, first, r, cols, G, W, xb)
                d.set(Sigma=Sigma)
                d.state = x
                d.init_block(first, G, cols, W, xb, r=r)
                got = d.sigma
                bad = got != wS
                what = f"N={N} r={r} s={s} first={first} {order}"
                assert not bad.any(), f"{what}: {bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
                assert np.array_equal(d.state, wx), what
                d.propagate(1)
                assert np.array_equal(d.sigma, F0 @ wS @ F0.T + Q0), what
                count += 1
    d.close()
    assert count >= 1


# ---- 2. untouched means untouched -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,r,s,first", [(43, 2, 3, 7), (300, 17, 16, 131), (403, 64, 64, 100), (129, 5, 0, 63),
                                         (300, 2, 0, 1)])
def test_init_leaves_the_rest_alone(hip, N, r, s, first):
    rng = np.random.default_rng(N + r + s)
    S = bc.unsymmetric_cov(N, rng)
    x = rng.normal(size=N)
    cols = ic.block_list(N, first, r, s, "scattered", rng) if s else None
    G = rng.normal(size=(r, s)) if s else None
    W = 1e-2 * rng.normal(size=(r, r))
    F0, Q0 = _ints(rng, -2, 3, (N, N)), _ints(rng, -5, 6, (N, N))
    b = np.zeros(N, dtype=bool)
    b[first:first + r] = True
    outside = np.outer(~b, ~b)
    d = hip.DensePropagator64(N)
    d.set(F=F0, Sigma=S, Q=Q0)
    d.state = x
    d.init_block(first, G, cols, W, rng.normal(size=r))
    got, gx = d.sigma, d.state
    assert _same_bits(got[outside], S[outside])
    assert _same_bits(gx[~b], x[~b])
    assert not np.array_equal(got[first:first + r], S[first:first + r])                 # (and the block did change)

    # NaN planted wherever the call must not read: the old block's rows and columns (its content never leaks), and
    # everything outside rows cols and columns cols -- at s = 0 all of Sigma
    may_read = np.zeros((N, N), dtype=bool)
    if s:
        may_read[cols, :] = True
        may_read[:, cols] = True
    may_read[b, :] = False
    may_read[:, b] = False
    Sn = np.where(may_read, S, np.nan)
    wx, wS = ic.np_init_block(x, S, first, r, cols, G, W)
    d.set(Sigma=Sn)
    d.init_block(first, G, cols, W)
    got = d.sigma
    rc = np.outer(b, np.ones(N, dtype=bool)) | np.outer(np.ones(N, dtype=bool), b)     # what the call wrote
    assert not np.isnan(got[rc]).any()
    e = _block_err(np.where(rc, got, S), wS, first, r)
    assert e <= TOL, e
    assert _same_bits(got[~rc], Sn[~rc])                                                # every other NaN where it was

    # the F and Q given to set() are as they were
    Si = _ints(rng, -3, 4, (N, N))
    d.set(Sigma=Si)
    d.propagate(1)
    assert np.array_equal(d.sigma, F0 @ Si @ F0.T + Q0)
    d.close()


# ---- 3. random operands -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [43, 129, 403, 1003])
def test_init_random_operands(hip, N):
    rng = np.random.default_rng(N)
    d, d2 = hip.DensePropagator64(N), hip.DensePropagator64(N)
    big = N > 1000                                  # (a case there costs numpy and a dense propagation)
    for r, s in (((2, 3), (17, 5), (64, 64)) if big else ((1, 1), (2, 3), (3, 16), (17, 17), (16, 64), (64, 5), (64, 64))):
        if r > N or s > N - r:
            continue
        for first in ([_firsts(N, r)[2]] if big else _firsts(N, r)):
            S = bc.unsymmetric_cov(N, rng)
            x = rng.normal(size=N)
            cols = ic.block_list(N, first, r, s, "scattered", rng)
            G = rng.normal(size=(r, s)) / np.sqrt(s)
            W = np.diag(rng.uniform(1e-4, 1e-2, size=r)) + 1e-4 * rng.normal(size=(r, r))
            xb = rng.normal(size=r)
            wx, wS = ic.np_init_block(x, S, first, r, cols, G, W, xb)
            d.set(Sigma=S)
            d.state = x
            d.init_block(first, G, cols, W, xb)
            got = d.sigma
            e = _block_err(got, wS, first, r)
            F, Q = ic.embedded_FQ(N, first, r, cols, G, W)
            d2.set(F, S, Q)
            d2.propagate(1)
            e2 = _block_err(got, d2.sigma, first, r)
            _note("random_vs_numpy", e); _note("random_vs_dense_propagate", e2)
            assert e <= TOL and e2 <= TOL, (r, s, first, e, e2)
            assert np.array_equal(d.state, wx)
    d.close(); d2.close()


# ---- 4. bit-level properties ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,s", [(2, 3), (2, 5), (16, 16), (17, 31), (64, 64)])
def test_init_corner_is_the_S_of_score_sparse(hip, r, s):
    """S_out of score_sparse(J = 1, m = r, s, cols, Hc = G, R = W) taken before the call, bit for bit"""
    N = 403
    rng = np.random.default_rng(10 * r + s)
    S = bc.unsymmetric_cov(N, rng)
    first = 171
    cols = ic.block_list(N, first, r, s, "scattered", rng)
    G = rng.normal(size=(r, s))
    W = 0.01 * np.eye(r) + 1e-3 * rng.normal(size=(r, r))
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    _, S_out, flags, _ = d.score_sparse(cols[None], G[None], W, want_S=True)
    d.init_block(first, G, cols, W)
    b = np.arange(first, first + r)
    corner = d.sigma_block(b, b)
    d.close()
    assert _same_bits(corner, S_out[0])


@pytest.mark.parametrize("r,s", [(2, 3), (17, 16), (64, 64)])
def test_init_same_bits_wherever_it_sits(hip, r, s):
    """the same source values (s x M row data, M x s column data, the s x s block) planted at three positions in each of
    N = 203 and N = 1003 give the same rows, columns and corner; and the same call twice gives the same bits"""
    rng = np.random.default_rng(60 + r + s)
    M = 203 - r - s                                   # the columns / rows outside b and cols that carry the data
    rowdat, coldat, block = rng.normal(size=(s, M)), rng.normal(size=(M, s)), rng.normal(size=(s, s))
    G = rng.normal(size=(r, s))
    W = 1e-3 * rng.normal(size=(r, r))
    outs = []
    for N in (203, 1003):
        d = hip.DensePropagator64(N)
        for first, order in ((0, "asc"), (((N - r) // 2) | 1, "desc"), (N - r, "scattered")):
            cols = ic.block_list(N, first, r, s, order, rng)
            other = np.ones(N, dtype=bool)
            other[first:first + r] = False
            other[cols] = False
            idx = np.nonzero(other)[0][:M]
            S = rng.normal(size=(N, N))
            S[np.ix_(cols, idx)] = rowdat
            S[np.ix_(idx, cols)] = coldat
            S[np.ix_(cols, cols)] = block
            b = np.arange(first, first + r)
            res = []
            for _ in range(2):
                d.set(Sigma=S)
                d.init_block(first, G, cols, W)
                res.append(d.sigma)
            assert _same_bits(res[0], res[1])                                              # run to run
            g = res[0]
            outs.append((g[np.ix_(b, idx)].copy(), g[np.ix_(idx, b)].copy(), g[np.ix_(b, b)].copy()))
            assert _block_err(g, ic.np_init_block(np.zeros(N), S, first, r, cols, G, W)[1], first, r) <= TOL
        d.close()
    for o in outs[1:]:
        for a, b_ in zip(outs[0], o):
            assert _same_bits(a, b_)


@pytest.mark.parametrize("N,r,first", [(43, 2, 41), (300, 64, 100), (403, 17, 0)])
def test_init_without_a_list_gives_exact_zeros_and_W(hip, N, r, first):
    rng = np.random.default_rng(N)
    S = bc.unsymmetric_cov(N, rng)
    W = rng.normal(size=(r, r))
    W[0, 0] = -0.0                                    # the corner is W's bits, not W plus something
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.init_block(first, W=W)
    got = d.sigma
    b = slice(first, first + r)
    assert _same_bits(got[b, b], W)
    rows, cols = np.delete(got[b, :], np.s_[first:first + r], axis=1), np.delete(got[:, b], np.s_[first:first + r], axis=0)
    assert not _bits(rows).any() and not _bits(cols).any()                              # +0, not -0
    d.set(Sigma=S)
    d.init_block(first, r=r)                          # no W either: the corner is +0
    assert not _bits(d.sigma[b, :]).any() and not _bits(d.sigma[:, b]).any()
    d.close()


# ---- 5. failure paths on a live handle ---------------------------------------------------------------------------------------

def test_init_errors_with_a_live_handle(hip):
    N = 30
    rng = np.random.default_rng(3)
    Sigma, x = rng.normal(size=(N, N)), rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    lib = hip.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    p = lambda a: a.ctypes.data_as(dp)
    q = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(ip)
    G, W, xb = np.ones((2, 3)), np.eye(2), np.ones(2)
    good = [0, 1, 2]
    calls = [(5, 2, 3, [0, 1, N]), (5, 2, 3, [0, 1, 1 << 30]), (5, 2, 3, [0, 1, 1]), (5, 2, 3, [0, -1, 2]),
             (5, 2, 3, [0, 1, 5]), (5, 2, 3, [0, 6, 1]), (-1, 2, 3, good), (N - 1, 2, 3, good), (5, 0, 3, good),
             (5, 65, 3, good), (5, 2, -1, good), (5, 2, 65, good), (0, N - 2, 3, good), (5, N + 1, 0, good)]
    for first, r, s, c in calls:
        keep = np.asarray(c, dtype=np.int32)
        st = lib.ekf_dense64_init_block(d._h, first, r, s, keep.ctypes.data_as(ip), p(G), p(W), p(xb), None)
        assert st == 1 and b"ekf_dense64_init_block" in lib.ekf_last_error(), (first, r, s, c)
    for c, g in ((None, p(G)), (q(good), None)):
        assert lib.ekf_dense64_init_block(d._h, 5, 2, 3, c, g, p(W), p(xb), None) == 1
    out = np.zeros(4)
    two = np.array([0, 1], dtype=np.int32)
    for rows in ([0, N], [-1, 0]):
        a = np.asarray(rows, dtype=np.int32)
        assert lib.ekf_dense64_get_sigma_block(d._h, 2, a.ctypes.data_as(ip), 2, two.ctypes.data_as(ip), p(out)) == 1
        assert lib.ekf_dense64_get_sigma_block(d._h, 2, two.ctypes.data_as(ip), 2, a.ctypes.data_as(ip), p(out)) == 1
        assert b"ekf_dense64_get_sigma_block" in lib.ekf_last_error()
    for first, count in ((N - 1, 2), (0, N + 1), (N, 1)):
        assert lib.ekf_dense64_get_state_block(d._h, first, count, p(out)) == 1
        assert lib.ekf_dense64_set_state_block(d._h, first, count, p(out)) == 1
        assert b"ekf_dense64_set_state_block" in lib.ekf_last_error()
    with pytest.raises(ValueError):
        d.init_block(5, G, [0, 1, 6], W)
    assert _same_bits(d.sigma, Sigma) and _same_bits(d.state, x)
    ms = d.init_block(5, G, good, W, xb)                                # the handle works afterwards
    wx, wS = ic.np_init_block(x, Sigma, 5, 2, good, G, W, xb)
    assert ms > 0.0 and _block_err(d.sigma, wS, 5, 2) <= TOL and np.array_equal(d.state, wx)
    d.close()


# ---- 6. readouts -----------------------------------------------------------------------------------------------------------------

def test_sigma_block_is_numpy_indexing(hip):
    N = 403
    rng = np.random.default_rng(12)
    S = rng.normal(size=(N, N))
    x = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = x
    lists = [([0, 1, 2], [0, 1, 2]), ([N - 1], [N - 1]), ([5], [7]), ([N - 1, 0, 7, 7, 3], [2, 2, N - 1, 0]),
             (rng.integers(0, N, size=256), rng.integers(0, N, size=256)),              # nr * nc = 65536
             (np.arange(N), [N - 1]), ([0], np.arange(N)[::-1]), (rng.integers(0, N, size=65536), [400])]
    for rows, cols in lists:
        got = d.sigma_block(rows, cols)
        assert got.shape == (len(rows), len(cols))
        assert _same_bits(got, S[np.ix_(rows, cols)])
    assert _same_bits(d.sigma, S) and _same_bits(d.state, x)                             # read-only
    d.close()


@pytest.mark.parametrize("N", [5, 128, 129, 403])
def test_state_slices_round_trip(hip, N):
    rng = np.random.default_rng(N)
    x = _ints(rng, -9, 10, N)
    S = _ints(rng, -3, 4, (N, N))
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Sigma=S, Q=np.zeros((N, N)))
    d.state = x
    want = x.copy()
    for first, count in ((0, 1), (0, 3), (N - 1, 1), (N - 2, 2), (1, N - 1), (0, N), (N // 2, 2)):
        assert _same_bits(d.state_block(first, count), want[first:first + count])
        v = _ints(rng, -9, 10, count)
        d.set_state_block(first, v)
        want[first:first + count] = v
        assert _same_bits(d.state, want)
        assert _same_bits(d.state_block(first, count), v)
    # the padding of the state and of Sigma is still zero: an exact block prediction and an exact identity propagation
    r = min(3, N)
    Fr, Qr, dx = _ints(rng, -2, 3, (r, r)), _ints(rng, -5, 6, (r, r)), _ints(rng, -4, 5, r)
    wx, wS = bc.np_predict_literal(want, S, N - r, Fr, Qr, dx)
    d.propagate_block(N - r, Fr, Qr, dx)
    d.propagate(1)
    assert np.array_equal(d.sigma, wS) and np.array_equal(d.state, wx)
    d.close()


# ---- 7. the reference, live -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [20, 200])
@pytest.mark.parametrize("init", ["init_block", "state_only"])
def test_init_against_the_reference_data_association(hip, oracle, n, init):
    """data_association() of the reference's own ekf_slam.cpp from an all-unknown map, 20 ticks that discover a landmark
    each and re-observe earlier ones, against the loop of INTEGRATION.md on the handle: propagate_block -> score_sparse
    over the known prefix -> the rule -> init_block(s = 0, W = 100 I, xb) or correct_sparse -> heading wrap through the
    state slices.  'init_block' starts the handle's landmark blocks at 7 I with stale state entries, so only init_block
    can make the runs agree; 'state_only' keeps the constructor's prior and uses set_state_block alone."""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    steps = ic.discovery_scenario()
    ref = oracle.RefEKF(n)
    known_ref = np.zeros(n, dtype=np.uint8)
    N = 3 + 2 * n
    d = hip.DensePropagator64(N)
    x0, S0 = ic.stale_start(n) if init == "init_block" else ic.prior_start(n)
    d.set(Sigma=S0)
    d.state = x0
    known, scores = 0, []
    for t, (dth, dx, readings) in enumerate(steps):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        known = ic.association_step(d, n, known, dth, dx, readings, init, scores)
        assert known == int(known_ref.sum()) and known_ref[:known].all(), (t, known, known_ref)
    assert known == min(n, len(steps))
    for k, nis in enumerate(scores):
        assert ds.margins_hold(nis), f"scored reading {k}: the scenario's seed must be replaced"
    P = 3 + 2 * known
    gs, gS, rs, rS = d.state, d.sigma, ref.state, ref.cov
    d.close()
    w, e = worst(gs[:P], gS[:P, :P], rs[:P], rS[:P, :P])
    _note(f"reference_live_{init}_n{n}", w)
    assert w <= FP64_TOL, e
    assert not gS[:P, P:].any() and not gS[P:, :P].any() and not rS[:P, P:].any() and not rS[P:, :P].any()
    if init == "state_only":                                                             # then the rest agrees as well
        assert np.array_equal(gS[P:, P:], rS[P:, P:]) and np.array_equal(gs[P:], rs[P:])


# ---- 8. slot recycling ------------------------------------------------------------------------------------------------------------

def test_init_slot_recycling_cycle(hip):
    """n = 200: ten steps with every landmark known, one evicted with init_block(s = 0), re-initialised correlated (s = 3,
    cols = the pose, G = the inverse sensor model's pose Jacobian, W = Gz R Gz^T) from a reading, ten more steps; against
    the same sequence in numpy"""
    N, S, x0, steps, slot = ic.recycling_scenario()
    d, h = hip.DensePropagator64(N), ic.NumpyHandle(N)
    d.set(Sigma=S)
    h.set(S)
    d.state = x0
    h.state = x0.copy()
    b = np.arange(3 + 2 * slot, 5 + 2 * slot)
    pose = np.arange(3)
    seen = {}

    def probe(stage, dev, G, W):
        if stage == "before":
            assert not dev.sigma_block(b, pose).any() and not dev.sigma_block(pose, b).any()
            assert np.array_equal(dev.sigma_block(b, b), ic.PRIOR * np.eye(2))
            seen["want"] = (G @ dev.sigma_block(pose, pose)) @ G.T + W
        else:
            assert np.abs(dev.sigma_block(b, pose)).min() > 0 and np.abs(dev.sigma_block(pose, b)).min() > 0
            corner = dev.sigma_block(b, b)
            seen["corner"] = float(np.abs(corner - seen["want"]).max() / np.abs(seen["want"]).max())
    ic.recycling_run(d, steps, slot, probe)
    ic.recycling_run(h, steps, slot)
    _note("recycling_corner", seen["corner"])
    assert seen["corner"] <= TOL
    w, e = worst(d.state, d.sigma, h.state, h.sigma)
    _note("recycling_cycle", w)
    d.close()
    assert w <= TOL, e


# ---- 9. N = 10003 ---------------------------------------------------------------------------------------------------------------------

def _median(f, iters=9, warmup=2):
    ms = [f() for _ in range(warmup + iters)][warmup:]
    return float(np.median(ms))


def test_init_full_size_n10003_and_time(hip):
    """init_block for (r, s) = (2, 0), (2, 3), (64, 64) on one handle, verified through sigma_block on sampled rows and
    columns against numpy on the gathered inputs (Sigma is never read back); then medians of 9 HIP-event times after 2
    untimed calls: init_block(2, 3) and init_block(64, 64) each below correct_sparse(m = 2, s = 5) timed here -- the
    correction streams 16 N^2 bytes, init_block touches under 32 (r + s) N, so a failure means the kernel walks Sigma.
    The ratios against propagate_block of the same r and the dense propagate are printed, not asserted."""
    N = 10003
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    Sigma = A @ A.T / 64 + np.eye(N)
    Sigma += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))           # unsymmetric
    del A
    x = rng.standard_normal(N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    last = (N - 1) // 64 * 64
    sample = np.array(sorted(set([0, 1, 2, 63, 64, N - 2, N - 1] + list(range(last, N, 5)) +
                                 list(rng.integers(0, N, size=30)))))
    assert _same_bits(d.sigma_block(sample, sample[::-1]), Sigma[np.ix_(sample, sample[::-1])])
    for r, s, first in ((2, 0, 4321), (2, 3, 7001), (64, 64, N - 64)):
        b = np.arange(first, first + r)
        cols = ic.block_list(N, first, r, s, "scattered", rng) if s else None
        if s == 3:
            cols = np.array([0, 1, 2], dtype=np.int32)                                   # the pose
        G = rng.standard_normal((r, s)) / np.sqrt(s) if s else None
        W = 0.01 * np.eye(r) + 1e-3 * rng.standard_normal((r, r))
        xb = rng.standard_normal(r)
        pick = np.array([i for i in sample if not first <= i < first + r])
        if s:
            rows_in, cols_in, blk = d.sigma_block(cols, pick), d.sigma_block(pick, cols), d.sigma_block(cols, cols)
            want = (G @ rows_in, cols_in @ G.T, (G @ blk) @ G.T + W)                     # numpy on the gathered inputs
        else:
            want = (np.zeros((r, len(pick))), np.zeros((len(pick), r)), W)
        before = d.sigma_block(pick, pick)
        d.init_block(first, G, cols, W, xb)
        got = (d.sigma_block(b, pick), d.sigma_block(pick, b), d.sigma_block(b, b))
        e = max(float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-3)) for g, w in zip(got, want))
        _note(f"full_size_r{r}_s{s}", e)
        assert e <= TOL, (r, s, e)
        assert s == 0 or min(float(np.abs(g).max()) for g in got) > 0.0
        assert _same_bits(d.sigma_block(pick, pick), before)                             # the rest is where it was
        assert _same_bits(d.state_block(first, r), xb)
        if s == 0:
            assert not _bits(got[0]).any() and not _bits(got[1]).any() and _same_bits(got[2], W)
    keep = np.ones(N, dtype=bool)
    for first, r in ((4321, 2), (7001, 2), (N - 64, 64)):
        keep[first:first + r] = False
    assert _same_bits(d.state[keep], x[keep])
    # time: the same handle, Sigma as the calls left it (times do not depend on the values)
    c5, H5, R5 = sp.index_list(N, 5, "scattered", rng), rng.standard_normal((2, 5)), 0.01 * np.eye(2)
    G3, W2 = rng.standard_normal((2, 3)), 0.01 * np.eye(2)
    c64 = ic.block_list(N, N - 64, 64, 64, "scattered", rng)
    G64, W64 = rng.standard_normal((64, 64)) / 8.0, 0.01 * np.eye(64)
    t_corr = _median(lambda: d.correct_sparse(c5, H5, R5)[1])
    t_23 = _median(lambda: d.init_block(7001, G3, [0, 1, 2], W2))
    t_6464 = _median(lambda: d.init_block(N - 64, G64, c64, W64))
    t_20 = _median(lambda: d.init_block(4321, W=W2))
    t_corr2 = _median(lambda: d.correct_sparse(c5, H5, R5)[1])
    t_blk2 = _median(lambda: d.propagate_block(7001, np.eye(2), W2))
    t_blk64 = _median(lambda: d.propagate_block(N - 64, np.eye(64), W64))
    t_dense = _median(lambda: d.propagate(1), iters=3, warmup=1)
    d.close()
    print(f"N={N}: init_block (2, 0) {t_20 * 1e3:.1f} us, (2, 3) {t_23 * 1e3:.1f} us, (64, 64) {t_6464 * 1e3:.1f} us; "
          f"correct_sparse(2, 5) {t_corr * 1e3:.1f} us (again {t_corr2 * 1e3:.1f}); propagate_block r = 2 "
          f"{t_blk2 * 1e3:.1f} us, r = 64 {t_blk64 * 1e3:.1f} us; dense propagate {t_dense:.2f} ms")
    print(f"ratios: init(2, 3) / propagate_block(2) {t_23 / t_blk2:.2f}, init(64, 64) / propagate_block(64) "
          f"{t_6464 / t_blk64:.2f}, dense propagate / init(64, 64) {t_dense / t_6464:.0f}, correct_sparse / init(2, 3) "
          f"{t_corr / t_23:.1f}, correct_sparse / init(64, 64) {t_corr / t_6464:.1f}")
    assert t_23 < t_corr, (t_23, t_corr)
    assert t_6464 < t_corr, (t_6464, t_corr)


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 init worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
