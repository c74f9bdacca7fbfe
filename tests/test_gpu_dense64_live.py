"""-m gpu: the live dimension of the fp64 dense handle (ekf_dense64_set_live, ekf_dense64_coupling): with live = Na < N the
structured calls run the filter of dimension Na in Sigma[:Na, :Na] and state[:Na], read and write nothing outside, and give
the bits of a handle created with N = Na.  Over the grid of tests/dense_live_cases.py (every (N, Na), every list order, every
(m, s) that fits): 1. the integer chains with everything outside the corner poisoned with NaNs, against numpy, against a twin
of dimension Na, and the poison bit for bit; 2. the same after wider calls have left K, T and panel rows beyond Na;
3. growing without a flush, shrinking with one; 4. equality with the full-width call on a decoupled tail; 5. the default
path; 6. refusals; 7. ekf_dense64_coupling; 8. the reference's data_association() with live = 3 + 2 known; 9. N = 10003 and
the time conditions T(live = 2003) <= 0.25 T(live = 10003) for the flush at p = 16 and for correct_sparse(2, 5).
tests/test_dense64_live_host.py proves the chains exact in float64."""
import ctypes

import numpy as np
import pytest

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_live_cases as lc
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst
from test_gpu_dense64_sparse import _bits, _full_size_sigma, _median, _same_bits

pytestmark = pytest.mark.gpu
PAIR_IDS = [f"N{N}-Na{Na}" for N, Na in lc.pairs()]


def _poison(N, Na, corner, x):
    """Sigma and state of dimension N: the corner and x[:Na] as given, every other entry a NaN with a payload of its own"""
    S = (np.uint64(0x7FF8000000000000) + np.arange(1, N * N + 1, dtype=np.uint64)).view(np.float64).reshape(N, N).copy()
    S[:Na, :Na] = corner
    xs = (np.uint64(0x7FF8000000000000) + np.arange(7, N + 7, dtype=np.uint64)).view(np.float64).copy()
    xs[:Na] = x
    return S, xs


def _read_all(d):
    """all of Sigma through the block readout: with the carry policy on it flushes nothing"""
    N, every = d.N, np.arange(d.N)
    step = max(1, 65536 // N)
    return np.vstack([d.sigma_block(np.arange(k, min(N, k + step)), every) for k in range(0, N, step)])


def _call(d, op):
    k = op["op"]
    if k == "eager":
        return d.correct_sparse(op["cols"], op["Hc"], op["R"], op["nu"])[0]
    if k == "deferred":
        return d.correct_sparse_deferred(op["cols"], op["Hc"], op["R"], op["nu"])[0]
    if k == "propagate":
        d.propagate_block(op["first"], op["Fr"], op["Qr"], op["dx"])
    elif k == "init":
        d.init_block(op["first"], G=op["G"], cols=op["cols"], W=op["W"], xb=op["xb"], r=op["r"])
    else:
        d.flush()
    return None


def _run_chain(d, twin, chain, carry, S0, x0, what):
    """the chain on `d` (live = Na inside N) and on `twin` (N = Na): after every call nis, the pending count, the state, the
    scores of two candidates and -- where reading does not flush -- the corner, against numpy and against the twin's bits;
    and every entry outside the corner against the bits of (S0, x0)"""
    Na, N = chain["Na"], d.N
    want = lc.run_model(chain, carry)
    d.carry = twin.carry = carry
    d.set(Sigma=S0)
    d.state = x0
    twin.set(Sigma=chain["Sigma0"])
    twin.state = chain["x0"]
    assert d.live == Na and d.pending == 0
    corner = np.arange(Na)
    out_S = np.ones((N, N), dtype=bool)
    out_S[:Na, :Na] = False
    for i, (op, w) in enumerate(zip(chain["ops"], want)):
        at = what + (carry, i, op["op"])
        a, b = _call(d, op), _call(twin, op)
        assert a == b == w["nis0"], at
        assert d.pending == twin.pending == w["pending"], (at, d.pending, twin.pending, w["pending"])
        xa = d.state
        assert _same_bits(xa[:Na], twin.state) and np.array_equal(xa[:Na], w["state"]), at
        assert _same_bits(xa[Na:], x0[Na:]), at
        cols, Hc, R, nu = op["cand"]
        na, Sa, fa, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
        nb, Sb, fb, _ = twin.score_sparse(cols, Hc, R, nu, want_S=True)
        assert _same_bits(Sa, Sb) and _same_bits(na, nb) and not fa.any() and not fb.any(), at
        assert np.array_equal(Sa, w["S"]) and np.array_equal(na, w["nis"]), at
        assert d.pending == w["pending"], at
        if carry or w["pending"] == 0:
            got = _read_all(d)
            assert np.array_equal(got[:Na, :Na], w["Sigma_cur"]), (at, np.argwhere(got[:Na, :Na] != w["Sigma_cur"])[:3])
            assert _same_bits(got[:Na, :Na], twin.sigma_block(corner, corner)), at
            bad = _bits(got)[out_S] != _bits(S0)[out_S]
            assert not bad.any(), (at, int(bad.sum()), np.argwhere(_bits(got) != _bits(S0))[:3])
    assert d.pending == 0
    got = d.sigma                                                     # the dense readout, all N
    assert np.array_equal(got[:Na, :Na], want[-1]["Sigma_cur"]) and _same_bits(got[:Na, :Na], twin.sigma), what
    assert np.array_equal(_bits(got)[out_S], _bits(S0)[out_S]), what


def _spd(N, rng):
    A = rng.normal(size=(N, N))
    return A @ A.T / N + np.eye(N)


def _leave_leftovers(d, Na, rng):
    """at live = N: a dense correct whose H touches tail columns only (K and T beyond Na stay in the workspace), then 64 rows
    of full-width deferred corrections and their flush (non-zero panel rows at every column)"""
    N = d.N
    d.live = N
    d.set(Sigma=_spd(N, rng))
    d.state = rng.normal(size=N)
    H = np.zeros((1, N))
    H[0, Na:] = rng.normal(size=N - Na) + 2.0
    d.correct(H, np.eye(1), np.ones(1))
    for _ in range(4):
        c = np.array(rng.permutation(N)[:16], dtype=np.int32)
        d.correct_sparse_deferred(c, rng.normal(size=(16, 16)), np.eye(16), rng.normal(size=16))
    assert d.pending == 64
    assert d.flush() > 0.0 and d.pending == 0


# ---- 1. the filter of dimension Na, everything outside poisoned --------------------------------------------------------------

@pytest.mark.parametrize("N,Na", lc.pairs(), ids=PAIR_IDS)
def test_live_is_the_sub_filter_with_everything_outside_poisoned(hip, N, Na):
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(Na)
    d.live = Na
    assert d.live == Na and twin.live == Na
    for order in lc.ORDERS:
        for m, s in lc.shapes(Na):
            chain = lc.live_chain(Na, order, m, s)
            S0, x0 = _poison(N, Na, chain["Sigma0"], chain["x0"])
            for carry in (True, False):
                _run_chain(d, twin, chain, carry, S0, x0, (N, Na, order, m, s))
    d.close()
    twin.close()


# ---- 2. what wider calls left in the workspace and the panels ---------------------------------------------------------------

@pytest.mark.parametrize("N,Na", lc.pairs(), ids=PAIR_IDS)
def test_live_after_wider_calls_left_k_t_and_panel_rows_beyond_it(hip, N, Na):
    """the results are those of a fresh handle: numpy's, the twin's, and the decoupled tail bit for bit"""
    rng = np.random.default_rng(31 * N + Na)
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(Na)
    _leave_leftovers(d, Na, rng)
    d.live = Na
    for order in lc.ORDERS:
        for m, s in lc.shapes(Na):
            chain = lc.live_chain(Na, order, m, s)
            S0, x0 = lc.embed(chain, N, seed=N)
            for carry in (True, False):
                _run_chain(d, twin, chain, carry, S0, x0, (N, Na, order, m, s))
    d.close()
    twin.close()


# ---- 3. growing without a flush, shrinking with one ----------------------------------------------------------------------------

def _grow_chain(Na, r, seed):
    """at dimension Na + r, the block [Na, Na + r) decoupled from the corner: two deferred corrections listed below Na,
    [the handle grows here], init_block of the new block from s = min(3, Na) listed states, a deferred correction that lists
    the new columns, one more below Na"""
    for attempt in range(12):
        rng = np.random.default_rng(100 * seed + attempt)
        Nb = Na + r
        S = np.zeros((Nb, Nb))
        S[:Na, :Na] = rng.integers(-1, 2, size=(Na, Na))
        S[Na:, Na:] = rng.integers(1, 4, size=(r, r))
        x = rng.integers(-9, 10, size=Nb).astype(np.float64)
        model, ops = cc.CarriedModel(S, x), []
        try:
            def correction(lst):
                m = min(2, len(lst))
                c, Hc, R, nu, _ = dd.exact_candidates(model.sigma_cur, 1, m, len(lst), "scattered", rng, first=lst)
                op = {"op": "deferred", "cols": c[0], "Hc": Hc[0], "R": R[0], "nu": nu[0]}
                lc.apply(model, op)
                ops.append(op)
            low = lambda k: np.array(rng.permutation(Na)[:min(k, Na)], dtype=np.int32)
            correction(low(5))
            correction(low(3))
            si = min(3, Na)
            op = {"op": "init", "first": Na, "r": r, "cols": low(si), "G": dd.sparse_rows(rng, r, si, 3),
                  "W": rng.integers(1, 3, size=(r, r)).astype(np.float64), "xb": rng.integers(-9, 10, size=r).astype(np.float64)}
            lc.apply(model, op)
            ops.append(op)
            correction(np.array([Na + r - 1] + [int(v) for v in low(min(4, Na))], dtype=np.int32))
            correction(low(5))
            return {"Na": Nb, "Sigma0": S, "x0": x, "ops": ops, "after": (model.state.copy(), model.sigma_cur, model.pending)}
        except cc.Inexact:
            continue
    raise cc.Inexact(f"no exact growth chain at Na = {Na}")


@pytest.mark.parametrize("N,Na", lc.pairs(), ids=PAIR_IDS)
def test_live_grows_without_a_flush_and_shrinks_with_one(hip, N, Na):
    r = min(2, N - Na)
    Nb = Na + r
    chain = _grow_chain(Na, r, 1000 * N + Na)
    rng = np.random.default_rng(N + Na)
    S0 = np.zeros((N, N))
    S0[:Nb, :Nb] = chain["Sigma0"]
    S0[Nb:, Nb:] = lc.tail_block(N - Nb, 5)[0]
    x0 = np.concatenate([chain["x0"], np.arange(N - Nb, dtype=np.float64)])
    A, B = hip.DensePropagator64(N), hip.DensePropagator64(N)
    for d in (A, B):
        _leave_leftovers(d, Na, rng)                                  # panel rows that are not zero beyond Na
        d.carry = True
        d.set(Sigma=S0)
        d.state = x0
    A.live, B.live = Na, Nb
    want = cc.CarriedModel(chain["Sigma0"], chain["x0"])
    corner = np.arange(Nb)
    for i, op in enumerate(chain["ops"]):
        if i == 2:
            before = A.pending
            A.live = Nb                                               # grows: nothing is flushed
            assert A.pending == before == B.pending > 0 and A.live == Nb
        assert _call(A, op) == _call(B, op) == lc.apply(want, op), (N, Na, i)
        assert A.pending == B.pending == want.pending
        if i >= 2:
            a, b = A.sigma_block(corner, corner), B.sigma_block(corner, corner)
            assert _same_bits(a, b) and np.array_equal(a, want.sigma_cur), (N, Na, i)
            assert _same_bits(A.state, B.state) and np.array_equal(A.state[:Nb], want.state), (N, Na, i)
    assert A.pending == chain["after"][2] > 0
    cur = A.sigma_block(corner, corner)
    assert np.array_equal(cur, chain["after"][1])
    A.live = Na                                                       # shrinks: the rows are applied first, at the old width
    assert A.pending == 0 and A.live == Na and B.pending > 0
    B.flush()
    SA, SB = A.sigma, B.sigma
    assert _same_bits(SA, SB) and np.array_equal(SA[:Nb, :Nb], cur)
    assert _same_bits(SA[Nb:, :], S0[Nb:, :]) and _same_bits(SA[:, Nb:], S0[:, Nb:]) and _same_bits(A.state[Nb:], x0[Nb:])
    A.close()
    B.close()


# ---- 4. equality with the full-width call ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Na", [(203, 83), (403, 203)])
@pytest.mark.parametrize("V", [2, 8])
def test_live_equals_the_full_width_call_on_a_decoupled_tail(hip, N, Na, V):
    """12 ticks of propagate_block(0, 3) and V deferred (2, 5) corrections, a flush every 4 ticks: live = Na on one handle,
    live = N on its twin.  Bits in the corner, in the tail block and in the state; values in the rectangles, where the
    full-width call writes 0 - K T with K = T = 0 and the sign of a zero may differ"""
    rng = np.random.default_rng(7 * N + V)
    S0 = np.zeros((N, N))
    S0[:Na, :Na] = _spd(Na, rng) + 1e-3 * rng.normal(size=(Na, Na))
    S0[Na:, Na:] = _spd(N - Na, rng) + 1e-3 * rng.normal(size=(N - Na, N - Na))
    x0 = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-2.0, 2.0, size=N - 3)])
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    for h in (d, twin):
        h.set(Sigma=S0)
        h.state = x0
        h.carry = True
    d.live = Na
    marks = rng.integers(0, (Na - 3) // 2, size=(12, V))
    for t in range(12):
        Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), 0.1 + 0.01 * t, 0.05)
        for h in (d, twin):
            h.propagate_block(0, Fr, Qr, upd)
        for i in marks[t]:
            c, hc, R, nu = sp.slam_cols(int(i)), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2)
            assert d.correct_sparse_deferred(c, hc, R, nu)[0] == twin.correct_sparse_deferred(c, hc, R, nu)[0]
        assert d.pending == twin.pending == ((t % 4) + 1) * 2 * V
        if t % 4 == 3:
            d.flush()
            twin.flush()
    assert d.coupling(Na)[0] == 0
    a, b = d.sigma, twin.sigma
    assert _same_bits(d.state, twin.state)
    assert _same_bits(a[:Na, :Na], b[:Na, :Na]) and _same_bits(a[Na:, Na:], b[Na:, Na:]) and _same_bits(a[Na:, Na:], S0[Na:, Na:])
    assert np.array_equal(a[:Na, Na:], b[:Na, Na:]) and np.array_equal(a[Na:, :Na], b[Na:, :Na])
    assert not _same_bits(a[:Na, :Na], S0[:Na, :Na])
    d.close()
    twin.close()


# ---- 5. the default path ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [65, 129])
def test_live_equal_to_n_is_the_handle_as_it_was(hip, N):
    """a handle whose setting is never touched, one with live = N set, one that went down to 17 and back: the same bits
    after every call of the sparse / deferred / carried chains, and numpy's numbers"""
    hs = [hip.DensePropagator64(N) for _ in range(3)]
    assert all(h.live == N for h in hs)
    hs[1].live = N
    hs[2].live = 17
    hs[2].live = N
    for order, (m, s) in (("asc", (16, 16)), ("scattered", (17, 5)), ("desc", (2, 64))):
        chain = lc.live_chain(N, order, m, s)
        for carry in (True, False):
            want = lc.run_model(chain, carry)
            for h in hs:
                h.carry = carry
                h.set(Sigma=chain["Sigma0"])
                h.state = chain["x0"]
            for i, (op, w) in enumerate(zip(chain["ops"], want)):
                got = [_call(h, op) for h in hs]
                assert got[0] == got[1] == got[2] == w["nis0"]
                assert [h.pending for h in hs] == [w["pending"]] * 3
                assert _same_bits(hs[0].state, hs[1].state) and _same_bits(hs[0].state, hs[2].state)
                assert np.array_equal(hs[0].state, w["state"])
            S = [h.sigma for h in hs]
            assert _same_bits(S[0], S[1]) and _same_bits(S[0], S[2]) and np.array_equal(S[0], want[-1]["Sigma_cur"])
    for h in hs:
        h.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------

def test_live_refusals_change_nothing_and_the_dense_calls_stay_full_width(hip):
    N, Na = 203, 83
    rng = np.random.default_rng(61)
    S0 = np.zeros((N, N))
    S0[:Na, :Na], S0[Na:, Na:] = _spd(Na, rng), _spd(N - Na, rng)
    x0 = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Sigma=S0, Q=np.zeros((N, N)))
    d.state = x0
    d.carry = True
    lib, dp, ip = hip.load(), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    na = ctypes.c_int(-5)
    assert lib.ekf_dense64_set_live(None, 3) == 1 and lib.ekf_dense64_get_live(None, ctypes.byref(na)) == 1
    assert lib.ekf_dense64_get_live(d._h, None) == 1 and na.value == -5
    for bad in (0, -1, N + 1):
        assert lib.ekf_dense64_set_live(d._h, bad) == 1 and d.live == N
    cnt, mx = ctypes.c_longlong(-5), ctypes.c_double(-5.0)
    assert lib.ekf_dense64_coupling(None, 3, ctypes.byref(cnt), ctypes.byref(mx), None) == 1
    assert lib.ekf_dense64_coupling(d._h, 3, None, ctypes.byref(mx), None) == 1
    assert lib.ekf_dense64_coupling(d._h, 0, ctypes.byref(cnt), ctypes.byref(mx), None) == 1
    assert lib.ekf_dense64_coupling(d._h, N + 1, ctypes.byref(cnt), ctypes.byref(mx), None) == 1
    assert cnt.value == -5 and mx.value == -5.0
    assert lib.ekf_dense64_coupling(d._h, N, ctypes.byref(cnt), None, None) == 0 and cnt.value == 0      # max_abs is nullable
    d.live = Na
    d.correct_sparse_deferred(sp.slam_cols(3), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2))
    assert d.pending == 2
    before = (_read_all(d), d.state)
    inside = np.array([0, 1, 2, 5, 6], dtype=np.int32)
    past = np.array([0, 1, 2, Na - 1, Na], dtype=np.int32)             # one index at the live dimension
    M, R2, v = np.ones((3, 5)), np.eye(2), np.ones(3)
    pm, pr, pv = M.ctypes.data_as(dp), R2.ctypes.data_as(dp), v.ctypes.data_as(dp)
    nis, flag = ctypes.c_double(), ctypes.c_int()
    assert lib.ekf_dense64_correct_sparse(d._h, 2, 5, past.ctypes.data_as(ip), pm, pr, pv, ctypes.byref(nis), None) == 1
    assert lib.ekf_dense64_correct_sparse_deferred(d._h, 2, 5, past.ctypes.data_as(ip), pm, pr, pv, ctypes.byref(nis), None) == 1
    assert lib.ekf_dense64_score_sparse(d._h, 1, 2, 5, past.ctypes.data_as(ip), pm, pr, 1, pv, ctypes.byref(nis), None,
                                        ctypes.byref(flag), None) == 1
    assert lib.ekf_dense64_propagate_block(d._h, Na - 2, 3, pm, None, None, None) == 1
    assert lib.ekf_dense64_init_block(d._h, Na - 1, 2, 0, None, None, None, None, None) == 1
    assert lib.ekf_dense64_init_block(d._h, 10, 2, 5, past.ctypes.data_as(ip), pm, None, None, None) == 1
    assert lib.ekf_dense64_propagate_block(d._h, Na - 3, 3, np.eye(3).ctypes.data_as(dp), None, None, None) == 0   # ends at Na
    assert lib.ekf_dense64_score_sparse(d._h, 1, 2, 5, inside.ctypes.data_as(ip), pm, pr, 1, pv, ctypes.byref(nis), None,
                                        ctypes.byref(flag), None) == 0
    assert d.pending == 2
    after = (_read_all(d), d.state)
    assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1])
    # the readouts keep [0, N); the dense calls flush and act on all N
    assert np.array_equal(d.sigma_block([N - 1, Na], [N - 1, Na]), S0[np.ix_([N - 1, Na], [N - 1, Na])])
    assert np.array_equal(d.state_block(N - 2, 2), x0[N - 2:])
    H = np.zeros((1, N))
    H[0, N - 1] = 1.0
    d.correct(H, np.eye(1), np.ones(1))
    assert d.pending == 0 and d.live == Na
    got = d.sigma
    assert not np.array_equal(got[Na:, Na:], S0[Na:, Na:]) and d.state[N - 1] != x0[N - 1]
    d.propagate(1)
    assert np.allclose(d.sigma, got, rtol=1e-12, atol=0)
    d.set(Sigma=S0)                                                    # leaves the setting alone, as it leaves carry
    assert d.live == Na and d.carry is True
    d.close()


# ---- 7. coupling ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Na", lc.pairs(), ids=PAIR_IDS)
def test_coupling_counts_and_maximum(hip, N, Na):
    rng = np.random.default_rng(3 * N + Na)
    S = np.full((N, N), -0.0)                                          # the rectangles: -0.0 everywhere, which does not count
    S[:Na, :Na] = rng.normal(size=(Na, Na)) + 5.0                      # the corner and the tail are not looked at
    S[Na:, Na:] = rng.normal(size=(N - Na, N - Na)) + 50.0
    outside = np.zeros((N, N), dtype=bool)
    outside[:Na, Na:] = outside[Na:, :Na] = True
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    assert d.coupling(Na)[:2] == (0, 0.0)
    up = lambda k: -(-Na // k) * k
    spots = sorted({j for j in (Na, up(16) - 1, up(16), up(64) - 1, up(64), up(128) - 1, up(128), N - 1) if Na <= j < N})
    planted = 0
    for step, (i, j, v) in enumerate([(0, spots[-1], 0.5), (spots[0], Na - 1, -0.25)]):      # one entry in each rectangle
        S[i, j] = v
        planted += 1
        d.set(Sigma=S)
        assert d.coupling(Na)[:2] == (planted, 0.5), (step, d.coupling(Na))
    for k, j in enumerate(spots):                                      # the 16 / 64 / 128 slack just past Na, both ways
        S[Na - 1, j], S[j, 0] = 1.0 + k, -(2.0 + k)
    S[0, spots[0]] = 1e-320                                            # a subnormal is not zero
    d.set(Sigma=S)
    want = (int(np.count_nonzero(S[outside] != 0.0)), float(np.abs(S[outside]).max()))
    assert want[0] >= 3 and want[1] == 1.0 + len(spots)
    first = d.coupling(Na)
    assert first[:2] == want and first[2] > 0.0
    assert d.coupling(Na)[:2] == want                                  # twice the same
    assert _same_bits(d.sigma, S)                                      # read-only
    assert d.coupling(N)[:2] == (0, 0.0)
    if Na >= 5:                                                        # it flushes first: the pending rows count
        d.correct_sparse_deferred(np.arange(5, dtype=np.int32), rng.normal(size=(2, 5)), np.eye(2), np.ones(2))
        assert d.pending == 2
        got = d.coupling(Na)
        assert d.pending == 0
        T = d.sigma
        assert got[:2] == (int(np.count_nonzero(T[outside] != 0.0)), float(np.abs(T[outside]).max())) and got[0] > want[0]
    d.close()


# ---- 8. the reference's loop ---------------------------------------------------------------------------------------------------------

class _Living:
    """the handle with every correction deferred, a flush at 32 rows, and live = 3 + 2 (known + 1) set before the
    init_block of a new landmark"""

    def __init__(self, d):
        self._d = d

    def __getattr__(self, name):
        return getattr(self._d, name)

    def init_block(self, first, **kw):
        self._d.live = first + 2
        return self._d.init_block(first, **kw)

    def correct_sparse(self, cols, Hc, R, nu=None):
        out = self._d.correct_sparse_deferred(cols, Hc, R, nu)
        if self._d.pending >= 32:
            self._d.flush()
        return out


@pytest.mark.parametrize("n", [20, 200])
def test_live_against_the_reference_data_association(hip, oracle, n):
    """test_carry_against_the_reference_data_association from an all-unknown map with live = 3 + 2 known throughout"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    steps = ic.discovery_scenario()
    ref = oracle.RefEKF(n)
    known_ref = np.zeros(n, dtype=np.uint8)
    d = hip.DensePropagator64(3 + 2 * n)
    x0, S0 = ic.prior_start(n)
    d.set(Sigma=S0)
    d.state = x0
    d.carry = True
    d.live = 3
    known, scores, most = 0, [], 0
    for t, (dth, dx, readings) in enumerate(steps):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        known = ic.association_step(_Living(d), n, known, dth, dx, readings, "init_block", scores)
        most = max(most, d.pending)
        assert d.live == 3 + 2 * known
        assert known == int(known_ref.sum()) and known_ref[:known].all(), (t, known, known_ref)
    assert known == min(n, len(steps)) and most > 2 * max(len(r) for _, _, r in steps)
    for k, nis in enumerate(scores):
        assert ds.margins_hold(nis), f"scored reading {k}: the scenario's seed must be replaced"
    d.flush()
    P = 3 + 2 * known
    assert d.coupling(P)[0] == 0
    gs, gS, rs, rS = d.state, d.sigma, ref.state, ref.cov
    d.close()
    w, e = worst(gs[:P], gS[:P, :P], rs[:P], rS[:P, :P])
    print(f"reference_live_n{n}: {w:.3e}")
    assert w <= FP64_TOL, e
    assert np.array_equal(gS[P:, P:], rS[P:, P:]) and np.array_equal(gs[P:], rs[P:])


# ---- 9. full size and time ---------------------------------------------------------------------------------------------------------

def test_live_full_size_n10003_and_time(hip):
    """N = 10003 with a decoupled tail: the flush at p = 16 and correct_sparse(2, 5), HIP-event medians of 9 after 2, at
    live = 2003 against live = N on the same handle.  The bytes go as (2048 / 10112)^2 = 0.04; the condition leaves a
    factor 6 above that for the launch floor of these launches at this width, which nobody has measured:
    T(live = 2003) <= 0.25 T(live = 10003).  coupling(2003) is timed and printed; nothing is asserted about it."""
    N, Na = 10003, 2003
    rng = np.random.default_rng(19)
    S = np.zeros((N, N))
    S[:Na, :Na] = _full_size_sigma(Na, rng)
    S[np.arange(Na, N), np.arange(Na, N)] = 100.0
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = rng.normal(size=N)
    del S
    corr = [(sp.slam_cols(int(i)), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2))
            for i in rng.choice(1000, size=9, replace=False)]

    def flush16():
        for c, h, R, nu in corr[:8]:
            d.correct_sparse_deferred(c, h, R, nu)
        assert d.pending == 16
        return d.flush()
    t = {}
    for live in (N, Na, N):
        d.live = live
        t[("flush", live)] = _median(flush16)
        t[("correct", live)] = _median(lambda: d.correct_sparse(*corr[8])[1])
    t_coupling = _median(lambda: d.coupling(Na)[2])
    assert d.coupling(Na)[0] == 0
    d.close()
    print(f"N = {N}: flush at p = 16: live = N {t[('flush', N)]:.4f} ms, live = {Na} {t[('flush', Na)]:.4f} ms "
          f"(ratio {t[('flush', Na)] / t[('flush', N)]:.3f}); correct_sparse(2, 5): live = N {t[('correct', N)]:.4f} ms, "
          f"live = {Na} {t[('correct', Na)]:.4f} ms (ratio {t[('correct', Na)] / t[('correct', N)]:.3f}); "
          f"coupling({Na}) {t_coupling:.4f} ms")
    assert t[("flush", Na)] <= 0.25 * t[("flush", N)], t
    assert t[("correct", Na)] <= 0.25 * t[("correct", N)], t
