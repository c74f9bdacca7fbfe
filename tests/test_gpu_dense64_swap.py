"""-m gpu: the exchange of two blocks of states of the fp64 dense handle (ekf_dense64_swap_blocks): Sigma <- P Sigma P^T,
state <- P state as a pure copy.  1. the bits over the edges of the masking (tests/dense_swap_cases.py's grid: NaN payloads,
-0.0, the padding, twice = identity, (a, b) = (b, a)); 2. carried through pending rows: the count, the read-through on
permuted lists, the flush, against the flush-first model -- integers in bits, random data at 1e-12; 3. the live dimension
with everything outside poisoned, against a twin of dimension Na; 4. refusals change nothing; 5. the removal recipe (swap
with the last block, init_block(s = 0), set_live) against a smaller twin, bit for bit; 6. the reference's
data_association() with two landmarks exchanged for five ticks; 7. N = 10003 and the time condition
median(swap) <= median(correct_sparse(2, 5)).  tests/test_dense64_swap_host.py proves the model."""
import ctypes

import numpy as np
import pytest

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_score_cases as ds
import dense_sparse_cases as sp
import dense_swap_cases as sc
from parity import FP64_TOL, worst
from test_gpu_dense64_sparse import TIGHT, _bits, _full_size_sigma, _median, _same_bits

pytestmark = pytest.mark.gpu


def _poison(N, Na, corner, x):
    """test_gpu_dense64_live._poison: the corner and x[:Na] as given, every other entry a NaN with a payload of its own"""
    S = (np.uint64(0x7FF8000000000000) + np.arange(1, N * N + 1, dtype=np.uint64)).view(np.float64).reshape(N, N).copy()
    S[:Na, :Na] = corner
    xs = (np.uint64(0x7FF8000000000000) + np.arange(7, N + 7, dtype=np.uint64)).view(np.float64).copy()
    xs[:Na] = x
    return S, xs


def _read_cur(d):
    """all of Sigma_cur through the block readout: with the carry policy on it flushes nothing"""
    N, every = d.N, np.arange(d.N)
    step = max(1, 65536 // N)
    return np.vstack([d.sigma_block(np.arange(k, min(N, k + step)), every) for k in range(0, N, step)])


# ---- 1. bits, over the edges of the masking -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", sc.GRID_N)
def test_swap_keeps_every_bit_over_the_edges_of_the_masking(hip, N):
    S, x = sc.unique_data(N)
    Si = (np.arange(N)[:, None] * float(N) + np.arange(N)[None, :]).astype(np.float64)      # the same without NaNs
    d, e = hip.DensePropagator64(N), hip.DensePropagator64(N)
    d.set(F=np.eye(N), Q=np.zeros((N, N)))
    count = 0
    for a, b, r in sc.cases(N):
        wS, wx = sc.swap_model(S, x, a, b, r)
        for h, (fa, fb) in ((d, (a, b)), (e, (b, a))):                  # either order of the arguments
            h.set(Sigma=S)
            h.state = x
            assert h.swap_blocks(fa, fb, r) > 0.0
        got, gx = d.sigma, d.state
        bad = _bits(got) != _bits(wS)
        assert not bad.any(), (N, a, b, r, int(bad.sum()), np.argwhere(bad)[:3])
        assert _same_bits(gx, wx), (N, a, b, r)
        assert _same_bits(e.sigma, wS) and _same_bits(e.state, wx), (N, a, b, r)
        d.swap_blocks(a, b, r)                                          # twice: the original bits
        assert _same_bits(d.sigma, S) and _same_bits(d.state, x), (N, a, b, r)
        # the padding: I Sigma I^T + 0 on the matrix cores returns the swapped integers, which a NaN or an Inf written
        # beyond column N would spoil (the poisoned surroundings of test 3 pin every other value there)
        d.set(Sigma=Si)
        d.swap_blocks(a, b, r)
        d.propagate(1)
        assert np.array_equal(d.sigma, sc.swap_model(Si, x, a, b, r)[0]), (N, a, b, r)
        count += 1
    d.close()
    e.close()
    assert count == len(sc.cases(N)) >= 1


# ---- 2. carried through the pending rows ---------------------------------------------------------------------------------------

def _pending_integers(hip, p, carry):
    """the corrections of cc.carry_chain(200, 3, 'straddle', p, 3) that make p pending rows, on a handle and on the model"""
    chain = cc.carry_chain(200, 3, "straddle", p, 3)
    n = len(cc.RECIPE[p])
    d = hip.DensePropagator64(chain["N"])
    d.carry = carry
    d.set(Sigma=chain["Sigma0"])
    d.state = chain["x0"]
    model = cc.CarriedModel(chain["Sigma0"], chain["x0"])
    listed = []
    for op in chain["ops"][:n]:
        assert op["op"] == "correct"
        nis = d.correct_sparse_deferred(op["cols"], op["Hc"], op["R"], op["nu"])[0]
        assert nis == model.correct_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
        listed += [int(v) for v in op["cols"]]
    assert d.pending == model.pending == p
    return chain, d, model, listed, chain["ops"][n - 1]["check"]["cand"]


@pytest.mark.parametrize("p", [2, 64])
def test_swap_carries_the_pending_rows_integers_bit_for_bit(hip, p):
    chain, d, model, listed, (cand, Hc, R, nu) = _pending_integers(hip, p, True)
    N, first = chain["N"], chain["first"]                              # the block [62, 65): dense in Sigma0 and in K, T
    for a, b, r in ((first, N - 3, 3), (listed[0], listed[1], 1), (0, 64, 64)):
        if abs(a - b) < r:
            continue
        q = sc.perm(N, a, b, r)
        rows = np.array([a, a + r - 1, b, b + r - 1, 0, N - 1, 63, 64] + listed[:6], dtype=np.int32)
        cols = np.array(list(rows[::-1]) + [first, first + 1], dtype=np.int32)
        before = (d.sigma_block(rows, cols), d.score_sparse(cand, Hc, R, nu, want_S=True), d.state)
        assert np.array_equal(before[0], model.read(rows, cols))
        assert d.swap_blocks(a, b, r) > 0.0
        assert d.pending == p                                           # nothing was flushed
        assert _same_bits(d.sigma_block(q[rows], q[cols]), before[0]), (p, a, b, r)
        after = d.score_sparse(q[cand], Hc, R, nu, want_S=True)
        assert _same_bits(after[1], before[1][1]) and _same_bits(after[0], before[1][0]), (p, a, b, r)
        assert not after[2].any() and d.pending == p
        assert _same_bits(d.state, before[2][q])
        # against the flush-first model: Sigma_cur now is the swap of Sigma_cur before
        want, wx = sc.swap_model(model.sigma_cur, model.state, a, b, r)
        assert np.array_equal(_read_cur(d), want) and np.array_equal(d.state, wx), (p, a, b, r)
        model.base, model.state = sc.swap_model(model.base, model.state, a, b, r)
        model.Kt, model.Tp = sc.swap_panels(model.Kt, model.Tp, a, b, r)
    d.flush()
    flat = cc.CarriedModel(chain["Sigma0"], chain["x0"])               # the flush-first sequence from the start
    for op in chain["ops"][:len(cc.RECIPE[p])]:
        flat.correct_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
    flat.flush()
    wS, wx = flat.base, flat.state
    for a, b, r in ((first, N - 3, 3), (listed[0], listed[1], 1), (0, 64, 64)):
        if abs(a - b) >= r:
            wS, wx = sc.swap_model(wS, wx, a, b, r)
    got = d.sigma
    assert _same_bits(got, wS), np.argwhere(_bits(got) != _bits(wS))[:3]
    assert _same_bits(d.state, wx) and d.pending == 0
    d.close()


def test_swap_with_the_carry_policy_off_flushes_first(hip):
    chain, d, model, listed, _ = _pending_integers(hip, 2, False)
    N, first = chain["N"], chain["first"]
    assert d.swap_blocks(N - 3, first, 3) > 0.0
    assert d.pending == 0
    model.flush()
    wS, wx = sc.swap_model(model.base, model.state, first, N - 3, 3)
    assert _same_bits(d.sigma, wS) and _same_bits(d.state, wx)
    d.carry = True                                                      # on, with nothing pending: the same one launch
    d.swap_blocks(first, N - 3, 3)
    assert _same_bits(d.sigma, model.base) and _same_bits(d.state, model.state) and d.pending == 0
    d.close()


@pytest.mark.parametrize("p", [2, 64])
def test_swap_carried_on_random_data_against_the_flush_first_sequence(hip, p):
    """random SPD data: carried swap then flush, against numpy's flush-first sequence, at the 1e-12 the handle's tests hold
    against numpy; whether the bits of a flush-first twin handle were matched too is printed (DESIGN 4.8.10 records it).
    The p rows come from p / 2 corrections of the SLAM shape (m = 2, s = 5, R = 0.01 I) that the other random chains of the
    handle's tests use: S = H Sigma H^T + R is then 2 x 2 with a condition number of a few, so what is compared is the
    swap and the flush, not the inversion of an ill-conditioned S by two different routines."""
    N, m = 200, 2
    rng = np.random.default_rng(40 + p)
    S0 = sc.spd(N, rng) + 1e-3 * rng.normal(size=(N, N))
    x0 = rng.normal(size=N)
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    model = dd.DeferredModel(S0, x0)
    for h in (d, twin):
        h.set(Sigma=S0)
        h.state = x0
    d.carry = True
    for _ in range(p // m):
        c = np.array(rng.permutation(N)[:5], dtype=np.int32)
        Hc, R, nu = rng.normal(size=(m, 5)), 0.01 * np.eye(m), 0.1 * rng.normal(size=m)
        model.correct_deferred(c, Hc, R, nu)
        for h in (d, twin):
            h.correct_sparse_deferred(c, Hc, R, nu)
    assert d.pending == twin.pending == model.pending == p
    swaps = ((62, N - 3, 3), (0, 64, 64), (7, 9, 2))
    model.flush()
    wS, wx = model.base, model.state
    for a, b, r in swaps:
        d.swap_blocks(a, b, r)                                          # carried
        twin.swap_blocks(a, b, r)                                       # the first of them flushes
        wS, wx = sc.swap_model(wS, wx, a, b, r)
    assert d.pending == p and twin.pending == 0
    d.flush()
    gS, gx, tS = d.sigma, d.state, twin.sigma
    w, e = worst(gx, gS, wx, wS)
    wt, _ = worst(twin.state, tS, wx, wS)
    print(f"swap_carried_random_p{p}: carried vs numpy {w:.3e}, flush-first handle vs numpy {wt:.3e}, "
          f"carried == flush-first handle in bits: {_same_bits(gS, tS)}")
    assert w <= TIGHT and wt <= TIGHT, e
    d.close()
    twin.close()


# ---- 3. the live dimension ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Na", [(203, 67), (259, 131)])
def test_swap_at_a_live_dimension_touches_nothing_outside(hip, N, Na):
    corner, xc = sc.unique_data(Na, seed=N)
    S0, x0 = _poison(N, Na, corner, xc)
    outside = np.ones((N, N), dtype=bool)
    outside[:Na, :Na] = False
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(Na)
    d.live = Na
    for a, b, r in sc.cases(Na):
        d.set(Sigma=S0)
        d.state = x0
        twin.set(Sigma=corner)
        twin.state = xc
        d.swap_blocks(b, a, r)
        twin.swap_blocks(a, b, r)
        got, gx = d.sigma, d.state
        wS, wx = sc.swap_model(corner, xc, a, b, r)
        assert _same_bits(got[:Na, :Na], twin.sigma) and _same_bits(got[:Na, :Na], wS), (N, Na, a, b, r)
        assert _same_bits(gx[:Na], twin.state) and _same_bits(gx[:Na], wx), (N, Na, a, b, r)
        bad = _bits(got)[outside] != _bits(S0)[outside]
        assert not bad.any() and _same_bits(gx[Na:], x0[Na:]), (N, Na, a, b, r, int(bad.sum()))
    # a block that reaches the live dimension is refused, and changes nothing
    d.set(Sigma=S0)
    d.state = x0
    for a, b, r in ((0, Na - 1, 2), (Na, 0, 1), (Na - 2, Na + 2, 2), (0, N - 3, 3)):
        with pytest.raises(hip.EkfError) as err:
            d.swap_blocks(a, b, r)
        assert err.value.status == 1
    assert _same_bits(d.sigma, S0) and _same_bits(d.state, x0)
    d.swap_blocks(0, Na - 2, 2)                                         # ends at Na: allowed
    d.close()
    twin.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------

def test_swap_refusals_change_nothing(hip):
    N = 67
    rng = np.random.default_rng(4)
    S0, x0 = sc.spd(N, rng) + 1e-3 * rng.normal(size=(N, N)), rng.normal(size=N)
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    for h in (d, twin):
        h.set(Sigma=S0)
        h.state = x0
        h.carry = True
        for i in (3, 11):
            h.correct_sparse_deferred(sp.slam_cols(i), np.ones((2, 5)) + np.eye(2, 5), 0.01 * np.eye(2), np.array([0.1, -0.2]))
        assert h.pending == 4
    before = (_read_cur(d), d.state)
    lib = hip.load()
    ms = ctypes.c_double(-5.0)
    bad = [(None, 0, 2, 2), (d._h, 0, 2, 0), (d._h, 0, 65, 65), (d._h, -1, 5, 2), (d._h, 5, -2, 2), (d._h, 4, 5, 2),
           (d._h, 5, 4, 2), (d._h, 10, 12, 3), (d._h, 7, 7, 1), (d._h, 7, 7, 2), (d._h, 0, N - 1, 2), (d._h, N, 0, 1),
           (d._h, 0, 2 ** 31 - 1, 2), (d._h, 0, 3, -1)]
    for h, a, b, r in bad:
        assert lib.ekf_dense64_swap_blocks(h, a, b, r, ctypes.byref(ms)) == 1, (a, b, r)
        assert ms.value == -5.0 and d.pending == 4
    for a, b, r in ((4, 5, 2), (7, 7, 1)):                               # the wrapper's own checks say the same
        with pytest.raises(ValueError):
            d.swap_blocks(a, b, r)
    assert _same_bits(_read_cur(d), before[0]) and _same_bits(d.state, before[1]) and d.pending == 4
    d.flush()
    twin.flush()
    assert _same_bits(d.sigma, twin.sigma) and _same_bits(d.state, twin.state)      # the pending rows were as they were
    assert lib.ekf_dense64_swap_blocks(d._h, 4, 6, 2, None) == 0        # adjacent blocks, a null elapsed_ms
    d.close()
    twin.close()


# ---- 5. the removal recipe against a smaller twin ---------------------------------------------------------------------------------

def _ticks(hs, rng, t0, count, landmarks, V=3):
    """`count` ticks of propagate_block(0, 3) and V deferred (2, 5) corrections with carry on, a flush every 4th tick, on every
    handle of hs alike -> the nis of every correction, per handle"""
    out = [[] for _ in hs]
    for t in range(t0, t0 + count):
        Fr, Qr, upd = bc.model_operands(hs[0].state_block(0, 3), 0.1 + 0.01 * t, 0.05)
        marks = rng.integers(0, landmarks, size=V)
        terms = [(sp.slam_cols(int(i)), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2)) for i in marks]
        for k, h in enumerate(hs):
            h.propagate_block(0, Fr, Qr, upd)
            out[k] += [h.correct_sparse_deferred(*tm)[0] for tm in terms]
            if t % 4 == 3:
                h.flush()
    return out


def test_removing_a_landmark_by_the_recipe_equals_a_smaller_twin(hip):
    N, n, gone = 203, 20, 7
    Na = 3 + 2 * n
    rng = np.random.default_rng(57)
    S0 = np.zeros((N, N))
    S0[:Na, :Na] = sc.spd(Na, rng) + 1e-3 * rng.normal(size=(Na, Na))
    S0[Na:, Na:] = ic.PRIOR * np.eye(N - Na)
    x0 = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-2.0, 2.0, size=N - 3)])
    d = hip.DensePropagator64(N)
    d.set(Sigma=S0)
    d.state = x0
    d.carry = True
    d.live = Na
    _ticks([d], rng, 0, 10, n)
    assert d.pending > 0
    d.flush()                                                           # the twin starts from Sigma in memory
    S, x = d.sigma, d.state
    first, last = 3 + 2 * gone, Na - 2
    keep = np.arange(last)
    keep[first:first + 2] = [last, last + 1]                            # landmark 19 in slot 7
    twin = hip.DensePropagator64(last)
    twin.set(Sigma=np.ascontiguousarray(S[np.ix_(keep, keep)]))
    twin.state = x[keep]
    twin.carry = True
    # the recipe
    d.swap_blocks(first, last, 2)
    d.init_block(last, W=ic.PRIOR * np.eye(2))
    d.live = last
    assert d.live == last and _same_bits(d.sigma[:last, :last], twin.sigma) and _same_bits(d.state[:last], twin.state)
    nis_d, nis_t = _ticks([d, twin], rng, 10, 5, n - 1)
    assert nis_d == nis_t and len(nis_d) == 15
    assert d.pending == twin.pending > 0
    corner = np.arange(last)
    assert _same_bits(d.sigma_block(corner, corner), twin.sigma_block(corner, corner))      # through the pending rows
    assert d.coupling(last)[0] == 0                                     # (flushes)
    twin.flush()
    gS, gx = d.sigma, d.state
    assert _same_bits(gS[:last, :last], twin.sigma) and _same_bits(gx[:last], twin.state)
    assert not _same_bits(gS[:last, :last], S[np.ix_(keep, keep)])
    assert np.array_equal(gS[last:Na, last:Na], ic.PRIOR * np.eye(2)) and _same_bits(gS[Na:, Na:], S0[Na:, Na:])
    d.close()
    twin.close()


# ---- 6. the reference's loop -------------------------------------------------------------------------------------------------------

class _Living:
    """test_gpu_dense64_live._Living: every correction deferred, a flush at 32 rows, live = 3 + 2 (known + 1) before the
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


def test_swap_inside_the_reference_data_association_loop(hip, oracle):
    """test_live_against_the_reference_data_association at n = 20; after tick 10 the landmarks in slots 2 and 8 are exchanged
    in the handle and in the caller's list of ids, after tick 15 exchanged back.  The loop associates by score, so it finds
    each landmark in whatever slot it sits: the same decisions, and the reference's state and covariance at the end."""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    n = 20
    steps = ic.discovery_scenario()
    ref = oracle.RefEKF(n)
    known_ref = np.zeros(n, dtype=np.uint8)
    d = hip.DensePropagator64(3 + 2 * n)
    x0, S0 = ic.prior_start(n)
    d.set(Sigma=S0)
    d.state = x0
    d.carry = True
    d.live = 3
    ids = list(range(n))                                                # the caller's bookkeeping: which landmark a slot holds
    known, scores, carried = 0, [], 0
    for t, (dth, dx, readings) in enumerate(steps):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        known = ic.association_step(_Living(d), n, known, dth, dx, readings, "init_block", scores)
        assert d.live == 3 + 2 * known
        assert known == int(known_ref.sum()) and known_ref[:known].all(), (t, known, known_ref)
        if t in (10, 15):
            assert known > 8
            carried = max(carried, d.pending)
            d.swap_blocks(3 + 2 * 2, 3 + 2 * 8, 2)
            ids[2], ids[8] = ids[8], ids[2]
    assert known == min(n, len(steps)) and carried > 0 and ids == list(range(n))
    for k, nis in enumerate(scores):
        assert ds.margins_hold(nis), f"scored reading {k}: the scenario's seed must be replaced"
    d.flush()
    P = 3 + 2 * known
    assert d.coupling(P)[0] == 0
    gs, gS, rs, rS = d.state, d.sigma, ref.state, ref.cov
    d.close()
    w, e = worst(gs[:P], gS[:P, :P], rs[:P], rS[:P, :P])
    print(f"reference_swap_n{n}: {w:.3e}")
    assert w <= FP64_TOL, e
    assert np.array_equal(gS[P:, P:], rS[P:, P:]) and np.array_equal(gs[P:], rs[P:])


# ---- 7. full size and time ---------------------------------------------------------------------------------------------------------

def test_swap_full_size_n10003_and_time(hip):
    """N = 10003, r = 2, the blocks at 3 and N - 2: sampled rows and columns bit for bit the model; HIP-event medians of 9
    after 2 in one process: median(swap) <= median(correct_sparse(2, 5)).  The swap moves 64 r N bytes, the correction's
    update 16 N^2."""
    N, a, b, r = 10003, 3, 10001, 2
    rng = np.random.default_rng(23)
    S = _full_size_sigma(N, rng)
    x = rng.normal(size=N)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = x
    assert d.swap_blocks(a, b, r) > 0.0
    q = sc.perm(N, a, b, r)
    every = np.arange(N)
    pick = np.array([a, a + 1, b, b + 1, 0, 5000], dtype=np.int32)
    assert _same_bits(d.sigma_block(pick, every), S[np.ix_(q[pick], q)])
    assert _same_bits(d.sigma_block(every, pick), S[np.ix_(q, q[pick])])
    more = np.array([2, 5, 63, 64, 127, 128, 9983, 9984, 10000], dtype=np.int32)      # the neighbours and the strip edges
    assert _same_bits(d.sigma_block(more, more), S[np.ix_(more, more)])
    assert _same_bits(d.state, x[q])
    del S
    c, h, R, nu = sp.slam_cols(17), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2)
    t_swap = _median(lambda: d.swap_blocks(a, b, r))
    t_corr = _median(lambda: d.correct_sparse(c, h, R, nu)[1])
    t_init = _median(lambda: d.init_block(b, G=np.ones((2, 3)), cols=[0, 1, 2], W=np.eye(2)))
    d.close()
    print(f"N = {N}: swap_blocks(r = 2) {t_swap:.4f} ms, correct_sparse(2, 5) {t_corr:.4f} ms, init_block(2, 3) {t_init:.4f} ms")
    assert t_swap <= t_corr, (t_swap, t_corr)
