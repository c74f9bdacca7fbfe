"""-m gpu: the pending rows of the fp64 dense handle carried across ticks (ekf_dense64_set_carry, ekf_dense64_carry.hip): with
the policy on propagate_block and init_block map the rows of both pending panels instead of flushing them and the block
readout reads through them.  Integer chains bit-exact against numpy over the grid of tests/dense_carry_cases.py
(tests/test_dense64_carry_host.py proves them exact in float64); untouched entries; random operands against the flush-first
sequence on a twin handle (carry off) within 1e-12 per block; the bit-level properties of the fixed order; the policy; the
reference's data_association() live with a flush only at 32 rows; N = 10003 with the time condition
T_carried <= 0.7 T_per_tick.

The grid: the issue's N x r x placement x p x s cannot be run as a full product with at most a quarter skipped (N = 1 and
N = 5 alone cannot hold more than a quarter of it), so a cell is (r, placement, p, s), it is run at EVERY N that can hold it,
and the assertion is that at most a quarter of the cells is held by no N at all (12 of 180: a one-wide block cannot
straddle column 64).

None of this file has been run on a GPU yet: the chains are proven exact and the carried model
equal to the flush-first model on the host, the time condition is derived, and no figure has been measured."""
import ctypes

import numpy as np
import pytest

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_init_cases as ic
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst
from test_gpu_dense64_sparse import TIGHT, _full_size_sigma, _median, _random_sigma, _rel, _same_bits

pytestmark = pytest.mark.gpu
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _handle(hip, Sigma, x, carry=True):
    N = len(x)
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Sigma=Sigma, Q=np.zeros((N, N)))
    d.state = x
    d.carry = carry
    return d


def test_carry_property_and_null_arguments(hip):
    d = hip.DensePropagator64(5)
    assert d.carry is False                                          # the default
    d.carry = True
    assert d.carry is True
    d.carry = False
    assert d.carry is False
    lib, on = hip.load(), ctypes.c_int(7)
    assert lib.ekf_dense64_set_carry(None, 1) == 1 and lib.ekf_dense64_get_carry(None, ctypes.byref(on)) == 1
    assert lib.ekf_dense64_get_carry(d._h, None) == 1 and on.value == 7
    assert lib.ekf_dense64_set_carry(d._h, 5) == 0 and d.carry is True   # anything but 0 is on
    d.close()


# ---- 1. exact integers ---------------------------------------------------------------------------------------------------

def _call(d, chain, op):
    first, r = chain["first"], chain["r"]
    if op["op"] == "correct":
        nis, _ = d.correct_sparse_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
        assert nis == op["nis"]
    elif op["op"] == "propagate":
        d.propagate_block(first, op["Fr"], op["Qr"], op["dx"])
    else:
        d.init_block(first, G=op["G"], cols=op["cols"], W=op["W"], xb=op["xb"], r=r)


@pytest.mark.parametrize("N", cc.GRID_N)
def test_carry_integer_chains_exact(hip, N):
    """every grid point this N holds, on one handle: after every call the state, the count, a readout through the pending
    rows, the scores of three candidates, and sigma_block(cols, cols) pushed through the scoring's order (exact here, so
    numpy's products) against S_out; after the flush all of Sigma, and an identity propagation that would show anything
    written into the padding of Sigma or of the panels"""
    run, cells, nowhere = cc.grid()
    assert len(nowhere) * 4 <= len(cells), (len(nowhere), len(cells))
    mine = [g for g in run if g[0] == N]
    assert mine
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Q=np.zeros((N, N)))
    d.carry = True
    for g in mine:
        chain = cc.carry_chain(*g)
        d.set(Sigma=chain["Sigma0"])
        d.state = chain["x0"]
        assert d.pending == 0
        for i, op in enumerate(chain["ops"]):
            _call(d, chain, op)
            ck, what = op["check"], (g, i, op["op"])
            assert d.pending == ck["pending"], (what, d.pending, ck["pending"])
            assert np.array_equal(d.state, ck["state"]), what
            got = d.sigma_block(ck["rows"], ck["cols"])
            assert np.array_equal(got, ck["block"]), (what, np.argwhere(got != ck["block"])[:3])
            cols, Hc, R, nu = ck["cand"]
            nis, S, flags, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
            assert np.array_equal(S, ck["S"]) and np.array_equal(nis, ck["nis"]) and not flags.any(), what
            blk = d.sigma_block(cols[0], cols[0])
            assert np.array_equal((Hc[0] @ blk) @ Hc[0].T + R[0], S[0]), what
            assert d.pending == ck["pending"], what                  # the readouts and the scores are read-only
        assert d.pending == chain["pending_end"] > 0
        assert d.flush() > 0.0 and d.pending == 0
        got = d.sigma
        bad = got != chain["Sigma"]
        assert not bad.any(), f"{g}: {bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
        d.propagate(1)                                               # I Sigma I^T + 0: exact unless a padding is not zero
        assert np.array_equal(d.sigma, chain["Sigma"]) and np.array_equal(d.state, chain["ops"][-1]["check"]["state"]), g
    d.close()


# ---- 2. untouched entries ------------------------------------------------------------------------------------------------------

def _deferred(N, count, rng, avoid=()):
    """`count` (2, 5) corrections in the reference's columns, a landmark never twice and none in `avoid`"""
    pool = [i for i in range((N - 3) // 2) if i not in avoid]
    out = []
    for i in rng.choice(pool, size=count, replace=False):
        out.append((sp.slam_cols(int(i)), rng.normal(size=(2, 5)), 0.01 * np.eye(2) + 1e-3 * rng.normal(size=(2, 2)),
                    0.1 * rng.normal(size=2)))
    return out


@pytest.mark.parametrize("call,first,r", [("propagate", 0, 3), ("propagate", 60, 17), ("init", 60, 17), ("init0", 101, 2),
                                          ("propagate", 139, 64)])
def test_carry_leaves_everything_else_untouched(hip, call, first, r):
    """handle A carries five corrections through the call, its twin B makes the same corrections and not the call; both
    flush.  Outside the block's rows and columns the flush reads Sigma_base[i][j], K^T[:, i] and T[:, j], so equal bits
    there say that the call wrote none of them on A.  Rows >= p of the panels are never read before a correction rewrites
    them whole, so what can be seen of them is that a further correction and flush on both give the same bits."""
    N = 203
    rng = np.random.default_rng(500 + first + r)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    chain = _deferred(N, 6, rng)
    Fr, Qr = np.eye(r) + 0.1 * rng.normal(size=(r, r)), 1e-3 * rng.normal(size=(r, r))
    cols = ic.block_list(N, first, r, 3, "scattered", rng)
    G = rng.normal(size=(r, 3))
    A, B = _handle(hip, Sigma, x), _handle(hip, Sigma, x)
    for c, h, R, nu in chain[:5]:
        A.correct_sparse_deferred(c, h, R, nu)
        B.correct_sparse_deferred(c, h, R, nu)
    if call == "propagate":
        A.propagate_block(first, Fr, Qr, np.ones(r))
    elif call == "init":
        A.init_block(first, G=G, cols=cols, W=Qr, xb=np.ones(r))
    else:
        A.init_block(first, W=Qr, r=r)
    assert A.pending == B.pending == 10
    outside = np.ones(N, dtype=bool)
    outside[first:first + r] = False
    keep = np.ix_(outside, outside)
    pre = A.sigma_block(np.nonzero(outside)[0][::7], np.nonzero(outside)[0][::5])       # carried readout, outside: B's bits
    assert _same_bits(pre, B.sigma_block(np.nonzero(outside)[0][::7], np.nonzero(outside)[0][::5]))
    assert A.pending == 10
    A.flush()
    B.flush()
    SA, SB = A.sigma, B.sigma
    assert _same_bits(SA[keep], SB[keep])
    assert not _same_bits(SA[first:first + r], SB[first:first + r])              # (the call did something)
    B.set(Sigma=SA)                                                              # the same covariance again, rows >= p next
    B.state = A.state
    c, h, R, nu = chain[5]
    A.correct_sparse_deferred(c, h, R, nu)
    B.correct_sparse_deferred(c, h, R, nu)
    A.flush()
    B.flush()
    assert _same_bits(A.sigma, B.sigma) and _same_bits(A.state, B.state)
    A.close()
    B.close()


# ---- 3. against the flush-first sequence ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [203, 1003])
@pytest.mark.parametrize("V", [2, 8])
def test_carry_against_flush_first_sequence(hip, N, V):
    """12 ticks of propagate_block(0, 3) and V deferred (2, 5) corrections, a correlated init_block(s = 3) of a fresh
    landmark at tick 5, the pose covariance through sigma_block every tick; carried with a flush every 4 ticks and at the
    end, against the same calls on a twin with the policy off"""
    rng = np.random.default_rng(41 * N + V)
    Sigma, x = _random_sigma(N, rng), np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-2.0, 2.0, size=N - 3)])
    fresh = (N - 3) // 2 - 1                                          # the landmark that tick 5 initialises
    chain = _deferred(N, 12 * V, rng, avoid=(fresh,))
    G, W = rng.normal(size=(2, 3)), 0.01 * np.eye(2) + 1e-3 * rng.normal(size=(2, 2))
    d, twin = _handle(hip, Sigma, x, carry=True), _handle(hip, Sigma, x, carry=False)
    pose, most = np.arange(3), 0
    for t in range(12):
        Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), 0.1 + 0.01 * t, 0.05)
        for h in (d, twin):
            h.propagate_block(0, Fr, Qr, upd)
        assert twin.pending == 0 and d.pending == (t % 4) * 2 * V
        for c, hc, R, nu in chain[t * V:(t + 1) * V]:
            got, want = d.correct_sparse_deferred(c, hc, R, nu)[0], twin.correct_sparse_deferred(c, hc, R, nu)[0]
            _note("vs_flush_first_nis", abs(got - want) / abs(want))
            assert abs(got - want) <= TIGHT * abs(want), (t, got, want)
        if t == 5:
            for h in (d, twin):
                h.init_block(3 + 2 * fresh, G=G, cols=[0, 1, 2], W=W, xb=np.array([0.5, -0.5]))
        most = max(most, d.pending)
        a, b = d.sigma_block(pose, pose), twin.sigma_block(pose, pose)
        _note("vs_flush_first_pose_block", _rel(a, b))
        assert _rel(a, b) <= TIGHT
        assert d.pending == ((t % 4) + 1) * 2 * V and twin.pending == 0
        if t % 4 == 3:
            d.flush()
    assert most == 8 * V
    d.flush()
    w, e = worst(d.state, d.sigma, twin.state, twin.sigma)
    _note(f"vs_flush_first_state_cov_V{V}", w)
    assert w <= TIGHT, e
    d.close()
    twin.close()


# ---- 4. bits -----------------------------------------------------------------------------------------------------------------

def _carried_sequence(hip, N, first, r, lists, data, carry=True):
    """Sigma zero but for `data` planted on the block and the listed columns (in their order of appearance), three
    corrections listed outside the block, propagate_block, init_block from the first list, readouts of everything planted"""
    spots = np.concatenate([np.arange(first, first + r)] + [np.asarray(c) for c in lists])
    k = len(spots)
    Sigma = np.zeros((N, N))
    Sigma[np.ix_(spots, spots)] = data["S"][:k, :k]
    d = _handle(hip, Sigma, np.zeros(N), carry=carry)
    log = []
    for c, (h, R, nu) in zip(lists, data["corr"]):
        log.append(d.correct_sparse_deferred(c, h, R, nu)[0])
    d.propagate_block(first, data["Fr"], data["Qr"], np.ones(r))
    log.append(d.sigma_block(spots, spots))
    d.init_block(first, G=data["G"], cols=lists[0], W=data["Qr"], xb=np.ones(r))
    log.append(d.sigma_block(spots, spots))
    log.append(d.pending)
    d.flush()
    log.append(d.sigma_block(spots, spots))
    d.close()
    return log


def test_carry_same_data_same_bits_anywhere_and_twice(hip):
    """the same block data and the same listed values at two `first` in each of two N, and twice in one place: the mapped
    panel entries enter every readout below through the fold, so equal bits of the readouts are equal bits of the map"""
    rng = np.random.default_rng(97)
    r, s = 17, 5
    k = r + 3 * s
    data = {"S": rng.normal(size=(k, k)) + 3.0 * np.eye(k), "Fr": np.eye(r) + 0.1 * rng.normal(size=(r, r)),
            "Qr": 1e-3 * rng.normal(size=(r, r)), "G": rng.normal(size=(r, s)),
            "corr": [(rng.normal(size=(2, s)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2)) for _ in range(3)]}
    seen = []
    for N, first, base in ((203, 0, 100), (203, 60, 20), (1003, 900, 3), (1003, 900, 3)):
        lists = [np.arange(base + 7 * i, base + 7 * i + s, dtype=np.int32)[::-1].copy() for i in range(3)]
        seen.append(_carried_sequence(hip, N, first, r, lists, data))
    for other in seen[1:]:
        assert seen[0][-2] == other[-2] == 6
        for a, b in zip(seen[0], other):
            assert _same_bits(a, b)


def test_carry_on_with_nothing_pending_is_carry_off(hip):
    N = 203
    rng = np.random.default_rng(98)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    Fr, Qr, G = np.eye(17) + 0.1 * rng.normal(size=(17, 17)), 1e-3 * rng.normal(size=(17, 17)), rng.normal(size=(17, 3))
    rows, cols = rng.integers(0, N, size=9), rng.integers(0, N, size=7)
    out = []
    for carry in (True, False):
        d = _handle(hip, Sigma, x, carry=carry)
        d.propagate_block(60, Fr, Qr, np.ones(17))
        a = d.sigma_block(rows, cols)
        d.init_block(60, G=G, cols=[0, 1, 2], W=Qr, xb=np.ones(17))
        d.init_block(7, W=np.eye(2), r=2)
        out.append((a, d.sigma_block(rows, cols), d.state, d.sigma))
        assert d.pending == 0
        d.close()
    for a, b in zip(*out):
        assert _same_bits(a, b)


# ---- 5. policy -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", ["propagate", "correct", "score", "correct_sparse", "sigma"])
def test_the_dense_calls_still_flush_with_carry_on(hip, call):
    """test_every_other_call_flushes for the five calls that need Sigma in memory, with the policy on"""
    from test_gpu_dense64_deferred import _other_calls, _random_chain
    N = 203
    rng = np.random.default_rng(77)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    chain = _random_chain(N, [(2, 5), (8, 16)], rng)
    F, Q, calls = _other_calls(N, rng)
    out = []
    for explicit in (False, True):
        d = hip.DensePropagator64(N)
        d.set(F=F, Sigma=Sigma, Q=Q)
        d.state = x
        d.carry = True
        for c, h, R, nu in chain:
            d.correct_sparse_deferred(c, h, R, nu)
        assert d.pending == 10
        if explicit:
            assert d.flush() > 0.0
        res = calls[call](d)
        assert d.pending == 0
        out.append(tuple(res) + (d.state, d.sigma))
        d.close()
    for u, v in zip(*out):
        assert _same_bits(u, v)


def test_carry_policy_set_switch_and_refused_calls(hip):
    N = 203
    rng = np.random.default_rng(79)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    chain = _deferred(N, 2, rng)
    other = rng.normal(size=(N, N))
    d, e = _handle(hip, Sigma, x), _handle(hip, Sigma, x, carry=False)
    for c, h, R, nu in chain:
        d.correct_sparse_deferred(c, h, R, nu)
        e.correct_sparse_deferred(c, h, R, nu)
    Fr = np.eye(3)
    d.propagate_block(0, Fr)
    assert d.pending == 4
    d.set(Sigma=other)                                               # the rows belonged to the covariance it replaces
    assert d.pending == 0 and d.carry is True and _same_bits(d.sigma, other)
    d.set(Sigma=Sigma)
    d.state = x
    for c, h, R, nu in chain:
        d.correct_sparse_deferred(c, h, R, nu)
    for on in (False, True, False, True):                            # switching touches nothing
        d.carry = on
        assert d.pending == 4
    lib, dp, ip = hip.load(), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    bad = np.array([0, 1, N], dtype=np.int32)
    inside = np.array([0, 1, 8], dtype=np.int32)
    M = np.ones((3, 3))
    assert lib.ekf_dense64_propagate_block(d._h, N - 2, 3, M.ctypes.data_as(dp), None, None, None) == 1
    assert lib.ekf_dense64_propagate_block(d._h, 0, 65, M.ctypes.data_as(dp), None, None, None) == 1
    assert lib.ekf_dense64_init_block(d._h, 7, 3, 3, bad.ctypes.data_as(ip), M.ctypes.data_as(dp), None, None, None) == 1
    assert lib.ekf_dense64_init_block(d._h, 7, 3, 3, inside.ctypes.data_as(ip), M.ctypes.data_as(dp), None, None, None) == 1
    assert lib.ekf_dense64_get_sigma_block(d._h, 3, bad.ctypes.data_as(ip), 1, bad.ctypes.data_as(ip),
                                           M.ctypes.data_as(dp)) == 1
    assert d.pending == 4
    d.flush()
    e.flush()
    assert _same_bits(d.state, e.state) and _same_bits(d.sigma, e.sigma)
    # switched off with rows pending: the next call flushes, as a handle that never carried
    for h in (d, e):
        for c, hc, R, nu in chain:
            h.correct_sparse_deferred(c, hc, R, nu)
    d.carry = False
    d.propagate_block(0, Fr + 0.01)
    e.propagate_block(0, Fr + 0.01)
    assert d.pending == e.pending == 0 and _same_bits(d.sigma, e.sigma)
    d.close()
    e.close()


# ---- 6. the reference, live ----------------------------------------------------------------------------------------------------

class _Carrying:
    """the handle with correct_sparse forwarded to correct_sparse_deferred and a flush only at 32 rows"""

    def __init__(self, d):
        self._d = d

    def __getattr__(self, name):
        return getattr(self._d, name)

    def correct_sparse(self, cols, Hc, R, nu=None):
        out = self._d.correct_sparse_deferred(cols, Hc, R, nu)
        if self._d.pending >= 32:
            self._d.flush()
        return out


@pytest.mark.parametrize("n", [20, 200])
def test_carry_against_the_reference_data_association(hip, oracle, n):
    """test_deferred_against_the_reference_data_association with the policy on: propagate_block no longer flushes, the
    rows of several ticks are pending while the readings are scored"""
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
    known, scores, most = 0, [], 0
    for t, (dth, dx, readings) in enumerate(steps):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        known = ic.association_step(_Carrying(d), n, known, dth, dx, readings, "state_only", scores)
        most = max(most, d.pending)
        assert known == int(known_ref.sum()) and known_ref[:known].all(), (t, known, known_ref)
    assert known == min(n, len(steps))
    assert most > 2 * max(len(r) for _, _, r in steps), most          # more than one tick produces: rows were carried
    for k, nis in enumerate(scores):
        assert ds.margins_hold(nis), f"scored reading {k}: the scenario's seed must be replaced"
    d.flush()
    P = 3 + 2 * known
    gs, gS, rs, rS = d.state, d.sigma, ref.state, ref.cov
    d.close()
    w, e = worst(gs[:P], gS[:P, :P], rs[:P], rS[:P, :P])
    _note(f"reference_live_carried_n{n}", w)
    assert w <= FP64_TOL, e
    assert np.array_equal(gS[P:, P:], rS[P:, P:]) and np.array_equal(gs[P:], rs[P:])


# ---- 7. full size and time -------------------------------------------------------------------------------------------------------

def test_carry_full_size_n10003_and_time(hip):
    """8 ticks of propagate_block(0, 3) and two deferred (2, 5) corrections at N = 10003, carried: sampled rows and columns
    through sigma_block (with 32 rows pending, and again after the flush) against numpy on the gathered data.  Then
    HIP-event sums, medians of 9 after 2, on the same handle: T_carried = the 8 ticks with the policy on and one flush at
    p = 32; T_per_tick = the same ticks with the policy off (every propagate_block flushes the tick before it) and the
    flush of the last tick.  The condition, derived and not measured: the per-tick form streams 16 N^2 bytes eight times,
    >= 8 x 0.30 ms; the carried form once at rank 32, less than the 0.90 ms of a dense correct at m = 32; both pay the
    same launch-bound calls: T_carried <= 0.7 T_per_tick."""
    N, ticks = 10003, 8
    rng = np.random.default_rng(18)
    Sigma = _full_size_sigma(N, rng)
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    d.carry = True
    picks = [int(i) for i in rng.choice(5000, size=2 * ticks, replace=False)]
    corr = [(sp.slam_cols(i), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2)) for i in picks]
    pred = [(np.eye(3) + 0.005 * rng.normal(size=(3, 3)), 1e-4 * np.eye(3), 0.01 * rng.normal(size=3)) for _ in range(ticks)]
    last = (N - 1) // 128 * 128
    rows = np.array(sorted(set([0, 1, 2, N - 1] + [3 + 2 * i for i in picks[:6]] + list(range(last, N, 5)) +
                               list(rng.integers(0, N, size=12)))))
    cl = np.array(sorted(set([0, 1, 2, N - 1, N - 2] + [4 + 2 * i for i in picks[:6]] + list(rng.integers(0, N, size=10)))))
    need = np.array(sorted(set(rows) | set(cl) | set(int(v) for c, _, _, _ in corr for v in c)))
    pos = {int(v): k for k, v in enumerate(need)}
    assert list(need[:3]) == [0, 1, 2]
    Rw, Cw, xs = Sigma[need, :].copy(), Sigma[:, need].copy(), x.copy()       # rows / columns of Sigma_cur that matter
    nis_want, got_nis = [], []
    for t in range(ticks):
        Fr, Qr, upd = pred[t]
        Rw[:, :3] = Rw[:, :3] @ Fr.T                                           # F Sigma F^T + Q on the gathered rows ..
        Rw[:3, :] = Fr @ Rw[:3, :]
        Rw[:3, :3] += Qr
        Cw[:, :3] = Cw[:, :3] @ Fr.T                                           # .. and columns
        Cw[:3, :] = Fr @ Cw[:3, :]
        Cw[:3, :3] += Qr
        xs[:3] += upd
        d.propagate_block(0, Fr, Qr, upd)
        for c, h, R, nu in corr[2 * t:2 * t + 2]:
            idx = [pos[int(v)] for v in c]
            T, U = h @ Rw[idx, :], Cw[:, idx] @ h.T
            Si = np.linalg.inv(T[:, c] @ h.T + R)
            K = U @ Si
            nis_want.append(float(nu @ Si @ nu))
            xs = xs + K @ nu
            Rw, Cw = Rw - K[need] @ T, Cw - K @ T[:, need]
            got_nis.append(d.correct_sparse_deferred(c, h, R, nu)[0])
    assert d.pending == 4 * ticks == 32
    ri, ci = [pos[int(v)] for v in rows], [pos[int(v)] for v in cl]
    every = np.arange(N)

    def sampled():
        return (_rel(np.vstack([d.sigma_block(rows[k:k + 6], every) for k in range(0, len(rows), 6)]), Rw[ri]),
                _rel(np.hstack([d.sigma_block(every, cl[k:k + 6]) for k in range(0, len(cl), 6)]), Cw[:, ci]))
    errs = sampled()                                                           # through 32 pending rows
    assert d.pending == 32
    d.flush()
    errs += sampled() + (_rel(d.state, xs), max(abs(a - b) / abs(b) for a, b in zip(got_nis, nis_want)))
    _note("full_size_carried_ticks", max(errs))
    assert max(errs) <= TIGHT, errs

    def run(carry):
        d.carry = carry
        parts = []
        for t in range(ticks):
            parts.append(d.propagate_block(0, *pred[t]))
            parts += [d.correct_sparse_deferred(c, h, R, nu)[1] for c, h, R, nu in corr[2 * t:2 * t + 2]]
        assert d.pending == (32 if carry else 4)
        parts.append(d.flush())
        run.parts[carry].append(parts)
        return sum(parts)
    run.parts = {True: [], False: []}
    t_per_tick = _median(lambda: run(False))
    t_carried = _median(lambda: run(True))
    t_per_tick2 = _median(lambda: run(False))
    pc, pt = (np.median(np.array(run.parts[k][2:]), axis=0) for k in (True, False))
    d.close()
    prop_c, prop_t = pc[0:-1:3], pt[0:-1:3]
    print(f"N = {N}, 8 ticks of propagate_block(0, 3) + 2 x (2, 5): per tick {t_per_tick:.4f} ms (again {t_per_tick2:.4f}), "
          f"carried {t_carried:.4f} ms: ratio {t_carried / t_per_tick:.3f}")
    print(f"  carried:  propagate_block {' '.join(f'{v * 1e3:.1f}' for v in prop_c)} us, corrections "
          f"{(pc[:-1].sum() - prop_c.sum()) / 16 * 1e3:.1f} us each, flush at p = 32 {pc[-1]:.4f} ms")
    print(f"  per tick: propagate_block (with the flush at p = 4 from the second on) {' '.join(f'{v * 1e3:.1f}' for v in prop_t)} "
          f"us, corrections {(pt[:-1].sum() - prop_t.sum()) / 16 * 1e3:.1f} us each, last flush at p = 4 {pt[-1]:.4f} ms")
    assert t_carried <= 0.7 * t_per_tick, (t_carried, t_per_tick)


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 carry worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
