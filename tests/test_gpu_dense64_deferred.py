"""-m gpu: the deferred sparse correction of the fp64 dense handle (ekf_dense64_correct_sparse_deferred, ekf_dense64_flush,
ekf_dense64_pending, ekf_dense64_sparse.hip): K and T of a correction wait in pending rows, score_sparse and further
deferred corrections read through them, Sigma is rewritten once per flush.  Integer chains bit-exact against numpy's eager
sequence (tests/test_dense64_deferred_host.py proves them exact in float64); the capacity of 64 rows; random operands
against the eager sequence through correct_sparse on a twin handle within 1e-12 per block; the bit-level properties of the
fixed order; every other call flushes; nothing touched on failure; the reference's data_association() live with every
correction deferred; N = 10003 with the time condition T_deferred <= 0.5 T_eager.

Seen on the MI355X so far: the integer chains, the capacity cases, the bit-level properties and the
flush of every other call pass; against the eager sequence state, Sigma, every nis and the full-map scores with 16 rows
pending differ by 0 (the matrix cores accumulate fp64 in ascending k through the same fused multiply-add, so the flush's
order is the fold's order there; the contract promises rounding only).  The failure cases, the refused-call case, the
reference live and the N = 10003 case with its time condition have not been run on a GPU yet."""
import numpy as np
import pytest

import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst
from test_gpu_dense64_sparse import TIGHT, _full_size_sigma, _general_case, _median, _random_sigma, _rel, _same_bits

pytestmark = pytest.mark.gpu
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


def _handle(hip, Sigma, x):
    N = len(x)
    d = hip.DensePropagator64(N)
    d.set(F=np.eye(N), Sigma=Sigma, Q=np.zeros((N, N)))
    d.state = x
    return d


def _score_exact(d, c, what):
    nis, S, flags, _ = d.score_sparse(c["cols"], c["Hc"], c["R"], c["nu"], want_S=True)
    assert np.array_equal(S, c["S"]) and np.array_equal(nis, c["nis"]) and not flags.any(), what


def _run_chain_exact(hip, chain, what):
    """every step deferred; after every call the state, the scores of the next candidates on Sigma_cur and the count"""
    d = _handle(hip, chain["Sigma0"], chain["x0"])
    steps = chain["steps"]
    _score_exact(d, steps[0], what)                                  # nothing pending: the launch of the sparse call
    rows = 0
    for i, st in enumerate(steps):
        if rows + st["m"] > dd.MAX_ROWS:
            rows = 0                                                 # the call flushes first
        nis, _ = d.correct_sparse_deferred(st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0])
        rows += st["m"]
        assert nis == st["nis0"] and np.array_equal(d.state, st["state"]), (what, i)
        assert d.pending == rows, (what, i, d.pending, rows)
        _score_exact(d, steps[i + 1] if i + 1 < len(steps) else chain["after"], (what, i))
    return d, rows


# ---- 1. exact integers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", dd.CHAIN_N)
def test_deferred_integer_chains_exact(hip, N):
    """pins the fold of the row strips against the column strips (Sigma is unsymmetric), the wave and the workgroup form of
    the scoring kernel with rows pending, the strips at the padding edge, every order of the list; the identity propagation
    after each chain would show anything written into the padding"""
    for order in dd.ORDERS:
        chain = dd.integer_chain(N, order)
        what = f"N={N} {order} {[(s['m'], s['s']) for s in chain['steps']]}"
        d, rows = _run_chain_exact(hip, chain, what)
        assert rows == sum(s["m"] for s in chain["steps"])
        assert d.flush() > 0.0 and d.pending == 0
        want = chain["steps"][-1]["Sigma"]
        got = d.sigma
        bad = got != want
        assert not bad.any(), f"{what}: {bad.sum()} wrong elements, first at {np.argwhere(bad)[0]}"
        d.propagate(1)                                               # I Sigma I^T + 0: exact unless the padding is not zero
        assert np.array_equal(d.sigma, want) and np.array_equal(d.state, chain["steps"][-1]["state"]), what
        assert d.flush() == 0.0                                      # nothing pending: a no-op
        d.close()


# ---- 2. capacity -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [65, 200])
@pytest.mark.parametrize("name", ["pairs", "big", "odd", "full"])
def test_deferred_capacity(hip, N, name):
    """pairs / big fill the store to exactly 64 rows and the next call (m = 1) flushes first; odd stops at 63 and a call of
    m = 2 flushes first; full is m = 64 on an empty store.  Sigma in memory cannot be read without a flush, so what is
    checked is every state, score and count on the way and Sigma at the end, exactly."""
    chain = dd.capacity_chain(N, name)
    d = _handle(hip, chain["Sigma0"], chain["x0"])
    rows, seen = 0, []
    for i, st in enumerate(chain["steps"]):
        if rows + st["m"] > dd.MAX_ROWS:
            rows = 0
        nis, _ = d.correct_sparse_deferred(st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0])
        rows += st["m"]
        seen.append(d.pending)
        assert nis == st["nis0"] and np.array_equal(d.state, st["state"]) and d.pending == rows, (name, i)
    assert seen[-2] == {"pairs": 64, "big": 64, "odd": 63, "full": 64}[name] and seen[-1] == chain["steps"][-1]["m"]
    _score_exact(d, chain["after"], name)
    assert np.array_equal(d.sigma, chain["steps"][-1]["Sigma"]) and d.pending == 0
    d.propagate(1)
    assert np.array_equal(d.sigma, chain["steps"][-1]["Sigma"])
    d.close()


# ---- 3. against the eager sequence ---------------------------------------------------------------------------------------------

def _random_chain(N, shapes, rng):
    """(2, 5): the reference's five columns, a landmark never twice (a second correction of one landmark takes 100 - 99.99
    and would measure that cancellation, not the code); other shapes: _general_case"""
    fresh = iter(rng.choice((N - 3) // 2, size=len(shapes), replace=False))
    out = []
    for m, s in shapes:
        if (m, s) == (2, 5):
            i = int(next(fresh))
            out.append((sp.slam_cols(i), rng.normal(size=(2, 5)), 0.01 * np.eye(2) + 1e-3 * rng.normal(size=(2, 2)),
                        0.1 * rng.normal(size=2)))
        else:
            c, h, R, nu = _general_case(N, m, s, rng)
            out.append((c, h, R, 0.1 * nu))
    return out


@pytest.mark.parametrize("N", [203, 1003])
@pytest.mark.parametrize("name", ["v8", "v32", "mixed"])
def test_deferred_against_eager_sequence(hip, N, name):
    """the same chain through correct_sparse on a twin handle; deferred with one flush at the end and with a flush every 4:
    state, Sigma and every nis within 1e-12 per block; score_sparse of the full map with 16 rows pending against the
    twin's"""
    rng = np.random.default_rng(31 * N + len(name))
    Sigma, x = _random_sigma(N, rng), np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-2.0, 2.0, size=N - 3)])
    shapes = {"v8": [(2, 5)] * 8, "v32": [(2, 5)] * 32, "mixed": [(2, 5), (8, 16), (2, 5), (2, 5), (8, 16), (2, 5)]}[name]
    chain = _random_chain(N, shapes, rng)
    fc, fH, fR, fnu = sp.candidate_terms(x, 0.7, -0.4)
    eager = _handle(hip, Sigma, x)
    for every in (0, 4):
        eager.set(Sigma=Sigma)
        eager.state = x
        d = _handle(hip, Sigma, x)
        rows = 0
        for i, (c, h, R, nu) in enumerate(chain):
            want, _ = eager.correct_sparse(c, h, R, nu)
            got, _ = d.correct_sparse_deferred(c, h, R, nu)
            rows += len(h)
            assert d.pending == rows
            _note("vs_eager_nis", abs(got - want) / abs(want))
            assert abs(got - want) <= TIGHT * abs(want), (i, got, want)
            if d.pending == 16 and every == 0:
                a, _, fa, _ = d.score_sparse(fc, fH, fR, fnu)
                b, _, fb, _ = eager.score_sparse(fc, fH, fR, fnu)
                assert not fa.any() and not fb.any()
                e = float((np.abs(a - b) / np.abs(b)).max())
                _note("vs_eager_full_map_scores_16_pending", e)
                assert e <= TIGHT, e
            if every and (i + 1) % every == 0:
                d.flush()
                rows = 0
        d.flush()
        w, e = worst(d.state, d.sigma, eager.state, eager.sigma)
        _note(f"vs_eager_state_cov_flush_{'end' if not every else 'every4'}", w)
        assert w <= TIGHT, e
        d.close()
    eager.close()


# ---- 4. bits ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,m,s", [(403, 2, 5), (403, 16, 16), (403, 17, 5)])
def test_deferred_same_operands_same_bits(hip, N, m, s):
    rng = np.random.default_rng(19 * N + 3 * m + s)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    chain = _random_chain(N, [(2, 5), (m, s), (2, 5)], rng)
    terms = [_general_case(N, m, s, rng) for _ in range(7)]
    cols, Hc, R, nu = (np.stack([t[k] for t in terms]) for k in range(4))
    runs = []
    for _ in range(2):
        d = _handle(hip, Sigma, x)
        log = []
        for c, h, r, v in chain:
            log.append(d.correct_sparse_deferred(c, h, r, v)[0])
        nis, S, flags, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)      # 2 + m + 2 rows pending
        assert not flags.any() and d.pending == 4 + m
        for j in (0, 3, 6):                                                    # alone
            a, b, _, _ = d.score_sparse(cols[j:j + 1], Hc[j:j + 1], R[j:j + 1], nu[j:j + 1], want_S=True)
            assert _same_bits(a[0], nis[j]) and _same_bits(b[0], S[j]), j
        perm = rng.permutation(7)                                              # at any position of a batch of 7
        a, b, _, _ = d.score_sparse(cols[perm], Hc[perm], R[perm], nu[perm], want_S=True)
        assert _same_bits(a, nis[perm]) and _same_bits(b, S[perm])
        cn, _ = d.correct_sparse_deferred(cols[3], Hc[3], R[3], nu[3])         # the score, then the deferred correction
        assert _same_bits(cn, nis[3])
        log += [cn, nis, S, d.state]
        d.flush()
        log.append(d.sigma)
        runs.append(log)
        d.close()
    for a, b in zip(*runs):                                                    # two runs: the same bits everywhere
        assert _same_bits(a, b)
    # nothing pending: one deferred correction and the flush are correct_sparse bit for bit
    c, h, r, v = chain[1]
    d, e = _handle(hip, Sigma, x), _handle(hip, Sigma, x)
    n_def, _ = d.correct_sparse_deferred(c, h, r, v)
    assert d.pending == m
    d.flush()
    n_eag, _ = e.correct_sparse(c, h, r, v)
    assert _same_bits(n_def, n_eag) and _same_bits(d.state, e.state) and _same_bits(d.sigma, e.sigma)
    d.close()
    e.close()


# ---- 5. every other call flushes ---------------------------------------------------------------------------------------------

def _other_calls(N, rng):
    F = np.eye(N) + 0.01 * rng.normal(size=(N, N))
    Q = 1e-4 * np.eye(N)
    H = 0.1 * rng.normal(size=(2, N))
    c, h, R, nu = _general_case(N, 2, 5, rng)
    G = rng.normal(size=(2, 3))
    rows, cols = rng.integers(0, N, size=9), rng.integers(0, N, size=7)
    Fr = np.eye(3) + 0.01 * F[:3, :3]
    return F, Q, {                                                   # each -> the arrays the call returns (times left out)
        "propagate": lambda d: (d.propagate(1), ())[1],
        "propagate_block": lambda d: (d.propagate_block(0, Fr, 1e-6 * np.eye(3), np.ones(3)), ())[1],
        "correct": lambda d: d.correct(H, 0.01 * np.eye(2), np.array([0.1, -0.2]))[:1],
        "score": lambda d: d.score(H[None], 0.01 * np.eye(2), np.array([[0.1, -0.2]]), want_S=True)[:3],
        "correct_sparse": lambda d: d.correct_sparse(c, h, R, nu)[:1],
        "init_block": lambda d: (d.init_block(N - 2, G=G, cols=[0, 1, 2], W=np.eye(2), xb=np.ones(2)), ())[1],
        "sigma": lambda d: (d.sigma,),
        "sigma_block": lambda d: (d.sigma_block(rows, cols),),
    }


@pytest.mark.parametrize("call", ["propagate", "propagate_block", "correct", "score", "correct_sparse", "init_block",
                                  "sigma", "sigma_block"])
def test_every_other_call_flushes(hip, call):
    """two deferred corrections and then the call, against the same two, an explicit flush, and the call: the same bits"""
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
        for c, h, R, nu in chain:
            d.correct_sparse_deferred(c, h, R, nu)
        assert d.pending == 10
        if explicit:
            assert d.flush() > 0.0
        res = calls[call](d)
        assert d.pending == 0
        out.append(tuple(res) + (d.state, d.sigma))
        d.close()
    assert len(out[0]) == len(out[1]) >= 2
    for u, v in zip(*out):
        assert _same_bits(u, v)


def test_set_drops_or_keeps_and_a_refused_call_changes_nothing(hip):
    N = 203
    rng = np.random.default_rng(78)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    chain = _random_chain(N, [(2, 5), (2, 5)], rng)
    other = rng.normal(size=(N, N))
    d = _handle(hip, Sigma, x)
    for c, h, R, nu in chain:
        d.correct_sparse_deferred(c, h, R, nu)
    d.set(Sigma=other)                                               # the pending rows belonged to the old covariance
    assert d.pending == 0 and _same_bits(d.sigma, other)
    d.set(Sigma=Sigma)
    d.state = x
    for c, h, R, nu in chain:
        d.correct_sparse_deferred(c, h, R, nu)
    d.set(F=np.eye(N))                                               # F alone: they stay
    assert d.pending == 4
    import ctypes
    lib, dp, ip = hip.load(), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    bad = np.array([0, 1, 2, 7, N], dtype=np.int32)
    Hc, R, nu = np.ones((2, 5)), np.eye(2), np.ones(2)
    for f in (lib.ekf_dense64_correct_sparse, lib.ekf_dense64_correct_sparse_deferred):
        assert f(d._h, 2, 5, bad.ctypes.data_as(ip), Hc.ctypes.data_as(dp), R.ctypes.data_as(dp), nu.ctypes.data_as(dp),
                 None, None) == 1
    assert lib.ekf_dense64_get_sigma_block(d._h, 5, bad.ctypes.data_as(ip), 1, bad.ctypes.data_as(ip),
                                           Hc.ctypes.data_as(dp)) == 1
    assert lib.ekf_dense64_propagate_block(d._h, N, 3, Hc.ctypes.data_as(dp), None, None, None) == 1
    assert d.pending == 4
    e = _handle(hip, Sigma, x)
    for c, h, R, nu in chain:
        e.correct_sparse_deferred(c, h, R, nu)
    assert _same_bits(d.state, e.state) and _same_bits(d.sigma, e.sigma)
    d.close()
    e.close()


# ---- 6. failure -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("why", ["equal_rows", "nan"])
def test_deferred_singular_S_leaves_everything(hip, why):
    """the error path of test_correct_sparse_singular_S_leaves_everything, with rows pending"""
    N, m, s = 203, 2, 5
    rng = np.random.default_rng(29)
    Sigma, x = _random_sigma(N, rng), rng.normal(size=N)
    chain = _random_chain(N, [(2, 5), (8, 16), (2, 5)], rng)
    cols = sp.index_list(N, s, "scattered", rng)
    Hc = np.tile(rng.integers(1, 4, size=(1, s)).astype(np.float64), (m, 1))
    R = np.zeros((m, m))      # equal rows of Hc: the rows of T' and all four entries of S are the same bits, pending or not
    if why == "nan":
        Hc, R = rng.normal(size=(m, s)), 0.01 * np.eye(m)
        R[1, 0] = np.nan
    out = []
    for with_failure in (False, True):
        d = _handle(hip, Sigma, x)
        for c, h, r, v in chain[:2]:
            d.correct_sparse_deferred(c, h, r, v)
        if with_failure:
            before = d.state
            with pytest.raises(hip.EkfError) as e:
                d.correct_sparse_deferred(cols, Hc, R, np.array([0.3, -0.1]))
            assert e.value.status == 5                               # EKF_ERR_STATE
            assert d.pending == 10 and _same_bits(d.state, before)
        c, h, r, v = chain[2]
        nis, _ = d.correct_sparse_deferred(c, h, r, v)
        assert d.pending == 12
        d.flush()
        out.append((nis, d.state, d.sigma))
        d.close()
    for a, b in zip(*out):
        assert _same_bits(a, b)


# ---- 7. the reference, live ----------------------------------------------------------------------------------------------------

class _Deferring:
    """the handle with correct_sparse forwarded to correct_sparse_deferred, everything else unchanged"""

    def __init__(self, d):
        self._d = d

    def __getattr__(self, name):
        return getattr(self._d, name)

    def correct_sparse(self, cols, Hc, R, nu=None):
        return self._d.correct_sparse_deferred(cols, Hc, R, nu)


@pytest.mark.parametrize("n", [20, 200])
def test_deferred_against_the_reference_data_association(hip, oracle, n):
    """test_init_against_the_reference_data_association ('state_only') with every correction deferred: the readings of a
    tick are scored through the pending corrections of the same tick, the next propagate_block flushes"""
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
    known, scores, most = 0, [], 0
    for t, (dth, dx, readings) in enumerate(steps):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        known = ic.association_step(_Deferring(d), n, known, dth, dx, readings, "state_only", scores)
        most = max(most, d.pending)
        assert known == int(known_ref.sum()) and known_ref[:known].all(), (t, known, known_ref)
    assert known == min(n, len(steps)) and most >= 4
    for k, nis in enumerate(scores):
        assert ds.margins_hold(nis), f"scored reading {k}: the scenario's seed must be replaced"
    P = 3 + 2 * known
    gs, gS, rs, rS = d.state, d.sigma, ref.state, ref.cov
    d.close()
    w, e = worst(gs[:P], gS[:P, :P], rs[:P], rS[:P, :P])
    _note(f"reference_live_deferred_n{n}", w)
    assert w <= FP64_TOL, e
    assert np.array_equal(gS[P:, P:], rS[P:, P:]) and np.array_equal(gs[P:], rs[P:])


# ---- 8. full size and time -------------------------------------------------------------------------------------------------------

def test_deferred_full_size_n10003_and_time(hip):
    """a deferred tick of V = 8 corrections of (2, 5) at N = 10003: sampled rows and columns through sigma_block against
    numpy on the gathered data; then HIP-event medians of 9 after 2 on one handle (Sigma as the last tick left it, as in
    test_sparse_full_size_n10003_and_time: the times do not depend on the values, and an upload of 800 MB per repetition
    would be most of the test): T_eager = 8 correct_sparse(2, 5), T_deferred = 8 deferred calls + the flush.  The condition, derived in the
    issue and not from a measurement (eight 16 N^2 streams against one at rank 16 plus eight launch-bound triples: about
    3 x predicted): T_deferred <= 0.5 T_eager."""
    N, V = 10003, 8
    rng = np.random.default_rng(8)
    Sigma = _full_size_sigma(N, rng)
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    d = hip.DensePropagator64(N)
    d.set(Sigma=Sigma)
    d.state = x
    picks = [int(i) for i in rng.choice(5000, size=V, replace=False)]
    tick = [(sp.slam_cols(i), rng.normal(size=(2, 5)), 0.01 * np.eye(2), 0.1 * rng.normal(size=2)) for i in picks]
    last = (N - 1) // 128 * 128
    rows = np.array(sorted(set([0, 1, 2, N - 1] + [3 + 2 * i for i in picks] + list(range(last, N, 5)) +
                               list(rng.integers(0, N, size=12)))))
    cc = np.array(sorted(set([0, 1, 2, N - 1, N - 2] + [4 + 2 * i for i in picks] + list(rng.integers(0, N, size=10)))))
    # numpy on the gathered data: the sequence needs the rows and columns listed by the tick and the sampled ones
    need = np.array(sorted(set(rows) | set(cc) | set(int(v) for c, _, _, _ in tick for v in c)))
    pos = {int(v): k for k, v in enumerate(need)}
    Rw, Cw, xs = Sigma[need, :].copy(), Sigma[:, need].copy(), x.copy()       # rows / columns of Sigma_cur that matter
    nis_want = []
    for c, h, R, nu in tick:
        idx = [pos[int(v)] for v in c]
        T, U = h @ Rw[idx, :], Cw[:, idx] @ h.T
        Si = np.linalg.inv(T[:, c] @ h.T + R)
        K = U @ Si
        nis_want.append(float(nu @ Si @ nu))
        xs = xs + K @ nu
        Rw, Cw = Rw - K[need] @ T, Cw - K @ T[:, need]
    got_nis = [d.correct_sparse_deferred(c, h, R, nu)[0] for c, h, R, nu in tick]
    assert d.pending == 2 * V
    d.flush()
    ri, ci = [pos[int(v)] for v in rows], [pos[int(v)] for v in cc]
    every = np.arange(N)
    errs = (_rel(np.vstack([d.sigma_block(rows[k:k + 6], every) for k in range(0, len(rows), 6)]), Rw[ri]),
            _rel(np.hstack([d.sigma_block(every, cc[k:k + 6]) for k in range(0, len(cc), 6)]), Cw[:, ci]),
            _rel(d.state, xs), max(abs(a - b) / abs(b) for a, b in zip(got_nis, nis_want)))
    _note("full_size_deferred_tick", max(errs))
    assert max(errs) <= TIGHT, errs
    def eager():
        return sum(d.correct_sparse(c, h, R, nu)[1] for c, h, R, nu in tick)

    def deferred():
        parts = [d.correct_sparse_deferred(c, h, R, nu)[1] for c, h, R, nu in tick] + [d.flush()]
        deferred.parts.append(parts)
        return sum(parts)
    deferred.parts = []
    t_eager = _median(eager)
    t_def = _median(deferred)
    t_eager2 = _median(eager)
    parts = np.median(np.array(deferred.parts[2:]), axis=0)
    d.close()
    print(f"N = {N}, V = {V} x (2, 5): eager {t_eager:.4f} ms (again {t_eager2:.4f}), deferred {t_def:.4f} ms "
          f"(calls {' '.join(f'{v * 1e3:.1f}' for v in parts[:-1])} us, flush at p = {2 * V} {parts[-1]:.4f} ms): "
          f"ratio {t_def / t_eager:.3f}")
    assert t_def <= 0.5 * t_eager, (t_def, t_eager)


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 deferred worst {k}: {WORST[k]:.3e}")
    assert all(v <= FP64_TOL for v in WORST.values())
