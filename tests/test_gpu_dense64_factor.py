"""-m gpu: ekf_dense64_factor, ekf_dense64_get_factor and ekf_dense64_whiten (ekf_dense64_factor.hip) against
dense_factor_cases.  Sizes around the block side NB the library reports: Na in {1, 2, 3, NB - 1, NB, NB + 1, 2 NB + 1,
3 NB + 2}, each once with N = Na and once with N = Na + 5, live = Na and everything outside the corner poisoned with payload
NaNs.  1. the integer family bit for bit; 2. the stop rule; 3. the derived residual and logdet bounds on slam_like; 4. whiten;
5. pending rows; 6. the snapshot; 7. N = 10003 and the time against one propagation."""
import ctypes
import math

import numpy as np
import pytest

import dense_factor_cases as fc
import dense_init_cases as ic
from test_gpu_dense64_live import _poison
from test_gpu_dense64_sparse import _median

pytestmark = pytest.mark.gpu
_NB = []
_REF = {}     # (family, Na) -> arrays computed once, never changed
STATE_ERR = 5   # EKF_ERR_STATE


def _nb(hip):
    if not _NB:
        d = hip.DensePropagator64(3)
        info = d.factor_launch_info()
        d.close()
        assert info["threads"] >= 64 and info["block"] >= 16 and 128 % info["block"] == 0
        _NB.append(info["block"])
    return _NB[0]


def _integer(Na):
    if ("int", Na) not in _REF:
        C, L0 = fc.integer_factor(Na)
        rep, L = fc.np_factor(C)
        assert fc.same_bits(L, L0)
        for a in (C, L0):
            a.setflags(write=False)
        _REF["int", Na] = (C, L0, rep)
    return _REF["int", Na]


def _slam(Na):
    if ("slam", Na) not in _REF:
        A, given = fc.slam_like(Na), fc.slam_like_input(Na)
        for a in (A, given):
            a.setflags(write=False)
        _REF["slam", Na] = (A, given)
    return _REF["slam", Na]


def _handle(hip, corner, tail, x=None):
    """a handle of dimension Na + tail that holds `corner` in its live corner Na; with a tail everything else is poison"""
    Na = corner.shape[0]
    N = Na + tail
    x = np.arange(1.0, Na + 1.0) if x is None else x
    S, xs = _poison(N, Na, corner, x) if tail else (np.array(corner), np.array(x))
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = xs
    d.live = Na
    return d, S, xs


def _put(d, S, corner):
    """another corner into the same handle"""
    S = S.copy()
    Na = corner.shape[0]
    S[:Na, :Na] = corner
    d.set(Sigma=S)
    return S


def _report(d):
    rep = d.factor()
    assert rep.pop("ms") >= 0.0 and set(rep) == set(fc.REPORT_FIELDS)
    return rep


def _refused(hip, call):
    with pytest.raises(hip.EkfError) as e:
        call()
    return e.value.status


SIZE_IDS = ["1", "2", "3", "NB-1", "NB", "NB+1", "2NB+1", "3NB+2"]
CASES = [(k, tail) for k in range(len(SIZE_IDS)) for tail in (0, 5)]
CASE_IDS = [f"{SIZE_IDS[k]}-{'tail' if tail else 'full'}" for k, tail in CASES]


# ---- 1. the integer family ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_integer_factor_bit_for_bit(hip, k, tail):
    Na = fc.sizes(_nb(hip))[k]
    C, L0, want = _integer(Na)
    d, S, xs = _handle(hip, C, tail)
    assert _refused(hip, d.get_factor) == STATE_ERR and _refused(hip, lambda: d.whiten(np.ones(Na))) == STATE_ERR
    got = _report(d)
    L = d.get_factor()
    again = _report(d)
    L2 = d.get_factor()
    sigma, state = d.sigma, d.state
    d.close()
    print(f"Na={Na} tail={tail}: {got}")
    assert fc.same_bits(L, L0)                                  # -0.0 above the diagonal would differ in bits
    assert fc.same_report(got, want), (got, want)
    assert got["ok"] == 1 and fc.same_bits(got["logdet"], fc.host_logdet(np.diagonal(L0)))
    assert fc.same_report(again, got) and fc.same_bits(L2, L)
    assert fc.same_bits(sigma, S) and fc.same_bits(state, xs)


# ---- 2. the stop rule -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_stop_rule(hip, k, tail):
    NB = _nb(hip)
    Na = fc.sizes(NB)[k]
    C, L0, ok_rep = _integer(Na)
    d, S, _ = _handle(hip, C, tail)
    for p in fc.fail_columns(NB, Na):
        corners = [fc.integer_indefinite(Na, p, c)[0] for c in (0, 3)]
        if p >= 1:
            corners += [fc.nan_entry(Na, p, j)[0] for j in sorted({0, p // 2, p - 1})]
        for bad in corners:
            want = fc.np_factor(bad)[0]
            assert (want["ok"], want["fail_index"]) == (0, p)
            _put(d, S, bad)
            got = _report(d)
            assert fc.same_report(got, want), (p, got, want)
            assert got["Na"] == Na and math.isnan(got["logdet"])
            piv = np.diagonal(L0)[:p] ** 2                       # the columns before p are L0's
            if p:
                assert (got["min_pivot"], got["max_pivot"], got["min_pivot_i"]) == (piv.min(), piv.max(), int(np.argmin(piv)))
            assert _refused(hip, d.get_factor) == STATE_ERR
            assert _refused(hip, lambda: d.whiten(np.ones(Na))) == STATE_ERR
        _put(d, S, C)                                            # a definite corner afterwards
        assert fc.same_report(_report(d), ok_rep) and fc.same_bits(d.get_factor(), L0)
    d.close()


# ---- 3. the derived bounds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_slam_like_residual_and_logdet_bounds(hip, k, tail):
    Na = fc.sizes(_nb(hip))[k]
    A, given = _slam(Na)
    d, S, xs = _handle(hip, given, tail)                         # garbage above the diagonal
    rep = _report(d)
    L = d.get_factor()
    sigma = d.sigma
    d.close()
    assert rep["ok"] == 1 and rep["fail_index"] == -1 and fc.same_bits(sigma, S)
    assert np.array_equal(np.triu(L, 1), np.zeros((Na, Na))) and not np.signbit(np.triu(L, 1)).any()
    ratio = fc.factor_residual_ratio(A, L)
    piv = np.diagonal(L) ** 2
    err, bound = abs(rep["logdet"] - np.linalg.slogdet(A)[1]), fc.logdet_bound(A, L)
    print(f"Na={Na} tail={tail}: residual / bound {ratio:.3f}; logdet {rep['logdet']!r}, error {err:.2e} of {bound:.2e}")
    assert ratio <= 1.0
    assert fc.same_bits(rep["logdet"], fc.host_logdet(np.diagonal(L)))
    assert err <= bound
    assert rep["min_pivot"] > 0 and abs(rep["min_pivot"] - piv.min()) <= 4 * fc.U * piv.min()     # sqrt, then squared
    assert abs(rep["max_pivot"] - piv.max()) <= 4 * fc.U * piv.max()


# ---- 4. whiten ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_whiten_integer_family(hip, k, tail):
    Na = fc.sizes(_nb(hip))[k]
    C, L0, _ = _integer(Na)
    d, _, _ = _handle(hip, C, tail)
    assert _report(d)["ok"] == 1
    for nrhs in (1, 3, 64):
        Z = np.random.default_rng(100 * Na + nrhs).integers(-3, 4, size=(nrhs, Na)).astype(np.float64)
        got = d.whiten(Z @ L0.T)
        assert fc.same_bits(got["Y"], Z) and fc.same_bits(got["d2"], (Z * Z).sum(axis=1)), nrhs
        only = d.whiten(Z @ L0.T, want_Y=False)
        assert only["Y"] is None and fc.same_bits(only["d2"], got["d2"])
    d.close()


@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_whiten_slam_like_bounds_and_position(hip, k, tail):
    Na = fc.sizes(_nb(hip))[k]
    A, given = _slam(Na)
    d, _, _ = _handle(hip, given, tail)
    assert _report(d)["ok"] == 1
    L = d.get_factor()
    B = np.random.default_rng(7 + Na).standard_normal((64, Na))
    got = d.whiten(B)
    worst_sub = max(fc.whiten_residual_ratio(L, got["Y"][r], B[r]) for r in range(0, 64, 7))
    worst_norm = max(fc.norm_ratio(got["Y"][r], got["d2"][r]) for r in range(64))
    alone = d.whiten(B[17])
    moved = B.copy()
    moved[[0, 63, 40]] = B[17]
    there = d.whiten(moved)
    d.close()
    print(f"Na={Na} tail={tail}: substitution residual / bound {worst_sub:.3f}, norm {worst_norm:.3f}")
    assert worst_sub <= 1.0 and worst_norm <= 1.0
    assert fc.same_bits(alone["Y"][0], got["Y"][17]) and fc.same_bits(alone["d2"][0], got["d2"][17])
    for r in (0, 63, 40):
        assert fc.same_bits(there["Y"][r], got["Y"][17]) and fc.same_bits(there["d2"][r], got["d2"][17])
    expect = np.linalg.solve(A, B[17]) @ B[17]
    assert abs(alone["d2"][0] - expect) <= 1e-6 * expect


def test_map_nees_is_whiten_on_the_wrapped_difference(hip):
    steps = ic.discovery_scenario()
    n = len(steps)
    f = hip.DenseEKFSLAM(n)
    for dth, dx, readings in steps:
        f.prediction(dth, dx)
        f.data_association(readings)
    rep = f.factor()
    assert rep["ok"] == 1 and rep["Na"] == 3 + 2 * n
    state = f.state
    truth = state + np.random.default_rng(4).normal(0.0, 0.05, size=state.shape)
    truth[0] = state[0] - 3.5                                    # a heading difference beyond pi: it has to be wrapped
    e = state - truth
    e[0] = hip.normalize_angles(e[:1])[0]
    assert abs(e[0] - (3.5 - 2 * math.pi)) < 1e-12
    nees = f.map_nees(truth)
    want = f.handle.whiten(e)["d2"][0]
    Sigma = f.handle.sigma
    f.close()
    Sl = np.tril(Sigma) + np.tril(Sigma, -1).T
    model = e @ np.linalg.solve(Sl, e)
    print(f"map NEES {nees!r} over {3 + 2 * n} states; numpy on the lower triangle {model!r}; logdet {rep['logdet']!r}")
    assert fc.same_bits(nees, want) and abs(nees - model) <= 1e-6 * model
    assert abs(rep["logdet"] - np.linalg.slogdet(Sl)[1]) <= 1e-6


# ---- 5. pending rows ------------------------------------------------------------------------------------------------------

def _two_deferred(d, Na):
    rng = np.random.default_rng(17)
    for j in (1, Na // 2 - 3):
        cols = np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j])
        d.correct_sparse_deferred(cols, rng.standard_normal((2, 5)), 0.5 * np.eye(2), 0.1 * rng.standard_normal(2))


@pytest.mark.parametrize("carry", [False, True])
def test_pending_rows_are_flushed_first(hip, carry):
    Na = _nb(hip) + 1
    A = _slam(Na)[0]
    d, _, _ = _handle(hip, A, 5, x=np.linspace(-1.0, 1.0, Na))
    twin, _, _ = _handle(hip, A, 5, x=np.linspace(-1.0, 1.0, Na))
    for h in (d, twin):
        h.carry = carry
        _two_deferred(h, Na)
        assert h.pending == 4
    twin.flush()
    assert twin.pending == 0 and d.pending == 4
    assert hip.load().ekf_dense64_factor(d._h, None, None) == 1 and d.pending == 4      # a refused call does not flush
    assert hip.load().ekf_dense64_factor(None, ctypes.byref(hip.FactorReport()), None) == 1
    got, want = _report(d), _report(twin)
    assert d.pending == 0
    same = (fc.same_report(got, want) and fc.same_bits(d.get_factor(), twin.get_factor())
            and fc.same_bits(d.sigma, twin.sigma) and fc.same_bits(d.state, twin.state))
    first = _report(_handle(hip, A, 5)[0])
    d.close(); twin.close()
    assert same and got["ok"] == 1 and not fc.same_bits(got["logdet"], first["logdet"])   # the corrections count


def test_refusals(hip):
    Na = 5
    d, _, _ = _handle(hip, _integer(Na)[0], 0)
    lib, buf = hip.load(), np.full(64 * Na, 7.0)
    a, b = ctypes.c_int(), ctypes.c_int()
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.ekf_dense64_factor_launch_info(d._h, None, ctypes.byref(b)) == 1
    assert lib.ekf_dense64_factor_launch_info(d._h, ctypes.byref(a), None) == 1
    assert lib.ekf_dense64_get_factor(d._h, None) == 1
    assert _report(d)["ok"] == 1
    assert lib.ekf_dense64_whiten(d._h, 1, None, p, p, None) == 1
    assert lib.ekf_dense64_whiten(d._h, 0, p, p, p, None) == 1 and lib.ekf_dense64_whiten(d._h, 65, p, p, p, None) == 1
    assert lib.ekf_dense64_whiten(d._h, 1, p, None, None, None) == 1
    assert np.array_equal(buf, np.full(64 * Na, 7.0))
    d.close()


# ---- 6. the snapshot ------------------------------------------------------------------------------------------------------

def test_the_factor_is_a_snapshot(hip):
    NB = _nb(hip)
    Na = 2 * NB + 1
    A = _slam(Na)[0]
    d, _, _ = _handle(hip, A, 5, x=np.linspace(-1.0, 1.0, Na))
    assert _report(d)["ok"] == 1
    L1 = d.get_factor()
    y1 = d.whiten(np.ones(Na))
    rng = np.random.default_rng(3)
    d.correct_sparse(np.array([0, 1, 2, 3 + 2 * 7, 4 + 2 * 7]), rng.standard_normal((2, 5)), 0.5 * np.eye(2), np.zeros(2))
    assert fc.same_bits(d.get_factor(), L1)                      # the old factor, whatever happened to Sigma
    y1b = d.whiten(np.ones(Na))
    assert fc.same_bits(y1b["Y"], y1["Y"]) and fc.same_bits(y1b["d2"], y1["d2"])
    S2 = d.sigma[:Na, :Na]
    assert _report(d)["ok"] == 1
    L2 = d.get_factor()
    assert not fc.same_bits(L2, L1) and fc.factor_residual_ratio(np.tril(S2) + np.tril(S2, -1).T, L2) <= 1.0
    d.live = Na - 2
    assert _refused(hip, lambda: d.whiten(np.ones(Na - 2))) == STATE_ERR
    assert fc.same_bits(d.get_factor(), L2)                      # still the snapshot taken at Na
    rep = _report(d)                                             # a factor at the new live dimension
    assert rep["ok"] == 1 and rep["Na"] == Na - 2 and d.get_factor().shape == (Na - 2, Na - 2)
    assert d.whiten(np.ones(Na - 2))["d2"][0] > 0.0
    d.close()


# ---- 7. full size ---------------------------------------------------------------------------------------------------------

def test_full_size_n10003_and_time(hip):
    """N = 10003, Sigma = A A^T / 64 + I with A of shape N x 64, exactly symmetric, eigenvalues >= 1.  ok == 1; 32 sampled
    rows of L L^T against Sigma within the componentwise bound; logdet against slogdet(I_64 + A^T A / 64) (the matrix
    determinant lemma) within the logdet bound with ||Sigma^-1||_2 <= 1; then the time condition: the median HIP-event
    time of factor < 2 x that of one ekf_dense64_propagate on the same handle (the propagation has twelve times the flops;
    the margin is for the factor's chain of dependent launches).  The measured figures are in DESIGN.md."""
    N = 10003
    NB = _nb(hip)
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    S = np.tril(S) + np.tril(S, -1).T
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    rep = d.factor()
    assert rep["ok"] == 1 and rep["Na"] == N and rep["min_pivot"] >= 1.0 - 1e-9
    L = d.get_factor()
    assert fc.same_bits(rep["logdet"], fc.host_logdet(np.diagonal(L)))
    rows = sorted({0, 1, NB - 1, NB, NB + 1, N - 1, N - 2, N - NB} | set(int(i) for i in rng.integers(0, N, size=24)))[:32]
    g = np.longdouble(fc.gamma(N + 1))
    worst = 0.0
    for i in rows:
        li = L[i, :i + 1].astype(np.longdouble)
        for lo in range(0, i + 1, 2048):
            blk = L[lo:min(i + 1, lo + 2048), :i + 1].astype(np.longdouble)
            res = np.abs(S[i, lo:lo + blk.shape[0]].astype(np.longdouble) - blk @ li)
            worst = max(worst, float(np.max(res / (g * (np.abs(blk) @ np.abs(li))))))
    want = np.linalg.slogdet(np.eye(64) + A.T @ A / 64)[1]
    np.abs(L, out=L)
    v = np.ones(N) / math.sqrt(N)
    for _ in range(40):                                          # || |L| |L|^T ||_2 = || |L| ||_2^2, from below
        v = L.T @ (L @ v)
        norm2, v = float(np.linalg.norm(v)), v / np.linalg.norm(v)
    del L
    bound = 2.0 * N * fc.gamma(N + 1) * norm2 * 1.0
    err = abs(rep["logdet"] - want)
    t_factor = _median(lambda: d.factor()["ms"])
    B = rng.standard_normal((64, N))
    t_w1 = _median(lambda: d.whiten(B[0], want_Y=False)["ms"])
    t_w64 = _median(lambda: d.whiten(B, want_Y=False)["ms"])
    t_prop = _median(lambda: d.propagate())
    d.close()
    print(f"N={N} NB={NB}: residual / bound {worst:.3f}; logdet {rep['logdet']!r} against {want!r}: {err:.2e} of {bound:.2e}; "
          f"factor {t_factor:.3f} ms, propagate {t_prop:.3f} ms, ratio {t_factor / t_prop:.3f}; "
          f"whiten nrhs=1 {t_w1:.3f} ms, nrhs=64 {t_w64:.3f} ms")
    assert worst <= 1.0
    assert err <= bound
    assert t_factor < 2.0 * t_prop, (t_factor, t_prop)
