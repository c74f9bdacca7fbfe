"""-m gpu: ekf_dense64_health and ekf_dense64_symmetrize (ekf_dense64_health.hip) against the op-by-op numpy models of
dense_health_cases, bit for bit.  Sizes around the tile side T the library reports: Na in {1, 2, 3, T - 1, T, T + 1,
2 T + 1, 3 T + 2}, each once with N = Na and once with N = Na + 5, live = Na and everything outside the corner poisoned
with payload NaNs.  1. the report; 2. the symmetrisation; 3. health is read-only; 4. pending rows; 5. refusals; 6. a filter's
life with and without the symmetrisation; 7. N = 10003 and the time against a flush of two pending rows."""
import ctypes

import numpy as np
import pytest

import dense_health_cases as hc
import dense_init_cases as ic
from parity import FP64_TOL, worst
from test_gpu_dense64_live import _poison
from test_gpu_dense64_sparse import _full_size_sigma, _median

pytestmark = pytest.mark.gpu
_REF = {}     # (family, Na) -> (corner, report, symmetrised corner, changed, max_asym): computed once, never changed
_TILE = []


def _tile(hip):
    if not _TILE:
        d = hip.DensePropagator64(3)
        info = d.health_launch_info()
        d.close()
        assert info["threads"] == 256 and info["tile"] >= 4
        _TILE.append(info["tile"])
    return _TILE[0]


def _reference(family, Na):
    if (family, Na) not in _REF:
        C = hc.corner(family, Na)
        out, changed, most = hc.np_symmetrize(C, Na)
        for a in (C, out):
            a.setflags(write=False)
        _REF[family, Na] = (C, hc.np_health(C, Na), out, changed, most)
    return _REF[family, Na]


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


def _report(d):
    rep = d.health()
    assert rep.pop("ms") >= 0.0 and set(rep) == set(hc.REPORT_FIELDS)
    return rep


# the sizes are cut from the tile side at run time: index k of hc.sizes(T)
SIZE_IDS = ["1", "2", "3", "T-1", "T", "T+1", "2T+1", "3T+2"]
CASES = [(f, k, tail) for f in hc.FAMILIES for k in range(len(SIZE_IDS)) for tail in (0, 5)]
CASE_IDS = [f"{f}-{SIZE_IDS[k]}-{'tail' if tail else 'full'}" for f, k, tail in CASES]


# ---- 1. the report ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,k,tail", CASES, ids=CASE_IDS)
def test_health_report_bit_for_bit(hip, family, k, tail):
    Na = hc.sizes(_tile(hip))[k]
    C, want = _reference(family, Na)[:2]
    d, S, xs = _handle(hip, C, tail)
    got = _report(d)
    again = _report(d)
    d.close()
    print(f"{family} Na={Na} tail={tail}: {got}")
    assert hc.same_report(got, want), (got, want)
    assert hc.same_report(again, got)


# ---- 2. the symmetrisation --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,k,tail", CASES, ids=CASE_IDS)
def test_symmetrize_bit_for_bit(hip, family, k, tail):
    Na = hc.sizes(_tile(hip))[k]
    C, rep, out, changed, most = _reference(family, Na)
    d, S, xs = _handle(hip, C, tail)
    want = S.copy()
    want[:Na, :Na] = out
    got = d.symmetrize()
    sigma = d.sigma
    after = _report(d)
    second = d.symmetrize()
    sigma2 = d.sigma
    state = d.state
    d.close()
    print(f"{family} Na={Na} tail={tail}: changed {got['changed']} max_asym {got['max_asym']!r}")
    assert got["changed"] == changed == rep["n_asym"] and hc.same_bits(got["max_asym"], most)
    assert hc.same_bits(sigma, want)                       # the whole N x N matrix: tail and diagonal untouched
    assert after["n_asym"] == 0
    if family != "degenerate":
        assert hc.same_bits(after["max_asym"], 0.0)        # (a NaN pair of the degenerate family keeps d a NaN)
    assert hc.same_report(after, hc.np_health(want, Na))
    assert second["changed"] == 0 and hc.same_bits(sigma2, sigma)
    assert hc.same_bits(state, xs)


def test_ties_take_the_lowest_location(hip):
    """three pairs that differ by the same 2.0, +0.0 and -0.0 on the diagonal, one NaN there; Na = 1 and an all-NaN diagonal"""
    S = np.array([[0.0, 1.0, 5.0, 2.0], [3.0, -0.0, 4.0, 8.0], [3.0, 4.0, 2.0, 1.0], [2.0, 6.0, 1.0, np.nan]])
    for C in (S, np.array([[np.nan]]), np.array([[np.nan, 1.0], [1.0, np.nan]])):
        d, _, _ = _handle(hip, C, 5)
        got = _report(d)
        d.close()
        assert hc.same_report(got, hc.np_health(C, C.shape[0])), got
    assert (got["min_diag"], got["min_diag_i"]) == (np.inf, -1)


# ---- 3. read-only -----------------------------------------------------------------------------------------------------------

def test_health_is_read_only(hip):
    T = _tile(hip)
    Na = 2 * T + 1
    C = _reference("random_spd", Na)[0]
    d, S, xs = _handle(hip, C, 5, x=np.linspace(-1.0, 1.0, Na))
    cols = np.array([[0, 1, 2, 3 + 2 * j, 4 + 2 * j] for j in range(8)])
    rng = np.random.default_rng(3)
    Hc, R, nu = rng.standard_normal((8, 2, 5)), 0.1 * np.eye(2), rng.standard_normal((8, 2))
    before = d.score_sparse(cols, Hc, R, nu, want_S=True)[:3]
    _report(d)
    assert hc.same_bits(d.sigma, S) and hc.same_bits(d.state, xs)
    after = d.score_sparse(cols, Hc, R, nu, want_S=True)[:3]
    d.close()
    assert hc.same_bits(after[0], before[0]) and hc.same_bits(after[1], before[1]) and np.array_equal(after[2], before[2])


# ---- 4. pending rows --------------------------------------------------------------------------------------------------------

def _two_deferred(d, Na):
    rng = np.random.default_rng(17)
    for j in (1, Na // 2 - 3):
        cols = np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j])
        d.correct_sparse_deferred(cols, rng.standard_normal((2, 5)), 0.5 * np.eye(2), 0.1 * rng.standard_normal(2))


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("call", ["health", "symmetrize"])
def test_pending_rows_are_flushed_first(hip, call, carry):
    T = _tile(hip)
    Na = T + 1
    C = _reference("random_spd", Na)[0]
    d, _, _ = _handle(hip, C, 5, x=np.linspace(-1.0, 1.0, Na))
    twin, _, _ = _handle(hip, C, 5, x=np.linspace(-1.0, 1.0, Na))
    for h in (d, twin):
        h.carry = carry
        _two_deferred(h, Na)
        assert h.pending == 4
    twin.flush()
    assert twin.pending == 0 and d.pending == 4
    if call == "health":
        got, want = _report(d), _report(twin)
        assert hc.same_report(got, want) and got["n_asym"] > 0
    else:
        got, want = d.symmetrize(), twin.symmetrize()
        assert got["changed"] == want["changed"] > 0 and hc.same_bits(got["max_asym"], want["max_asym"])
    assert d.pending == 0
    same = hc.same_bits(d.sigma, twin.sigma) and hc.same_bits(d.state, twin.state)
    d.close(); twin.close()
    assert same


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(hip):
    T = _tile(hip)
    Na = T + 1
    C = _reference("random_spd", Na)[0]
    d, _, _ = _handle(hip, C, 5, x=np.linspace(-1.0, 1.0, Na))
    _two_deferred(d, Na)
    lib = hip.load()
    rep, n, most = hip.HealthReport(), ctypes.c_longlong(7), ctypes.c_double(7.0)
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.ekf_dense64_health(None, ctypes.byref(rep), None) == 1
    assert lib.ekf_dense64_health(d._h, None, None) == 1
    assert d.pending == 4                                                      # the refused call did not flush
    assert lib.ekf_dense64_symmetrize(None, ctypes.byref(n), ctypes.byref(most), None) == 1
    assert (n.value, most.value) == (7, 7.0) and d.pending == 4
    assert lib.ekf_dense64_health_launch_info(None, ctypes.byref(a), ctypes.byref(b)) == 1
    assert lib.ekf_dense64_health_launch_info(d._h, None, ctypes.byref(b)) == 1
    assert lib.ekf_dense64_health_launch_info(d._h, ctypes.byref(a), None) == 1
    assert lib.ekf_dense64_symmetrize(d._h, None, None, None) == 0             # every output is nullable
    assert d.pending == 0
    d.close()


# ---- 6. in a filter's life --------------------------------------------------------------------------------------------------

def test_a_filters_life_with_and_without_symmetrisation(hip):
    """the discovery scenario of dense_init_cases (20 ticks, 20 landmarks; the scenario the landmark front end and the
    duplicate search are tested on) through DenseEKFSLAM on two handles, one symmetrised after every tick: the same
    association decisions, state and Sigma within FP64_TOL, and the handle that never symmetrised reports the drift and
    nothing worse"""
    steps = ic.discovery_scenario()
    n = len(steps)
    plain, kept = hip.DenseEKFSLAM(n), hip.DenseEKFSLAM(n)
    written = 0
    for t, (dth, dx, readings) in enumerate(steps):
        picks = []
        for f in (plain, kept):
            f.prediction(dth, dx)
            picks.append(list(f.data_association(readings)))
        assert picks[0] == picks[1] and plain.known == kept.known, (t, picks)
        written += kept.symmetrize()["changed"]
    rep, rep_kept = plain.health(), kept.health()
    w, e = worst(kept.handle.state, kept.handle.sigma, plain.handle.state, plain.handle.sigma)
    plain.close(); kept.close()
    print(f"life: n_asym {rep['n_asym']} max_asym {rep['max_asym']:.3e}; pairs written over the run {written}; "
          f"symmetrised against plain {w:.3e}")
    assert plain.known == n and w <= FP64_TOL, e
    assert rep["n_asym"] > 0 and rep["n_minor"] == rep["n_diag_bad"] == rep["n_nonfinite"] == 0, rep
    assert rep_kept["n_asym"] == 0 and rep_kept["max_asym"] == 0.0 and written > 0


# ---- 7. full size -----------------------------------------------------------------------------------------------------------

def test_full_size_n10003_and_time(hip):
    """N = 10003: a symmetric Sigma (the _full_size_sigma of the sparse test, its two halves averaged on the host) with
    64 planted asymmetric entries, so the report is known without the model's pair arrays; then the time condition:
    symmetrize and health each take <= 3 x the HIP-event time of ekf_dense64_flush of two pending rows, measured here on the
    same handle (medians, _median).  The flush rewrites the same 16 N^2 bytes; the factor allows for half the traffic going
    through an LDS transpose and catches a column-strided walk, which costs far more.  symmetrize is timed twice: on the
    symmetric matrix (the read alone) and on _full_size_sigma as it comes, where every pair has to be written.
    Measured on an MI355X: profiles/r23/dense64_health_bench.txt."""
    N = 10003
    T = _tile(hip)
    rng = np.random.default_rng(8)
    raw = _full_size_sigma(N, rng)
    S = 0.5 * (raw + raw.T)
    dg = np.diagonal(S).copy()
    off = S.copy()
    np.fill_diagonal(off, 0.0)
    assert max(off.max(), -off.min()) ** 2 < dg.min() ** 2                     # no minor can be negative
    del off
    tiles = (N + T - 1) // T
    spots = {(0, 1), (0, N - 1), (N - 2, N - 1), (T - 1, T), (T, T + 1), (T * (tiles - 1) - 1, T * (tiles - 1)),
             (5, T * (tiles - 1) + 2), (3333, 7777)}
    while len(spots) < 64:
        i, j = sorted(rng.integers(0, N, size=2))
        if i != j:
            spots.add((int(i), int(j)))
    spots = sorted(spots)
    big = [spots[20], spots[40]]                                               # the same largest difference twice
    for i, j in spots:
        if (i, j) in big:
            S[i, j], S[j, i] = 0.75, 0.25                                      # d = 0.5 exactly
        else:
            S[i, j] = S[j, i] + 1e-9 * (1 + i % 7)
        if (i + j) % 2:
            S[i, j], S[j, i] = S[j, i], S[i, j]                                # on either side of the diagonal
    diffs = {p: abs(S[p] - S[p[1], p[0]]) for p in spots}
    assert min(diffs.values()) > 0.0 and sorted(p for p in spots if diffs[p] == 0.5) == big and max(diffs.values()) == 0.5
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    rep = d.health()
    assert (rep["n_asym"], rep["n_nonfinite"], rep["n_diag_bad"], rep["n_minor"]) == (64, 0, 0, 0), rep
    assert hc.same_bits(rep["max_asym"], 0.5) and (rep["asym_i"], rep["asym_j"]) == big[0]
    assert hc.same_bits(rep["min_diag"], dg.min()) and rep["min_diag_i"] == int(np.argmin(dg))
    t_health = _median(lambda: d.health()["ms"])
    got = d.symmetrize()
    assert got["changed"] == 64 and hc.same_bits(got["max_asym"], 0.5)
    rows = np.array(sorted({p[0] for p in spots} | {p[1] for p in spots}))

    def sampled(src):
        """the rows x rows entries of the handle against those of src symmetrised"""
        E = src[np.ix_(rows, rows)]
        E = np.where(hc.bits(E) != hc.bits(E.T.copy()), 0.5 * (E + E.T), E)
        return all(hc.same_bits(d.sigma_block(rows[lo:lo + 32], rows), E[lo:lo + 32]) for lo in range(0, len(rows), 32))

    assert sampled(S)
    after = d.health()
    assert after["n_asym"] == 0 and after["max_asym"] == 0.0
    t_sym_clean = _median(lambda: d.symmetrize()["ms"])                        # nothing to write: the read alone
    assert d.symmetrize()["changed"] == 0 and sampled(S)
    cols, Hc, R, nu = np.array([0, 1, 2, 3 + 2 * 3333, 4 + 2 * 3333]), rng.standard_normal((2, 5)), np.eye(2), np.zeros(2)

    def flush_two():
        d.correct_sparse_deferred(cols, Hc, R, nu)
        assert d.pending == 2
        return d.flush()

    t_flush = _median(flush_two)

    def symmetrize_all():
        d.set(Sigma=raw)
        got = d.symmetrize()
        assert got["changed"] > 0.99 * (N * (N - 1) // 2)
        return got["ms"]

    t_sym = _median(symmetrize_all, iters=5, warmup=1)
    assert sampled(raw)
    d.close()
    tb = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12
    print(f"N={N}: flush(2 rows) {t_flush:.4f} ms; health {t_health:.4f} ms ({tb(8 * N * N, t_health):.2f} TB/s on 8 N^2); "
          f"symmetrize {t_sym:.4f} ms ({tb(16 * N * N, t_sym):.2f} TB/s on 16 N^2), nothing to write {t_sym_clean:.4f} ms")
    assert t_health <= 3.0 * t_flush, (t_health, t_flush)
    assert t_sym <= 3.0 * t_flush and t_sym_clean <= 3.0 * t_flush, (t_sym, t_sym_clean, t_flush)
