"""-m gpu: ekf_dense64_map_congruence and ekf_dense64_reframe_landmarks (ekf_dense64_frame.hip) against the models of
dense_frame_cases.  Sizes around both tile sides the library reports: Na = the odd numbers nearest {3, 5, 7, T - 1, T, T + 1,
2 T + 1, 3 T + 2}, each once with N = Na and once with N = Na + 5, live = Na and everything outside the corner poisoned with
payload NaNs.  1. the congruence on the integer families, bit for bit; 2. on floats against the componentwise bound; 3. no
symmetrisation, and the identity keeps every bit; 4. FIXED; 5. ROBOT; 6. pending rows and refusals; 7. DenseEKFSLAM end to
end; 8. N = 10003 and the time."""
import ctypes
import math

import numpy as np
import pytest

import dense_frame_cases as fr
import dense_model_cases as dm
from parity import FP64_TOL, worst
from test_gpu_dense64_live import _poison
from test_gpu_dense64_sparse import _full_size_sigma, _median

pytestmark = pytest.mark.gpu
_TILES, _REF, _RATIOS = [], {}, {}
N_SIZES = len(fr.sizes(64, 128))   # the number of distinct sizes does not depend on the tile sides as long as they differ


def _tiles(hip):
    if not _TILES:
        d = hip.DensePropagator64(3)
        info = d.frame_launch_info()
        d.close()
        assert info["threads"] == 256 and info["tile_rows"] % 2 == 0 and info["tile_cols"] % 2 == 0
        _TILES.extend([info["tile_rows"], info["tile_cols"]])
    return _TILES


def _size(hip, k):
    s = fr.sizes(*_tiles(hip))
    assert len(s) == N_SIZES
    return s[k]


def _handle(hip, corner, tail, x=None):
    """a handle of dimension Na + tail that holds `corner` in its live corner; with a tail everything else is poison"""
    Na = corner.shape[0]
    x = np.arange(1.0, Na + 1.0) if x is None else x
    S, xs = _poison(Na + tail, Na, corner, x) if tail else (np.array(corner), np.array(x, dtype=np.float64))
    d = hip.DensePropagator64(Na + tail)
    d.set(Sigma=S)
    d.state = xs
    d.live = Na
    return d, S, xs


def _expect(S, Na, corner):
    want = S.copy()
    want[:Na, :Na] = corner
    return want


def _note(key, text):
    """the figures of this run; the full-size test prints them together (profiles/r26/dense64_frame_bench.txt is that output)"""
    _RATIOS[key] = text


CASES = [(k, tail) for k in range(N_SIZES) for tail in (0, 5)]
CASE_IDS = [f"size{k}-{'tail' if tail else 'full'}" for k, tail in CASES]


# ---- 1. integer families ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_congruence_integer_families_bit_for_bit(hip, k, tail):
    Na = _size(hip, k)
    corner, C = fr.integer_corner(Na), fr.integer_C(Na)
    for family, G in sorted(fr.GS.items()):
        for Cm in (None, C):
            d, S, xs = _handle(hip, corner, tail)
            d.map_congruence(G, Cm)
            got, state = d.sigma, d.state
            d.close()
            want = _expect(S, Na, fr.exact_congruence(corner, G, Cm))
            what = f"{family} Na={Na} tail={tail} C={'yes' if Cm is not None else 'no'}"
            assert fr.same_bits(got[:Na, :Na], want[:Na, :Na]), what
            assert fr.same_bits(got, want), what + ": the poison moved"
            assert fr.same_bits(state, xs), what + ": the state was touched"


# ---- 2. floats --------------------------------------------------------------------------------------------------------------

def _float_case(Na):
    if Na not in _REF:
        S = fr.slam_like(Na)
        G = fr.fixed_terms(0.7)
        C = np.random.default_rng(7000 + Na).standard_normal((Na, 3))
        for a in (S, G, C):
            a.setflags(write=False)
        _REF[Na] = (S, G, C)
    return _REF[Na]


@pytest.mark.parametrize("k", range(N_SIZES))
def test_congruence_floats_within_the_componentwise_bound(hip, k):
    """|Sigma' - J Sigma J^T|_ij <= gamma_16 (|J| |Sigma| |J|^T)_ij against long double; the same bits from N = Na and from
    N = Na + 5 and from two runs; at Na <= 7 the op-by-op model bit for bit."""
    Na = _size(hip, k)
    corner, G, C = _float_case(Na)
    outs = []
    for tail in (0, 5, 5):
        d, S, xs = _handle(hip, corner, tail)
        d.map_congruence(G, C)
        got = d.sigma
        d.close()
        assert fr.same_bits(got, _expect(S, Na, got[:Na, :Na]))
        outs.append(got[:Na, :Na].copy())
    ratio = fr.bound_ratio(outs[0], corner, G, C)
    d, _, _ = _handle(hip, corner, 5)
    d.map_congruence(G, None)
    ratio_d = fr.bound_ratio(d.sigma[:Na, :Na], corner, G, None)
    d.close()
    print(f"Na={Na}: error / bound {ratio:.4f} with C, {ratio_d:.4f} without")
    _note(("bound", Na), f"Na={Na}: max |err| / (gamma_16 |J||S||J|^T) = {ratio:.4f} with C, {ratio_d:.4f} with C = NULL")
    assert fr.same_bits(outs[0], outs[1]) and fr.same_bits(outs[1], outs[2])
    assert ratio <= 1.0 and ratio_d <= 1.0
    if Na <= 7:
        assert fr.same_bits(outs[0], fr.np_congruence(corner, G, C))


# ---- 3. no symmetrisation ---------------------------------------------------------------------------------------------------

def test_an_antisymmetric_part_comes_out_as_its_own_congruence(hip):
    Tr, Tc = _tiles(hip)
    Na = fr.odd_near(Tc + 1)
    rng = np.random.default_rng(11)
    sym = fr.integer_corner(Na)
    sym = np.triu(sym) + np.triu(sym, 1).T
    K = np.triu(rng.integers(1, 64, size=(Na, Na)).astype(np.float64), 1)
    K = K - K.T
    G, C = fr.GS["shear"], fr.integer_C(Na)
    outs = []
    for corner in (sym, sym + K):
        d, _, _ = _handle(hip, corner, 5)
        d.map_congruence(G, C)
        outs.append(d.sigma[:Na, :Na].copy())
        d.close()
    diff = outs[1] - outs[0]                                  # integers: exact
    want = fr.exact_congruence(K, G, C)
    assert fr.same_bits(diff + 0.0, want + 0.0) and np.array_equal(want, -want.T) and np.any(want != 0)


@pytest.mark.parametrize("tail", [0, 5])
def test_identity_keeps_every_bit(hip, tail):
    Tr, Tc = _tiles(hip)
    Na = fr.odd_near(Tc + 1)
    corner = fr.slam_like(Na)
    corner[2, 3], corner[Na - 1, 4], corner[0, 0] = -0.0, -0.0, -0.0
    for t, (i, j) in enumerate([(0, 5), (4, 4), (Na - 1, Na - 2), (Tr + 2, 1), (7, Tc)]):
        corner[i, j] = fr.payload_nan(t)
    d, S, xs = _handle(hip, corner, tail)
    d.map_congruence(np.eye(2), None)
    got, state = d.sigma, d.state
    d.close()
    assert fr.same_bits(got, S) and fr.same_bits(state, xs)


# ---- 4. FIXED ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_reframe_fixed(hip, k, tail):
    Na = _size(hip, k)
    corner, x = fr.slam_like(Na), fr.slam_state(Na)
    dth, tx, ty = 0.7, 3.0, -2.0
    d, S, xs = _handle(hip, corner, tail, x)
    twin, _, _ = _handle(hip, corner, tail, x)
    G, C, _ = d.reframe(fr.FIXED, dth, tx, ty, want_terms=True)
    twin.map_congruence(G, None)
    got, state, tw = d.sigma, d.state, twin.sigma
    d.close(); twin.close()
    assert C is None and fr.same_bits(G, [[math.cos(dth), -math.sin(dth)], [math.sin(dth), math.cos(dth)]])
    assert fr.same_bits(got, tw)                              # the poison included
    err = np.abs(state[:Na].astype(np.longdouble) - fr.g_fixed(x, dth, tx, ty, np.longdouble))
    assert np.all(err <= fr.fixed_state_bound(x, dth, tx, ty)), float(np.max(err))
    assert fr.same_bits(state[Na:], xs[Na:])


def test_reframe_fixed_by_nothing_leaves_every_bit(hip):
    Tr, Tc = _tiles(hip)
    Na = fr.odd_near(Tc + 1)
    d, S, xs = _handle(hip, fr.slam_like(Na), 5, fr.slam_state(Na))
    d.reframe(fr.FIXED, 0.0, 0.0, 0.0)
    got, state = d.sigma, d.state
    d.close()
    assert fr.same_bits(got, S) and fr.same_bits(state, xs)


# ---- 5. ROBOT ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tail", CASES, ids=CASE_IDS)
def test_reframe_robot(hip, k, tail):
    Na = _size(hip, k)
    corner, x = fr.slam_like(Na), fr.slam_state(Na)
    d, S, xs = _handle(hip, corner, tail, x)
    twin, _, _ = _handle(hip, corner, tail, x)
    G, C, _ = d.reframe(fr.ROBOT, want_terms=True)
    twin.map_congruence(G, C)
    got, state, tw = d.sigma, d.state, twin.sigma
    assert fr.same_bits(got, tw)
    wG, wC = fr.robot_terms(x)
    eG, eC = fr.row_scale_err(G, wG), fr.row_scale_err(C, wC)
    assert eG <= 1e-12 and eC <= 1e-12, (eG, eC)
    assert fr.row_scale_err(state[:Na][None, :], fr.g_robot(x)[None, :]) <= 1e-12 and fr.same_bits(state[Na:], xs[Na:])
    d.reframe(fr.ROBOT)
    back, xback = d.sigma, d.state
    d.close(); twin.close()
    w, e = worst(xback[:Na], back[:Na, :Na], x, corner)
    print(f"Na={Na} tail={tail}: ROBOT twice against the start {w:.3e}")
    _note(("twice", Na, tail), f"Na={Na} tail={tail}: ROBOT twice, worst |d| / sqrt(S_ii S_jj) = {w:.3e}")
    assert w <= FP64_TOL, e
    assert fr.same_bits(back, _expect(S, Na, back[:Na, :Na])) and fr.same_bits(xback[Na:], xs[Na:])


# ---- 6. pending rows, refusals ------------------------------------------------------------------------------------------------

def _two_deferred(d, Na):
    rng = np.random.default_rng(17)
    for j in (1, Na // 2 - 3):
        cols = np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j])
        d.correct_sparse_deferred(cols, rng.standard_normal((2, 5)), 0.5 * np.eye(2), 0.1 * rng.standard_normal(2))


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("call", ["congruence", "fixed", "robot"])
def test_pending_rows_are_flushed_first(hip, call, carry):
    Tr, Tc = _tiles(hip)
    Na = fr.odd_near(Tr + 1)
    corner, x = fr.slam_like(Na), fr.slam_state(Na)
    d, _, _ = _handle(hip, corner, 5, x)
    twin, _, _ = _handle(hip, corner, 5, x)
    for h in (d, twin):
        h.carry = carry
        _two_deferred(h, Na)
        assert h.pending == 4
    twin.flush()
    assert twin.pending == 0 and d.pending == 4
    C = np.random.default_rng(3).standard_normal((Na, 3))
    for h in (d, twin):
        if call == "congruence":
            h.map_congruence(fr.GS["shear"], C)
        else:
            h.reframe(fr.FIXED if call == "fixed" else fr.ROBOT, 0.3, 1.0, 2.0)
    assert d.pending == 0
    same = fr.same_bits(d.sigma, twin.sigma) and fr.same_bits(d.state, twin.state)
    d.close(); twin.close()
    assert same


def test_refusals_change_nothing(hip):
    Tr, Tc = _tiles(hip)
    Na = fr.odd_near(Tr + 1)
    d, S, xs = _handle(hip, fr.slam_like(Na), 5, fr.slam_state(Na))
    twin, _, _ = _handle(hip, fr.slam_like(Na), 5, fr.slam_state(Na))
    _two_deferred(d, Na)
    _two_deferred(twin, Na)
    lib = hip.load()
    G, terms = np.eye(2), np.full(4 + 3 * Na, 7.0)
    assert lib.ekf_dense64_map_congruence(d._h, None, None, None) == 1                      # NULL G
    assert lib.ekf_dense64_reframe_landmarks(d._h, 7, 0.0, 0.0, 0.0, hip._d(terms), None) == 1   # mode 7
    assert lib.ekf_dense64_reframe_landmarks(d._h, 0, math.inf, 0.0, 0.0, hip._d(terms), None) == 1
    assert np.array_equal(terms, np.full(4 + 3 * Na, 7.0)) and d.pending == 4
    with pytest.raises(ValueError):
        d.reframe(fr.ROBOT, want_terms=np.empty(3 + 3 * Na))                                # terms too short: the wrapper
    with pytest.raises(ValueError):
        d.map_congruence(G, np.zeros((Na - 1, 3)))
    with pytest.raises(hip.EkfError):
        d.reframe(7)
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ekf_dense64_frame_launch_info(d._h, None, ctypes.byref(b), ctypes.byref(c)) == 1
    assert d.pending == 4
    same = fr.same_bits(d.sigma, twin.sigma) and fr.same_bits(d.state, twin.state)          # (reading Sigma flushes both)
    d.close(); twin.close()
    assert same


def test_refusals_leave_the_pending_rows(hip):
    """Na even on a handle that was never shrunk: the rows stay pending and Sigma_cur is what it was"""
    Na = 12
    corner = fr.slam_like(13)[:Na, :Na]
    d, S, xs = _handle(hip, corner, 5, np.linspace(-1.0, 1.0, Na))
    _two_deferred(d, Na)
    for call in (lambda: d.map_congruence(fr.GS["rot90"]), lambda: d.reframe(fr.FIXED, 0.1, 0.0, 0.0), lambda: d.reframe(fr.ROBOT)):
        with pytest.raises(hip.EkfError):
            call()
        assert d.pending == 4
    d.close()


# ---- 7. DenseEKFSLAM end to end -----------------------------------------------------------------------------------------------

def test_slam_filter_reframes_and_returns(hip):
    """20 ticks of dense_model_cases' discovery scenario on a filter with room for two landmarks it never sees (so the frame
    change runs below the live dimension, behind the coupling guard); reframe(0.7, 3, -2): the NEES of the whole map against
    the transformed truth equals the one before to 1e-9 relative; robot_frame() twice and five more ticks stay within 1e-9
    of the filter that never left its frame, with identical decisions"""
    steps = dm.discovery_scenario(n=6, ticks=25)
    f, plain = hip.DenseEKFSLAM(8), hip.DenseEKFSLAM(8)
    for dth, dx, readings in steps[:20]:
        for h in (f, plain):
            h.prediction(dth, dx)
            h.data_association(readings)
    assert f.known == plain.known >= 3 and f.handle.live == 19 > 3 + 2 * f.known
    live = f.handle.live
    x = f.handle.state_block(0, live)
    sd = np.sqrt(np.diagonal(f.handle.sigma)[:live])
    truth = x + 0.5 * sd * np.random.default_rng(4).standard_normal(live)
    assert f.factor()["ok"] == 1
    nees = f.map_nees(truth)
    f.reframe(0.7, 3.0, -2.0)
    assert f.handle.live == live
    W = 3 + 2 * f.known
    truth2 = truth.copy()
    truth2[:W] = fr.g_fixed(truth[:W], 0.7, 3.0, -2.0)
    assert f.factor()["ok"] == 1
    nees2 = f.map_nees(truth2)
    print(f"map NEES {nees:.12g} before, {nees2:.12g} after reframe")
    _note(("nees",), f"DenseEKFSLAM: map NEES {nees:.12g} before, {nees2:.12g} after reframe(0.7, 3, -2)")
    assert abs(nees2 - nees) <= 1e-9 * nees
    f.reframe(-0.7, *(-(fr.fixed_terms(-0.7) @ np.array([3.0, -2.0]))))                     # and back
    f.robot_frame()
    f.robot_frame()
    for dth, dx, readings in steps[20:]:
        picks = []
        for h in (f, plain):
            h.prediction(dth, dx)
            picks.append(list(h.data_association(readings)))
        assert picks[0] == picks[1]
    w, e = worst(f.handle.state, f.handle.sigma, plain.handle.state, plain.handle.sigma)
    f.close(); plain.close()
    print(f"there and back and five more ticks against the filter that stayed: {w:.3e}")
    _note(("life",), f"DenseEKFSLAM: reframe there and back, robot_frame twice, five ticks: {w:.3e} against the filter that stayed")
    assert w <= FP64_TOL, e


def test_coupling_guard_raises_on_a_coupled_tail(hip):
    f = hip.DenseEKFSLAM(4)
    S = fr.slam_like(11)
    f.handle.set(Sigma=S)
    for call in (lambda: f.reframe(0.1, 1.0, 1.0), f.robot_frame):
        with pytest.raises(ValueError):
            call()
    same = fr.same_bits(f.handle.sigma, S) and f.handle.live == 11
    f.close()
    assert same


# ---- 8. full size -----------------------------------------------------------------------------------------------------------

def test_full_size_n10003_and_time(hip):
    """N = 10003 on _full_size_sigma: HIP-event medians of 9 after 2 for reframe(ROBOT), map_congruence(C = None),
    symmetrize with every pair to write and correct_sparse(2, 5), on one handle in one process.  Asserted: reframe <= 2 x
    correct_sparse (both move 16 N^2 bytes; the margin the Joseph and the factor tests give such a call).  The goal, not
    asserted, is parity with symmetrize.  32 sampled rows are held to the componentwise bound.  Measured on an MI355X:
    profiles/r26/dense64_frame_bench.txt."""
    N = 10003
    rng = np.random.default_rng(8)
    raw = _full_size_sigma(N, rng)
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-7.0, 7.0, size=N - 3)])
    d = hip.DensePropagator64(N)
    d.set(Sigma=raw)
    d.state = x
    Tr, Tc = _tiles(hip)
    rows = np.array(sorted({0, 1, 2, 3, 4, Tr + 2, Tr + 3, Tc + 2, Tc + 3, N - 2, N - 1} |
                           {int(v) for v in rng.integers(3, N, size=40)})[:32])
    G, C, _ = d.reframe(fr.ROBOT, want_terms=True)
    assert fr.row_scale_err(C, fr.robot_terms(x)[1]) <= 1e-12
    # the sampled rows of J S J^T and of |J| |S| |J|^T in extended precision, without an N x N Jacobian
    every = np.arange(N)
    got = np.vstack([d.sigma_block(rows[lo:lo + 4], every) for lo in range(0, 32, 4)])
    Jr = fr.jacobian_rows(N, rows, G, C, np.longdouble)
    nz = np.unique(np.nonzero(Jr)[1])
    Sx = raw[nz].astype(np.longdouble)
    want = fr.times_jacobian_T(Jr[:, nz] @ Sx, G, C, False)
    bound = np.longdouble(fr.gamma(16)) * fr.times_jacobian_T(np.abs(Jr[:, nz]) @ np.abs(Sx), G, C, True)
    ratio = float(np.max(np.abs(got.astype(np.longdouble) - want) / bound))
    assert ratio <= 1.0, ratio

    t_reframe = _median(lambda: d.reframe(fr.ROBOT))
    t_cong = _median(lambda: d.map_congruence(fr.fixed_terms(0.7)))
    cols, Hc, R, nu = np.array([0, 1, 2, 3 + 2 * 3333, 4 + 2 * 3333]), rng.standard_normal((2, 5)), np.eye(2), np.zeros(2)
    d.set(Sigma=raw)
    t_corr = _median(lambda: d.correct_sparse(cols, Hc, R, nu)[-1])

    def symmetrize_all():
        d.set(Sigma=raw)
        out = d.symmetrize()
        assert out["changed"] > 0.99 * (N * (N - 1) // 2)
        return out["ms"]

    t_sym = _median(symmetrize_all, iters=5, warmup=1)
    d.close()
    tb = lambda ms: 16.0 * N * N / (ms * 1e-3) / 1e12
    lines = [f"N={N}: reframe(ROBOT) {t_reframe:.4f} ms ({tb(t_reframe):.2f} TB/s on 16 N^2); map_congruence(C=NULL) "
             f"{t_cong:.4f} ms ({tb(t_cong):.2f} TB/s); symmetrize, every pair written {t_sym:.4f} ms ({tb(t_sym):.2f} TB/s); "
             f"correct_sparse(2, 5) {t_corr:.4f} ms ({tb(t_corr):.2f} TB/s)",
             f"N={N}: reframe / correct_sparse = {t_reframe / t_corr:.3f} (asserted <= 2), reframe / symmetrize = "
             f"{t_reframe / t_sym:.3f}; 32 sampled rows: max |err| / bound = {ratio:.4f}"]
    lines += [_RATIOS[k] for k in sorted(_RATIOS, key=str)]
    print("\n".join(lines))
    assert t_reframe <= 2.0 * t_corr, (t_reframe, t_corr)
