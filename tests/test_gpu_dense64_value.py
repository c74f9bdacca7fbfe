"""-m gpu: ekf_dense64_value_operands and ekf_dense64_rank_landmarks (ekf_dense64_value.hip) against the models of
dense_value_cases.  Sizes around the tile the library reports (vc.sizes), each once with N = Na and once with N = Na + 6,
live = Na and everything outside the corner poisoned with payload NaNs.  1. the integer family, exact; 2. the float families
against the numpy model, bit for bit; 3. S and flag are score_sparse's, Hc is score_landmarks'; 4. a landmark's bits do not
depend on the batch, the run or the capacity; 5. the figures are the drops of an actual correction; 6. read-only, pending
rows, an open region; 7. flags, ties, gating; 8. refusals.  live = one and two tile_rows exactly (one spare state behind the
last landmark) rides with 2."""
import numpy as np
import pytest

import dense_init_cases as ic
import dense_value_cases as vc
from test_gpu_dense64_live import _poison

pytestmark = pytest.mark.gpu
LD = np.longdouble
_INFO, _REF = [], {}   # the launch geometry; (family, n_lm) -> (C, Hc, R, model): computed once, never changed
OUT = ("dtrace", "dtrace_pose", "detS", "S")
TAILS = (0, 6)


def _info(hip):
    if not _INFO:
        d = hip.DensePropagator64(5)
        _INFO.append(d.value_launch_info())
        d.close()
        assert _INFO[0]["tile_rows"] >= 4 and _INFO[0]["tile_lm"] >= 2 and _INFO[0]["threads"] % 64 == 0
    return _INFO[0]


def _sizes(hip):
    return vc.sizes(_info(hip)["tile_rows"], _info(hip)["tile_lm"])


def _reference(hip, family, n_lm):
    if (family, n_lm) not in _REF:
        C, Hc, R = vc.integer_family(n_lm) if family == "int" else vc.float_family(n_lm, 0, family)
        model = (vc.exact_value(C, 3 + 2 * n_lm, 0, Hc, R) if family == "int"
                 else vc.np_value(C, 3 + 2 * n_lm, 0, Hc, R, _info(hip)["tile_rows"]))
        for a in (C, Hc, R):
            a.setflags(write=False)
        _REF[family, n_lm] = (C, Hc, R, model)
    return _REF[family, n_lm]


def _handle(hip, corner, tail=0, x=None):
    """a handle of dimension Na + tail that holds `corner` in its live corner Na; with a tail everything else is poison"""
    Na = corner.shape[0]
    N = Na + tail
    x = np.arange(1.0, Na + 1.0) if x is None else x
    S, xs = _poison(N, Na, corner, x) if tail else (np.array(corner), np.array(x))
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = xs
    d.live = Na
    return d


def _same(got, want, keys=OUT):
    for k in keys:
        assert vc.same_bits(getattr(got, k), want[k] if isinstance(want, dict) else getattr(want, k)), k


def _no_poison(r):
    for k in OUT:   # a payload NaN of the tail would show as a NaN here: every figure of these families is finite
        assert np.isfinite(getattr(r, k)).all(), k


SIZE_IDS = list(range(9))   # index into vc.sizes(...), cut from the tile at run time: nine sizes while tile_lm = tile_rows


def _cases(hip, k):
    s = _sizes(hip)
    assert len(s) == len(SIZE_IDS), "the tile changed: SIZE_IDS must follow"
    return s[k]


# ---- 1. exact integers --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("k", SIZE_IDS)
def test_integer_family_is_exact(hip, k, tail):
    n_lm = _cases(hip, k)
    C, Hc, R, ex = _reference(hip, "int", n_lm)
    assert ex["exact"] and not ex["flags"].any()
    d = _handle(hip, C, tail)
    r = d.value_operands(Hc, R)
    d.close()
    _no_poison(r)
    _same(r, ex)
    assert not r.flags.any()
    for j in range(n_lm):   # tr(adj(S) G), an integer: G itself through the outputs
        assert r.dtrace[j] * r.detS[j] == ex["dtrace_det"][j]
    want = vc.winners(dict(trace=ex["dtrace"], pose=ex["dtrace_pose"], det=ex["detS"]), ex["flags"], np.ones(n_lm))
    assert {k_: r.best[k_] for k_ in want} == want


# ---- 2. against numpy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("family", vc.FLOAT_KINDS)
@pytest.mark.parametrize("k", SIZE_IDS)
def test_float_families_bit_for_bit(hip, k, family, tail):
    n_lm = _cases(hip, k)
    C, Hc, R, want = _reference(hip, family, n_lm)
    d = _handle(hip, C, tail)
    r = d.value_operands(Hc, R)
    d.close()
    for key in OUT:
        a, b = getattr(r, key), want[key]
        print(f"{family} n_lm={n_lm} tail={tail} {key}: max |device - numpy| {np.abs(a - b).max():.3g}")
    _no_poison(r)
    _same(r, want)
    assert np.array_equal(r.flags, want["flags"]) and {k_: r.best[k_] for k_ in want["best"]} == want["best"]


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("rows", (1, 2))
def test_a_last_row_tile_that_is_exactly_full(hip, rows, tail):
    """live = one and two tile_rows: with an even tile side that is one live state behind the last landmark, whose row is
    summed like every other (3 + 2 (first_lm + count) <= live is all the call asks)"""
    tr = _info(hip)["tile_rows"]
    n_lm, spare = vc.full_tile_cases(tr)[rows - 1]
    Na = 3 + 2 * n_lm + spare
    assert Na == rows * tr
    C, Hc, R = vc.integer_family(n_lm, spare=spare)
    ex = vc.exact_value(C, Na, 0, Hc, R)
    assert ex["exact"] and C.shape == (Na, Na)
    d = _handle(hip, C, tail)
    r = d.value_operands(Hc, R)
    d.close()
    _no_poison(r)
    _same(r, ex)
    for kind in vc.FLOAT_KINDS:
        C, Hc, R = vc.float_family(n_lm, 0, kind, spare=spare)
        want = vc.np_value(C, Na, 0, Hc, R, tr)
        d = _handle(hip, C, tail)
        r = d.value_operands(Hc, R)
        d.close()
        _no_poison(r)
        _same(r, want)
        assert {k_: r.best[k_] for k_ in want["best"]} == want["best"]
        if spare:
            assert not vc.same_bits(vc.np_value(C, Na - 1, 0, Hc, R, tr)["dtrace"], r.dtrace)   # the spare row counts


# ---- 3. the same S as scoring ---------------------------------------------------------------------------------------------------

def test_S_and_flag_are_score_sparse_and_Hc_is_score_landmarks(hip):
    n_lm = 37
    C, x = vc.symmetric_map(n_lm)
    d = _handle(hip, C, 6, x)
    r = d.rank_landmarks()
    _, S, flags, _, (cols, Hc, _) = d.score_landmarks(0.7, -1.9, want_S=True, want_terms=True)
    assert vc.same_bits(r.Hc, Hc) and np.array_equal(cols, vc.all_cols(0, n_lm))
    assert vc.same_bits(r.S, S) and np.array_equal(r.flags, flags)
    Hw, Rw = vc.float_family(n_lm, 4, "wide")[1:]
    Hw[5, :, :] = 0.0   # S = R (a flagged candidate is case 7's)
    ro = d.value_operands(Hw, Rw)
    _, S2, flags2, _ = d.score_sparse(vc.all_cols(0, n_lm), Hw, Rw, want_S=True)
    assert vc.same_bits(ro.S, S2) and np.array_equal(ro.flags, flags2)
    part = d.value_operands(Hw[9:20], Rw, first_lm=9)
    _, S3, flags3, _ = d.score_sparse(vc.all_cols(9, 11), Hw[9:20], Rw, want_S=True)
    assert vc.same_bits(part.S, S3) and np.array_equal(part.flags, flags3)
    d.close()


# ---- 4. position independence ----------------------------------------------------------------------------------------------------

def test_a_landmark_keeps_its_bits_in_any_batch_run_and_capacity(hip):
    n_lm = _info(hip)["tile_lm"] + 3
    C, Hc, R = vc.float_family(n_lm, 5, "slam")
    d = _handle(hip, C, 0)
    full = d.value_operands(Hc, R)
    _same(d.value_operands(Hc, R), full)
    lo, hi = 7, n_lm - 2
    mid = d.value_operands(Hc[lo:hi], R, first_lm=lo)
    for key in OUT:
        assert vc.same_bits(getattr(mid, key), getattr(full, key)[lo:hi]), key
    for i in (0, lo, _info(hip)["tile_lm"], n_lm - 1):
        one = d.value_operands(Hc[i:i + 1], R, first_lm=i)
        for key in OUT:
            assert vc.same_bits(getattr(one, key), getattr(full, key)[i:i + 1]), (key, i)
        assert one.best["i_trace"] == 0 and one.best["v_trace"] == full.dtrace[i]
    d.close()
    big = _handle(hip, C, 2 * _info(hip)["tile_rows"] + 6)
    _same(big.value_operands(Hc, R), full)
    big.close()


# ---- 5. the point of the call ------------------------------------------------------------------------------------------------------

def test_figures_are_the_drops_of_an_actual_correction(hip):
    steps = ic.discovery_scenario(40)
    n = len(steps)
    f = hip.DenseEKFSLAM(n)
    for dth, dx, readings in steps:
        f.prediction(dth, dx)
        f.data_association(readings)
    assert f.known == n
    f.symmetrize()
    assert f.health()["n_asym"] == 0
    Na = 3 + 2 * n
    r = f.observation_value()
    C = f.handle.sigma[:Na, :Na]
    lv = vc.long_value(C, Na, 0, r.Hc, r.R)
    logdet0 = f.factor()["logdet"]
    detR = r.R[0, 0] * r.R[1, 1] - r.R[0, 1] * r.R[1, 0]   # (as the result object forms it: info_gain is then the same bits)
    assert not r.flags.any() and r.in_view.all()
    measured = np.empty(n)
    for j in range(n):
        g = f.clone()
        g.handle.correct_sparse(vc.lm_cols(j), r.Hc[j], r.R, np.zeros(2))
        Cp = g.handle.sigma[:Na, :Na]
        drops = {rows: (np.diag(C).astype(LD)[:rows] - np.diag(Cp).astype(LD)[:rows]).sum() for rows in (Na, 3)}
        measured[j] = float(drops[Na])
        if j in (0, n // 2, n - 1):
            for key, b, rows in (("dtrace", "bound_trace", Na), ("dtrace_pose", "bound_pose", 3)):
                bound = lv[b][j] + vc.drop_bound(lv, j, C, rows)
                err = abs(LD(getattr(r, key)[j]) - drops[rows])
                print(f"j={j} {key}: {getattr(r, key)[j]:.9g} measured {float(drops[rows]):.9g} err {float(err):.3g} "
                      f"bound {float(bound):.3g}")
                assert err <= bound
            # d log det = tr(Sigma^-1 dSigma) with the factor's backward error |dSigma| <= gamma_{Na + 1} |L| |L|^T, both
            # sides; Sigma+ is not symmetric in bits and the factor reads its lower triangle: tr(|Sigma^-1| |skew|) more
            rep = g.factor()
            assert rep["ok"] == 1
            bound = 8 * vc.U * (abs(logdet0) + abs(rep["logdet"]) + 1) + 2 * float(lv["bound_det"][j] / abs(lv["detS"][j]))
            for M in (C, Cp):
                L = np.linalg.cholesky(0.5 * (M + M.T))
                inv = np.abs(np.linalg.inv(M))
                bound += vc.gamma(Na + 1) * float((inv * (np.abs(L) @ np.abs(L).T)).sum()) + float((inv * np.abs(M - M.T)).sum())
            gain2, actual2 = np.log(r.detS[j] / detR), logdet0 - rep["logdet"]
            print(f"j={j} log(detS / detR) {gain2:.9g} log det drop {actual2:.9g} bound {bound:.3g}")
            assert abs(gain2 - actual2) <= bound and r.info_gain[j] == 0.5 * gain2
        g.close()
    order = np.argsort(-measured, kind="stable")
    top, second = order[0], order[1]
    margin = float(lv["bound_trace"][top] + vc.drop_bound(lv, top, C, Na) + lv["bound_trace"][second]
                   + vc.drop_bound(lv, second, C, Na))
    print(f"best {top} {measured[top]:.9g}, runner-up {second} {measured[second]:.9g}, margin needed {margin:.3g}")
    assert measured[top] - measured[second] > margin
    assert r.best["i_trace"] == top and f.best_view(1)[0] == top and list(f.best_view(3, "trace")) == list(r.order("trace")[:3])
    f.close()


# ---- 6. read-only and flush ----------------------------------------------------------------------------------------------------

def test_read_only_and_pending_rows(hip):
    n_lm = 20
    C, x = vc.symmetric_map(n_lm)
    d, twin = _handle(hip, C, 6, x), _handle(hip, C, 6, x)
    assert d.factor()["ok"] == 1
    L0, S0, x0 = d.get_factor(), d.sigma, d.state
    r = d.rank_landmarks(range_max=6.0)
    assert vc.same_bits(d.sigma, S0) and vc.same_bits(d.state, x0) and vc.same_bits(d.get_factor(), L0)
    cols, Hc, R = vc.lm_cols(3), r.Hc[3], r.R
    for h in (d, twin):
        h.correct_sparse_deferred(cols, Hc, R, np.array([0.01, -0.02]))
        assert h.pending == 2
    twin.flush()
    with pytest.raises(hip.EkfError):
        d.rank_landmarks(first_lm=n_lm)          # refused: the rows stay
    assert d.pending == 2
    a, b = d.rank_landmarks(), twin.rank_landmarks()
    assert d.pending == 0
    _same(a, b)
    assert a.best == b.best and vc.same_bits(d.sigma, twin.sigma) and vc.same_bits(d.state, twin.state)
    d.close(); twin.close()


def test_an_open_region_is_ended_before_the_terms_are_built(hip):
    """rank_landmarks over landmarks OUTSIDE an open region that has absorbed a correction: the global update of the region's
    end moves their state, and the Jacobians, the predicted ranges and the gating are taken from the state it leaves -- bit
    for bit what a twin that called region_end() first returns, Hc that of score_landmarks() afterwards"""
    n_lm, inside = 12, 4
    C, x = vc.symmetric_map(n_lm)
    d, twin = _handle(hip, C, 0, x), _handle(hip, C, 0, x)
    pre = d.rank_landmarks()
    x_before = d.state
    for h in (d, twin):
        h.region_begin(3 + 2 * inside)
        h.correct_sparse(vc.lm_cols(1), pre.Hc[1], pre.R, np.array([0.05, -0.03]))
        assert h.region_info()["active"] and h.region_info()["corrections"] == 1
    twin.region_end()
    x_after = twin.state
    assert (x_after[3 + 2 * inside:] != x_before[3 + 2 * inside:]).all()   # the landmarks outside did move
    rng_ = np.hypot(x_after[3::2] - x_after[1], x_after[4::2] - x_after[2])[inside:]
    cut = float(np.median(rng_))
    a = d.rank_landmarks(first_lm=inside, count=n_lm - inside, range_max=cut)   # (the default count follows the region's live)
    b = twin.rank_landmarks(first_lm=inside, count=n_lm - inside, range_max=cut)
    info = d.region_info()
    assert not info["active"] and info["ended_by_other_call"] == 1 and d.live == 3 + 2 * n_lm
    _same(a, b, OUT + ("Hc", "in_view", "flags"))
    assert a.best == b.best and 0 < int(a.in_view.sum()) < n_lm - inside
    assert vc.same_bits(d.sigma, twin.sigma) and vc.same_bits(d.state, x_after)
    Hc = d.score_landmarks(0.4, 1.1, first_lm=inside, want_terms=True)[4][1]
    assert vc.same_bits(a.Hc, Hc) and not vc.same_bits(a.Hc, pre.Hc[inside:])
    d.close(); twin.close()


# ---- 7. flags, ties, gating -------------------------------------------------------------------------------------------------------

def test_flags_ties_and_gating(hip):
    tl = _info(hip)["tile_lm"]
    C, Hc, R = vc.float_family(tl + 2, 3, "wide")
    a, b = 1, tl + 1   # in different landmark tiles
    ca, cb = vc.lm_cols(a)[3:], vc.lm_cols(b)[3:]
    C[:, cb] = C[:, ca]
    C[cb, :] = C[ca, :]
    C[np.ix_(cb, cb)] = C[np.ix_(ca, ca)]
    Hc[b] = Hc[a]
    d = _handle(hip, C, 6)
    r = d.value_operands(Hc, R)
    for key in OUT:
        assert vc.same_bits(getattr(r, key)[a:a + 1], getattr(r, key)[b:b + 1]), key
    only = np.zeros(tl + 2, dtype=np.uint8)
    only[[a, b]] = 1
    tie = d.value_operands(Hc, R, in_view=only)
    assert (tie.best["i_trace"], tie.best["i_pose"], tie.best["i_det"]) == (a, a, a)
    assert tie.best["v_trace"] == r.dtrace[b] and tie.best["v_det"] == r.detS[b]
    only[a] = 0
    assert d.value_operands(Hc, R, in_view=only).best["i_trace"] == b
    nothing = d.value_operands(Hc, R, in_view=np.zeros(tl + 2, dtype=np.uint8))
    assert (nothing.best["i_trace"], nothing.best["i_pose"], nothing.best["i_det"]) == (-1, -1, -1)
    assert np.isnan(nothing.best["v_trace"]) and vc.same_bits(nothing.dtrace, r.dtrace)
    d.close()
    # R = 0 over a zero 5 x 5 block: flag 1, NaN, never the winner
    Z = C.copy()
    c = vc.lm_cols(2)
    Z[np.ix_(c, c)] = 0.0
    d = _handle(hip, Z, 0)
    z = d.value_operands(Hc, np.zeros((2, 2)))
    want = vc.np_value(Z, Z.shape[0], 0, Hc, np.zeros((2, 2)), _info(hip)["tile_rows"])
    assert z.flags[2] == 1 and np.isnan(z.dtrace[2]) and np.isnan(z.dtrace_pose[2]) and np.isnan(z.detS[2])
    assert np.array_equal(z.flags, want["flags"]) and 2 not in (z.best["i_trace"], z.best["i_pose"], z.best["i_det"])
    assert {k: z.best[k] for k in want["best"]} == want["best"]
    d.close()
    # the reach of the sensor between two predicted ranges
    Cm, x = vc.symmetric_map(12)
    d = _handle(hip, Cm, 6, x)
    free = d.rank_landmarks()
    rng_ = np.hypot(x[3::2] - x[1], x[4::2] - x[2])
    far = int(free.best["i_trace"])   # the unrestricted winner goes out of reach; the next nearer landmark stays in
    nearer = [rng_[j] for j in range(12) if rng_[j] < rng_[far]]
    cut = 0.5 * ((max(nearer) if nearer else 0.0) + rng_[far])
    gated = d.rank_landmarks(range_max=cut)
    assert np.array_equal(gated.in_view, (rng_ <= cut).astype(np.uint8)) and gated.in_view[far] == 0
    assert int(gated.in_view.sum()) == len(nearer) and gated.best["i_trace"] != far
    seen = [j for j in range(12) if gated.in_view[j]]
    assert gated.best["i_trace"] == (max(seen, key=lambda j: (free.dtrace[j], -j)) if seen else -1)
    assert vc.same_bits(gated.dtrace, free.dtrace) and free.in_view.all()
    assert d.rank_landmarks(range_max=1e-3).best["i_trace"] == -1
    d.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_in_the_documented_order(hip):
    import ctypes as ct
    n_lm = 4
    C, x = vc.symmetric_map(n_lm)
    d = _handle(hip, C, 6, x)
    lib, h = d._lib, d._h
    S0, x0 = d.sigma, d.state
    d.correct_sparse_deferred(vc.lm_cols(0), np.ones((2, 5)), np.eye(2), np.zeros(2))
    Hc, R = np.ones((n_lm, 2, 5)), np.eye(2)
    out = np.empty(n_lm)
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))   # noqa: E731
    best = hip.ValueBest()

    def operands(first, count, hc=Hc, r=R, o=out):
        return lib.ekf_dense64_value_operands(h, first, count, dp(hc) if hc is not None else None, dp(r) if r is not None else None,
                                              None, dp(o) if o is not None else None, None, None, None, None, None, None)

    def rank(first, count, o=out):
        return lib.ekf_dense64_rank_landmarks(h, None, first, count, 0.0, dp(o) if o is not None else None, None, None, None,
                                              None, None, None, None, None)

    def refused(st, word):
        assert st == 1 and word in lib.ekf_last_error().decode() and d.pending == 2

    refused(operands(-1, 0, None, None, None), "every output is NULL")   # before the count, the range and the operands
    refused(rank(-1, 0, None), "every output is NULL")
    refused(operands(0, 0, None, None), "count >= 1")                    # before the range and the operands
    refused(operands(-1, n_lm + 1, None, None), "count >= 1")
    refused(rank(-1, n_lm + 1), "count >= 1")
    refused(operands(0, n_lm + 1, None, None), "live dimension")         # before the operands
    refused(operands(n_lm, 1, None, None), "live dimension")
    refused(rank(1, n_lm), "live dimension")
    refused(operands(0, n_lm, None, R), "null Hc or R")
    refused(operands(0, n_lm, Hc, None), "null Hc or R")
    assert lib.ekf_dense64_value_operands(None, 0, 1, dp(Hc), dp(R), None, dp(out), None, None, None, None, None, None) == 1
    assert lib.ekf_dense64_rank_landmarks(h, None, 0, n_lm, 0.0, None, None, None, None, None, ct.byref(best), None, None,
                                          None) == 0 and d.pending == 0   # best alone is an output
    d.close()
    d = _handle(hip, C, 6, x)
    with pytest.raises(hip.EkfError):
        d.value_operands(Hc, R, first_lm=1)
    with pytest.raises(ValueError):
        d.value_operands(np.ones((n_lm, 2, 4)), R)
    assert vc.same_bits(d.sigma, S0) and vc.same_bits(d.state, x0)
    d.close()
