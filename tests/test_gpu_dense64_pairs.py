"""GPU: ekf_dense64_score_landmark_pairs (all pairs of landmarks in one pass, ekf_dense64_pairs.hip) against
ekf_dense64_score_sparse on the defining operands, bit for bit; against the numpy model; read-only, live and flushing;
refusals; ekf_dense64_merge_landmarks against the spelled sequence on a twin handle; a map's lifecycle with a duplicate;
the full-size map with the time condition."""
import ctypes as C
import math

import numpy as np
import pytest

import dense_block_cases as bc
import dense_init_cases as ic
import dense_pairs_cases as pc
import dense_sparse_cases as sp
from parity import FP64_TOL, worst
from test_gpu_dense64_live import _poison
from test_gpu_dense64_sparse import _full_size_sigma, _median

pytestmark = pytest.mark.gpu

T = 32   # the kernel's landmark tile
SIZES = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 2]
WORST = {"model": 0.0}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _handle(hip, state, Sigma, live=None):
    d = hip.DensePropagator64(len(state))
    d.set(Sigma=Sigma)
    d.state = state
    if live is not None:
        d.live = live
    return d


def _family(name, n_lm, N):
    if name == "integers":
        return pc.integer_family(n_lm, N, 11 + n_lm)
    if name == "random":
        return pc.random_family(n_lm, N, 23 + n_lm)
    return pc.degenerate_family(n_lm, N, 37 + n_lm)[:2]


def _against_score_sparse(d, state, n_lm, r_merge, gate):
    """the scan's outputs and the same four quantities folded from ONE score_sparse call over all pairs"""
    got = d.landmark_pairs(n_lm, r_merge, gate)[:4]
    pairs = pc.all_pairs(n_lm)
    if not pairs:
        return got, (np.array([-1], dtype=np.int32), np.array([np.inf]), 0, 0)
    cols, Hc, R, nu = pc.stacked_operands(state, pairs, r_merge)
    nis, _, flags, _ = d.score_sparse(cols, Hc, R, nu)
    return got, pc.fold(n_lm, pairs, nis, flags, gate)


def test_tile_is_what_the_library_reports(hip):
    d = hip.DensePropagator64(7)
    assert d.pairs_launch_info() == {"tile_landmarks": T, "threads": 256}
    d.close()


@pytest.mark.parametrize("tail", [0, 5])
@pytest.mark.parametrize("n_lm", SIZES)
@pytest.mark.parametrize("family,r_merges", [("integers", pc.R_MERGES), ("random", (0.5,)), ("degenerate", (0.0, 0.5))])
def test_bits_against_score_sparse(hip, family, r_merges, n_lm, tail):
    assert n_lm * (n_lm - 1) // 2 * 2 <= hip.DensePropagator64.SCORE_SPARSE_MAX_ROWS
    P = 3 + 2 * n_lm
    N = P + tail
    state, Sigma = _family(family, n_lm, N)
    if tail:   # what lies beyond the n_lm landmarks must not matter: NaNs, every one with a payload of its own
        Sigma, state = _poison(N, P, Sigma[:P, :P], state[:P])
    d = _handle(hip, state, Sigma, live=P if tail else None)   # (score_sparse stays inside the corner as well)
    for r_merge in r_merges:
        gate = 1.0 if family != "integers" else 3.0
        (nearest, d2, below, flagged), (w_near, w_d2, w_below, w_flagged) = _against_score_sparse(d, state, n_lm, r_merge, gate)
        assert np.array_equal(nearest, w_near), (r_merge, nearest, w_near)
        assert _same(d2, w_d2), r_merge
        assert (below, flagged) == (w_below, w_flagged), r_merge
        again = d.landmark_pairs(n_lm, r_merge, gate)
        assert np.array_equal(again[0], nearest) and _same(again[1], d2) and again[2:4] == (below, flagged)
        if family == "degenerate" and n_lm >= 6:
            assert flagged == (n_lm - 1) + (1 if r_merge == 0.0 else 0)   # the NaN landmark's pairs, the exact copy at r = 0
            assert nearest[2] == -1 and d2[2] == np.inf and nearest[3] == 4 and (nearest[0] == 1) == (r_merge > 0.0)
    d.close()


@pytest.mark.parametrize("n_lm", [T + 1, 2 * T + 1])
def test_against_the_numpy_model(hip, n_lm):
    N = 3 + 2 * n_lm + 5
    state, Sigma = pc.random_family(n_lm, N, 23 + n_lm)
    d = _handle(hip, state, Sigma)
    for r_merge in (0.5, 4.0):
        nearest, d2, below, flagged, _ = d.landmark_pairs(n_lm, r_merge, 1.0)
        w_near, w_d2, w_below, w_flagged = pc.model_scan(Sigma, state, n_lm, r_merge, 1.0)
        err = float(np.max(np.abs(d2 - w_d2) / np.maximum(np.abs(w_d2), 1e-3)))
        WORST["model"] = max(WORST["model"], err)
        print(f"pairs n_lm={n_lm} r_merge={r_merge}: max relative deviation from the numpy model {err:.3e} (FP64_TOL {FP64_TOL:g})")
        assert err <= FP64_TOL
        assert np.array_equal(nearest, w_near) and (below, flagged) == (w_below, w_flagged)
    d.close()


def test_live_read_only_and_flushing(hip):
    n_lm = T + 3
    P = 3 + 2 * n_lm
    N, live = P + 9, P + 4
    state, Sigma = pc.random_family(n_lm, P, 91)
    Sp, xp = _poison(N, P, Sigma, state)
    d, twin = _handle(hip, xp, Sp, live=live), _handle(hip, state, Sigma)
    S0, x0 = d.sigma, d.state
    got, want = d.landmark_pairs(n_lm, 0.5, 1.0), twin.landmark_pairs(n_lm, 0.5, 1.0)
    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and got[2:4] == want[2:4]
    assert _same(d.sigma, S0) and _same(d.state, x0) and d.live == live
    d.close()
    # rows pending: the scan applies them first
    cols, Hc, R, nu = pc.pair_operands(state, 4, 9, 0.5)
    twin.correct_sparse_deferred(cols, Hc, R, -nu)
    assert twin.pending == 2
    other = _handle(hip, state, Sigma)
    other.correct_sparse_deferred(cols, Hc, R, -nu)
    other.flush()
    got, want = twin.landmark_pairs(n_lm, 0.5, 1.0), other.landmark_pairs(n_lm, 0.5, 1.0)
    assert twin.pending == 0
    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and got[2:4] == want[2:4]
    assert _same(twin.sigma, other.sigma) and _same(twin.state, other.state)
    twin.close()
    other.close()


def test_refusals_change_nothing(hip):
    n_lm = 6
    P = 3 + 2 * n_lm
    state, Sigma = pc.random_family(n_lm, P + 4, 5)
    d = _handle(hip, state, Sigma, live=P)
    cols, Hc, R, nu = pc.pair_operands(state, 1, 2, 0.5)
    d.correct_sparse_deferred(cols, Hc, R, -nu)
    d.carry = True
    before = (d.sigma_block(np.arange(P), np.arange(P)), d.state, d.pending)   # (read through the rows: nothing is flushed)
    lib, h = hip.load(), d._h
    near, d2 = np.zeros(n_lm, dtype=np.int32), np.zeros(n_lm)
    pn, pd = near.ctypes.data_as(C.POINTER(C.c_int)), d2.ctypes.data_as(C.POINTER(C.c_double))
    nan, inf = float("nan"), float("inf")
    bad = [(None, n_lm, 0.5, 1.0, pn, pd), (h, n_lm, 0.5, 1.0, None, None), (h, 0, 0.5, 1.0, pn, pd),
           (h, n_lm + 1, 0.5, 1.0, pn, pd), (h, n_lm, -0.5, 1.0, pn, pd), (h, n_lm, inf, 1.0, pn, pd),
           (h, n_lm, nan, 1.0, pn, pd), (h, n_lm, 0.5, nan, pn, pd)]
    for hh, n, r, g, a, b in bad:
        assert lib.ekf_dense64_score_landmark_pairs(hh, n, r, g, a, b, None, None, None) == 1, (n, r, g)
    known = C.c_int(n_lm)
    for a, b, r, k in [(1, 1, 0.5, n_lm), (0, n_lm, 0.5, n_lm), (-1, 2, 0.5, n_lm), (0, 1, -1.0, n_lm), (0, 1, nan, n_lm),
                       (0, 1, 0.5, n_lm + 1)]:
        known.value = k
        assert lib.ekf_dense64_merge_landmarks(h, None, a, b, r, C.byref(known), 0, None, None, None) == 1, (a, b, r, k)
        assert known.value == k
    assert lib.ekf_dense64_merge_landmarks(h, None, 0, 1, 0.5, C.byref(known), 4, None, None, None) == 1
    assert lib.ekf_dense64_merge_landmarks(None, None, 0, 1, 0.5, C.byref(known), 0, None, None, None) == 1
    after = (d.sigma_block(np.arange(P), np.arange(P)), d.state, d.pending)
    assert _same(before[0], after[0]) and _same(before[1], after[1]) and before[2] == after[2] == 2
    assert not near.any() and not d2.any()
    d.close()


def _spelled_merge(d, a, b, r_merge, known, deferred, grow):
    """INTEGRATION.md's sequence with the public calls -> known, moved_from, nis"""
    lo, hi, last = min(a, b), max(a, b), known - 1
    cols, Hc, R, nu = pc.merge_operands(d.state, a, b, r_merge)
    nis, _ = (d.correct_sparse_deferred if deferred else d.correct_sparse)(cols, Hc, R, nu)
    if hi != last:
        d.swap_blocks(3 + 2 * hi, 3 + 2 * last, 2)
    d.init_block(3 + 2 * last, W=100.0 * np.eye(2))
    if grow:
        d.live = 3 + 2 * last
    return last, (last if hi != last else -1), nis


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("a,b", [(5, 6), (6, 5), (0, 1), (1, 0)])
def test_merge_is_the_spelled_sequence(hip, a, b, deferred):
    """hi last ((5, 6) of 7) and hi in mid-map ((0, 1)), either argument order; eager with the live dimension following, and
    deferred with carry on, so that the swap and the re-initialisation carry the correction's pending rows"""
    known = 7
    P = 3 + 2 * known
    state, Sigma = pc.random_family(known, P + 6, 77)
    Sigma[P:, :P] = 0.0
    Sigma[:P, P:] = 0.0
    d, twin = _handle(hip, state, Sigma, live=P), _handle(hip, state, Sigma, live=P)
    flags = d.LM_DEFERRED if deferred else d.LM_GROW_LIVE
    if deferred:
        for h in (d, twin):
            h.carry = True
            h.correct_sparse_deferred(*pc.merge_operands(state, 2, 3, 0.25))
    nearest, d2 = d.landmark_pairs(known, 0.5, 1.0)[:2]    # (applies the pending rows: so does the twin)
    twin.flush()
    lo, hi = min(a, b), max(a, b)
    assert nearest[lo] == hi and nearest[hi] == lo, "the planted near-duplicates are each other's nearest"
    got = d.merge_landmarks(a, b, 0.5, known, flags)[:3]
    want = _spelled_merge(twin, a, b, 0.5, known, deferred, not deferred)
    assert got[:2] == want[:2] and _bits(got[2]) == _bits(want[2]) == _bits(d2[lo])
    assert d.live == twin.live == (P if deferred else P - 2) and d.pending == twin.pending == (2 if deferred else 0)
    every = np.arange(d.N)
    assert _same(d.sigma_block(every, every), twin.sigma_block(every, every)) and _same(d.state, twin.state)
    assert d.pending == twin.pending == (2 if deferred else 0)
    assert _same(d.sigma, twin.sigma)
    d.close()
    twin.close()


def test_singular_merge_leaves_everything(hip):
    known = 6
    state, Sigma, what = pc.degenerate_family(known, 3 + 2 * known, 43)
    Sigma[7, 8] = 0.25   # (no NaN here: the exact copy alone)
    d = _handle(hip, state, Sigma)
    cols, Hc, R, nu = pc.merge_operands(state, 2, 3, 0.5)
    d.correct_sparse_deferred(cols, Hc, R, nu)
    d.carry = True
    every = np.arange(d.N)
    before = (d.sigma_block(every, every), d.state, d.pending)
    with pytest.raises(hip.EkfError) as e:
        d.merge_landmarks(0, 1, 0.0, known, d.LM_DEFERRED)
    assert e.value.status == 5
    assert _same(d.sigma_block(every, every), before[0]) and _same(d.state, before[1]) and d.pending == before[2] == 2
    d.close()


def test_lifecycle_duplicate_found_and_merged(hip):
    """six tubes discovered over six ticks; then the robot is displaced by 0.8 m that the odometry does not report and takes
    ONE reading of tube 0: its score is beyond gate_new and the rule creates landmark 6, a second copy.  find_duplicates
    names (0, 6) and nothing else, merge restores the count, and the fused landmark lies within 3 sigma of the truth under
    the pair's own S.  The same calls on the numpy handle (ic.association_step, pc.np_merge) agree to FP64_TOL."""
    n_true, cap, r_merge, gate = 6, 8, 1.0, 1.0
    steps = ic.discovery_scenario(steps=n_true, seed=5)
    ang = 2 * math.pi * np.arange(n_true) / n_true
    rad = 1.5 + 1.0 * (np.arange(n_true) % 4)
    world = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    f = hip.DenseEKFSLAM(cap)
    m = ic.NumpyHandle(3 + 2 * cap)
    x0, S0 = ic.prior_start(cap)
    m.set(S0)
    m.state = x0
    known, pose = 0, np.zeros(3)
    for dth, dx, readings in steps:
        pose = pose + bc.model_operands(pose, dth, dx)[2]
        f.prediction(dth, dx)
        f.data_association(readings)
        known = ic.association_step(m, cap, known, dth, dx, readings, "init_block")
    assert f.known == known == n_true
    # the jump: the truth moves 0.8 m towards tube 0 beyond what the odometry says
    dth, dx = 0.1, 0.05
    pose = pose + bc.model_operands(pose, dth, dx)[2]
    to0 = world[0] - pose[1:]
    pose[1:] += 0.8 * to0 / np.linalg.norm(to0)
    c, s = math.cos(pose[0]), math.sin(pose[0])
    d0 = world[0] - pose[1:]
    reading = np.array([[c * d0[0] + s * d0[1], -s * d0[0] + c * d0[1]]])
    f.prediction(dth, dx)
    f.data_association(reading)
    known = ic.association_step(m, cap, known, dth, dx, reading, "init_block")
    assert f.known == known == n_true + 1, "the displaced reading must create a duplicate"
    dups, below = f.find_duplicates(gate, r_merge)
    assert [(a, b) for a, b, _ in dups] == [(0, n_true)] and below == 1
    xs, Ss = f.handle.state, f.handle.sigma
    S_pair = pc.model_score(Ss, xs, 0, n_true, r_merge)[2]
    moved, d2 = f.merge(n_true, 0, r_merge)
    assert moved == -1 and f.known == n_true and _bits(d2) == _bits(dups[0][2])
    ms, mS, mk, mmoved, md2 = pc.np_merge(m.state, m.sigma, known, 0, n_true, r_merge)
    assert (mk, mmoved) == (n_true, -1) and abs(md2 - d2) <= FP64_TOL * abs(md2)
    w, e = worst(f.handle.state, f.handle.sigma, ms, mS)
    print(f"lifecycle: worst per-block deviation from the numpy model {w:.3e}")
    assert w <= FP64_TOL, e
    off = f.handle.state[3:5] - world[0]
    assert float(off @ np.linalg.inv(S_pair) @ off) <= 9.0
    assert f.find_duplicates(gate, r_merge) == ([], 0)
    f.close()


def test_full_size_n10003_and_time(hip):
    """N = 10003, 5000 landmarks: d2 is the bits of score_sparse on the pairs (a, nearest[a]); about 27 000 other pairs
    (seeded, plus the pairs at tile boundaries) are neither below their landmarks' minima nor tie them from a lower index;
    and median(scan) <= median(correct_sparse(2, 5)), both measured here: the scan reads 8 N^2 bytes where that call reads
    and writes 16 N^2."""
    N, n = 10003, 5000
    rng = np.random.default_rng(8)
    Sigma = _full_size_sigma(N, rng)
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    for j in range(7, n, 97):   # planted near-duplicates, some across tile boundaries
        i = j - (1 if j % 2 else 40)
        x[3 + 2 * j:5 + 2 * j] = x[3 + 2 * i:5 + 2 * i] + 0.01
    d = _handle(hip, x, Sigma)
    del Sigma
    nearest, d2, below, flagged, ms = d.landmark_pairs(n, 0.5, 1.0)
    assert flagged == 0 and nearest.min() >= 0 and np.all(nearest != np.arange(n)) and below >= len(range(7, n, 97))
    mine = [(min(a, int(b)), max(a, int(b))) for a, b in enumerate(nearest)]
    nis, _, flags, _ = d.score_sparse(*pc.stacked_operands(x, mine, 0.5))
    assert not flags.any() and _same(nis, d2)
    others = set()
    for a in rng.integers(0, n, size=2800):
        others.update((min(int(a), int(b)), max(int(a), int(b))) for b in rng.integers(0, n, size=9) if b != a)
    for edge in range(T, n, T):
        others.update({(edge - 1, edge), (edge - T, edge), (edge - 1, min(n - 1, edge + T - 1)), (0, edge), (edge - 1, n - 1)})
    others = sorted(others)
    assert 25000 <= len(others) <= 32768
    nis, _, flags, _ = d.score_sparse(*pc.stacked_operands(x, others, 0.5))
    for (a, b), v in zip(others, nis):
        for me, o in ((a, b), (b, a)):
            assert not v < d2[me] and not (v == d2[me] and o < nearest[me]), (a, b, v, d2[me], nearest[me])
    cols, Hc, R, nu = sp.slam_terms(x[:3], x, 3333, 0.7, -0.4)[:4]
    t_scan = _median(lambda: d.landmark_pairs(n, 0.5, 1.0)[4])
    t_corr = _median(lambda: d.correct_sparse(cols, Hc, R, nu)[1])
    t_scan2 = _median(lambda: d.landmark_pairs(n, 0.5, 1.0)[4])
    rate = 8.0 * N * N / (t_scan * 1e-3) / 1e12
    line = (f"landmark_pairs n_lm={n} at N={N}: {t_scan:.4f} ms (again {t_scan2:.4f}) = {rate:.2f} TB/s on 8 N^2 bytes, "
            f"{rate / 8.0:.2f} of 8 TB/s; correct_sparse(2, 5) {t_corr:.4f} ms")
    print(line)
    d.close()
    assert t_scan <= t_corr, (t_scan, t_corr)


def test_zz_report():
    print(f"dense64 pairs: maximum deviation from the numpy model {WORST['model']:.3e} (FP64_TOL {FP64_TOL:g})")
    assert WORST["model"] <= FP64_TOL
