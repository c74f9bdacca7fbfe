"""GPU: ekf_dense64_scan_evidence (ekf_dense64_evidence.hip) against the numpy model of tests/dense_evidence_cases.py --
expected ranges within 1e-12, every integer exact outside the beams the host test lists as marginal --, its tolerance
against ekf_dense64_score_landmarks' S bit for bit, bit stability, read-only, refusals in the documented order; and
ekf_dense64_remove_landmark against the spelled recipe on a twin handle.  The handle offers no launch reporter, so that
kappa == 0 skips the scoring launch is not asserted here (it is a branch on the host, ekf_capi_dense64.hip); what is asserted
is that kappa == 0 gives tol_abs on a Sigma full of NaNs."""
import ctypes as C

import numpy as np
import pytest

import dense_evidence_cases as ev
import dense_pairs_cases as pc
from test_gpu_dense64_live import _poison

pytestmark = pytest.mark.gpu

RANGE_TOL = 1e-12   # the project's contract is 1e-9; the measured maximum is printed (5.5e-14 on an MI355X)
WORST = {"range": 0.0}
NAMES = sorted(ev.CASES)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _lidar(hip, nb, rmax, border, radius):
    return hip.default_lidar(n_beams=nb, range_max=rmax, border_width=border, tube_radius=radius)


def _handle(hip, pose, lms, tail=0, Sigma=None):
    """a handle whose state is the case's map; with a tail everything outside the live corner is poisoned"""
    P = 3 + 2 * len(lms)
    x = np.concatenate([pose, np.asarray(lms, dtype=np.float64).reshape(-1)])
    S = 0.01 * np.eye(P) if Sigma is None else Sigma
    if tail:
        S, x = _poison(P + tail, P, S, x)
    d = hip.DensePropagator64(len(x))
    d.set(Sigma=S)
    d.state = x
    if tail:
        d.live = P
    return d


def _case_handle(hip, name, tail=0):
    pose, lms, nb, rmax, border, radius = ev.case(name)
    return _handle(hip, pose, lms, tail), _lidar(hip, nb, rmax, border, radius)


def _check_beams(got, want, risky):
    ok = ~risky
    err = float(np.max(np.abs(got.expected[ok] - want["expected"][ok]))) if ok.any() else 0.0
    WORST["range"] = max(WORST["range"], err)
    print(f"scan evidence: max |expected - model| {err:.3e} (bound {RANGE_TOL:g}), {int(risky.sum())} marginal beams left out")
    assert err <= RANGE_TOL
    assert np.array_equal(got.hit[ok], want["hit"][ok])
    assert np.array_equal(got.cls[ok], want["cls"][ok])


def test_launch_info_is_what_the_cases_straddle(hip):
    d = hip.DensePropagator64(5)
    assert d.evidence_launch_info() == {"beam_tile": 64, "lm_chunk": 128, "threads": 64}
    d.close()


def test_exact_family(hip):
    d, lp = _case_handle(hip, "exact")
    got = d.scan_evidence(None, lp, kappa=0.0)
    assert got.expected[0] == 0.75 and list(got.hit) == [0, -1, -1, -1] and got.report["n_on_tube"] == 1
    obs = np.array([0.75, 1.0, 1.0, 1.0])
    got = d.scan_evidence(obs, lp, tol_abs=0.0, kappa=0.0)
    assert list(got.cls) == [1, 0, 0, 0] and (got.n_expected[0], got.n_agree[0], got.n_through[0], got.n_short[0]) == (1, 1, 0, 0)
    got = d.scan_evidence(obs + 0.25, lp, tol_abs=0.125, kappa=0.0)
    assert list(got.cls) == [2, 0, 0, 0] and (got.n_through[0], got.n_agree[0]) == (1, 0)
    d.close()


@pytest.mark.parametrize("tail", [0, 6])
@pytest.mark.parametrize("name", NAMES)
def test_expected_scan_hits_and_classes(hip, name, tail):
    """the geometry (occlusion, ties, NaN landmarks, the edges, 1 .. 130 landmarks in reach) with ranges NULL, then the
    classes on a scan built from the model's expected one"""
    d, lp = _case_handle(hip, name, tail)
    n = (d.live - 3) // 2
    want = ev.case_model(name)
    risky = ev.margins(want)
    got = d.scan_evidence(None, lp, kappa=0.0)
    _check_beams(got, want, risky)
    assert not got.cls.any() and not any(a.any() for a in (got.n_expected, got.n_agree, got.n_through, got.n_short))
    assert got.report["n_candidates"] == want["report"]["n_candidates"]
    assert (got.report["n_unexplained"], got.report["n_invalid"]) == (0, 0)
    obs, wc = ev.classed_scan(name)
    risky = ev.margins(wc, obs)
    got = d.scan_evidence(obs, lp, tol_abs=0.05, kappa=0.0)
    _check_beams(got, wc, risky)
    assert _same(got.tol, np.full(n, 0.05))
    if not risky.any():
        for k in ("n_expected", "n_agree", "n_through", "n_short"):
            assert np.array_equal(getattr(got, k), wc[k]), k
        assert got.report == wc["report"]
    # the counters are those of the call's own beams
    for i in range(n):
        mine = (got.hit == i) & (got.cls != 4)
        assert got.n_expected[i] == mine.sum() and got.n_agree[i] == (mine & (got.cls == 1)).sum()
        assert got.n_through[i] == (mine & (got.cls == 2)).sum() and got.n_short[i] == (mine & (got.cls == 3)).sum()
    again = d.scan_evidence(obs, lp, tol_abs=0.05, kappa=0.0)
    assert _same(again.expected, got.expected) and np.array_equal(again.hit, got.hit) and np.array_equal(again.cls, got.cls)
    d.close()


def _sigma_case(n_lm, N, seed):
    """a covariance from the pair tests' random family with the map of a case in the state"""
    return pc.random_family(n_lm, N, seed)[1]


@pytest.mark.parametrize("pending", [False, True])
def test_tolerance_is_score_landmarks_S(hip, pending):
    pose, lms, nb, rmax, border, radius = ev.case("world_130")
    n = len(lms)
    P = 3 + 2 * n
    Sigma = _sigma_case(n, P, 5)
    d = _handle(hip, pose, lms, 0, Sigma)
    if pending:
        cols, Hc, R, nu = pc.merge_operands(d.state, 2, 3, 0.25)
        d.correct_sparse_deferred(cols, Hc, R, nu)
        assert d.pending == 2
    lp = _lidar(hip, nb, rmax, border, radius)
    S = d.score_landmarks(0.3, -0.2, 0, n, want_S=True)[1]
    got = d.scan_evidence(None, lp, tol_abs=0.05, kappa=2.5)
    assert _same(got.tol, 0.05 + 2.5 * np.sqrt(np.maximum(S[:, 0, 0], 0.0)))
    assert d.pending == (2 if pending else 0)
    d.close()


def test_tolerance_decides_and_a_flagged_landmark_agrees(hip):
    pose, lms, nb, rmax, border, radius = ev.case("heading_not_wrapped")
    lp = _lidar(hip, nb, rmax, border, radius)
    m = ev.case_model("heading_not_wrapped")
    beams = np.nonzero(m["hit"] == 1)[0]
    obs = ev.observed(m, through=list(beams))
    out = {}
    for kind, var in (("tight", 1e-6), ("prior", 100.0), ("flagged", np.nan)):
        S = 1e-6 * np.eye(9)
        S[5, 5] = S[6, 6] = var
        d = _handle(hip, pose, lms, 0, S)
        out[kind] = d.scan_evidence(obs, lp, tol_abs=0.05, kappa=3.0)
        if kind == "flagged":   # kappa == 0 does not read Sigma
            blind = d.scan_evidence(obs, lp, tol_abs=0.05, kappa=0.0)
            assert _same(blind.tol, np.full(3, 0.05)) and blind.n_through[1] == len(beams)
        d.close()
    assert out["tight"].n_through[1] == len(beams) > 0 and out["tight"].n_agree[1] == 0
    assert out["prior"].n_agree[1] == len(beams) and out["prior"].n_through[1] == 0 and out["prior"].tol[1] > 10.0
    assert out["flagged"].tol[1] == np.inf and out["flagged"].n_agree[1] == len(beams)
    assert np.isfinite(out["flagged"].tol[[0, 2]]).all()


def test_bit_stability(hip):
    """landmark 1 of three that do not hide each other: alone, in a slice, in the batch, at a larger N, with 100 landmarks
    out of reach behind it, and again"""
    pose, lms, nb, rmax, border, radius = ev.case("heading_not_wrapped")
    lp = _lidar(hip, nb, rmax, border, radius)
    m = ev.case_model("heading_not_wrapped")
    obs = ev.observed(m, through=list(np.nonzero(m["hit"] == 1)[0][::2]))
    Sigma = 1e-4 * _sigma_case(3, 9, 8)   # (small enough that 0.5 m behind the tube is through it)
    d = _handle(hip, pose, lms, 0, Sigma)
    full = d.scan_evidence(obs, lp, kappa=2.0)
    pick = lambda r, i: (r.n_expected[i], r.n_agree[i], r.n_through[i], r.n_short[i], _bits(r.tol[i]))
    want = pick(full, 1)
    assert want[0] > 0 and want[2] > 0
    assert pick(d.scan_evidence(obs, lp, first_lm=1, count=1, kappa=2.0), 0) == want
    assert pick(d.scan_evidence(obs, lp, first_lm=1, count=2, kappa=2.0), 0) == want
    assert pick(d.scan_evidence(obs, lp, kappa=2.0), 1) == want
    d.close()
    far = np.array([[9.0 + 0.1 * k, -8.0 - 0.05 * k] for k in range(100)])
    big = np.zeros((209, 209))
    big[:9, :9] = Sigma
    big[9:, 9:] = np.eye(200)
    d = _handle(hip, pose, np.vstack([lms, far]), 6, big)
    more = d.scan_evidence(obs, lp, kappa=2.0)
    assert pick(more, 1) == want and more.report["n_candidates"] == 3
    assert _same(more.expected, full.expected) and np.array_equal(more.hit, full.hit) and np.array_equal(more.cls, full.cls)
    d.close()


def test_read_only_and_the_region(hip):
    pose, nb, rmax, border, radius = np.array([0.4, 0.1, -0.2]), 360, 3.5, float("inf"), 0.0762
    lms = ev.disk_world(40, 0, 77)[0]
    n = len(lms)
    P = 3 + 2 * n
    Sigma = _sigma_case(n, P, 9)
    d, twin = _handle(hip, pose, lms, 6, Sigma), _handle(hip, pose, lms, 6, Sigma)   # the twin is never cast at
    lp = _lidar(hip, nb, rmax, border, radius)
    for h in (d, twin):
        h.carry = True
        h.correct_sparse_deferred(*pc.merge_operands(h.state_block(0, P), 4, 9, 0.25))
    every = np.arange(P)
    before = (d.sigma_block(every, every), d.state_block(0, P), d.pending, d.live)
    m = ev.np_scan_evidence(pose, lms, nb, rmax, border, radius)
    obs = ev.observed(m, through=list(np.nonzero(m["hit"] >= 0)[0][::3]))
    d.scan_evidence(obs, lp, kappa=2.0)
    after = (d.sigma_block(every, every), d.state_block(0, P), d.pending, d.live)
    assert _same(before[0], after[0]) and _same(before[1], after[1]) and before[2:] == after[2:] == (2, P)
    # Sigma in memory and the pending rows themselves: applied now, they give the bits they give on the twin
    d.flush()
    twin.flush()
    raw = d.sigma
    assert _same(raw[:P, :P], twin.sigma[:P, :P]) and _same(d.state_block(0, P), twin.state_block(0, P))
    twin.close()
    d.scan_evidence(obs, lp, kappa=2.0)
    assert _same(d.sigma[:P, :P], raw[:P, :P])
    # inside a region the call ends it, as rank_landmarks does
    d.region_begin(3 + 2 * 8)
    ended = d.region_info()["ended_by_other_call"]
    d.scan_evidence(obs, lp, kappa=0.0)
    info = d.region_info()
    assert not info["active"] and info["ended_by_other_call"] == ended + 1 and d.live == P
    d.close()


def test_refusals_in_the_documented_order(hip):
    d, lp = _case_handle(hip, "heading_not_wrapped", 6)
    lib, h, n = hip.load(), d._h, 3
    cnt = np.zeros(n, dtype=np.int32)
    pc_ = cnt.ctypes.data_as(C.POINTER(C.c_int))
    before = (d.sigma_block(np.arange(9), np.arange(9)), d.state_block(0, 9), d.pending, d.live)

    def call(hh=h, lidar=lp, out=pc_, first=0, count=n, tol_abs=0.05, kappa=0.0):
        st = lib.ekf_dense64_scan_evidence(hh, None, C.byref(lidar) if lidar is not None else None, None, first, count,
                                           tol_abs, kappa, out, None, None, None, None, None, None, None, None, None)
        return st, lib.ekf_last_error()

    def lidar(**kw):
        nb, rmax, border, radius = ev.CASES["heading_not_wrapped"]["lidar"]
        base = dict(n_beams=nb, range_max=rmax, border_width=border, tube_radius=radius)
        base.update(kw)
        return hip.default_lidar(**base)

    nan, inf = float("nan"), float("inf")
    # each call breaks rule k and rules behind it: the message names rule k
    steps = [
        (dict(hh=None, out=None, count=0), b"null handle or lidar"),
        (dict(lidar=None, out=None, count=0), b"null handle or lidar"),
        (dict(out=None, count=0, lidar=lidar(n_beams=0)), b"every output is NULL"),
        (dict(count=0, lidar=lidar(n_beams=0, model=1)), b"count >= 1"),
        (dict(first=-1, lidar=lidar(n_beams=0, model=1)), b"count >= 1"),
        (dict(count=n + 1, lidar=lidar(n_beams=0, model=1)), b"inside the live dimension"),
        (dict(first=1, lidar=lidar(n_beams=0, model=1)), b"inside the live dimension"),
        (dict(lidar=lidar(n_beams=0, tube_radius=-1.0, model=1)), b"n_beams"),
        (dict(lidar=lidar(n_beams=1025, tube_radius=-1.0, model=1)), b"n_beams"),
        (dict(lidar=lidar(tube_radius=0.0, model=1), tol_abs=-1.0), b"tube_radius and range_max"),
        (dict(lidar=lidar(tube_radius=nan, model=1), tol_abs=-1.0), b"tube_radius and range_max"),
        (dict(lidar=lidar(range_max=inf, model=1), tol_abs=-1.0), b"tube_radius and range_max"),
        (dict(lidar=lidar(model=1), tol_abs=-1.0), b"tol_abs and kappa"),
        (dict(lidar=lidar(model=1), tol_abs=nan), b"tol_abs and kappa"),
        (dict(lidar=lidar(model=1), kappa=-0.5), b"tol_abs and kappa"),
        (dict(lidar=lidar(model=1), kappa=nan), b"tol_abs and kappa"),
        (dict(lidar=lidar(model=1)), b"model 0"),
    ]
    for kw, text in steps:
        st, msg = call(**kw)
        assert st == 1 and text in msg, (kw, msg)
    after = (d.sigma_block(np.arange(9), np.arange(9)), d.state_block(0, 9), d.pending, d.live)
    assert _same(before[0], after[0]) and _same(before[1], after[1]) and before[2:] == after[2:]
    assert not cnt.any()
    assert call()[0] == 0
    d.close()


def _spelled_removal(d, i, known, grow):
    """INTEGRATION.md, "Removing a landmark", with the public calls -> known, moved_from"""
    last = known - 1
    if i != last:
        d.swap_blocks(3 + 2 * i, 3 + 2 * last, 2)
    d.init_block(3 + 2 * last, W=100.0 * np.eye(2))
    if grow:
        d.live = 3 + 2 * last
    return last, (last if i != last else -1)


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("i", [0, 3, 6])
def test_remove_landmark_is_the_spelled_recipe(hip, i, carry):
    """a landmark in mid-map and the last one (which moves nothing); with carry on the swap and the re-initialisation carry
    the pending rows, with carry off they are applied; the live dimension follows with LM_GROW_LIVE"""
    known = 7
    P = 3 + 2 * known
    state, Sigma = pc.random_family(known, P + 6, 77)
    Sigma[P:, :P] = 0.0
    Sigma[:P, P:] = 0.0
    hs = []
    for _ in range(2):
        h = hip.DensePropagator64(len(state))
        h.set(Sigma=Sigma)
        h.state = state
        h.live = P
        h.carry = carry
        h.correct_sparse_deferred(*pc.merge_operands(state, 2, 3, 0.25))
        hs.append(h)
    d, twin = hs
    grow = not carry
    got = d.remove_landmark(i, known, d.LM_GROW_LIVE if grow else 0)[:2]
    want = _spelled_removal(twin, i, known, grow)
    assert got == want and got[1] == (-1 if i == known - 1 else known - 1)
    assert d.live == twin.live == (P - 2 if grow else P) and d.pending == twin.pending == (2 if carry else 0)
    every = np.arange(d.N)
    assert _same(d.sigma_block(every, every), twin.sigma_block(every, every)) and _same(d.state, twin.state)
    assert _same(d.sigma, twin.sigma)
    for h in hs:
        h.close()


def test_merge_keeps_the_spelled_sequence(hip):
    """merge_landmarks runs its removal through the function remove_landmark shares: still the spelled sequence in bits"""
    from test_gpu_dense64_pairs import _spelled_merge
    known = 7
    P = 3 + 2 * known
    state, Sigma = pc.random_family(known, P + 6, 77)
    Sigma[P:, :P] = 0.0
    Sigma[:P, P:] = 0.0
    hs = []
    for _ in range(2):
        h = hip.DensePropagator64(len(state))
        h.set(Sigma=Sigma)
        h.state = state
        h.live = P
        hs.append(h)
    d, twin = hs
    got = d.merge_landmarks(1, 0, 0.5, known, d.LM_GROW_LIVE)[:3]
    want = _spelled_merge(twin, 1, 0, 0.5, known, False, True)
    assert got[:2] == want[:2] and _bits(got[2]) == _bits(want[2])
    assert d.live == twin.live == P - 2 and _same(d.sigma, twin.sigma) and _same(d.state, twin.state)
    for h in hs:
        h.close()


def test_filter_prunes_a_planted_landmark(hip):
    """DenseEKFSLAM on the evidence alone: three landmarks initialised by data_association at their true places, a fourth
    where nothing stands; scans of the true world take the fourth below the threshold and prune() removes exactly it"""
    world = np.array([[1.0, 0.2], [-0.3, 1.1], [-0.8, -0.7]])
    ghost = np.array([[0.7, -0.9]])
    f = hip.DenseEKFSLAM(6)
    f.data_association(np.vstack([world, ghost]))   # (pose 0: the readings are the positions)
    assert f.known == 4 and len(f.logodds) == 4 and not f.logodds.any()
    lp = _lidar(hip, 360, 3.5, float("inf"), 0.0762)
    m = ev.np_scan_evidence(np.zeros(3), np.vstack([world, ghost]), 360, 3.5, float("inf"), 0.0762)
    assert min((m["hit"] == i).sum() for i in range(4)) >= 5   # every landmark expects beams: margin of >= 2 over min_beams
    truth = ev.np_scan_evidence(np.zeros(3), world, 360, 3.5, float("inf"), 0.0762)["expected"]
    for k in range(6):
        v = f.scan_evidence(truth + 0.002 * (-1) ** k, lp, kappa=0.0)
        assert list(v) == [1, 1, 1, -1]
    assert np.all(f.logodds[:3] > 2.0) and f.logodds[3] < -3.9
    assert f.prune(-2.0) == [3] and f.known == 3 and len(f.logodds) == 3 and np.all(f.logodds > 2.0)
    assert np.allclose(f.state[3:9], world.reshape(-1))
    f.close()


def test_lifecycle_planted_landmark_and_distant_tube(hip):
    """a DenseEKFSLAM at rest among seven near tubes; add_landmark plants a landmark where nothing stands and the true tube
    at 1.5 m that the circle fit cannot see; 15 seeded noisy scans through scan_association(evidence=True) (kappa > 0: the
    tolerance reads Sigma).  The planted landmark's log-odds fall and prune removes exactly it; the distant tube gains
    log-odds although it is never among the circles; the handle equals a clone the landmark was removed from by the recipe.
    (tests/test_dense64_evidence_host.py: every counter is >= 2 beams from its threshold on the model.)"""
    near, distant, ghost = ev.life_world()
    n_map = 2 + len(near)
    f = hip.DenseEKFSLAM(12)
    W = ev.LIFE_PLANT_W * np.eye(2)
    assert f.add_landmark(ghost, W) == 0 and f.add_landmark(distant, W) == 1 and f.known == 2
    threshold = -2.0
    history = []
    lp = _lidar(hip, *ev.LIFE_LIDAR)
    for k, obs in enumerate(ev.life_scans()):
        centres, assoc = f.scan_association(obs, evidence=True, lidar=lp)
        assert len(centres) == len(near) and f.known == n_map, k
        assert np.hypot(*(centres - distant).T).min() > 0.3 and np.hypot(*(centres - ghost).T).min() > 0.3
        assert list(assoc) == list(range(2, n_map)), (k, assoc)       # every circle went to its own near tube
        evd = f.evidence
        assert np.all(evd.tol >= ev.LIFE_TOL[0]) and np.all(evd.tol <= ev.LIFE_TOL[1]), evd.tol
        e, a, t = ev.life_counts(obs, ev.LIFE_TOL[0])
        want = ev.np_evidence_update(np.zeros(n_map), e, a, t, ev.LIFE_MIN_BEAMS, 0.4, 0.85, -4.0, 4.0)[1]
        got = ev.np_evidence_update(np.zeros(n_map), evd.n_expected, evd.n_agree, evd.n_through, ev.LIFE_MIN_BEAMS,
                                    0.4, 0.85, -4.0, 4.0)[1]
        assert list(got) == list(want) == [-1] + [1] * (n_map - 1), (k, evd.n_expected, evd.n_agree, evd.n_through)
        history.append(f.logodds.copy())
    history = np.array(history)
    print(f"lifecycle: log-odds after {len(history)} scans {np.round(history[-1], 2)}")
    assert np.all(np.diff(history[:, 0]) <= 0) and history[-1, 0] < threshold
    assert np.all(np.diff(history[:, 1]) >= 0) and history[-1, 1] > 2.0       # the distant tube, never among the circles
    assert np.all(history[-1, 1:] > 2.0)
    snap = f.clone()
    assert f.prune(threshold) == [0] and f.known == n_map - 1
    assert np.all(f.logodds > 2.0) and len(f.logodds) == n_map - 1
    # the recipe of INTEGRATION.md on the clone: landmark 0 exchanged with the last, the last dropped
    last = 3 + 2 * (n_map - 1)
    snap.handle.swap_blocks(3, last, 2)
    snap.handle.init_block(last, W=100.0 * np.eye(2))
    assert _same(f.handle.sigma, snap.handle.sigma) and _same(f.handle.state, snap.handle.state)
    assert f.handle.live == snap.handle.live and f.handle.pending == snap.handle.pending == 0
    got = f.state[3:3 + 2 * (n_map - 1)].reshape(-1, 2)
    want = np.vstack([near[-1:], distant[None, :], near[:-1]])
    assert np.abs(got - want).max() < 0.02
    snap.close()
    f.close()
