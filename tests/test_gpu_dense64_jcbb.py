"""GPU: the joint compatibility association of the dense fp64 handle -- ekf_dense64_jcbb_candidates (the candidates of every
reading and the cross blocks W between them), ekf_dense64_associate_jcbb (the search on them, then the initialisation and the
stacked corrections of the joint rule).  The bit-level claims are tested as such: W against the numpy model with the exact fma
on the operands the device built, its diagonal blocks against score_landmarks' S, the candidates' scores against
score_readings, a block at P = 17 against the same block inside a P = 128 run, the whole call against a twin handle driven
by the public calls it is composed of; the decisions and the numbers against the numpy model of dense_jcbb_cases."""
import ctypes as C

import numpy as np
import pytest

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_jcbb_cases as jb
import dense_joint_cases as jc
import dense_landmark_cases as lc
import dense_scan_cases as sc
from parity import FP64_TOL

pytestmark = pytest.mark.gpu
INVALID = 1


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _handle(hip, x, S, pending=0, live=None):
    d = hip.DensePropagator64(len(x))
    d.set(Sigma=S)
    if live is not None:
        d.live = live
    if pending:
        Na = d.live
        chain = dd.integer_chain(Na, "asc", seed=77, shapes=cc.RECIPE[pending], Sigma0=S[:Na, :Na])
        for st in chain["steps"]:
            d.correct_sparse_deferred(st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0])
        assert d.pending == pending
    d.state = x
    return d


def _params(hip, prm):
    p = hip.default_params()
    for name in ("r_meas", "gate_new", "gate_update", "sigma0_landmark"):
        setattr(p, name, getattr(prm, name))
    return p


def _snapshot(d):
    """pending count, then the state (ld,) and Sigma (ld, ld) as they sit in memory behind a flush, padding included"""
    p = d.pending
    S, x = d.padded()
    return p, x, S


def _same(got, want):
    assert got[0] == want[0], (got[0], want[0])
    assert _bits(got[1], want[1]), np.argwhere(got[1] != want[1])[:4]
    assert _bits(got[2], want[2]), np.argwhere(got[2] != want[2])[:4]


def _device_terms(d, z, known, cand, p):
    """per candidate the operands and S the device builds for score_landmarks: cols [P][5], Hc [P][2][5], S [P][2][2]"""
    per = [d.score_landmarks(sx, sy, count=known, want_S=True, want_terms=True, params=p) for sx, sy in z]
    pick = list(zip(cand["reading_of"], cand["lm_of"]))
    return ([per[j][4][0][i] for j, i in pick], [per[j][4][1][i] for j, i in pick], [per[j][1][i] for j, i in pick],
            [per[j][4][2][i] for j, i in pick])


def _check_candidates(d, z, known, gic, p, cand, max_cand=4):
    """the selection against np_select on the device's own scores, cand_nis bit for bit those scores"""
    nis, _, _ = d.score_readings(z, count=known, params=p)
    cand_lm, cand_nis, best, is_new = jb.np_select(nis, gic, max_cand, p.gate_new)
    assert [list(cand["cand_lm"][j][:cand["cand_count"][j]]) for j in range(len(z))] == cand_lm
    reading_of, lm_of, flat = jb.flatten(cand_lm, cand_nis)
    assert _bits(cand["nis"], flat) and list(cand["reading_of"]) == list(reading_of) and list(cand["lm_of"]) == list(lm_of)
    assert _bits(cand["best"], np.array(best)) and list(cand["is_new"]) == is_new and cand["P"] == len(reading_of)
    for j in range(len(z)):
        n = cand["cand_count"][j]
        assert (cand["cand_lm"][j][n:] == -1).all() and np.isinf(cand["cand_nis"][j][n:]).all()
    return nis


def _integer_case(hip):
    x, S, known, z, prm, gic = jb.integer()
    return x, S, known, z, _params(hip, prm), gic


def _ties_case(hip):
    """two landmarks with equal score bits, a NaN candidate, and gate_ic set to the bits of a score of reading 0"""
    x, S, z0 = lc.tie_fixture(12, 2, 7, nan_at=4)
    z = np.array([z0, lc.reading_of(x, 9)])
    p = hip.default_params()
    p.gate_new = 1e9
    d = _handle(hip, x, S)
    nis, _, _ = d.score_readings(z, count=12, params=p)
    d.close()
    row = np.sort(nis[0][~np.isnan(nis[0])])
    assert row[0] == row[1] and np.isnan(nis[0][4])
    return x, S, 12, z, p, float(row[3])                        # the fourth-lowest score is the gate: not a candidate


def _fixture_case(hip, name):
    x, S, known, z, prm, gic, _ = getattr(jb, name)()
    return x, S, known, z, _params(hip, prm), gic


CASES = {"integer": _integer_case, "ties": _ties_case, "crossed": lambda hip: _fixture_case(hip, "crossed"),
         "spurious": lambda hip: _fixture_case(hip, "spurious")}


# ---- 1. W on the device --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["integer", "ties", "crossed", "spurious"])
def test_cross_blocks_against_the_model(hip, name):
    x, S, known, z, p, gic = CASES[name](hip)
    d = _handle(hip, x, S)
    cand = d.jcbb_candidates(z, known, gic, params=p)
    nis = _check_candidates(d, z, known, gic, p, cand)
    P = cand["P"]
    assert P >= 3
    cols, Hc, S_out, nu = _device_terms(d, z, known, cand, p)
    want = jb.np_cross(S, cols, Hc, p.r_meas)
    if name == "integer":                                       # exact in any order: a wrong index, not a wrong order
        H = np.zeros((2 * P, len(x)))
        for q in range(P):
            H[2 * q:2 * q + 2, cols[q]] = Hc[q]
        assert np.array_equal(want, H @ S @ H.T + p.r_meas * np.eye(2 * P))
        assert np.array_equal(cand["W"], want) and not np.array_equal(want, want.T)
    else:
        assert _bits(cand["W"], want), np.argwhere(cand["W"] != want)[:4]
    for q in range(P):                                          # the diagonal blocks are the scoring kernel's S
        assert _bits(cand["W"][2 * q:2 * q + 2, 2 * q:2 * q + 2], S_out[q]), q
    assert _bits(cand["nu"], np.array(nu))
    if name == "ties":
        lm0 = list(cand["cand_lm"][0][:cand["cand_count"][0]])
        assert lm0 == [2, 7] + lm0[2:] and 4 not in lm0 and cand["cand_count"][0] == 3   # the exact-gate entry is left out
        assert float(np.sort(nis[0][~np.isnan(nis[0])])[3]) == gic
    d.close()


def _dense_map(n_lm, seed=5):
    """landmarks on a ring 4 .. 6 m out and a full covariance: SPD plus a small part that is not symmetric"""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n_lm) / n_lm
    r = 4.0 + 2.0 * rng.random(n_lm)
    x = np.concatenate([[0.1, 0.2, -0.1], np.stack([r * np.cos(a), r * np.sin(a)], axis=1).reshape(-1)])
    N = len(x)
    A = rng.standard_normal((N, N))
    return x, 0.01 * (A @ A.T / N + np.eye(N)) + 1e-6 * rng.standard_normal((N, N))


@pytest.fixture(scope="module")
def big_run(hip):
    """P = 128 on a 40-landmark handle: 32 readings, 4 candidates each under a loose gate"""
    x, S = _dense_map(40)
    z = np.array([lc.reading_of(x, i, (0.03, -0.02)) for i in range(32)])
    p = hip.default_params()
    p.gate_new = 1e12
    d = _handle(hip, x, S)
    cand = d.jcbb_candidates(z, 40, 1e11, 4, params=p)
    assert cand["P"] == 128
    return x, S, z, p, d, cand


def test_cross_blocks_at_p_128(hip, big_run):
    x, S, z, p, d, cand = big_run
    assert d.jcbb_launch_info() == (16, 256)
    _check_candidates(d, z, 40, 1e11, p, cand)
    cols, Hc, S_out, _ = _device_terms(d, z, 40, cand, p)
    W = cand["W"]
    for q in range(128):
        assert _bits(W[2 * q:2 * q + 2, 2 * q:2 * q + 2], S_out[q]), q
    some = [0, 15, 16, 17, 63, 64, 111, 112, 127]               # both sides of the tile edges, the last tile's corner
    want = jb.np_cross(S, [cols[q] for q in some], [Hc[q] for q in some], p.r_meas)
    rows = np.array([2 * q + a for q in some for a in range(2)])
    assert _bits(W[np.ix_(rows, rows)], want)


@pytest.mark.parametrize("P", [1, 16, 17])
def test_cross_blocks_do_not_depend_on_the_run(hip, big_run, P):
    """P readings with one candidate each: the blocks of the P = 128 run at those candidates, bit for bit, and the model"""
    x, S, z, p, d, big = big_run
    cand = d.jcbb_candidates(z[:P], 40, 1e11, 1, params=p)
    assert cand["P"] == P and list(cand["lm_of"]) == [big["lm_of"][4 * j] for j in range(P)]
    rows = np.array([8 * j + a for j in range(P) for a in range(2)])
    assert _bits(cand["W"], big["W"][np.ix_(rows, rows)])
    cols, Hc, _, _ = _device_terms(d, z[:P], 40, cand, p)
    assert _bits(cand["W"], jb.np_cross(S, cols, Hc, p.r_meas))


# ---- 2. read-only ---------------------------------------------------------------------------------------------------------------

def _live_case(hip, name="crossed"):
    """N = 135 with live = 131: 64 landmarks inside the live corner, two beyond it"""
    x, S, _, z, prm, gic, truth = getattr(jb, name)(66)
    return x, S, 64, z, _params(hip, prm), gic, truth


def test_candidates_are_read_only(hip):
    x, S, known, z, p, gic, _ = _live_case(hip)
    d = _handle(hip, x, S, live=131)
    before = d.padded()                                         # the slack beyond live and beyond N included
    cand = d.jcbb_candidates(z, known, gic, params=p)
    assert cand["P"] == 3 and d.pending == 0 and d.live == 131
    after = d.padded()
    assert _bits(after[0], before[0]) and _bits(after[1], before[1])
    a, b = _handle(hip, x, S, 2, live=131), _handle(hip, x, S, 2, live=131)
    b.flush()
    ca, cb = a.jcbb_candidates(z, known, gic, params=p), b.jcbb_candidates(z, known, gic, params=p)
    assert a.pending == 0
    for key in ("cand_count", "cand_lm", "cand_nis", "best", "is_new", "W", "nu"):
        assert _bits(ca[key], cb[key]), key
    _same(_snapshot(a), _snapshot(b))
    for h in (d, a, b):
        h.close()


def test_candidates_refusals(hip):
    x, S, known, z, p, gic, _ = _live_case(hip)
    d = _handle(hip, x, S, 2, live=131)
    for args in ((z, 65, gic), (z, known, 0.0), (z, known, float("nan")), (z, known, 2 * p.gate_new), (z, -1, gic)):
        with pytest.raises(hip.EkfError) as e:
            d.jcbb_candidates(*args, params=p)
        assert e.value.status == INVALID
    with pytest.raises(hip.EkfError) as e:
        d.associate_jcbb(z, known, 66, gic, gate_joint=[1.0, -1.0], params=p)
    assert e.value.status == INVALID and e.value.known == known
    with pytest.raises(hip.EkfError) as e:
        d.associate_jcbb(z, known, 66, gic, max_nodes=0, params=p)
    assert e.value.status == INVALID and d.pending == 2         # nothing was flushed by a refused call
    d.close()


# ---- 3. the twin ------------------------------------------------------------------------------------------------------------------

def _twin_jcbb(hip, make, twin, z, known, n_max, gic, deferred, grow, p, max_nodes=1 << 16):
    """the call replayed on `twin` with the public calls it is composed of: jcbb_candidates, jcbb_search, init_block per
    group of 32, joint_operands + correct_sparse[_deferred] + the heading per group of 30.  The new landmarks' positions
    come from a third handle on which the call only initialises (gate_update = 0): init_block takes them as bits, and only the
    device's own initialize_landmark gives those bits, so for NEW readings the twin is not independent of the call under
    test.  What makes up for it: xb is held to ic.inverse_sensor at the pose read back within 1e-12 here, and the tests
    compare the whole call with the numpy model within FP64_TOL -> known, assoc, report"""
    J = len(z)
    cand = twin.jcbb_candidates(z, known, gic, params=p)
    assign, rep = hip.DensePropagator64.jcbb_search(J, cand["reading_of"], cand["lm_of"], cand["nis"], cand["W"], cand["nu"],
                                                    jb.default_gates(J, gic), max_nodes)
    kinds, lms, slot = [jc.DROP] * J, [-1] * J, known
    for j in range(J):
        if assign[j] >= 0:
            kinds[j], lms[j] = jc.MATCH, int(cand["lm_of"][assign[j]])
        elif cand["is_new"][j] and slot < n_max:
            kinds[j], lms[j], slot = jc.NEW, slot, slot + 1
    fresh = [j for j, k in enumerate(kinds) if k == jc.NEW]
    if fresh:
        q = _params(hip, p)
        q.gate_update = 0.0
        third = make()
        # (only the readings that become landmarks: they are NEW whatever else the scan holds, and take the same slots)
        k3, a3, _, r3, g3, _ = third.associate_jcbb(z[fresh], known, n_max, gic, None, max_nodes, deferred, grow, params=q)
        assert k3 == known + len(fresh) and (a3 == -1).all() and g3 == 0 and r3["n_new"] == len(fresh)
        xb = third.state_block(3 + 2 * known, 2 * len(fresh))
        third.close()
        want = np.concatenate([ic.inverse_sensor(twin.state_block(0, 3), *z[j]) for j in fresh])
        assert np.abs(xb - want).max() <= 1e-12
        if grow and twin.live < 3 + 2 * (known + len(fresh)):
            twin.live = 3 + 2 * (known + len(fresh))
        for g in range(0, len(fresh), jc.INIT_GROUP):
            n = min(jc.INIT_GROUP, len(fresh) - g)
            twin.init_block(3 + 2 * (known + g), W=p.sigma0_landmark * np.eye(2 * n), xb=xb[2 * g:2 * (g + n)])
        known += len(fresh)
    assoc = np.full(J, -1, dtype=np.int32)
    for grp in jc.groups_of(jc.pairs_of(kinds, lms, p.gate_update)):
        cols, Hc, nu, _ = twin.joint_operands([i for _, i in grp], [z[j] for j, _ in grp], params=p)
        (twin.correct_sparse_deferred if deferred else twin.correct_sparse)(cols, Hc, p.r_meas * np.eye(2 * len(grp)), nu)
        lc.wrap_heading_always(twin)
        for j, i in grp:
            assoc[j] = i
    rep.update(n_new=len(fresh), n_drop=J - rep["n_pairs"] - len(fresh))
    return known, assoc, rep


def _close(model, got):
    assert np.abs(got - model).max() <= FP64_TOL * max(1.0, np.abs(model).max())


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("name", ["crossed", "spurious"])
def test_jcbb_twin_and_model(hip, name, deferred):
    x, S, known, z, p, gic, truth = _live_case(hip, name)
    make = lambda: _handle(hip, x, S, live=131)
    d, twin = make(), make()
    k, assoc, best, rep, ng, _ = d.associate_jcbb(z, known, 66, gic, deferred=deferred, params=p)
    k2, assoc2, rep2 = _twin_jcbb(hip, make, twin, z, known, 66, gic, deferred, False, p)
    assert k == k2 == known and list(assoc) == list(assoc2) == truth and rep == rep2 and ng == 1
    assert d.pending == (2 * sum(t >= 0 for t in truth) if deferred else 0) == twin.pending
    _same(_snapshot(d), _snapshot(twin))
    m = jc.numpy_handle(x[:131], S[:131, :131])
    km, am, bm, repm, ngm = jb.np_associate_jcbb(m, p, z, known, 64, gic)
    assert km == k and list(am) == list(assoc) and ngm == ng
    assert {key: rep[key] for key in repm if key != "d2"} == {key: repm[key] for key in repm if key != "d2"}
    assert abs(rep["d2"] - repm["d2"]) <= 1e-6 * repm["d2"]
    _close(bm, best)
    _close(m.state, d.state[:131])
    _close(m.sigma, d.sigma[:131, :131])
    for h in (d, twin):
        h.close()


@pytest.mark.parametrize("mode", ["eager", "deferred", "eager_grow", "deferred_grow"])
def test_jcbb_twin_and_model_on_the_scan_fixture(hip, mode):
    """ticks of 8 seen landmarks and one object nobody knows: matches and a new landmark per call"""
    deferred, grow = mode.startswith("deferred"), mode.endswith("grow")
    x, S, known, steps = jc.scan_fixture(ticks=3)
    n_max = (len(x) - 3) // 2
    p = hip.default_params()
    d, twin = (_handle(hip, x, S, live=3 + 2 * known if grow else None) for _ in range(2))
    m = jc.numpy_handle(x, S)
    kd = kt = km = known
    for dth, dx, z in steps:
        for h in (d, twin):
            h.predict_landmarks(dth, dx)
        Fr, Qr, upd = bc.model_operands(m.state_block(0, 3), dth, dx)
        m.propagate_block(0, Fr, Qr, upd)
        # (called behind the twin's jcbb_candidates, which has applied the pending rows: reading Sigma moves nothing)
        make = lambda: _handle(hip, twin.state, twin.sigma, live=twin.live)
        k0 = kd
        kd, assoc, best, rep, ng, _ = d.associate_jcbb(z, kd, n_max, 1.0, deferred=deferred, grow_live=grow)
        kt, assoc2, rep2 = _twin_jcbb(hip, make, twin, z, kt, n_max, 1.0, deferred, grow, p)
        assert kd == kt == k0 + 1 and list(assoc) == list(assoc2) and rep == rep2 and ng == 1
        assert sorted(assoc)[:8] == [0, 1, 2, 3, 5, 6, 8, 9] and assoc[8] == k0 and rep["n_new"] == 1 and rep["n_pairs"] == 8
        assert d.pending == twin.pending and d.live == twin.live
        assert _bits(d.state, twin.state)
        km, am, bm, repm, _ = jb.np_associate_jcbb(m, None, z, km, n_max, 1.0)
        assert km == kd and list(am) == list(assoc)
        assert {key: rep[key] for key in repm if key != "d2"} == {key: repm[key] for key in repm if key != "d2"}
    _same(_snapshot(d), _snapshot(twin))
    n = 3 + 2 * kd
    _close(m.state[:n], d.state[:n])
    _close(m.sigma[:n, :n], d.sigma[:n, :n])
    for h in (d, twin):
        h.close()


# ---- 4. behaviour -----------------------------------------------------------------------------------------------------------------

def test_crossed_is_paired_as_the_truth_and_not_by_the_per_reading_rule(hip):
    x, S, known, z, p, gic, truth = _fixture_case(hip, "crossed") + ([0, 1],)
    d, clone = _handle(hip, x, S), _handle(hip, x, S)
    k, assoc, _, rep, _, _ = d.associate_jcbb(z, known, known, gic, params=p)
    assert list(assoc) == truth and k == known and rep["n_pairs"] == 2 and rep["exhausted"] == 0
    k2, assoc2, _, _, _ = clone.associate_joint(z, known, known, params=p)
    assert list(assoc2) != truth and list(assoc2) == [1, -1]
    for h in (d, clone):
        h.close()


def test_spurious_reading_is_left_out_and_is_no_new_landmark(hip):
    x, S, known, z, p, gic = _fixture_case(hip, "spurious")
    d = _handle(hip, x[:3 + 2 * 8], S[:3 + 2 * 8, :3 + 2 * 8])
    k, assoc, best, rep, _, _ = d.associate_jcbb(z, 6, 8, gic, params=p)    # two free slots: a NEW reading would take one
    assert list(assoc) == [0, 1, 2, -1] and k == 6 and best[3] < gic
    assert (rep["n_pairs"], rep["n_new"], rep["n_drop"], rep["n_cand"]) == (3, 0, 1, 4)
    d.close()


def test_nothing_known_makes_every_reading_new(hip):
    x, S = lc.spiral_map(12)
    d = _handle(hip, x, S, live=3)
    z = np.array([lc.reading_of(x, i) for i in (0, 3, 5)])
    k, assoc, best, rep, ng, _ = d.associate_jcbb(z, 0, 12, 1.0, grow_live=True)
    assert k == 3 and list(assoc) == [0, 1, 2] and (best == 10.0).all() and ng == 1 and d.live == 9
    assert (rep["n_cand"], rep["n_pairs"], rep["n_new"], rep["n_drop"], rep["nodes"]) == (0, 0, 3, 0, 4)
    d.close()


def test_associate_joint_is_unmoved_by_jcbb_calls_on_the_handle(hip):
    x, S, known, steps = jc.scan_fixture(ticks=1)
    n_max = (len(x) - 3) // 2
    dth, dx, z = steps[0]
    a, b = _handle(hip, x, S), _handle(hip, x, S)
    for h in (a, b):
        h.predict_landmarks(dth, dx)
    b.jcbb_candidates(z, known, 1.0)
    clone = hip.DensePropagator64(len(x))
    clone.extract_map(b)                                        # every bit of b's map; b is unchanged
    assert _bits(clone.state, b.state) and _bits(clone.sigma, b.sigma)
    clone.associate_jcbb(z, known, n_max, 1.0)
    ra, rb = a.associate_joint(z, known, n_max), b.associate_joint(z, known, n_max)
    assert ra[0] == rb[0] and list(ra[1]) == list(rb[1]) and _bits(ra[2], rb[2]) and ra[3] == rb[3]
    _same(_snapshot(a), _snapshot(b))
    for h in (a, b, clone):
        h.close()


# ---- 5. a scan as the input, and the object's spellings ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["eager", "deferred_grow"])
@pytest.mark.parametrize("circles,max_readings", [(0, 32), (3, 32), (3, 8), (3, 1)])
def test_associate_scan_jcbb_twin(hip, mode, circles, max_readings):
    """fit_scan followed by associate_jcbb on a twin, bit for bit; gate_joint holds max_readings entries of which the call
    reads the first count"""
    n, known0 = 10, 4
    x, S = lc.spiral_map(n)                                     # N = 23
    x[3:5] = x[:3][1:] + np.array([1.25, 0.0])                  # landmark 0 near where the first tube is seen
    deferred = grow = mode != "eager"
    live = 3 + 2 * known0 if grow else None
    a, b, c = (_handle(hip, x, S, 2 if deferred else 0, live) for _ in range(3))
    r = sc.circles_scan(circles)
    gates = 1.5 * np.arange(1, max_readings + 1)
    ka, cen, assoc, best, rep = a.associate_scan_jcbb(r, known0, n, max_readings, 1.0, gates, 1 << 12, deferred, grow,
                                                      want_report=True)
    cen_b, _, _ = b.fit_scan(r, max_out=max_readings)
    want = min(circles, max_readings)
    assert len(cen) == len(assoc) == len(best) == want and _bits(cen, cen_b)
    kb = known0
    if want:
        kb, assoc_b, best_b, rep_b, _, _ = b.associate_jcbb(cen_b, known0, n, 1.0, gates[:want], 1 << 12, deferred, grow)
        assert _bits(assoc, assoc_b) and _bits(best, best_b) and rep == rep_b, (assoc, assoc_b, rep, rep_b)
        assert (assoc >= 0).any() and not _bits(a.state, x) and rep["n_pairs"] + rep["n_new"] + rep["n_drop"] == want
    else:
        assert _bits(a.state, x) and rep["nodes"] == 0 and rep["n_cand"] == 0   # nothing of the filter was written
    assert ka == kb and a.live == b.live
    # the same call through the C ABI with every nullable output NULL but the time: the legs' times join the fit's
    k, cnt, ms = C.c_int(known0), C.c_int(-1), C.c_double(-1.0)
    flags = (c.LM_DEFERRED | c.LM_GROW_LIVE) if deferred else 0
    rr = np.ascontiguousarray(r, dtype=np.float64)
    st = c._lib.ekf_dense64_associate_scan_jcbb(c._h, None, rr.ctypes.data_as(C.POINTER(C.c_double)), len(rr), max_readings, n,
                                                C.byref(k), 1.0, gates.ctypes.data_as(C.POINTER(C.c_double)), 1 << 12, flags,
                                                C.byref(cnt), None, None, None, None, C.byref(ms))
    assert st == 0 and k.value == ka and cnt.value == want and ms.value > 0.0
    got = _snapshot(a)
    _same(got, _snapshot(b))
    _same(got, _snapshot(c))
    for h in (a, b, c):
        h.close()


def test_dense_ekf_slam_jcbb_association(hip):
    """the object's spellings: jcbb_association(readings) with its report, scan_association(ranges, joint="jcbb"), and the
    meanings joint=False / True had before"""
    x, S, known, z, prm, gic, truth = jb.crossed()
    n = (len(x) - 3) // 2
    slam = hip.DenseEKFSLAM(n, params=_params(hip, prm))
    assert slam.jcbb_report is None
    slam.handle.set(Sigma=S)
    slam.handle.state = x
    slam._known = known
    twin = _handle(hip, x, S)
    assoc = slam.jcbb_association(z, gate_ic=gic)
    k2, assoc2, _, rep2, _, _ = twin.associate_jcbb(z, known, n, gic, params=_params(hip, prm))
    assert list(assoc) == truth == list(assoc2) and slam.known == known == k2 and slam.jcbb_report == rep2
    assert slam.jcbb_report["n_pairs"] == 2 and slam.jcbb_report["exhausted"] == 0
    _same(_snapshot(slam.handle), _snapshot(twin))
    slam.close(); twin.close()
    ring = np.stack([8.0 * np.cos(0.1 + 2.1 * np.arange(3)), 8.0 * np.sin(0.1 + 2.1 * np.arange(3))], axis=1)
    r = sc.circles_scan(3)
    runs = {}
    for joint in (False, True, "jcbb"):
        slam = hip.DenseEKFSLAM(12)
        assert list(slam.jcbb_association(ring)) == [0, 1, 2] and slam.known == 3       # nothing known: three new landmarks
        assert (slam.jcbb_report["n_new"], slam.jcbb_report["n_cand"], slam.jcbb_report["nodes"]) == (3, 0, 4)
        slam.jcbb_report = "stale"
        cen, assoc = slam.scan_association(r, joint=joint)
        assert len(cen) == len(assoc) == 3 and slam.known <= 12
        if joint == "jcbb":
            rep = slam.jcbb_report
            assert rep["n_pairs"] + rep["n_new"] + rep["n_drop"] == 3 and rep["nodes"] >= 4
        else:
            assert slam.jcbb_report == "stale"                  # the other two spellings do not touch it
        runs[joint] = (slam.known, cen, assoc, _snapshot(slam.handle))
        with pytest.raises(ValueError):
            slam.scan_association(r, joint="other")
        slam.close()
    # joint=False / True are what the handle's two calls give, as before
    for joint, call in ((False, "associate_scan"), (True, "associate_scan_joint")):
        ref = hip.DenseEKFSLAM(12)
        ref.jcbb_association(ring)
        k, cen, assoc, _ = getattr(ref.handle, call)(r, 3, 12)
        assert k == runs[joint][0] and _bits(cen, runs[joint][1]) and _bits(assoc, runs[joint][2])
        _same(_snapshot(ref.handle), runs[joint][3])
        ref.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_jcbb_refusals_change_nothing(hip):
    """every INVALID case of the three calls through the C ABI on a live handle with rows pending, each with the fault of
    the check behind it as well: the first of two faults is the one reported, and nothing changes"""
    count, known = 20, 10
    x, S = lc.spiral_map(count)
    live = 3 + 2 * 12
    d, ref = _handle(hip, x, S, 2, live=live), _handle(hip, x, S, 2, live=live)
    lib, h = d._lib, d._h
    dp = C.POINTER(C.c_double)
    z = (C.c_double * 66)(*lc.reading_of(x, 3), *lc.reading_of(x, 4))
    k = C.c_int(known)
    good, neg, nan_g = (C.c_double * 32)(*[1.0 + j for j in range(32)]), (C.c_double * 32)(*([1.0] * 32)), (C.c_double * 32)(*([1.0] * 32))
    neg[1], nan_g[0] = -1.0, float("nan")
    last_bad = (C.c_double * 32)(*([1.0] * 32))
    last_bad[31] = 0.0
    inf, nan, BIG = float("inf"), float("nan"), (1 << 22) + 1
    assoc, best, rep, ng = (C.c_int * 32)(*([7] * 32)), (C.c_double * 32)(), hip.JcbbReport(), C.c_int(-5)
    rep.nodes = -9

    def refused(res, text):
        assert res == INVALID and text in lib.ekf_last_error(), (res, lib.ekf_last_error())

    def jcbb(hh, J, zz, n_max, kk, gic, gj, nodes, flags):
        return lib.ekf_dense64_associate_jcbb(hh, None, J, zz, n_max, kk, gic, gj, nodes, flags, assoc, best, C.byref(rep),
                                              C.byref(ng), None)
    kb = lambda v: C.byref(C.c_int(v))
    refused(jcbb(None, 0, None, -1, None, 0.0, neg, 0, 4), b"null handle")
    refused(jcbb(h, 0, None, -1, C.byref(k), 0.0, neg, 0, 4), b"null argument")
    refused(jcbb(h, 0, z, -1, None, 0.0, neg, 0, 4), b"null argument")
    refused(jcbb(h, 0, z, -1, C.byref(k), 0.0, neg, 0, 4), b"J must lie")
    refused(jcbb(h, 33, z, -1, C.byref(k), 0.0, neg, 0, 4), b"J must lie")
    refused(jcbb(h, 2, z, -1, C.byref(k), 0.0, neg, 0, 4), b"n_max must lie")
    refused(jcbb(h, 2, z, count + 1, C.byref(k), 0.0, neg, 0, 4), b"n_max must lie")
    for bad in (-1, count + 1):
        refused(jcbb(h, 2, z, count, kb(bad), 0.0, neg, 0, 4), b"*known must lie")
    refused(jcbb(h, 2, z, count, kb(13), 0.0, neg, 0, 4), b"inside the live dimension")       # 3 + 2 * 13 > live
    refused(jcbb(h, 2, z, count, C.byref(k), 0.0, neg, 0, 4), b"unknown flag bits")
    refused(jcbb(h, 2, z, count, C.byref(k), 0.0, neg, 0, 8), b"unknown flag bits")           # the Joseph form: as associate_joint
    for gic in (0.0, -1.0, nan, inf, 10.5):                                                    # gate_new = 10
        refused(jcbb(h, 2, z, count, C.byref(k), gic, neg, 0, 0), b"gate_ic must be")
    for gj in (neg, nan_g):
        refused(jcbb(h, 2, z, count, C.byref(k), 1.0, gj, 0, 0), b"every joint gate")
    for nodes in (0, -1, BIG):
        refused(jcbb(h, 2, z, count, C.byref(k), 1.0, good, nodes, 0), b"max_nodes must lie")
        refused(jcbb(h, 2, z, count, C.byref(k), 1.0, None, nodes, 1), b"max_nodes must lie")
    assert list(assoc) == [7] * 32 and ng.value == -5 and rep.nodes == -9 and k.value == known

    out = (C.c_int * 128)()
    def cand(hh, J, zz, kn, gic, mc, first_out=out):
        return lib.ekf_dense64_jcbb_candidates(hh, None, J, zz, kn, gic, mc, first_out, None, None, None, None, None, None,
                                               None, None)
    refused(cand(None, 0, None, -1, 0.0, 0), b"null handle")
    refused(cand(h, 0, None, -1, 0.0, 0), b"null argument")
    refused(cand(h, 0, z, -1, 0.0, 0), b"J must lie")
    refused(cand(h, 33, z, -1, 0.0, 0), b"J must lie")
    refused(cand(h, 2, z, -1, 0.0, 0), b"inside the live dimension")
    refused(cand(h, 2, z, 13, 0.0, 0), b"inside the live dimension")
    for gic in (0.0, nan, inf, 10.5):
        refused(cand(h, 2, z, known, gic, 0), b"gate_ic must be")
    for mc in (0, 5, -1):
        refused(cand(h, 2, z, known, 1.0, mc, None), b"max_cand must lie")
    refused(cand(h, 2, z, known, 1.0, 4, None), b"every output is NULL")

    r = (C.c_double * 360)(*sc.circles_scan(3))
    cnt = C.c_int(-7)
    def scan(hh, rr, nb, mr, n_max, kk, gic, gj, nodes, flags, ccnt):
        return lib.ekf_dense64_associate_scan_jcbb(hh, None, rr, nb, mr, n_max, kk, gic, gj, nodes, flags, ccnt, None, assoc,
                                                   best, C.byref(rep), None)
    refused(scan(None, None, 0, 0, -1, None, 0.0, neg, 0, 4, None), b"null handle")
    refused(scan(h, None, 0, 0, -1, C.byref(k), 0.0, neg, 0, 4, C.byref(cnt)), b"null argument")
    refused(scan(h, r, 0, 0, -1, None, 0.0, neg, 0, 4, C.byref(cnt)), b"null argument")
    refused(scan(h, r, 0, 0, -1, C.byref(k), 0.0, neg, 0, 4, None), b"null argument")
    refused(scan(h, r, 0, 32, -1, C.byref(k), 0.0, neg, 0, 4, C.byref(cnt)), b"n_beams must lie")
    refused(scan(h, r, 1025, 32, -1, C.byref(k), 0.0, neg, 0, 4, C.byref(cnt)), b"n_beams must lie")
    for mr in (0, 33):                                                                         # 33 .. 128 are the joint call's
        refused(scan(h, r, 360, mr, -1, C.byref(k), 0.0, neg, 0, 4, C.byref(cnt)), b"n_beams must lie")
    refused(scan(h, r, 360, 32, -1, C.byref(k), 0.0, neg, 0, 4, C.byref(cnt)), b"n_max must lie")
    refused(scan(h, r, 360, 32, count, kb(count + 1), 0.0, neg, 0, 4, C.byref(cnt)), b"*known must lie")
    refused(scan(h, r, 360, 32, count, kb(13), 0.0, neg, 0, 4, C.byref(cnt)), b"inside the live dimension")
    refused(scan(h, r, 360, 32, count, C.byref(k), 0.0, neg, 0, 4, C.byref(cnt)), b"unknown flag bits")
    for gic in (0.0, nan, 10.5):
        refused(scan(h, r, 360, 32, count, C.byref(k), gic, neg, 0, 0, C.byref(cnt)), b"gate_ic must be")
    refused(scan(h, r, 360, 32, count, C.byref(k), 1.0, neg, 0, 0, C.byref(cnt)), b"every joint gate")
    refused(scan(h, r, 360, 32, count, C.byref(k), 1.0, last_bad, 0, 0, C.byref(cnt)), b"every joint gate")   # all max_readings
    for nodes in (0, BIG):
        refused(scan(h, r, 360, 32, count, C.byref(k), 1.0, good, nodes, 0, C.byref(cnt)), b"max_nodes must lie")
    assert k.value == known and cnt.value == -7 and d.live == live and list(assoc) == [7] * 32 and rep.nodes == -9
    got, want = _snapshot(d), _snapshot(ref)
    assert got[0] == want[0] == 2                                                              # nothing was flushed
    _same(got, want)
    d.close(); ref.close()
