"""GPU: the joint association of the dense fp64 handle -- ekf_dense64_score_readings (all readings of a scan scored in one
call), ekf_dense64_joint_operands (the stacked operands of a group of pairs), ekf_dense64_associate_joint (one assignment, the
new landmarks initialised in groups, stacked corrections) and ekf_dense64_associate_scan_joint.  The bit-level claims are
tested as such: the scores against score_landmarks per reading, the whole call against a twin handle driven by the public
calls it is composed of, one reading per call against associate_landmarks; the numbers against the numpy model of
dense_joint_cases and, for a chain of single readings, against the reference's own data_association()."""
import ctypes as C

import numpy as np
import pytest

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_correct_cases as dc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_joint_cases as jc
import dense_landmark_cases as lc
import dense_scan_cases as sc
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst

pytestmark = pytest.mark.gpu
TOL = 1e-12
INVALID, STATE = 1, 5
PENDING = {2: cc.RECIPE[2], 62: [(17, 5), (17, 5), (17, 5), (11, 5)], 64: cc.RECIPE[64]}   # (m, s) that make p rows


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _handle(hip, x, S, pending=0, carry=False, live=None):
    """a handle with the state x, the covariance S, the live dimension `live` and `pending` rows left by deferred corrections
    of an integer chain inside it; built twice it holds the same bits twice"""
    d = hip.DensePropagator64(len(x))
    d.set(Sigma=S)
    if live is not None:
        d.live = live
    if pending:
        Na = d.live
        chain = dd.integer_chain(Na, "asc", seed=77, shapes=PENDING[pending], Sigma0=S[:Na, :Na])
        for st in chain["steps"]:
            d.correct_sparse_deferred(st["cols"][0], st["Hc"][0], st["R"][0], st["nu"][0])
        assert d.pending == pending and d.live == Na
    d.state = x
    d.carry = carry
    return d


def _snapshot(d):
    """pending count, state, and Sigma after a flush"""
    p = d.pending
    d.flush()
    return p, d.state, d.sigma


def _same(got, want):
    assert got[0] == want[0], (got[0], want[0])
    assert _bits(got[1], want[1]), np.argwhere(got[1] != want[1])[:4]
    assert _bits(got[2], want[2]), np.argwhere(got[2] != want[2])[:4]


def _stale_beyond(S, known):
    S[3 + 2 * known:, :] = 0.0
    S[:, 3 + 2 * known:] = 0.0
    S[3 + 2 * known:, 3 + 2 * known:] = 7.0 * np.eye(S.shape[0] - 3 - 2 * known)


def _ring(k, rad=8.0):
    """k readings far from every landmark of a spiral map and from each other"""
    a = 0.1 + 2 * np.pi * np.arange(k) / k
    return np.stack([rad * np.cos(a), rad * np.sin(a)], axis=1)


# ---- 1. scoring ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pending", [0, 2, 64])
@pytest.mark.parametrize("count", [1, 5, 257])
def test_score_readings_is_score_landmarks_per_reading(hip, count, pending):
    n = max(count, 12)                                                         # (room for the pending chain's lists)
    x, S = lc.spiral_map(n, seed=count)
    d, ref = _handle(hip, x, S, pending), _handle(hip, x, S, pending)
    z = np.array([lc.reading_of(x, (5 * j) % count, (0.01 * j, -0.003 * j)) for j in range(8)])
    want = [d.score_landmarks(sx, sy, count=count) for sx, sy in z]
    for J in (1, 2, 8):
        nis, flags, _ = d.score_readings(z[:J], count=count)
        assert nis.shape == flags.shape == (J, count) and flags.dtype == np.int32
        for j in range(J):
            assert _bits(nis[j], want[j][0]) and _bits(flags[j], want[j][2]), (J, j)
    if count > 2:                                                              # a window of the map
        nis, flags, _ = d.score_readings(z[:2], first_lm=1, count=count - 2)
        assert _bits(nis[1], want[1][0][1:count - 1]) and _bits(flags[1], want[1][2][1:count - 1])
    assert d.pending == pending and _bits(d.state, ref.state)                  # read-only
    _same(_snapshot(d), _snapshot(ref))
    d.close(); ref.close()


def test_score_readings_splits_its_launches(hip):
    """J = 32 readings against 1025 landmarks are 65600 rows: two launches of 31 and 1 readings"""
    count, J = 1025, 32
    x, S = lc.spiral_map(count)
    x[3 + 2 * 700], x[4 + 2 * 700] = x[1], x[2]                                # a flagged candidate in every reading's row
    d = _handle(hip, x, S)
    z = np.array([lc.reading_of(x, 31 * j, (0.01, 0.002 * j)) for j in range(J)])
    nis, flags, _ = d.score_readings(z)
    assert flags[:, 700].all() and flags.sum() == J and np.isnan(nis[:, 700]).all()
    for j in (0, 1, 15, 30, 31):
        n1, _, f1, _ = d.score_landmarks(z[j, 0], z[j, 1])
        assert _bits(nis[j], n1) and _bits(flags[j], f1), j
        assert int(np.nanargmin(nis[j])) == 31 * j
    d.close()


# ---- 2. the stacked operands -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2, 30])
def test_joint_operands(hip, V):
    count = 63
    x, S = lc.spiral_map(count)
    d, ref = _handle(hip, x, S, 2), _handle(hip, x, S, 2)
    lm = [(5 * v + 3) % count for v in range(V)]                               # distinct, in no order
    assert len(set(lm)) == V
    z = np.array([lc.reading_of(x, i, (0.02, -0.01)) for i in lm])
    cols, Hc, nu, _ = d.joint_operands(lm, z)
    wc, wH, wnu = jc.np_joint_operands(x, lm, z)
    assert cols.dtype == np.int32 and np.array_equal(cols, wc)
    assert (Hc != 0).sum() == 9 * V and np.array_equal(Hc != 0, wH != 0)       # (H[0][0] is a zero)
    assert np.abs(Hc - wH).max() <= TOL and np.abs(nu - wnu).max() <= TOL
    if V == 1:                                                                 # the operands of the sequential correction
        _, _, _, _, (c1, H1, u1) = d.score_landmarks(z[0, 0], z[0, 1], first_lm=lm[0], count=1, want_terms=True)
        assert _bits(cols, c1[0]) and _bits(Hc, H1[0])
        assert _bits(nu, np.array([u1[0, 0], dc.normalize_angle(float(u1[0, 1]))]))
    far = lc.reading_of(x, lm[0], (0.0, 0.0))                                  # a bearing that needs its wrap
    x2 = x.copy()
    x2[0] = 3.1
    d.state = x2
    back = (-far[0], -far[1])
    _, _, nu2, _ = d.joint_operands([lm[0]], [back])
    w2 = jc.np_joint_operands(x2, [lm[0]], [back])[2]
    assert abs(nu2[1]) <= np.pi and np.abs(nu2 - w2).max() <= TOL
    d.state = x
    assert d.pending == 2
    _same(_snapshot(d), _snapshot(ref))                                        # read-only
    d.close(); ref.close()


# ---- 3. the twin -----------------------------------------------------------------------------------------------------------------

def _twin_joint(hip, make, twin, z, known, n_max, deferred, grow=False, params=None):
    """the joint call replayed on `twin` with the public calls it is composed of: score_landmarks per reading, the rule on the
    host, init_block per group of 32, joint_operands + correct_sparse[_deferred] + the heading per group of 30.  The new
    landmarks' positions come from a third handle (made by `make`) on which the call only initialises (gate_update = 0).
    -> known, assoc, best, n_groups"""
    p = params if params is not None else hip.default_params()
    nis = [twin.score_landmarks(sx, sy, count=known)[0] if known else [] for sx, sy in z]
    kinds, lms, best = jc.joint_rule(nis, known, n_max, p.gate_new, p.gate_update)
    fresh = [j for j, k in enumerate(kinds) if k == jc.NEW]
    if fresh:
        q = hip.default_params()
        for name in ("sigma0_landmark", "r_meas", "gate_new"):
            setattr(q, name, getattr(p, name))
        q.gate_update = 0.0
        third = make()
        k3, a3, _, g3, _ = third.associate_joint(z, known, n_max, deferred, grow, params=q)
        assert k3 == known + len(fresh) and (a3 == -1).all() and g3 == 0
        xb = third.state_block(3 + 2 * known, 2 * len(fresh))
        want = np.concatenate([ic.inverse_sensor(twin.state_block(0, 3), *z[j]) for j in fresh])
        assert np.abs(xb - want).max() <= TOL
        third.close()
        if grow and twin.live < 3 + 2 * (known + len(fresh)):
            twin.live = 3 + 2 * (known + len(fresh))
        for g in range(0, len(fresh), jc.INIT_GROUP):
            n = min(jc.INIT_GROUP, len(fresh) - g)
            twin.init_block(3 + 2 * (known + g), W=p.sigma0_landmark * np.eye(2 * n), xb=xb[2 * g:2 * (g + n)])
        known += len(fresh)
    assoc = np.full(len(z), -1, dtype=np.int32)
    groups = jc.groups_of(jc.pairs_of(kinds, lms, p.gate_update))
    for grp in groups:
        cols, Hc, nu, _ = twin.joint_operands([i for _, i in grp], [z[j] for j, _ in grp], params=p)
        (twin.correct_sparse_deferred if deferred else twin.correct_sparse)(cols, Hc, p.r_meas * np.eye(2 * len(grp)), nu)
        lc.wrap_heading_always(twin)
        for j, i in grp:
            assoc[j] = i
    return known, assoc, np.array(best), len(groups), kinds


def _between_the_gates(x, S, i, known):
    """a reading of landmark i pushed outwards until numpy's rule drops it with the best score well inside (2, 8)"""
    u = x[3 + 2 * i:5 + 2 * i] - x[1:3]
    u = u / np.hypot(*u)
    R = ic.R_MEAS * np.eye(2)
    for step in np.arange(0.05, 2.0, 0.025):
        z = lc.reading_of(x, i, tuple(step * u))
        cols, Hc, _, nu = sp.candidate_terms(x, z[0], z[1], count=known)
        nis = np.array([ds.np_scores(S[np.ix_(c, c)], h[None], R, v[None])[1][0] for c, h, v in zip(cols, Hc, nu)])
        if lc.rule(nis, known, known + 1)[1] == "drop" and 2.0 < nis.min() < 8.0:
            return z
    raise AssertionError("no reading between the gates")


def _twin_case(kind):
    count, known = 63, 40
    x, S = lc.spiral_map(count)
    _stale_beyond(S, known)
    z = {"all match": [lc.reading_of(x, i) for i in (3, 11, 23, 30)],
         "match + new": [lc.reading_of(x, 3), lc.reading_of(x, 50), lc.reading_of(x, 23), lc.reading_of(x, 55)],
         "conflict": [lc.reading_of(x, 23, (0.02, 0.0)), lc.reading_of(x, 23, (0.002, 0.0)), lc.reading_of(x, 5)],
         "drop only": [_between_the_gates(x, S, 23, known), _between_the_gates(x, S, 11, known)]}[kind]
    want = {"all match": ([3, 11, 23, 30], 40), "match + new": ([3, 40, 23, 41], 42), "conflict": ([-1, 23, 5], 40),
            "drop only": ([-1, -1], 40)}[kind]
    return count, known, x, S, np.array(z), want


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("pending,carry", [(0, False), (2, True), (62, True), (2, False)])
@pytest.mark.parametrize("kind", ["all match", "match + new", "conflict", "drop only"])
def test_joint_twin(hip, kind, pending, carry, deferred):
    count, known, x, S, z, (want_assoc, want_known) = _twin_case(kind)
    make = lambda: _handle(hip, x, S, pending, carry)
    d, twin = make(), make()
    k1, assoc, best, ng, _ = d.associate_joint(z, known, count, deferred)
    k2, assoc2, best2, ng2, kinds = _twin_joint(hip, make, twin, z, known, count, deferred)
    assert (k1, list(assoc), ng) == (k2, list(assoc2), ng2), (kinds, assoc, assoc2)
    assert (list(assoc), k1) == (want_assoc, want_known), (kinds, assoc, best)
    assert _bits(best, best2)
    got = _snapshot(d)                                                         # (once: it flushes)
    _same(got, _snapshot(twin))
    if kind == "drop only":
        _same(got, _snapshot(make()))                                          # nothing at all was written
    else:
        assert not _bits(got[1], x)
    d.close(); twin.close()


# ---- 4. one reading per call is the sequential call --------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("pending,carry", [(0, False), (2, True), (64, True)])
def test_one_reading_is_associate_landmarks(hip, pending, carry, deferred):
    count, known = 63, 40
    x, S = lc.spiral_map(count)
    x[0] = -0.0
    _stale_beyond(S, known)
    for z in (lc.reading_of(x, 23), lc.reading_of(x, 50), _between_the_gates(x, S, 23, known)):
        a, b = _handle(hip, x, S, pending, carry), _handle(hip, x, S, pending, carry)
        ka, assoc_a, best_a, ng, _ = a.associate_joint([z], known, count, deferred)
        kb, assoc_b, best_b, _ = b.associate_landmarks([z], known, count, deferred)
        assert ka == kb and _bits(assoc_a, assoc_b) and _bits(best_a, best_b) and ng == int(assoc_a[0] >= 0)
        _same(_snapshot(a), _snapshot(b))
        a.close(); b.close()


@pytest.mark.parametrize("mode", ["eager", "deferred_grow_carry"])
def test_chain_of_single_readings_against_the_reference_data_association(hip, oracle, mode):
    """the discovery scenario at n = 20, every reading its own joint call: bit for bit associate_landmarks on a twin, the
    decisions and `known` of the reference's data_association(), state and Sigma within FP64_TOL"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    n = 20
    ref = oracle.RefEKF(n)
    known_ref = np.zeros(n, dtype=np.uint8)
    x0, S0 = ic.prior_start(n)
    d, seq = (hip.DensePropagator64(3 + 2 * n) for _ in range(2))
    deferred = grow = mode != "eager"
    for h in (d, seq):
        h.set(Sigma=S0)
        h.state = x0
        if grow:
            h.carry = True
            h.live = 3
    kd = ks = 0
    for t, (dth, dx, readings) in enumerate(ic.discovery_scenario()):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        for h in (d, seq):
            Fr, Qr, upd = bc.model_operands(h.state_block(0, 3), dth, dx)
            h.propagate_block(0, Fr, Qr, upd)
        ks, want, want_best, _ = seq.associate_landmarks(readings, ks, n, deferred, grow)
        got = []
        for j, z in enumerate(readings):
            kd, a1, b1, _, _ = d.associate_joint([z], kd, n, deferred, grow)
            got.append(int(a1[0]))
            assert _bits(b1[0], want_best[j]), (t, j)
        assert got == list(want) and kd == ks == int(known_ref.sum()) and known_ref[:kd].all(), (t, got, want)
        assert d.pending == seq.pending and d.live == seq.live
    assert kd == n
    gs, gS = d.state, d.sigma
    assert _bits(gs, seq.state) and _bits(gS, seq.sigma)
    d.close(); seq.close()
    w, e = worst(gs, gS, ref.state, ref.cov)
    print(f"joint_single_readings_reference_{mode}: {w:.3e}")
    assert w <= FP64_TOL, e


# ---- 5. the numpy model --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", [False, True])
def test_joint_against_the_numpy_model(hip, deferred):
    """the scan fixture (8 matches and one new landmark per tick, 5 ticks with prediction): decisions identical, state and
    all of Sigma within FP64_TOL"""
    x, S, known, steps = jc.scan_fixture()
    n_max = (len(x) - 3) // 2
    d, m = _handle(hip, x, S), jc.numpy_handle(x, S)
    kd = km = known
    assert len(steps) == 5
    for t, (dth, dx, readings) in enumerate(steps):
        for h in (d, m):
            Fr, Qr, upd = bc.model_operands(h.state_block(0, 3), dth, dx)
            h.propagate_block(0, Fr, Qr, upd)
        kd, assoc, best, ng, _ = d.associate_joint(readings, kd, n_max, deferred)
        km, want, want_best, want_ng = jc.np_associate_joint(m, None, readings, km, n_max)
        assert (kd, list(assoc), ng) == (km, list(want), want_ng), (t, assoc, want)
        assert np.abs(best - want_best).max() <= 1e-9 * np.abs(want_best).max()
    assert kd == known + 5
    _, gs, gS = _snapshot(d)
    w, e = worst(gs, gS, m.state, m.sigma)
    print(f"joint_numpy_model_{'deferred' if deferred else 'eager'}: {w:.3e}")
    d.close()
    assert w <= FP64_TOL, e


# ---- 6. groups -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", [False, True])
def test_31_matches_are_two_groups(hip, deferred):
    count = 40
    x, S = lc.spiral_map(count)
    z = np.array([lc.reading_of(x, i, (0.004, -0.002)) for i in range(31)])
    make = lambda: _handle(hip, x, S, 2 if deferred else 0)
    d, twin = make(), make()
    k1, assoc, best, ng, _ = d.associate_joint(z, count, count, deferred)
    assert k1 == count and list(assoc) == list(range(31)) and ng == 2
    k2, assoc2, best2, ng2, _ = _twin_joint(hip, make, twin, z, count, count, deferred)
    assert (k2, list(assoc2), ng2) == (k1, list(assoc), 2) and _bits(best, best2)
    _same(_snapshot(d), _snapshot(twin))
    d.close(); twin.close()


def test_33_new_landmarks_are_two_init_groups(hip):
    count, known = 40, 2
    x, S = lc.spiral_map(count)
    _stale_beyond(S, known)
    z = _ring(33)
    make = lambda: _handle(hip, x, S, 2, True)
    d, twin = make(), make()
    k1, assoc, best, ng, _ = d.associate_joint(z, known, count, True)
    assert k1 == known + 33 and list(assoc) == list(range(known, known + 33)) and ng == 2 and (best == 10.0).all()
    k2, assoc2, _, ng2, kinds = _twin_joint(hip, make, twin, z, known, count, True)
    assert kinds == [jc.NEW] * 33 and (k2, list(assoc2), ng2) == (k1, list(assoc), 2)
    _same(_snapshot(d), _snapshot(twin))
    # more new readings than slots: the first ones in ascending j take them, the rest are dropped
    e = make()
    k3, assoc3, _, _, _ = e.associate_joint(z, known, known + 5, True)
    assert k3 == known + 5 and list(assoc3) == list(range(known, known + 5)) + [-1] * 28
    d.close(); twin.close(); e.close()


# ---- 7. the live dimension ------------------------------------------------------------------------------------------------------

def test_joint_inside_the_live_corner(hip):
    """live < N with everything outside poisoned: the poison's bits survive and the corner is a handle of dimension live"""
    n, known, lim = 20, 10, 12
    live = 3 + 2 * lim
    x, S = lc.spiral_map(n)
    _stale_beyond(S, known)
    xs, Ss = x[:live].copy(), S[:live, :live].copy()
    poison = np.float64(-7.25e250)
    x[live:] = poison
    S[live:, :] = poison
    S[:, live:] = poison
    z = np.array([lc.reading_of(xs, 3), (6.0, 6.0), lc.reading_of(xs, 7), (-6.0, 5.0)])
    for deferred in (False, True):
        d, small = _handle(hip, x, S, live=live), _handle(hip, xs, Ss)
        kd, assoc, _, _, _ = d.associate_joint(z, known, lim, deferred)
        ks, assoc_s, _, _, _ = small.associate_joint(z, known, lim, deferred)
        assert kd == ks == known + 2 and list(assoc) == list(assoc_s) == [3, 10, 7, 11]
        got, want = _snapshot(d), _snapshot(small)
        assert got[0] == want[0] and _bits(got[1][:live], want[1]) and _bits(got[2][:live, :live], want[2])
        assert _bits(got[1][live:], x[live:]) and _bits(got[2][live:, :], S[live:, :]) and _bits(got[2][:, live:], S[:, live:])
        d.close(); small.close()


def test_joint_grow_live(hip):
    """two new landmarks at the live edge with rows pending: refused without the flag and nothing changes; with it the live
    dimension grows once, the pending rows are kept (carry on)"""
    count, known = 20, 10
    x, S = lc.spiral_map(count)
    _stale_beyond(S, known)
    live = 3 + 2 * known
    make = lambda: _handle(hip, x, S, 2, True, live)
    d, twin = make(), make()
    z = np.array([(6.0, 6.0), lc.reading_of(x, 4), (-6.0, 5.0)])
    with pytest.raises(hip.EkfError) as e:
        d.associate_joint(z, known, count, deferred=True)
    assert e.value.status == INVALID and e.value.known == known and d.live == live
    _same(_snapshot(d), _snapshot(make()))
    d.close()
    d = make()
    k, assoc, _, ng, _ = d.associate_joint(z, known, count, deferred=True, grow_live=True)
    assert k == known + 2 and list(assoc) == [10, 4, 11] and d.live == live + 4 and d.pending == 2 + 6 and ng == 1
    k2, assoc2, _, _, _ = _twin_joint(hip, make, twin, z, known, count, True, grow=True)
    assert k2 == k and list(assoc2) == list(assoc) and twin.live == d.live
    _same(_snapshot(d), _snapshot(twin))
    d.close(); twin.close()


# ---- 8. failures -----------------------------------------------------------------------------------------------------------------

def test_joint_singular_group(hip):
    """R = 0 and sigma0_landmark = 0 with the pose's covariance zero: the new landmark's rows of S are zero, the one group is
    refused -- EKF_ERR_STATE, the correction undone, the initialisation stands and is counted"""
    count = 6
    x, S = lc.spiral_map(count)
    S[:3, :] = 0.0
    S[:, :3] = 0.0
    p = hip.default_params()
    p.r_meas, p.sigma0_landmark = 0.0, 0.0
    d = _handle(hip, x, S)
    far = (40.0, 40.0)
    with pytest.raises(hip.EkfError) as e:
        d.associate_joint([lc.reading_of(x, 1), far], 4, count, params=p)
    err = e.value
    assert err.status == STATE and err.known == 5 and list(err.assoc) == [-1, -1], (err.status, err.known, err.assoc)
    got, gS = d.state, d.sigma
    assert _bits(got[:11], x[:11])                                             # the group's correction wrote nothing
    assert np.abs(got[11:13] - ic.inverse_sensor(x[:3], *far)).max() <= TOL    # the initialisation stands
    want = S.copy()
    want[11:13, :] = 0.0
    want[:, 11:13] = 0.0
    assert _bits(gS, want)
    d.close()


def test_joint_refusals_change_nothing(hip):
    count, known = 20, 10
    x, S = lc.spiral_map(count)
    live = 3 + 2 * 12
    d, ref = _handle(hip, x, S, 2, live=live), _handle(hip, x, S, 2, live=live)
    lib, h = d._lib, d._h
    z = (C.c_double * 4)(*lc.reading_of(x, 3), *lc.reading_of(x, 4))
    lm = (C.c_int * 2)(3, 4)
    k = C.c_int(known)
    buf, ibuf = (C.c_double * 256)(), (C.c_int * 64)()

    def joint(hh, J, zz, n_max, kk, flags):
        return lib.ekf_dense64_associate_joint(hh, None, J, zz, n_max, kk, flags, None, None, None, None), lib.ekf_last_error()

    def refused(res, text):
        assert res[0] == INVALID and text in res[1], res

    # each check, and in front of it the one that comes before: the first of two faults is the one reported
    refused(joint(None, 0, None, -1, None, 4), b"null handle")
    refused(joint(h, 0, z, -1, None, 4), b"null argument")
    refused(joint(h, 0, None, -1, C.byref(k), 4), b"null argument")
    refused(joint(h, 0, z, -1, C.byref(k), 4), b"J must lie")
    refused(joint(h, 129, z, -1, C.byref(k), 4), b"J must lie")
    refused(joint(h, 2, z, -1, C.byref(C.c_int(-1)), 4), b"n_max must lie")
    refused(joint(h, 2, z, count + 1, C.byref(k), 4), b"n_max must lie")
    for bad in (-1, count + 1):
        refused(joint(h, 2, z, count, C.byref(C.c_int(bad)), 4), b"*known must lie")
    refused(joint(h, 2, z, count, C.byref(C.c_int(13)), 4), b"inside the live dimension")   # 3 + 2 * 13 > live
    refused(joint(h, 2, z, count, C.byref(k), 4), b"unknown flag bits")
    sr = lambda hh, J, zz, first, cnt, out, fl: lib.ekf_dense64_score_readings(hh, None, J, zz, first, cnt, out, fl, None)
    assert sr(None, 2, z, 0, 2, buf, None) == INVALID
    for J, zz, first, cnt, out in ((0, z, 0, 2, buf), (129, z, 0, 2, buf), (2, None, 0, 2, buf), (2, z, -1, 2, buf),
                                   (2, z, 0, 0, buf), (2, z, 0, 13, buf), (2, z, 11, 2, buf), (2, z, 0, 32769, buf),
                                   (2, z, 0, 2, None)):
        assert sr(h, J, zz, first, cnt, out, None) == INVALID, (J, first, cnt)
    jo = lambda hh, V, ll, zz, c, H, u: lib.ekf_dense64_joint_operands(hh, None, V, ll, zz, c, H, u, None)
    assert jo(None, 2, lm, z, ibuf, buf, buf) == INVALID
    for V, ll, zz, c in ((0, lm, z, ibuf), (31, lm, z, ibuf), (2, None, z, ibuf), (2, lm, None, ibuf), (2, lm, z, None),
                         (2, (C.c_int * 2)(3, 3), z, ibuf), (2, (C.c_int * 2)(3, 12), z, ibuf),
                         (2, (C.c_int * 2)(-1, 3), z, ibuf)):
        assert jo(h, V, ll, zz, c, None, None) == INVALID, (V, c)
    r = (C.c_double * 360)(*sc.circles_scan(3))
    cnt = C.c_int(-7)
    scan = lambda hh, rr, nb, mr, nmax, kk, flags, ccnt: (
        lib.ekf_dense64_associate_scan_joint(hh, None, rr, nb, mr, nmax, kk, flags, ccnt, None, None, None, None),
        lib.ekf_last_error())
    refused(scan(None, None, 0, 0, -1, None, 4, None), b"null handle")
    refused(scan(h, None, 0, 0, -1, C.byref(k), 4, C.byref(cnt)), b"null argument")
    refused(scan(h, r, 360, 64, -1, None, 4, C.byref(cnt)), b"null argument")
    refused(scan(h, r, 0, 64, -1, C.byref(k), 4, C.byref(cnt)), b"n_beams must lie")
    refused(scan(h, r, 360, 129, -1, C.byref(k), 4, C.byref(cnt)), b"n_beams must lie")
    refused(scan(h, r, 360, 64, -1, C.byref(k), 4, C.byref(cnt)), b"n_max must lie")
    refused(scan(h, r, 360, 64, count, C.byref(C.c_int(13)), 4, C.byref(cnt)), b"inside the live dimension")
    refused(scan(h, r, 360, 64, count, C.byref(k), 4, C.byref(cnt)), b"unknown flag bits")
    assert k.value == known and cnt.value == -7 and d.live == live
    got, want = _snapshot(d), _snapshot(ref)
    assert got[0] == want[0] == 2
    _same(got, want)
    d.close(); ref.close()


# ---- 9. a scan as the input ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["eager", "deferred_grow_carry"])
@pytest.mark.parametrize("circles,max_readings", [(0, 64), (3, 64), (3, 1)])
def test_associate_scan_joint_twin(hip, mode, circles, max_readings):
    n, known0 = 10, 4
    x, S = lc.spiral_map(n)                                                    # N = 23
    x[3:5] = x[:3][1:] + np.array([1.25, 0.0])                                 # landmark 0 near where the first tube is seen
    deferred = grow = mode != "eager"
    live = 3 + 2 * known0 if grow else None
    a, b = (_handle(hip, x, S, 2 if deferred else 0, grow, live) for _ in range(2))
    r = sc.circles_scan(circles)
    ka, cen, assoc, best = a.associate_scan_joint(r, known0, n, max_readings, deferred, grow)
    cen_b, _, _ = b.fit_scan(r, max_out=max_readings)
    want = min(circles, max_readings)
    assert len(cen) == len(assoc) == len(best) == want and _bits(cen, cen_b)
    kb = known0
    if want:
        kb, assoc_b, best_b, _, _ = b.associate_joint(cen_b, known0, n, deferred, grow)
        assert _bits(assoc, assoc_b) and _bits(best, best_b), (assoc, assoc_b)
        assert (assoc >= 0).any() and not _bits(a.state, x)
    else:
        assert _bits(a.state, x)                                               # nothing of the filter was written
    assert ka == kb and a.live == b.live
    _same(_snapshot(a), _snapshot(b))
    a.close(); b.close()


def test_dense_ekf_slam_joint_association(hip):
    """the object's two spellings: joint_association(readings) and scan_association(ranges, joint=True)"""
    x, S, known, steps = jc.scan_fixture()
    n = (len(x) - 3) // 2
    slam = hip.DenseEKFSLAM(n)
    assert list(slam.joint_association(_ring(3))) == [0, 1, 2] and slam.known == 3
    cen, assoc = slam.scan_association(sc.circles_scan(3), joint=True)
    assert len(cen) == len(assoc) == 3 and slam.known <= n
    slam.close()
