"""GPU: the landmark front end of the fp64 dense handle -- ekf_dense64_score_landmarks (the reference's model evaluated on the
device from the handle's state, scored by score_sparse's kernel) and ekf_dense64_associate_landmarks (the reference's
data_association() per reading: rule on the device, init_block's path for a new landmark, the sparse or deferred correction,
the heading wrap).  The bit-level claims are tested as such: the operands against numpy, the scores against score_sparse on
the returned operands, the tie rule across wave and stride boundaries, and a twin handle driven by the existing public calls
with the device-built operands."""
import time

import numpy as np
import pytest

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_correct_cases as dc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_landmark_cases as lc
import dense_score_cases as ds
import dense_sparse_cases as sp
from parity import FP64_TOL, worst

pytestmark = pytest.mark.gpu
TOL = 1e-12
INVALID, STATE = 1, 5
R = ic.R_MEAS * np.eye(2)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _handle(hip, x, S, pending=0, carry=False, live=None):
    """a handle with the state x, the covariance S, the live dimension `live` and `pending` rows left by deferred corrections
    of an integer chain (dense_deferred_cases, the shapes of dense_carry_cases) inside it; built twice it holds the same
    bits twice"""
    N = len(x)
    d = hip.DensePropagator64(N)
    d.set(Sigma=S)
    if live is not None:
        d.live = live
    if pending:
        Na = d.live
        chain = dd.integer_chain(Na, "asc", seed=77, shapes=cc.RECIPE[pending], Sigma0=S[:Na, :Na])
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


# ---- 1. operands ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025])
def test_landmark_operands(hip, count):
    x, S = lc.spiral_map(count, seed=count)
    sx, sy = lc.reading_of(x, count // 2)
    d = _handle(hip, x, S)
    nis, _, flags, _, (cols, Hc, nu) = d.score_landmarks(sx, sy, want_terms=True)
    wc, wH, _, wnu = sp.candidate_terms(x, sx, sy)
    assert cols.dtype == np.int32 and np.array_equal(cols, wc)
    assert _bits(Hc, wH), np.argwhere(Hc != wH)[:4]
    assert np.abs(nu - wnu).max() <= TOL
    assert not flags.any() and np.isfinite(nis).all()
    for first, cnt in ((1, count - 1), (count // 2, count - count // 2), (count - 1, 1)):
        if cnt < 1 or first < 1:
            continue
        n2, _, f2, _, (c2, H2, u2) = d.score_landmarks(sx, sy, first_lm=first, count=cnt, want_terms=True)
        assert _bits(c2, cols[first:first + cnt]) and _bits(H2, Hc[first:first + cnt]) and _bits(u2, nu[first:first + cnt])
        assert _bits(n2, nis[first:first + cnt]) and _bits(f2, flags[first:first + cnt])
    d.close()


# ---- 2. the same kernel, read-only ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pending", [0, 2, 64])
def test_landmark_scores_are_score_sparse_on_the_returned_operands(hip, pending):
    count = 63
    x, S = lc.spiral_map(count)
    sx, sy = lc.reading_of(x, 17)
    d = _handle(hip, x, S, pending)
    state0 = d.state
    nis, Sj, flags, _, (cols, Hc, nu) = d.score_landmarks(sx, sy, want_S=True, want_terms=True)
    assert d.pending == pending and _bits(d.state, state0)
    n2, S2, f2, _ = d.score_sparse(cols, Hc, R, nu, want_S=True)
    assert _bits(nis, n2) and _bits(Sj, S2) and _bits(flags, f2)
    n3, _, f3, _ = d.score_landmarks(sx, sy)                                   # without S: another layout, the same bits
    assert _bits(n3, nis) and _bits(f3, flags)
    twin = _handle(hip, x, S, pending)                                         # read-only: Sigma against an untouched twin
    got, want = _snapshot(d), _snapshot(twin)
    assert got[0] == want[0] == pending and _bits(got[1], want[1]) and _bits(got[2], want[2])
    d.close(); twin.close()


# ---- 3. the rule on the device --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count,a,b", [(5, 0, 1), (70, 62, 65), (260, 254, 257)])
def test_landmark_rule_ties_and_nan(hip, count, a, b):
    nan_at = a + 1 if b != a + 1 else b + 1
    x, S, (sx, sy) = lc.tie_fixture(count, a, b, nan_at)
    d = _handle(hip, x, S)
    nis, _, flags, _ = d.score_landmarks(sx, sy)
    assert _bits(nis[a], nis[b]) and flags[nan_at] == 1 and np.isnan(nis[nan_at]) and flags.sum() == 1
    rest = np.delete(nis, [a, b, nan_at])
    assert nis[a] < 1.0 and (rest > nis[a]).all()
    x2, S2, _ = lc.tie_fixture(count, a, b, None)                              # the neighbours' bits without the NaN
    d2 = _handle(hip, x2, S2)
    m2 = d2.score_landmarks(sx, sy)[0]
    keep = np.arange(count) != nan_at
    assert _bits(nis[keep], m2[keep])
    d2.close()
    known, assoc, best, _ = d.associate_landmarks([(sx, sy)], count, count)
    assert known == count and assoc[0] == a and _bits(best[0], nis[a])
    d.close()


# ---- 4. the twin ----------------------------------------------------------------------------------------------------------------

def _twin_step(hip, twin, probe, sx, sy, known, assoc, grew, deferred):
    """the decision of the first handle replayed on `twin` with the existing public calls and the device-built operands"""
    if grew:
        twin.init_block(3 + 2 * known, W=ic.PRIOR * np.eye(2), xb=probe)
        known += 1
    if assoc >= 0:
        _, _, _, _, (cols, Hc, nu) = twin.score_landmarks(sx, sy, first_lm=assoc, count=1, want_terms=True)
        wrapped = np.array([nu[0, 0], dc.normalize_angle(float(nu[0, 1]))])
        (twin.correct_sparse_deferred if deferred else twin.correct_sparse)(cols[0], Hc[0], R, wrapped)
        lc.wrap_heading_always(twin)
    return known


def _between_the_gates(x, S, i, known):
    """a reading of landmark i pushed outwards until numpy's rule drops it with the best score well inside (2, 8)"""
    u = x[3 + 2 * i:5 + 2 * i] - x[1:3]
    u = u / np.hypot(*u)
    for step in np.arange(0.05, 2.0, 0.025):
        z = lc.reading_of(x, i, tuple(step * u))
        cols, Hc, _, nu = sp.candidate_terms(x, z[0], z[1], count=known)
        nis = np.array([ds.np_scores(S[np.ix_(c, c)], h[None], R, v[None])[1][0] for c, h, v in zip(cols, Hc, nu)])
        if lc.rule(nis, known, known + 1)[1] == "drop" and 2.0 < nis.min() < 8.0:
            return z
    raise AssertionError("no reading between the gates")


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("pending,carry", [(0, False), (2, True), (64, True), (2, False)])
@pytest.mark.parametrize("kind", ["new", "update", "drop"])
def test_landmark_twin(hip, kind, pending, carry, deferred):
    count, known = 63, 40
    x, S = lc.spiral_map(count)
    if kind == "update":
        x[0] = -0.0
        S[0, :] = S[:, 0] = 0.0                                                # the heading decoupled: it stays a zero
    S[3 + 2 * known:, :] = 0.0
    S[:, 3 + 2 * known:] = 0.0
    S[3 + 2 * known:, 3 + 2 * known:] = 7.0 * np.eye(2 * (count - known))     # stale blocks beyond the known prefix
    sx, sy = {"new": lc.reading_of(x, 50), "update": lc.reading_of(x, 23), "drop": _between_the_gates(x, S, 23, known)}[kind]
    make = lambda: _handle(hip, x, S, pending, carry)
    d, twin = make(), make()
    want_kind = lc.rule(d.score_landmarks(sx, sy, count=known)[0], known, count)[1]
    assert want_kind == kind, want_kind
    probe = None
    if kind == "new":                                                          # xb: a third handle that only initialises
        p = hip.default_params()
        p.gate_update = 0.0
        third = make()
        k3, a3, _, _ = third.associate_landmarks([(sx, sy)], known, count, deferred, params=p)
        assert k3 == known + 1 and a3[0] == -1
        probe = third.state_block(3 + 2 * known, 2)
        assert np.abs(probe - ic.inverse_sensor(x[:3], sx, sy)).max() <= TOL
        t3 = make()
        t3.init_block(3 + 2 * known, W=ic.PRIOR * np.eye(2), xb=probe)
        got, want = _snapshot(third), _snapshot(t3)
        assert got[0] == want[0] and _bits(got[1], want[1]) and _bits(got[2], want[2])
        third.close(); t3.close()
    k1, assoc, best, _ = d.associate_landmarks([(sx, sy)], known, count, deferred)
    assert (k1, assoc[0]) == {"new": (known + 1, known), "update": (known, 23), "drop": (known, -1)}[kind]
    k2 = _twin_step(hip, twin, probe, sx, sy, known, int(assoc[0]), kind == "new", deferred)
    assert k2 == k1
    got, want = _snapshot(d), _snapshot(twin)
    assert got[0] == want[0], (got[0], want[0])
    assert _bits(got[1], want[1]) and _bits(got[2], want[2])
    if kind == "update":
        assert _bits(got[1][0], np.float64(0.0))                               # -0.0 became +0.0
    if kind == "drop":
        untouched = _snapshot(make())
        assert got[0] == untouched[0] and _bits(got[1], untouched[1]) and _bits(got[2], untouched[2])
    d.close(); twin.close()


# ---- 5. refusals and failures ---------------------------------------------------------------------------------------------------

def test_landmark_refusals_change_nothing(hip):
    import ctypes as C
    count, known = 20, 10
    x, S = lc.spiral_map(count)
    live = 3 + 2 * 12
    d, ref = _handle(hip, x, S, 2, live=live), _handle(hip, x, S, 2, live=live)
    lib, h = d._lib, d._h
    z = (C.c_double * 2)(*lc.reading_of(x, 3))
    k = C.c_int(known)
    call = lambda hh, J, zz, n_max, kk, flags: lib.ekf_dense64_associate_landmarks(hh, None, J, zz, n_max, kk, flags, None,
                                                                                    None, None)
    assert call(None, 1, z, count, C.byref(k), 0) == INVALID
    assert call(h, 1, z, count, None, 0) == INVALID and call(h, 1, None, count, C.byref(k), 0) == INVALID
    assert call(h, 0, z, count, C.byref(k), 0) == INVALID
    assert call(h, 1, z, -1, C.byref(k), 0) == INVALID and call(h, 1, z, count + 1, C.byref(k), 0) == INVALID
    for bad in (-1, count + 1):
        assert call(h, 1, z, count, C.byref(C.c_int(bad)), 0) == INVALID
    assert call(h, 1, z, count, C.byref(C.c_int(13)), 0) == INVALID             # 3 + 2 * 13 > live
    assert call(h, 1, z, count, C.byref(k), 4) == INVALID
    sc = lambda hh, first, cnt, out: lib.ekf_dense64_score_landmarks(hh, None, 0.5, 0.5, first, cnt, out, None, None, None,
                                                                     None, None, None)
    buf = (C.c_double * 64)()
    for first, cnt, out in ((0, 0, buf), (-1, 2, buf), (0, 13, buf), (11, 2, buf), (0, 32769, buf), (0, 2, None)):
        assert sc(h, first, cnt, out) == INVALID
    assert sc(None, 0, 1, buf) == INVALID
    assert k.value == known and d.live == live
    got, want = _snapshot(d), _snapshot(ref)
    assert got[0] == want[0] == 2 and _bits(got[1], want[1]) and _bits(got[2], want[2])
    d.close(); ref.close()


def test_landmark_grow_live(hip):
    """GROW_LIVE off at the live edge: refused, nothing changes; on: live grows, the pending rows are kept (carry on)"""
    count, known = 20, 10
    x, S = lc.spiral_map(count)
    S[23:, :] = 0.0
    S[:, 23:] = 0.0
    S[23:, 23:] = 7.0 * np.eye(2 * count - 20)
    live = 3 + 2 * known
    d, ref = _handle(hip, x, S, 2, True, live), _handle(hip, x, S, 2, True, live)
    far = (6.0, 6.0)                                                           # every known landmark beyond gate_new
    with pytest.raises(hip.EkfError) as e:
        d.associate_landmarks([far], known, count, deferred=True)
    assert e.value.status == INVALID and e.value.known == known and d.live == live and d.pending == 2
    assert _bits(d.state, ref.state)
    k, assoc, _, _ = d.associate_landmarks([far], known, count, deferred=True, grow_live=True)
    assert k == known + 1 and assoc[0] == known and d.live == live + 2 and d.pending == 4
    p = hip.default_params()                                                   # xb: a third handle that only initialises
    p.gate_update = 0.0
    third = _handle(hip, x, S, 2, True, live)
    assert third.associate_landmarks([far], known, count, deferred=True, grow_live=True, params=p)[0] == known + 1
    xb = third.state_block(3 + 2 * known, 2)
    assert np.abs(xb - ic.inverse_sensor(x[:3], *far)).max() <= TOL
    ref.live = live + 2                                                        # the twin: the existing calls
    assert ref.pending == 2
    assert _twin_step(hip, ref, xb, far[0], far[1], known, known, True, True) == known + 1
    got, want = _snapshot(d), _snapshot(ref)
    assert got[0] == want[0] == 4 and _bits(got[1], want[1]) and _bits(got[2], want[2])
    d.close(); ref.close(); third.close()


def test_landmark_singular_winner(hip):
    """R = 0 (params.r_meas = 0) and a zero 5 x 5 block: the second reading's new landmark (sigma0_landmark = 0, the pose's
    covariance zero) has S = 0, so its correction returns EKF_ERR_STATE; the first reading stands, the initialisation is
    counted, the third reading is not reached"""
    count = 6
    x, S = lc.spiral_map(count)
    S[:3, :] = 0.0
    S[:, :3] = 0.0
    p = hip.default_params()
    p.r_meas, p.sigma0_landmark = 0.0, 0.0
    d = _handle(hip, x, S)
    far = (40.0, 40.0)
    with pytest.raises(hip.EkfError) as e:
        d.associate_landmarks([lc.reading_of(x, 1), far, lc.reading_of(x, 2)], 4, count, params=p)
    err = e.value
    assert err.status == STATE and err.known == 5 and list(err.assoc) == [1, -1, -2], (err.status, err.known, err.assoc)
    got = d.state
    assert not _bits(got[5:7], x[5:7])                                         # the first reading's correction stands
    assert np.abs(got[11:13] - ic.inverse_sensor(got[:3], *far)).max() <= 1e-9  # and the initialisation
    d.close()


# ---- 6. the reference, live -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [20, 200])
@pytest.mark.parametrize("mode", ["eager", "deferred", "deferred_grow_carry"])
def test_landmarks_against_the_reference_data_association(hip, oracle, n, mode):
    """the discovery scenario, each tick propagate_block + ONE associate_landmarks call with all of the tick's readings,
    against the reference's own data_association(): `known` after every tick, the winners of the spelled loop, the end
    state and Sigma; every vector of scores a read-only score_landmarks takes before a reading keeps ds.margins_hold"""
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    steps = ic.discovery_scenario()
    ref = oracle.RefEKF(n)
    known_ref = np.zeros(n, dtype=np.uint8)
    N = 3 + 2 * n
    x0, S0 = ic.prior_start(n)
    d, spelled, probe = (hip.DensePropagator64(N) for _ in range(3))
    for h in (d, spelled, probe):
        h.set(Sigma=S0)
        h.state = x0
    deferred, grow = mode != "eager", mode == "deferred_grow_carry"
    if grow:
        for h in (d, probe):
            h.carry = True
            h.live = 3
    known = ks = kp = 0
    scored = 0
    for t, (dth, dx, readings) in enumerate(steps):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        Fr, Qr, upd = bc.model_operands(spelled.state_block(0, 3), dth, dx)     # the spelled loop's winners
        spelled.propagate_block(0, Fr, Qr, upd)
        ks, winners, _ = lc.np_associate(spelled, None, readings, ks, n)
        # the probe: the same mode reading by reading, so that a read-only score_landmarks sees, before each reading, the
        # covariance the one call scores against (through the pending and carried rows where the mode leaves them)
        Fr, Qr, upd = bc.model_operands(probe.state_block(0, 3), dth, dx)
        probe.propagate_block(0, Fr, Qr, upd)
        singles = []
        for z in readings:
            if kp:
                nis, _, flags, _ = probe.score_landmarks(z[0], z[1], count=kp)
                assert not flags.any() and ds.margins_hold(nis), (t, "the scenario's seed must be replaced", np.sort(nis)[:3])
                scored += 1
            kp, a1, _, _ = probe.associate_landmarks([z], kp, n, deferred, grow)
            singles.append(int(a1[0]))
        Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), dth, dx)
        d.propagate_block(0, Fr, Qr, upd)
        known, assoc, _, _ = d.associate_landmarks(readings, known, n, deferred, grow)   # ONE call per tick
        assert list(assoc) == list(winners) == singles, (t, assoc, winners, singles)
        assert known == ks == kp == int(known_ref.sum()) and known_ref[:known].all(), (t, known, known_ref)
        assert d.pending == probe.pending and d.live == probe.live
    assert known == min(n, len(steps)) and scored > len(steps)
    if grow:
        assert d.live == 3 + 2 * known
    P = 3 + 2 * known
    gs, gS, rs, rS = d.state, d.sigma, ref.state, ref.cov
    assert _bits(gs, probe.state) and _bits(gS, probe.sigma)                   # J readings in one call = J calls of one
    d.close(); spelled.close(); probe.close()
    w, e = worst(gs[:P], gS[:P, :P], rs[:P], rS[:P, :P])
    print(f"reference_live_{mode}_n{n}: {w:.3e}")
    assert w <= FP64_TOL, e


# ---- 7. full size ---------------------------------------------------------------------------------------------------------------

def _wall_median(f, iters=9, warmup=2):
    out = []
    for _ in range(warmup + iters):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out[warmup:]))


def test_landmarks_full_size_n10003_and_time(hip):
    """N = 10003, known = n_max = 5000, the state and Sigma of the full-map sparse test; one reading that corrects, DEFERRED,
    against the spelled loop on a twin at 1e-12 on sampled rows and columns, the decision identical; then the time
    condition, wall-clock medians of 9 after 2 in this process: A, one associate_landmarks reading, below B, the parent's
    spelling of the same reading with its handle calls alone (state_block, score_sparse, correct_sparse_deferred, the
    heading read / write) and every candidate array prebuilt outside the timed region (measured: 0.145 against 0.490 ms)."""
    N, n = 10003, 5000
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    Sigma = A @ A.T / 64 + np.eye(N)
    Sigma += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    j = 3333
    sx, sy = lc.reading_of(x, j, (0.002, -0.001))
    d, twin = hip.DensePropagator64(N), hip.DensePropagator64(N)
    for h in (d, twin):
        h.set(Sigma=Sigma)
        h.state = x
    del Sigma
    cols, Hc, _, nu = sp.candidate_terms(x, sx, sy)
    nis_t = twin.score_sparse(cols, Hc, R, nu)[0]
    win, kind, best_t = lc.rule(nis_t, n, n)
    assert (win, kind) == (j, "update"), (win, kind, best_t)
    c, h5, _, _, wrapped = sp.slam_terms(x[:3], x, win, sx, sy)
    twin.correct_sparse_deferred(c, h5, R, wrapped)
    lc.wrap_heading_always(twin)
    nis_d = d.score_landmarks(sx, sy)[0]
    known, assoc, best, _ = d.associate_landmarks([(sx, sy)], n, n, deferred=True)
    assert known == n and assoc[0] == j and _bits(best[0], nis_d[j])
    # against the host-built operands: nu agrees to 1e-12 absolute (atan2, hypot) on an innovation of 2e-3, 5e-10 relative,
    # and the score is quadratic in it: 1e-9
    assert abs(best[0] - best_t) <= FP64_TOL * abs(best_t)
    assert d.pending == twin.pending == 2
    last = (N - 1) // 128 * 128
    rows = np.array(sorted(set([0, 1, 2, N - 1, 3 + 2 * j, 4 + 2 * j] + list(range(last, N, 3)) +
                               list(rng.integers(0, N, size=18)))))
    cc_ = np.array(sorted(set([0, 1, 2, N - 1, N - 2, 3 + 2 * j, 4 + 2 * j] + list(rng.integers(0, N, size=12)))))
    d.flush(); twin.flush()
    g, w = d.sigma_block(rows, cc_), twin.sigma_block(rows, cc_)
    assert np.abs(g - w).max() / np.abs(w).max() <= TOL
    gs, ws = d.state, twin.state
    assert np.abs(gs - ws).max() / np.abs(ws).max() <= TOL

    def reading_a():
        d.associate_landmarks([(sx, sy)], n, n, deferred=True)

    def reading_b():
        twin.state_block(0, 3 + 2 * n)
        twin.score_sparse(cols, Hc, R, nu)
        twin.state_block(0, 3 + 2 * n)
        twin.correct_sparse_deferred(c, h5, R, wrapped)
        th = float(twin.state_block(0, 1)[0])
        twin.set_state_block(0, np.array([dc.normalize_angle(th)]))

    ta, tb = _wall_median(reading_a), _wall_median(reading_b)
    print(f"one reading at N={N}, known={n}: associate_landmarks {ta:.4f} ms, the spelled handle calls {tb:.4f} ms, "
          f"A / B = {ta / tb:.3f}")
    d.close(); twin.close()
    assert ta < tb, (ta, tb)
