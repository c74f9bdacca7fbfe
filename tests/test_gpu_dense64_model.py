"""GPU: the reference's prediction() and measurement() on the fp64 dense handle's own state -- ekf_dense64_predict_landmarks
(the motion model built on the device from state[0], then propagate_block's launches), ekf_dense64_measure_landmarks (the
pose captured once per call, the first-call initialisation of all landmarks, per visible landmark the sparse or deferred
correction and the heading wrap) and capi.DenseEKFSLAM over both and associate_landmarks.  The bit-level claims are tested
as such: a twin handle driven by the existing public calls with the device-built operands; the device transcendentals are
held to numpy at 1e-12 (the bound of tests/test_gpu_dense64_landmarks.py; dense_model_cases.TWISTS says why it holds at the
branch boundary), the loops to the reference's own class at FP64_TOL."""
import ctypes as C

import numpy as np
import pytest

import dense_init_cases as ic
import dense_landmark_cases as lc
import dense_model_cases as mc
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
    """a handle with the state x, the covariance S, the live dimension `live` and `pending` rows left by seeded deferred
    corrections inside it (at most 12 rows each, so that they fit a live dimension of 13); built twice it holds the same
    bits twice"""
    d = hip.DensePropagator64(len(x))
    d.set(Sigma=S)
    if live is not None:
        d.live = live
    rng = np.random.default_rng(55)
    left = pending
    while left:
        m = min(left, 12)
        cols = rng.choice(d.live, size=5, replace=False)
        d.correct_sparse_deferred(cols, 0.1 * rng.standard_normal((m, 5)), np.eye(m), 0.01 * rng.standard_normal(m))
        left -= m
    assert d.pending == pending
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


def _ref(oracle):
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    return oracle.RefEKF


# ---- 1. the operands of prediction() --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", mc.THETAS)
def test_prediction_operands(hip, theta):
    x, S = lc.spiral_map(2)
    d = hip.DensePropagator64(len(x))
    d.set(Sigma=S)
    eye = np.eye(3)
    keep = np.ones((3, 3), dtype=bool)
    keep[1, 0] = keep[2, 0] = False
    for dth, dx in mc.TWISTS:
        x[0] = theta
        d.state = x
        _, Fr, upd = d.predict_landmarks(dth, dx, want_terms=True)
        wF, _, wu = mc.np_predict_terms(theta, dth, dx)
        err = max(np.abs(Fr - wF).max(), np.abs(upd - wu).max())
        print(f"theta={theta} dtheta={dth!r} dx={dx}: |operands - numpy| {err:.3e}")
        assert _bits(Fr[keep], eye[keep]), Fr                                  # the seven structural entries
        assert err <= TOL, (dth, Fr - wF, upd - wu)
        assert _bits(upd[0], np.float64(0.0 if mc.straight(dth) else dth))
        assert _bits(d.state_block(0, 1)[0], np.float64(theta) + upd[0])       # the heading is not wrapped (:99)
    p = hip.default_params()                                                   # the two fields that are used
    p.q_pose, p.straight_eps = 2e-4, 1e-3
    d.state = x
    assert d.predict_landmarks(0.999e-3, 0.1, want_terms=True, params=p)[2][0] == 0.0
    before = d.sigma_block([0, 1, 2], [0, 1, 2])
    d.state = x
    _, Fr, upd = d.predict_landmarks(1e-3, 0.1, want_terms=True, params=p)
    assert upd[0] == 1e-3
    want = (Fr @ before) @ Fr.T + 2e-4 * np.eye(3)                             # q_pose reaches Sigma
    assert np.abs(d.sigma_block([0, 1, 2], [0, 1, 2]) - want).max() <= TOL
    d.close()


# ---- 2. prediction against a twin ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("live", [23, 13])
@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("pending", [0, 2, 64])
def test_prediction_twin(hip, pending, carry, live):
    x, S = lc.spiral_map(10)                                                   # N = 23
    x[0] = 2.9
    d, twin = (_handle(hip, x, S, pending, carry, live) for _ in range(2))
    for dth, dx in ((0.3, 0.1), (0.0, 0.07)):                                  # both branches; the first passes pi unwrapped
        _, Fr, upd = d.predict_landmarks(dth, dx, want_terms=True)
        twin.propagate_block(0, Fr, mc.Q_POSE * np.eye(3), upd)
        assert d.pending == twin.pending == (pending if carry else 0)
    assert d.live == live
    got, want = _snapshot(d), _snapshot(twin)
    _same(got, want)
    assert got[1][0] > np.pi
    if live < len(x):
        assert _bits(got[1][live:], x[live:])
        assert _bits(got[2][live:, :], S[live:, :]) and _bits(got[2][:, live:], S[:, live:])
    d.close(); twin.close()


# ---- 3. the first-call initialisation --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_lm", [1, 255, 256, 257])
def test_first_call_initialisation(hip, n_lm):
    rng = np.random.default_rng(n_lm)
    N = 3 + 2 * n_lm
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-9.0, 9.0, size=N - 3)])   # stale landmark entries
    S = np.zeros((N, N))
    S[:3, :3] = 1e-3 * np.eye(3)
    S[3:, 3:] = ic.PRIOR * np.eye(N - 3)
    z = rng.uniform(1.0, 4.0, size=(n_lm, 2)) * rng.choice([-1.0, 1.0], size=(n_lm, 2))
    seen = n_lm // 2
    none, one = np.zeros(n_lm, dtype=np.uint8), np.zeros(n_lm, dtype=np.uint8)
    one[seen] = 1
    want = np.concatenate([ic.inverse_sensor(x[:3], *zi) for zi in z])
    d, untouched = _handle(hip, x, S), _handle(hip, x, S)
    flag, done, _ = d.measure_landmarks(z, none, False)
    assert flag is True and done == 0
    got = d.state
    assert _bits(got[:3], x[:3]) and np.abs(got[3:] - want).max() <= TOL, np.abs(got[3:] - want).max()
    assert _bits(d.sigma, untouched.sigma)                                     # Sigma is not touched (:113-128)
    d2 = _handle(hip, x, S)
    flag, done, _ = d2.measure_landmarks(z, one, False)                         # one visible: everyone is placed all the same
    assert flag is True and done == 1
    got2 = d2.state
    others = np.ones(N, dtype=bool)
    others[[0, 1, 2, 3 + 2 * seen, 4 + 2 * seen]] = False
    assert _bits(got2[others], got[others]) and np.abs(got2[3:] - want).max() <= 1e-9
    flag, done, _ = d2.measure_landmarks(z + 0.5, one, flag)                    # a second call initialises nothing
    assert flag is True and done == 1
    got3 = d2.state
    assert _bits(got3[others], got2[others])
    assert not _bits(got3[3 + 2 * seen:5 + 2 * seen], got2[3 + 2 * seen:5 + 2 * seen])
    for h in (d, d2, untouched):
        h.close()


# ---- 4. measurement against a twin ------------------------------------------------------------------------------------------------

def _visible(n_lm, V):
    vis = np.zeros(n_lm, dtype=np.uint8)
    vis[[0, n_lm - 1, n_lm // 2, 31, 7][:V]] = 1
    return vis


@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("pending", [0, 62])
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("V", [1, 2, 5])
@pytest.mark.parametrize("n_lm", [33, 64])
def test_measurement_twin(hip, n_lm, V, deferred, pending, carry):
    x, S = lc.spiral_map(n_lm)
    z = np.array([lc.reading_of(x, i, (0.03, -0.02)) for i in range(n_lm)])
    vis = _visible(n_lm, V)
    d, twin = (_handle(hip, x, S, pending, carry) for _ in range(2))
    flag, done, _, (Hc, nu) = d.measure_landmarks(z, vis, True, deferred, want_terms=True)
    assert flag is True and done == V and Hc.shape == (V, 2, 5)
    pose0 = x[:3].copy()
    for v, i in enumerate(np.nonzero(vis)[0]):
        if v == 0:                                                             # the first correction sees the state as it was
            _, wH, _, _, wnu = sp.slam_terms(pose0, x, i, z[i, 0], z[i, 1])
            assert _bits(Hc[0], wH) and np.abs(nu[0] - wnu).max() <= TOL
        (twin.correct_sparse_deferred if deferred else twin.correct_sparse)(sp.slam_cols(i), Hc[v], R, nu[v])
        lc.wrap_heading_always(twin)
    # 62 + 2 fit, the second pair forces the flush-first; the eager path flushes at once
    assert d.pending == twin.pending == ((pending + 2 * V if pending + 2 * V <= 64 else 2 * (V - 1)) if deferred else 0)
    _same(_snapshot(d), _snapshot(twin))
    d.close(); twin.close()


# ---- 5. the pose of the top of the call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", [False, True])
def test_snapshot_pose_against_the_reference(hip, oracle, deferred):
    Ref = _ref(oracle)
    x0, S0, z, vis = mc.snapshot_fixture()
    ref = Ref(2)
    ref.state, ref.cov = x0, S0
    ref.set_init_flag(True)
    ref.measurement(z.reshape(-1), vis)
    d = _handle(hip, x0, S0)
    flag, done, _ = d.measure_landmarks(z, vis, True, deferred)
    assert flag is True and done == 2
    w, e = worst(d.state, d.sigma, ref.state, ref.cov)
    d.close()
    print(f"snapshot fixture on the device (deferred={deferred}): {w:.3e}")
    assert w <= FP64_TOL, e


# ---- 6. a refused correction ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deferred", [False, True])
def test_measurement_singular_second(hip, deferred):
    """r_meas = 0 and the pose's and landmark 1's covariance zero: S of landmark 1 is 0.  Landmarks 0, 1, 2 visible: the
    call returns EKF_ERR_STATE from the second correction, the first stands, the third is not reached"""
    n = 6
    x, S = lc.spiral_map(n)
    for b in (slice(0, 3), slice(5, 7)):
        S[b, :] = 0.0
        S[:, b] = 0.0
    p = hip.default_params()
    p.r_meas = 0.0
    z = np.array([lc.reading_of(x, i) for i in range(n)])
    d, only0 = _handle(hip, x, S), _handle(hip, x, S)
    with pytest.raises(hip.EkfError) as e:
        d.measure_landmarks(z, [1, 1, 1, 0, 0, 0], True, deferred, params=p)
    assert e.value.status == STATE and e.value.corrected == 1 and e.value.initialised is True
    assert only0.measure_landmarks(z, [1, 0, 0, 0, 0, 0], True, deferred, params=p)[1] == 1
    assert d.pending == only0.pending == (2 if deferred else 0)
    assert not _bits(d.state_block(3, 2), x[3:5])                              # the first correction stands
    _same(_snapshot(d), _snapshot(only0))
    flag, done, _ = d.measure_landmarks(z, [0, 0, 1, 0, 0, 0], True, deferred, params=p)   # usable afterwards
    assert done == 1 and not _bits(d.state_block(7, 2), x[7:9])
    d.close(); only0.close()


# ---- 7. argument checks -----------------------------------------------------------------------------------------------------------

def test_model_refusals_change_nothing(hip):
    n = 10
    x, S = lc.spiral_map(n)
    live = 3 + 2 * 8
    d, ref = _handle(hip, x, S, 2, live=live), _handle(hip, x, S, 2, live=live)
    lib, h = d._lib, d._h
    z = (C.c_double * (2 * n))(*np.array([lc.reading_of(x, i) for i in range(n)]).reshape(-1))
    vis = (C.c_uint8 * n)(*([1] * n))
    flag = C.c_int(0)
    meas = lambda hh, n_lm, zz, vv, ff, flags: lib.ekf_dense64_measure_landmarks(hh, None, n_lm, zz, vv, ff, flags, None, None,
                                                                                  None, None)
    assert meas(None, 8, z, vis, C.byref(flag), 0) == INVALID
    assert meas(h, 8, None, vis, C.byref(flag), 0) == INVALID and meas(h, 8, z, None, C.byref(flag), 0) == INVALID
    assert meas(h, 8, z, vis, None, 0) == INVALID
    assert meas(h, 0, z, vis, C.byref(flag), 0) == INVALID and meas(h, -1, z, vis, C.byref(flag), 0) == INVALID
    assert meas(h, 9, z, vis, C.byref(flag), 0) == INVALID                      # 3 + 2 * 9 > live
    for bad in (2, 3, 4, 1 << 31):                                             # GROW_LIVE included
        assert meas(h, 8, z, vis, C.byref(flag), bad) == INVALID
    pred = lambda hh: lib.ekf_dense64_predict_landmarks(hh, None, 0.1, 0.05, None, None, None)
    assert pred(None) == INVALID
    d.live = ref.live = 2                                                       # (shrinking flushes: on both)
    assert pred(h) == INVALID
    assert flag.value == 0
    _same(_snapshot(d), _snapshot(ref))
    d.live = live
    assert pred(h) == 0                                                         # and the handle works
    d.close(); ref.close()


# ---- 8. both nodes' loops ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["eager", "deferred_carry"])
def test_slam_loop_against_the_reference(hip, oracle, mode):
    """the slam node: prediction() + measurement(), n = 6, 40 ticks, through capi.DenseEKFSLAM"""
    Ref = _ref(oracle)
    n = 6
    ref = Ref(n)
    f = hip.DenseEKFSLAM(n, deferred=mode != "eager", carry=mode != "eager")
    assert f.init_flag is False and f.known == 0 and _bits(f.state, np.zeros(3 + 2 * n))
    for t, (dth, dx, z, vis) in enumerate(mc.slam_scenario(n)):
        ref.prediction(dth, dx)
        ref.measurement(z.reshape(-1), vis)
        f.prediction(dth, dx)
        assert f.measurement(z, vis) == int(vis.sum())
        assert f.init_flag is True
        w = np.abs(f.pose - ref.state[:3]).max()
        assert w <= FP64_TOL, (t, w)
    if mode != "eager":
        assert f.handle.pending > 0                                            # prediction() carried them
    w, e = worst(f.state, f.handle.sigma, ref.state, ref.cov)
    f.close()
    print(f"slam loop through DenseEKFSLAM ({mode}): {w:.3e}")
    assert w <= FP64_TOL, e


def test_discovery_loop_against_the_reference(hip, oracle):
    """the unknown_data_assoc node: prediction() + data_association() from an empty map with grow_live, n = 6 in a handle
    with room for 8; `known` after every tick against the reference's known list, the decisions against the spelled numpy
    loop (which tests/test_dense64_model_host.py holds to the reference), state and Sigma at the end"""
    Ref = _ref(oracle)
    n = 6
    ref, known_ref = Ref(n), np.zeros(n, dtype=np.uint8)
    model, km = mc.numpy_filter(n), 0
    f = hip.DenseEKFSLAM(n, capacity=8, deferred=True, carry=True, grow_live=True)
    assert f.handle.live == 3 and f.handle.N == 19
    for t, (dth, dx, readings) in enumerate(mc.discovery_scenario(n)):
        ref.prediction(dth, dx)
        ref.data_association(readings, known_ref)
        mc.np_predict(model, dth, dx)
        km, want, _ = lc.np_associate(model, None, readings, km, n)
        f.prediction(dth, dx)
        assoc = f.data_association(readings)
        assert list(assoc) == list(want), (t, assoc, want)
        assert f.known == km == int(known_ref.sum()) and known_ref[:f.known].all(), (t, f.known, known_ref)
        assert f.handle.live == 3 + 2 * f.known
    assert f.known == n
    P = 3 + 2 * n
    gS = f.handle.sigma
    w, e = worst(f.state, gS[:P, :P], ref.state, ref.cov)
    assert _bits(gS[P:, P:], ic.PRIOR * np.eye(4)) and not gS[:P, P:].any() and not gS[P:, :P].any()   # the spare capacity
    f.close()
    print(f"discovery loop through DenseEKFSLAM: {w:.3e}")
    assert w <= FP64_TOL, e
