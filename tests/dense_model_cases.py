"""Shared by tests/test_gpu_dense64_model.py and tests/test_dense64_model_host.py: the reference's prediction() (ekf_slam.cpp:55-106)
and measurement() (:108-197) in numpy over the calls of ic.NumpyHandle -- the motion model as operands of propagate_block,
measurement() with the pose captured once per call (snapshot=True, the reference) or re-read per landmark (snapshot=False,
what data_association's model would do: the wrong one here) -- and the fixtures: the branch boundary of :79, a known-
association scenario whose visible sets have 0, 1, 2 and all landmarks, the snapshot discriminator, a discovery scenario."""
import math

import numpy as np

import dense_block_cases as bc
import dense_init_cases as ic
import dense_landmark_cases as lc
import dense_sparse_cases as sp

Q_POSE, STRAIGHT_EPS = 1e-4, 1e-6   # the reference's constants (:41-43, :79)

# (dtheta, dx) at the branch boundary of :79 and away from it.  |dtheta| == 1e-6 takes the ARC branch (strict <), where
# update = -(dx/dtheta) sin(theta) + (dx/dtheta) sin(theta + dtheta) cancels: with sin / cos good to 2 ulp on the device and
# 1 on the host, each of the two terms may differ by q * 3.3e-16, q = |dx / dtheta|.  dx is chosen so that q <= 500 there:
# 2 * 500 * 3.3e-16 = 3.3e-13, inside the 1e-12 the device transcendentals are held to.
TWISTS = [(0.0, 0.07), (-0.0, 0.07), (0.999e-6, 0.07), (1e-6, 5e-4), (-1e-6, 5e-4), (0.3, 0.1), (-2.5, 0.2)]
THETAS = [0.0, 3.1, -3.1, 40.0]   # 40: a heading prediction() has not wrapped (:99)


def _p(params, name, default):
    return default if params is None else float(getattr(params, name))


def straight(dtheta, params=None):
    return abs(dtheta) < _p(params, "straight_eps", STRAIGHT_EPS)


def np_predict_terms(theta, dtheta, dx, params=None):
    """-> Fr (3 x 3 = I + A), Qr = q_pose I, update (3) of :67-96 for the heading theta, in the reference's expression order"""
    th = float(theta)
    A, upd = np.zeros((3, 3)), np.zeros(3)
    if straight(dtheta, params):
        upd[0] = 0
        upd[1] = dx * math.cos(th)
        upd[2] = dx * math.sin(th)
        A[1, 0] = -dx * math.sin(th)
        A[2, 0] = dx * math.cos(th)
    else:
        upd[0] = dtheta
        upd[1] = -(dx / dtheta) * math.sin(th) + (dx / dtheta) * math.sin(th + dtheta)
        upd[2] = (dx / dtheta) * math.cos(th) - (dx / dtheta) * math.cos(th + dtheta)
        A[1, 0] = -(dx / dtheta) * math.cos(th) + (dx / dtheta) * math.cos(th + dtheta)
        A[2, 0] = -(dx / dtheta) * math.sin(th) + (dx / dtheta) * math.sin(th + dtheta)
    return np.eye(3) + A, np.eye(3) * _p(params, "q_pose", Q_POSE), upd


def np_predict(d_model, dtheta, dx, params=None):
    """prediction() on a handle with the calls of ic.NumpyHandle"""
    Fr, Qr, upd = np_predict_terms(d_model.state_block(0, 1)[0], dtheta, dx, params)
    d_model.propagate_block(0, Fr, Qr, upd)


def np_measure(d_model, sensor_xy, visible, init_flag, snapshot=True):
    """measurement() on a handle with the calls of ic.NumpyHandle (state_block, set_state_block, correct_sparse): the
    first-call initialisation of ALL landmarks (:113-128), then per visible landmark in ascending order the correction with
    the pose of the top of the call (snapshot=True, :109-111) or the current one (False) and the landmark from the current
    state, and the unconditional heading wrap (:187).  -> the new init flag"""
    z = np.asarray(sensor_xy, dtype=np.float64).reshape(-1, 2)
    n = len(z)
    pose = d_model.state_block(0, 3)
    if not init_flag:
        for i in range(n):
            d_model.set_state_block(3 + 2 * i, ic.inverse_sensor(pose, z[i, 0], z[i, 1]))
    for i in range(n):
        if not visible[i]:
            continue
        x = d_model.state_block(0, 3 + 2 * n)
        c, h, R, _, wrapped = sp.slam_terms(pose if snapshot else x[:3], x, i, z[i, 0], z[i, 1])
        d_model.correct_sparse(c, h, R, wrapped)
        lc.wrap_heading_always(d_model)
    return True


def numpy_filter(n):
    """the reference's constructor (:27-46) as an ic.NumpyHandle"""
    d = ic.NumpyHandle(3 + 2 * n)
    x0, S0 = ic.prior_start(n)
    d.set(S0)
    d.state = x0
    return d


# ---- fixtures ------------------------------------------------------------------------------------------------------------------

def _body(pose, pts):
    c, s = math.cos(pose[0]), math.sin(pose[0])
    d = np.asarray(pts) - pose[1:]
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)


def _world(n):
    ang = 2 * math.pi * np.arange(n) / n
    rad = 1.5 + 1.0 * (np.arange(n) % 3)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)


def _twist(t):
    return (0.0, 0.05) if t % 7 == 3 else (0.2 + 0.01 * (t % 3), 0.06)   # both branches; the heading passes pi


def slam_scenario(n=6, ticks=40, seed=21):
    """the slam node's loop: per tick a twist, a reading of EVERY landmark (n, 2) and a visible list.  The first call sees
    landmark 3 only (all n are initialised from it); the visible sets then cycle through 0, 1, 2 and all n landmarks.
    -> [(dtheta, dx, sensor_xy (n, 2), visible (n,) uint8)]"""
    rng = np.random.default_rng(seed)
    world, pose, out = _world(n), np.zeros(3), []
    for t in range(ticks):
        dth, dx = _twist(t)
        pose = pose + bc.model_operands(pose, dth, dx)[2]
        z = _body(pose, world + rng.normal(0, 0.004, size=(n, 2)))
        vis = np.zeros(n, dtype=np.uint8)
        if t == 0:
            vis[3] = 1
        else:
            k = (0, 1, 2, n)[t % 4]
            vis[rng.permutation(n)[:k]] = 1
        out.append((dth, dx, z, vis))
    return out


def discovery_scenario(n=6, ticks=40, seed=22):
    """the unknown_data_assoc node's loop from an empty map: landmark k may be seen from tick 3 k on, a tick brings one to
    three readings of the landmarks seen so far and the next one, in a seeded order; the landmarks sit 60 degrees and a
    metre apart, so a wrong candidate scores far beyond the gate.  -> [(dtheta, dx, readings (k, 2))]"""
    rng = np.random.default_rng(seed)
    world, pose, out = _world(n), np.zeros(3), []
    for t in range(ticks):
        dth, dx = _twist(t)
        pose = pose + bc.model_operands(pose, dth, dx)[2]
        allowed = min(n, 1 + t // 3)
        seen = rng.permutation(allowed)[:int(rng.integers(1, 4))]
        out.append((dth, dx, _body(pose, world[seen] + rng.normal(0, 0.004, size=(len(seen), 2)))))
    return out


def snapshot_fixture():
    """n = 2, both visible, where the pose of :109-111 and the current pose differ by more than 1e-3 at the second
    correction: ten predictions and a measurement() that initialises (numpy, deterministic), five more predictions, then
    the call under test, whose reading of landmark 0 is off by 0.4 m so that its correction moves the pose.
    -> state0, Sigma0 in front of that call (init flag set), sensor_xy (2, 2), visible (2,)"""
    world = np.array([[2.0, 0.5], [-0.5, 1.8]])
    d = numpy_filter(2)
    for t in range(10):
        np_predict(d, *_twist(t))
    np_measure(d, _body(d.state_block(0, 3), world), [1, 1], False)
    for t in range(10, 15):
        np_predict(d, *_twist(t))
    z = _body(d.state_block(0, 3), world + np.array([[0.4, -0.3], [0.01, 0.02]]))
    return d.state.copy(), d.sigma.copy(), z, np.array([1, 1], dtype=np.uint8)
