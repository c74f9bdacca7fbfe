"""Shared by tests/test_gpu_dense64_correct.py, tests/test_dense64_correct_host.py and
tests/golden/make_dense_correct_golden.py: the dense correction in numpy (the reference's literal spelling,
ekf_slam.cpp:178-192), the operands of the reference's own measurement model (:109-183) built from a state snapshot, and
the scenario that drives a RefEKF-like object to a correlated covariance."""
import math

import numpy as np


def normalize_angle(a):
    """rigid2d::normalize_angle (rigid2d.cpp:336-345)"""
    ang = math.fmod(math.fmod(a, 2 * math.pi) + 2 * math.pi, 2 * math.pi)
    return ang - 2 * math.pi if ang > math.pi else ang


def np_correct(state, Sigma, H, R, nu):
    """-> state', Sigma', nis with the reference's expressions: Ki = sigma*Hj.t()*(Hj*sigma*Hj.t() + R).i();
    state + Ki*z_diff; (eye - Ki*Hj)*sigma"""
    S = H @ Sigma @ H.T + R
    Si = np.linalg.inv(S)
    K = Sigma @ H.T @ Si
    return state + K @ nu, (np.eye(len(state)) - K @ H) @ Sigma, float(nu @ Si @ nu)


def measurement_terms(pose, state, i, sx, sy):
    """Hj (2 x N), R, z_diff un-wrapped, z_diff wrapped for landmark i and the reading (sx, sy): pose terms from `pose`
    (captured before the loop over landmarks, :109-111), landmark terms from the current `state` (:140-183)"""
    N = len(state)
    th, x, y = pose
    dx, dy = state[3 + 2 * i] - x, state[4 + 2 * i] - y
    d = dx * dx + dy * dy
    q = math.sqrt(d)
    H = np.zeros((2, N))
    H[0, :3] = [0.0, -dx / q, -dy / q]
    H[1, :3] = [-1.0, dy / d, -dx / d]
    H[0, 3 + 2 * i:5 + 2 * i] = [dx / q, dy / q]
    H[1, 3 + 2 * i:5 + 2 * i] = [-dy / d, dx / d]
    z = np.array([math.hypot(sx, sy), math.atan2(sy, sx)])
    zhat = np.array([q, normalize_angle(math.atan2(dy, dx) - th)])
    raw = z - zhat
    return H, np.eye(2) * 0.01, raw, np.array([raw[0], normalize_angle(raw[1])])


def replay_case(case, correct):
    """The recorded measurement() call as one correction per visible landmark.  correct(state, Sigma, H, R, nu) ->
    (state', Sigma', nis).  -> state, Sigma after the call and the nis of the FIRST visible landmark with the un-wrapped
    innovation (what calculate_maha_dis returns)"""
    state, Sigma = case["state0"].copy(), case["cov0"].copy()
    pose = state[:3].copy()
    sensor = case["sensor"]
    first_nis = None
    for i in np.nonzero(case["vis"])[0]:
        H, R, raw, wrapped = measurement_terms(pose, state, int(i), sensor[2 * i], sensor[2 * i + 1])
        if first_nis is None:
            first_nis = correct(state, Sigma, H, R, raw)[2]
        state, Sigma, _ = correct(state, Sigma, H, R, wrapped)
        state[0] = normalize_angle(state[0])   # :187
    return state, Sigma, first_nis


def record_case(Ref, n, n_visible, seed):
    """Run the reference a few steps in, then record one measurement() call with n_visible landmarks."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(-2.0, 2.0, size=(n, 2))
    world[np.hypot(world[:, 0], world[:, 1]) < 0.3] += 0.6
    r = Ref(n)
    pose = np.zeros(3)

    def frame(p):
        c, s = math.cos(p[0]), math.sin(p[0])
        d = world - p[1:]
        return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)

    def step(p, dth, dx):
        rr = dx / dth
        return np.array([p[0] + dth, p[1] - rr * math.sin(p[0]) + rr * math.sin(p[0] + dth),
                         p[2] + rr * math.cos(p[0]) - rr * math.cos(p[0] + dth)])

    for t in range(4):
        r.prediction(0.2, 0.1)
        pose = step(pose, 0.2, 0.1)
        vis = np.zeros(n, dtype=np.uint8)
        if t:
            vis[rng.choice(n, size=min(n, 3), replace=False)] = 1
        r.measurement((frame(pose) + rng.normal(0, 0.004, size=(n, 2))).reshape(-1), vis)
    r.prediction(0.15, 0.08)
    pose = step(pose, 0.15, 0.08)
    state0, cov0 = r.state, r.cov
    sensor = (frame(pose) + rng.normal(0, 0.004, size=(n, 2))).reshape(-1)
    vis = np.zeros(n, dtype=np.uint8)
    vis[rng.choice(n, size=n_visible, replace=False)] = 1
    i = int(np.nonzero(vis)[0][0])
    maha = r.maha(sensor[2 * i], sensor[2 * i + 1], i)
    r.measurement(sensor, vis)
    return {"n": n, "state0": state0, "cov0": cov0, "sensor": sensor, "vis": vis, "maha": maha,
            "state1": r.state, "cov1": r.cov}


CASES = [("one", 1, 11), ("three", 3, 12)]   # name, visible landmarks, seed offset
