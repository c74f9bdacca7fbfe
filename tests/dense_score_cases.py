"""Shared by tests/test_gpu_dense64_score.py, tests/test_dense64_score_host.py and
tests/golden/make_dense_score_golden.py: the candidate scores in numpy (the reference's literal spelling,
ekf_slam.cpp:266-269), the operands of calculate_maha_dis (:217-276) for every landmark built from a state snapshot, the
reference's decision rule (:293-330) and the scenario whose readings a RefEKF-like object scores."""
import math

import numpy as np

import dense_correct_cases as dc

MARGIN = 1e-6   # relative distance every score keeps from a gate, and every winner from its runner-up


def np_scores(Sigma, H, R, nu=None):
    """-> S [J][m][m], nis [J] (None without nu) with the reference's expressions, one candidate at a time:
    psi = Hj*sigma*Hj.t() + R;  d = z_diff.t()*psi.i()*z_diff"""
    J, m, _ = H.shape
    S = np.empty((J, m, m))
    nis = None if nu is None else np.empty(J)
    for j in range(J):
        S[j] = H[j] @ Sigma @ H[j].T + (R if R.ndim == 2 else R[j])
        if nu is not None:
            nis[j] = float(nu[j] @ np.linalg.inv(S[j]) @ nu[j])
    return S, nis


def candidate_terms(state, sx, sy, count=None):
    """H [n][2][N], R [2][2] (shared), nu [n][2] of the reading (sx, sy) against every landmark: the pose and the landmark
    from the current state, the innovation UN-wrapped (z - z_hat, :269)"""
    n = (len(state) - 3) // 2 if count is None else count
    terms = [dc.measurement_terms(state[:3], state, i, sx, sy) for i in range(n)]
    return np.stack([t[0] for t in terms]), terms[0][1], np.stack([t[2] for t in terms])


def reference_rule(scores):
    """data_association()'s decision for one reading (:293-330): scan in ascending order, strict <, start value 10.0; the
    winner is updated when its score is below 1.0.  -> (winner or len(scores) for 'no known landmark', class) with class
    'new' (nobody below 10: a landmark is initialised), 'update' (< 1.0) or 'ignore' (between the gates)"""
    best, idx = 10.0, len(scores)
    for i, d in enumerate(scores):
        if d < best:
            best, idx = d, i
    if idx == len(scores):
        return idx, "new"
    return idx, "update" if best < 1.0 else "ignore"


def margins_hold(scores, margin=MARGIN):
    """every score at least `margin` (relative) away from 10.0 and 1.0, the winner that far from its runner-up"""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    if not np.all(np.isfinite(s)):
        return False
    for gate in (10.0, 1.0):
        if np.any(np.abs(s - gate) <= margin * gate):
            return False
    return len(s) < 2 or s[1] - s[0] > margin * abs(s[1])


def record_scores(Ref, n, seed, n_readings=8):
    """Run the reference a few predict / measure steps (every landmark seen once, then a few at a time), then score
    n_readings readings -- most of them noisy sightings of known landmarks, the last two of nothing on the map -- against
    every landmark with calculate_maha_dis."""
    rng = np.random.default_rng(seed)
    world = rng.uniform(-2.0, 2.0, size=(n, 2))
    world[np.hypot(world[:, 0], world[:, 1]) < 0.3] += 0.6
    r = Ref(n)
    pose = np.zeros(3)

    def frame(p, pts):
        c, s = math.cos(p[0]), math.sin(p[0])
        d = pts - p[1:]
        return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)

    def step(p, dth, dx):
        rr = dx / dth
        return np.array([p[0] + dth, p[1] - rr * math.sin(p[0]) + rr * math.sin(p[0] + dth),
                         p[2] + rr * math.cos(p[0]) - rr * math.cos(p[0] + dth)])

    for t in range(4):
        r.prediction(0.2, 0.1)
        pose = step(pose, 0.2, 0.1)
        vis = np.zeros(n, dtype=np.uint8)
        if t == 0:
            vis[:] = 1
        else:
            vis[rng.choice(n, size=min(n, 3), replace=False)] = 1
        r.measurement((frame(pose, world) + rng.normal(0, 0.004, size=(n, 2))).reshape(-1), vis)
    r.prediction(0.15, 0.08)
    pose = step(pose, 0.15, 0.08)
    seen = rng.choice(n, size=n_readings - 2, replace=False)
    pts = np.concatenate([world[seen] + rng.normal(0, 0.03, size=(len(seen), 2)),
                          rng.uniform(2.5, 3.5, size=(2, 2)) * rng.choice([-1.0, 1.0], size=(2, 2))])
    readings = frame(pose, pts)
    maha = np.array([[r.maha(mx, my, i) for i in range(n)] for mx, my in readings])
    return {"n": n, "state": r.state, "cov": r.cov, "readings": readings, "maha": maha}


SEEDS = {20: 2020, 200: 2200}   # per n: the seed of the recorded scenario (its margins are asserted where it is used)
