"""Shared by tests/test_gpu_dense64_landmarks.py and tests/test_dense64_landmarks_host.py: the landmark front end of the
dense fp64 handle (ekf_dense64_score_landmarks, ekf_dense64_associate_landmarks) in numpy -- the reference's decision rule
(ekf_slam.cpp:293-330) as a function on a score vector, data_association() for a list of readings over ic.NumpyHandle built
from sp.candidate_terms / sp.slam_terms / ic.inverse_sensor -- and the fixtures of the rule's edges: equal scores, a
flagged (NaN) candidate, a full map."""
import math

import numpy as np

import dense_correct_cases as dc
import dense_init_cases as ic
import dense_sparse_cases as sp

DEFAULTS = {"sigma0_landmark": ic.PRIOR, "r_meas": ic.R_MEAS, "gate_new": 10.0, "gate_update": 1.0}
NOT_REACHED, DROPPED = -2, -1


def _p(params, name):
    return DEFAULTS[name] if params is None else float(getattr(params, name))


def rule(scores, known, n_max, gate_new=10.0, gate_update=1.0):
    """:293-330 on the scores of the known landmarks -> (win, kind, best): best = gate_new, win = known, ascending index
    with a strict < (the first of equals wins; a NaN never wins); kind 'new' (win == known < n_max: initialised, then
    corrected as the gate sees 0), 'update' (best < gate_update) or 'drop' (win = -1: between the gates, or a full map with
    nothing under gate_new).  best is the winning score, gate_new when no known landmark won."""
    best, win = float(gate_new), known
    for i, v in enumerate(scores):
        if v < best:
            best, win = float(v), i
    if win == known:
        return (known, "new", best) if known < n_max else (DROPPED, "drop", best)
    return (win, "update", best) if best < gate_update else (DROPPED, "drop", best)


def wrap_heading_always(d):
    """state(0) = normalize_angle(state(0)) stored unconditionally (:187 / :385): -0.0 becomes +0.0"""
    d.set_state_block(0, np.array([dc.normalize_angle(float(d.state_block(0, 1)[0]))]))


def np_associate(d, params, readings, known, n_max, deferred=False, scores=None):
    """data_association (:278-402) for the readings in order on a handle with the calls of ic.NumpyHandle (the eager and the
    deferred correction are the same algebra there) -> known, assoc [J], best [J]"""
    R = _p(params, "r_meas") * np.eye(2)
    assoc, best_out = [], []
    for sx, sy in readings:
        nis = []
        if known:
            x = d.state_block(0, 3 + 2 * known)
            cols, Hc, _, nu = sp.candidate_terms(x, sx, sy, count=known)
            nis = d.score_sparse(cols, Hc, R, nu)[0]
            if scores is not None:
                scores.append(np.array(nis))
        win, kind, best = rule(nis, known, n_max, _p(params, "gate_new"), _p(params, "gate_update"))
        best_out.append(best)
        if kind == "drop":
            assoc.append(DROPPED)
            continue
        if kind == "new":
            xb = ic.inverse_sensor(d.state_block(0, 3), sx, sy)
            d.init_block(3 + 2 * known, W=_p(params, "sigma0_landmark") * np.eye(2), xb=xb)
            known += 1
            if not 0.0 < _p(params, "gate_update"):
                assoc.append(DROPPED)
                continue
        x = d.state_block(0, 3 + 2 * known)
        c, h, _, _, wrapped = sp.slam_terms(x[:3], x, win, sx, sy)
        d.correct_sparse(c, h, R, wrapped)
        wrap_heading_always(d)
        assoc.append(win)
    return known, np.array(assoc, dtype=np.int32), np.array(best_out)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------

def spiral_map(count, seed=3):
    """state [3 + 2 count] with the landmarks on a spiral (neighbours far apart in terms of their 0.1 m sigma) and a
    covariance that is SPD with every landmark correlated with the pose and with nothing else -> state, Sigma"""
    rng = np.random.default_rng(seed)
    i = np.arange(count)
    rad, ang = 2.0 + 0.05 * i, 0.7 * i
    x = np.concatenate([[0.3, 0.1, -0.2], np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1)])
    N = 3 + 2 * count
    S = np.zeros((N, N))
    S[:3, :3] = 1e-3 * (np.eye(3) + 0.1 * rng.standard_normal((3, 3)))
    for k in range(count):
        b = slice(3 + 2 * k, 5 + 2 * k)
        S[b, b] = 1e-2 * (np.eye(2) + 0.1 * rng.standard_normal((2, 2)))
        S[:3, b] = 1e-4 * rng.standard_normal((3, 2))
        S[b, :3] = 1e-4 * rng.standard_normal((2, 3))
    return x, S


def reading_of(state, i, off=(0.01, -0.005)):
    """the reading (sx, sy) that sees landmark i of `state`, a little off"""
    th, x, y = state[:3]
    dx, dy = state[3 + 2 * i] - x + off[0], state[4 + 2 * i] - y + off[1]
    c, s = math.cos(th), math.sin(th)
    return c * dx + s * dy, -s * dx + c * dy


def tie_fixture(count, a, b, nan_at=None):
    """landmarks a < b with identical coordinates and identical 5 x 5 blocks against the pose: equal score bits; nan_at:
    a landmark placed exactly at the robot's position (d = 0: a flagged NaN candidate) -> state, Sigma, (sx, sy)"""
    x, S = spiral_map(count)
    ia, ib = slice(3 + 2 * a, 5 + 2 * a), slice(3 + 2 * b, 5 + 2 * b)
    x[ib] = x[ia]
    S[ib, ib], S[:3, ib], S[ib, :3] = S[ia, ia], S[:3, ia], S[ia, :3]
    if nan_at is not None:
        x[3 + 2 * nan_at], x[4 + 2 * nan_at] = x[1], x[2]
    return x, S, reading_of(x, a)


def full_map_fixture(n=4):
    """known == n_max == n -> state, Sigma, a reading far from everything (dropped), a reading on landmark 2 (corrected)"""
    x, S = spiral_map(n, seed=11)
    return x, S, (40.0, -35.0), reading_of(x, 2)
