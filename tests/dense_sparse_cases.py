"""Shared by tests/test_gpu_dense64_sparse.py and tests/test_dense64_sparse_host.py: a Jacobian given by its non-zero
columns (cols, Hc) and its dense form, the five columns of the reference's Hj (ekf_slam.cpp:140-178), and the numpy
spelling of the sparse calls -- which is the dense spelling (dc.np_correct, ds.np_scores) on the embedded H."""
import math

import numpy as np

import dense_correct_cases as dc
import dense_score_cases as ds


def embed(cols, Hc, N):
    """(cols [s], Hc [m][s]) -> H [m][N], or ([J][s], [J][m][s]) -> [J][m][N]: zero except H[:, cols[k]] = Hc[:, k]"""
    cols, Hc = np.asarray(cols), np.asarray(Hc, dtype=np.float64)
    if Hc.ndim == 2:
        H = np.zeros((Hc.shape[0], N))
        H[:, cols] = Hc
        return H
    return np.stack([embed(c, h, N) for c, h in zip(cols, Hc)])


def slam_cols(i):
    """the non-zero columns of the reference's Hj for landmark i: the pose and the landmark's pair"""
    return np.array([0, 1, 2, 3 + 2 * i, 4 + 2 * i], dtype=np.int32)


def extract(H, cols):
    """H [m][N] -> Hc [m][s]; every entry of H outside the listed columns must be exactly 0, so nothing is lost"""
    rest = np.ones(H.shape[1], dtype=bool)
    rest[cols] = False
    assert not H[:, rest].any()
    return np.ascontiguousarray(H[:, cols])


def slam_terms(pose, state, i, sx, sy):
    """dc.measurement_terms in sparse form, built without the N-wide rows (a full map has 5000 of them)
    -> cols [5], Hc [2][5], R, raw innovation, wrapped innovation"""
    th, x, y = pose
    dx, dy = state[3 + 2 * i] - x, state[4 + 2 * i] - y
    d = dx * dx + dy * dy
    q = math.sqrt(d)
    Hc = np.array([[0.0, -dx / q, -dy / q, dx / q, dy / q], [-1.0, dy / d, -dx / d, -dy / d, dx / d]])
    z = np.array([math.hypot(sx, sy), math.atan2(sy, sx)])
    zhat = np.array([q, dc.normalize_angle(math.atan2(dy, dx) - th)])
    raw = z - zhat
    return slam_cols(i), Hc, np.eye(2) * 0.01, raw, np.array([raw[0], dc.normalize_angle(raw[1])])


def candidate_terms(state, sx, sy, count=None):
    """ds.candidate_terms in sparse form -> cols [n][5], Hc [n][2][5], R [2][2] (shared), nu [n][2] (un-wrapped)"""
    n = (len(state) - 3) // 2 if count is None else count
    terms = [slam_terms(state[:3], state, i, sx, sy) for i in range(n)]
    return np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms]), terms[0][2], np.stack([t[3] for t in terms])


def np_correct(state, Sigma, cols, Hc, R, nu):
    return dc.np_correct(state, Sigma, embed(cols, Hc, len(state)), R, nu)


def np_scores(Sigma, cols, Hc, R, nu=None):
    return ds.np_scores(Sigma, embed(cols, Hc, Sigma.shape[0]), R, nu)


def sparse_correct_of(correct):
    """a dense-signature correct(state, Sigma, H, R, nu) for dc.replay_case out of a sparse one
    correct(state, Sigma, cols, Hc, R, nu): the five columns are extracted from the H that measurement_terms built (the
    landmark is read off the only non-zero column beyond the pose)"""
    def dense_signature(state, Sigma, H, R, nu):
        beyond = np.nonzero(H[:, 3:].any(axis=0))[0]
        cols = slam_cols(int(beyond[0]) // 2)
        return correct(state, Sigma, cols, extract(H, cols), R, nu)
    return dense_signature


def index_list(N, s, order, rng):
    """s distinct indices in [0, N): 'asc', 'desc' or 'scattered' (a random order)"""
    c = np.sort(rng.choice(N, size=s, replace=False))
    if order == "desc":
        c = c[::-1]
    elif order == "scattered":
        c = rng.permutation(c)
    return np.ascontiguousarray(c, dtype=np.int32)
