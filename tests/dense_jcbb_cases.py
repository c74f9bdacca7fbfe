"""Shared by tests/test_gpu_dense64_jcbb.py and tests/test_dense64_jcbb_host.py: the joint compatibility association of the
dense fp64 handle (ekf_dense64_jcbb_candidates, ekf_dense64_jcbb_search, ekf_dense64_associate_jcbb) in numpy, in the order
of operations include/ekfslam.h states -- the selection of the candidates on a score matrix (np_select), the cross blocks
(np_cross, with the exact fma of dense_frame_cases), the bounded search with its incremental Cholesky factor (np_search), the
whole call over ic.NumpyHandle (np_associate_jcbb) -- and the fixtures: crossed, spurious, ties, integer, budget."""
import math

import numpy as np

import dense_init_cases as ic
import dense_joint_cases as jc
import dense_landmark_cases as lc
import dense_sparse_cases as sp
from dense_frame_cases import fma

MAX_READINGS, MAX_CAND, MAX_NODES = 32, 4, 1 << 22
MARGIN = jc.MARGIN


class P:
    """the fields of ekf_params the models read (lc._p)"""

    def __init__(self, r_meas=1e-4, gate_new=10.0, gate_update=1.0, sigma0_landmark=ic.PRIOR):
        self.r_meas, self.gate_new, self.gate_update, self.sigma0_landmark = r_meas, gate_new, gate_update, sigma0_landmark


# ---- the models -----------------------------------------------------------------------------------------------------------

def np_select(scores, gate_ic, max_cand=MAX_CAND, gate_new=10.0):
    """scores [J][known] -> cand_lm [J] (lists in ascending (score, index), score < gate_ic, NaN never), cand_nis [J],
    best [J] (the minimum, gate_new when nothing lies below it), is_new [J]"""
    cand_lm, cand_nis, best, is_new = [], [], [], []
    for row in scores:
        pairs = sorted((float(v), i) for i, v in enumerate(row) if v == v)
        keep = [(v, i) for v, i in pairs if v < gate_ic][:max_cand]
        cand_lm.append([i for _, i in keep])
        cand_nis.append([v for v, _ in keep])
        lo = pairs[0][0] if pairs else math.inf
        best.append(lo if lo < gate_new else float(gate_new))
        is_new.append(0 if lo < gate_new else 1)
    return cand_lm, cand_nis, best, is_new


def flatten(cand_lm, cand_nis):
    """the candidates numbered in ascending (j, rank) -> reading_of [P], lm_of [P], nis [P]"""
    reading_of = [j for j, row in enumerate(cand_lm) for _ in row]
    return (np.array(reading_of, dtype=np.int32), np.array([i for row in cand_lm for i in row], dtype=np.int32),
            np.array([v for row in cand_nis for v in row], dtype=np.float64))


def np_cross(Sigma, cols, Hc, r_meas):
    """cols [P][5], Hc [P][2][5] -> W [2P][2P]: block (p, q) = Hc_p Sigma[cols_p, cols_q] Hc_q^T, every dot product from +0 in
    ascending k with one fma per term, T' rounded in between; p == q: + r_meas delta_ab by one plain addition"""
    n = len(cols)
    W = np.zeros((2 * n, 2 * n))
    Hc = np.asarray(Hc, dtype=np.float64)
    for p in range(n):
        for q in range(n):
            G = Sigma[np.ix_(cols[p], cols[q])]
            T = np.zeros((2, 5))
            for k in range(5):
                T = fma(Hc[p][:, k:k + 1], G[k:k + 1, :], T)
            B = np.zeros((2, 2))
            for k in range(5):
                B = fma(T[:, k:k + 1], Hc[q][:, k:k + 1].T, B)
            if p == q:
                B = B + r_meas * np.eye(2)
            W[2 * p:2 * p + 2, 2 * q:2 * q + 2] = B
    return W


def np_search(J, reading_of, lm_of, W, nu, gate_joint, max_nodes=1 << 16, cmps=None):
    """the search of ekf_dense64_jcbb.hpp -> assign [J], report {n_pairs, exhausted, nodes, d2}.  cmps (a list): every
    deciding comparison (value, against) -- a joint d2 against its gate, a leaf's d2 against the incumbent's at equal pairings"""
    P = len(reading_of)
    nu = np.asarray(nu, dtype=np.float64).reshape(-1)
    first = [0] * (J + 1)
    for p in range(P):
        first[reading_of[p] + 1] += 1
    for j in range(J):
        first[j + 1] += first[j]
    to_come = [0] * (J + 1)
    for j in range(J - 1, -1, -1):
        to_come[j] = to_come[j + 1] + (1 if first[j + 1] > first[j] else 0)
    L, z = np.zeros((2 * J, 2 * J)), np.zeros(2 * J)
    path, cur = [0] * J, [-1] * J
    st = {"best": [-1] * J, "pairs": 0, "d2": 0.0, "nodes": 0, "exhausted": 0}

    def extend(m, p, d2):
        for a in range(2):
            r = 2 * m + a
            for c in range(r):
                mc = c >> 1
                v = W[2 * p + a, 2 * (p if mc == m else path[mc]) + (c & 1)]
                for t in range(c):
                    v = v - L[r, t] * L[c, t]
                L[r, c] = v / L[c, c]
            d = W[2 * p + a, 2 * p + a]
            for t in range(r):
                d = d - L[r, t] * L[r, t]
            if not (math.isfinite(d) and d > 0.0):
                return None
            L[r, r] = math.sqrt(d)
            s = nu[2 * p + a]
            for t in range(r):
                s = s - L[r, t] * z[t]
            z[r] = s / L[r, r]
            d2 = d2 + z[r] * z[r]
        return float(d2)

    def visit(j, m, d2):
        if st["nodes"] >= max_nodes:
            st["exhausted"] = 1
            return
        st["nodes"] += 1
        if j == J:
            if m == st["pairs"] and m > 0 and cmps is not None:
                cmps.append((d2, st["d2"]))
            if m > st["pairs"] or (m == st["pairs"] and d2 < st["d2"]):
                st["pairs"], st["d2"], st["best"] = m, d2, list(cur)
            return
        if m + to_come[j] < st["pairs"]:
            return
        for p in range(first[j], first[j + 1]):
            if any(lm_of[path[i]] == lm_of[p] for i in range(m)):
                continue
            e = extend(m, p, d2)
            if e is not None and cmps is not None:
                cmps.append((e, float(gate_joint[m])))
            if e is None or not e < gate_joint[m]:
                continue
            path[m], cur[j] = p, p
            visit(j + 1, m + 1, e)
            cur[j] = -1
            if st["exhausted"]:
                return
        visit(j + 1, m, d2)

    visit(0, 0, 0.0)
    return (np.array(st["best"], dtype=np.int32),
            {"n_pairs": st["pairs"], "exhausted": st["exhausted"], "nodes": st["nodes"], "d2": float(st["d2"])})


def default_gates(J, gate_ic):
    return np.array([float(k + 1) * gate_ic for k in range(J)])


def np_decide(d, params, readings, known, gate_ic, gate_joint=None, max_nodes=1 << 16, cmps=None, scores=None):
    """scores, candidates, cross blocks and the search on a handle with the calls of ic.NumpyHandle -> (lms [J]: the landmark
    of a paired reading or -1, is_new [J], best [J], report with n_cand)"""
    readings = [tuple(float(v) for v in z) for z in readings]
    J = len(readings)
    nis = jc.np_scores(d, params, readings, known)
    if scores is not None:
        scores.append(nis.copy())
    cand_lm, cand_nis, best, is_new = np_select(nis, gate_ic, MAX_CAND, lc._p(params, "gate_new"))
    reading_of, lm_of, _ = flatten(cand_lm, cand_nis)
    x = d.state_block(0, 3 + 2 * known)
    terms = [sp.slam_terms(x[:3], x, int(i), *readings[j]) for j, i in zip(reading_of, lm_of)]
    cols, Hc = [t[0] for t in terms], [t[1] for t in terms]
    nu = np.array([t[3] for t in terms]).reshape(-1)
    W = np_cross(d.sigma, cols, Hc, lc._p(params, "r_meas")) if len(terms) else np.zeros((0, 0))
    gates = default_gates(J, gate_ic) if gate_joint is None else np.asarray(gate_joint, dtype=np.float64)
    assign, rep = np_search(J, reading_of, lm_of, W, nu, gates, max_nodes, cmps)
    rep["n_cand"] = len(reading_of)
    return [int(lm_of[a]) if a >= 0 else -1 for a in assign], is_new, best, rep


def np_associate_jcbb(d, params, readings, known, n_max, gate_ic, gate_joint=None, max_nodes=1 << 16):
    """ekf_dense64_associate_jcbb on a handle with the calls of ic.NumpyHandle -> known, assoc [J], best [J], report, n_groups:
    np_decide, then the slots, the initialisation and the stacked corrections of jc.np_associate_joint"""
    readings = [tuple(float(v) for v in z) for z in readings]
    J = len(readings)
    r_meas, sigma0, gate_update = lc._p(params, "r_meas"), lc._p(params, "sigma0_landmark"), lc._p(params, "gate_update")
    lms, is_new, best, rep = np_decide(d, params, readings, known, gate_ic, gate_joint, max_nodes)
    kinds, slot = [jc.DROP] * J, known
    for j in range(J):
        if lms[j] >= 0:
            kinds[j] = jc.MATCH
        elif is_new[j] and slot < n_max:
            kinds[j], lms[j], slot = jc.NEW, slot, slot + 1
    pose = d.state_block(0, 3)
    fresh = [j for j, k in enumerate(kinds) if k == jc.NEW]
    for g in range(0, len(fresh), jc.INIT_GROUP):
        grp = fresh[g:g + jc.INIT_GROUP]
        xb = np.concatenate([ic.inverse_sensor(pose, *readings[j]) for j in grp])
        d.init_block(3 + 2 * (known + g), W=sigma0 * np.eye(2 * len(grp)), xb=xb)
    known += len(fresh)
    assoc = [lc.DROPPED] * J
    groups = jc.groups_of(jc.pairs_of(kinds, lms, gate_update))
    for grp in groups:
        x = d.state_block(0, 3 + 2 * known)
        cols, Hc, nu = jc.np_joint_operands(x, [i for _, i in grp], [readings[j] for j, _ in grp])
        d.correct_sparse(cols, Hc, r_meas * np.eye(2 * len(grp)), nu)
        lc.wrap_heading_always(d)
        for j, i in grp:
            assoc[j] = i
    rep.update(n_new=len(fresh), n_drop=J - rep["n_pairs"] - len(fresh))
    return known, np.array(assoc, dtype=np.int32), np.array(best), rep, len(groups)


def margins_hold(scores, cmps, gate_ic, gate_new=10.0, gate_update=1.0):
    """every score keeps MARGIN (relative) from gate_ic, gate_new and gate_update, every recorded comparison from its bound"""
    for v in np.asarray(scores, dtype=np.float64).reshape(-1):
        if v == v and any(abs(v - g) < MARGIN * g for g in (gate_ic, gate_new, gate_update)):
            return False
    return all(abs(v - g) >= MARGIN * max(abs(g), abs(v)) for v, g in cmps)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
# The robot stands at the origin with heading 0 and a pose covariance that is large along y; the map is tight in relative
# terms (1e-4 per landmark coordinate) and uncorrelated with the pose, so a pose error along y moves every reading by ONE
# common offset.  `extra` landmarks far away pad the map to the handle under test; n_max = every landmark.

def _map(points, n_lm, pose_var_y=0.04, rel=1e-4):
    pts = list(points) + [(30.0 + 3.0 * i, 25.0 - 2.0 * i) for i in range(n_lm - len(points))]
    x = np.concatenate([[0.0, 0.0, 0.0], np.array(pts, dtype=np.float64).reshape(-1)])
    S = np.diag(np.concatenate([[1e-6, 1e-6, pose_var_y], rel * np.ones(2 * n_lm)]))
    return x, S


def crossed(n_lm=12):
    """A and B 0.3 m apart, both readings 0.2 m off along y: reading a is nearer to B than to A -> x, S, known, readings,
    params, gate_ic, truth [J] (the landmark each reading saw)"""
    x, S = _map([(2.0, 0.15), (2.0, -0.15)], n_lm)
    readings = np.array([(2.0, 0.15 - 0.2), (2.0, -0.15 - 0.2)])
    return x, S, n_lm, readings, P(), 4.0, [0, 1]


def spurious(n_lm=12):
    """three readings 0.15 m off along -y from landmarks 0, 1, 2; a fourth 0.15 m off along +y from landmark 3: under gate_ic
    (and gate_update) on its own, jointly incompatible with the three -> as crossed(); truth -1: belongs to nothing"""
    pts = [(2.0, 1.5), (2.5, 0.0), (2.0, -1.5), (3.0, 0.8)]
    x, S = _map(pts, n_lm)
    readings = np.array([(px, py - 0.15) for px, py in pts[:3]] + [(pts[3][0], pts[3][1] + 0.15)])
    return x, S, n_lm, readings, P(), 4.0, [0, 1, 2, -1]


def ties_scores():
    """a score matrix of exactly representable values: two landmarks with equal scores, one NaN, one score exactly gate_ic
    -> scores [2][6], gate_ic, the candidates np_select must give"""
    nan = float("nan")
    scores = [[0.5, nan, 0.25, 0.25, 2.0, 1.0], [2.0, 3.0, nan, 2.0, 0.125, 2.0]]
    return scores, 2.0, [[2, 3, 0, 5], [4]]


def integer(n_lm=12):
    """the robot at the origin, landmarks on the axes at powers of two, Sigma = 64 I + small integers (not symmetric): Hj holds
    0, +-1 and +-1/q only, so every product and sum of np_cross is exact whatever the order -> x, S, known, readings, params,
    gate_ic"""
    pts = [(1.0, 0.0), (2.0, 0.0), (4.0, 0.0), (8.0, 0.0), (0.0, 1.0), (0.0, 2.0), (0.0, 4.0), (0.0, -1.0), (0.0, -2.0),
           (-1.0, 0.0), (-2.0, 0.0), (-4.0, 0.0)][:n_lm]
    x = np.concatenate([[0.0, 0.0, 0.0], np.array(pts).reshape(-1)])
    N = len(x)
    rng = np.random.default_rng(17)
    S = 64.0 * np.eye(N) + rng.integers(-3, 4, size=(N, N)).astype(np.float64)
    readings = np.array([(1.5, 0.25), (0.25, 1.5), (-1.5, 0.0), (0.0, -1.5), (4.0, 1.0)])
    return x, S, len(pts), readings, P(r_meas=0.25, gate_new=1e6), 1e5


def budget(J=8, C=4):
    """J readings x C mutually compatible candidates on distinct landmarks, W = I, the innovation growing with the rank: the
    first leaf (every reading at rank 0) is the best hypothesis there is -> J, reading_of, lm_of, nis, W, nu, gates, and the
    incumbent a search of 50 nodes must end with"""
    n = J * C
    reading_of = np.repeat(np.arange(J, dtype=np.int32), C)
    lm_of = np.arange(n, dtype=np.int32)
    nu = np.zeros((n, 2))
    nu[:, 0] = 0.125 * (1 + np.tile(np.arange(C), J))
    nis = nu[:, 0] ** 2
    return J, reading_of, lm_of, nis, np.eye(2 * n), nu, default_gates(J, 100.0), np.arange(0, n, C, dtype=np.int32)
