"""Shared by tests/test_gpu_dense64_joint.py and tests/test_dense64_joint_host.py: the joint association of the dense fp64
handle (ekf_dense64_score_readings, ekf_dense64_joint_operands, ekf_dense64_associate_joint) in numpy -- the joint rule as a
function on a J x known score matrix, the stacked operands of a group of pairs, and the whole call over ic.NumpyHandle -- and
the fixture in which the joint and the sequential rule decide alike with every deciding score well away from both gates."""
import numpy as np

import dense_block_cases as bc
import dense_correct_cases as dc
import dense_init_cases as ic
import dense_landmark_cases as lc
import dense_sparse_cases as sp

MAX_READINGS, MAX_PAIRS, INIT_GROUP = 128, 30, 32
MATCH, NEW, DROP = "match", "new", "drop"
MARGIN = 1e-3   # relative distance every deciding score keeps from both gates in joint_vs_sequential()


def joint_rule(scores, known, n_max, gate_new=10.0, gate_update=1.0):
    """scores [J][known] (NaN: a flagged candidate) -> (kinds [J], lms [J], best [J]).  Per reading lc.rule's minimum; MATCH
    when win < known and best < gate_update, NEW when win == known, otherwise DROP.  Of the MATCH readings that claim one
    landmark the smallest (best, j) keeps it; the NEW readings take the slots known, known + 1, .. in ascending j while
    slot < n_max.  lms: the landmark (the slot of a NEW reading), -1 for a DROP."""
    J = len(scores)
    kinds, lms, best = [DROP] * J, [-1] * J, [float(gate_new)] * J
    for j in range(J):
        b, win = float(gate_new), known
        for i, v in enumerate(scores[j][:known] if known else []):
            if v < b:
                b, win = float(v), i
        best[j] = b
        if win == known:
            kinds[j], lms[j] = NEW, known
        elif b < gate_update:
            kinds[j], lms[j] = MATCH, win
    for j in range(J):
        if kinds[j] != MATCH:
            continue
        rivals = [o for o in range(J) if o != j and kinds[o] == MATCH and lms[o] == lms[j]]
        if any((best[o], o) < (best[j], j) for o in rivals):
            kinds[j] = "lost"
    slot = known
    for j in range(J):
        if kinds[j] == "lost":
            kinds[j], lms[j] = DROP, -1
        elif kinds[j] == NEW:
            if slot < n_max:
                lms[j], slot = slot, slot + 1
            else:
                kinds[j], lms[j] = DROP, -1
    return kinds, lms, best


def pairs_of(kinds, lms, gate_update=1.0):
    """the (reading, landmark) pairs of the correction in ascending j: MATCH and NEW, MATCH only with gate_update <= 0"""
    return [(j, lms[j]) for j, k in enumerate(kinds) if k == MATCH or (k == NEW and 0.0 < gate_update)]


def groups_of(pairs):
    return [pairs[g:g + MAX_PAIRS] for g in range(0, len(pairs), MAX_PAIRS)]


def np_joint_operands(state, lm_idx, readings):
    """the stacked operands of the pairs (lm_idx[v], readings[v]) from `state` -> cols [3 + 2V], Hc [2V][3 + 2V], nu [2V]
    with the bearing wrapped (sp.slam_terms per pair)"""
    V = len(lm_idx)
    cols = np.zeros(3 + 2 * V, dtype=np.int32)
    Hc, nu = np.zeros((2 * V, 3 + 2 * V)), np.zeros(2 * V)
    cols[:3] = (0, 1, 2)
    for v, (i, (sx, sy)) in enumerate(zip(lm_idx, readings)):
        c, h, _, _, wrapped = sp.slam_terms(state[:3], state, int(i), sx, sy)
        assert list(c[:3]) == [0, 1, 2]
        cols[3 + 2 * v:5 + 2 * v] = c[3:]
        Hc[2 * v:2 * v + 2, :3] = h[:, :3]
        Hc[2 * v:2 * v + 2, 3 + 2 * v:5 + 2 * v] = h[:, 3:]
        nu[2 * v:2 * v + 2] = wrapped
    return cols, Hc, nu


def np_scores(d, params, readings, known):
    """[J][known] scores of every reading against the handle's state as it is"""
    R = lc._p(params, "r_meas") * np.eye(2)
    out = np.zeros((len(readings), known))
    if known:
        x = d.state_block(0, 3 + 2 * known)
        for j, (sx, sy) in enumerate(readings):
            cols, Hc, _, nu = sp.candidate_terms(x, sx, sy, count=known)
            out[j] = d.score_sparse(cols, Hc, R, nu)[0]
    return out


def np_associate_joint(d, params, readings, known, n_max, scores=None):
    """ekf_dense64_associate_joint on a handle with the calls of ic.NumpyHandle -> known, assoc [J], best [J], n_groups"""
    readings = [tuple(float(v) for v in z) for z in readings]
    r_meas, sigma0 = lc._p(params, "r_meas"), lc._p(params, "sigma0_landmark")
    gate_new, gate_update = lc._p(params, "gate_new"), lc._p(params, "gate_update")
    nis = np_scores(d, params, readings, known)
    if scores is not None:
        scores.append(nis.copy())
    kinds, lms, best = joint_rule(nis, known, n_max, gate_new, gate_update)
    pose = d.state_block(0, 3)
    fresh = [j for j, k in enumerate(kinds) if k == NEW]
    for g in range(0, len(fresh), INIT_GROUP):
        grp = fresh[g:g + INIT_GROUP]
        xb = np.concatenate([ic.inverse_sensor(pose, *readings[j]) for j in grp])
        d.init_block(3 + 2 * (known + g), W=sigma0 * np.eye(2 * len(grp)), xb=xb)
    known += len(fresh)
    assoc = [lc.DROPPED] * len(readings)
    groups = groups_of(pairs_of(kinds, lms, gate_update))
    for grp in groups:
        x = d.state_block(0, 3 + 2 * known)
        cols, Hc, nu = np_joint_operands(x, [i for _, i in grp], [readings[j] for j, _ in grp])
        d.correct_sparse(cols, Hc, r_meas * np.eye(2 * len(grp)), nu)
        lc.wrap_heading_always(d)
        for j, i in grp:
            assoc[j] = i
    return known, np.array(assoc, dtype=np.int32), np.array(best), len(groups)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------

def numpy_handle(x, S):
    d = ic.NumpyHandle(len(x))
    d.set(S)
    d.set_state_block(0, np.array(x, dtype=np.float64))
    return d


def scan_fixture(count=16, known=10, seen=(0, 1, 2, 3, 5, 6, 8, 9), ticks=5, seed=3):
    """spiral_map(count) with `known` landmarks known and the rest stale; per tick a small motion and the readings of the
    8 distinct landmarks `seen` plus one reading of an object nobody knows (on a wide circle outside the spiral, far from
    everything; tick t adds it as landmark known + t) -> x, S, known, steps [(dtheta, dx, readings [9][2])].  The readings
    are taken from the TRUE positions, seen from the true pose, which the motion is applied to exactly."""
    assert len(seen) == 8 and len(set(seen)) == 8 and max(seen) < known and known + ticks <= count
    x, S = lc.spiral_map(count, seed=seed)
    S[3 + 2 * known:, :] = 0.0
    S[:, 3 + 2 * known:] = 0.0
    S[3 + 2 * known:, 3 + 2 * known:] = 7.0 * np.eye(2 * (count - known))
    truth = x.copy()
    for t in range(ticks):                                   # the unseen objects: 6 m out, 1.2 rad apart
        truth[3 + 2 * (known + t):5 + 2 * (known + t)] = 6.0 * np.cos(0.4 + 1.2 * t), 6.0 * np.sin(0.4 + 1.2 * t)
    rng = np.random.default_rng(seed + 100)
    steps = []
    for t in range(ticks):
        dth, dx = 0.02 + 0.01 * t, 0.05
        _, _, upd = bc.model_operands(truth[:3], dth, dx)
        truth[:3] = truth[:3] + upd
        truth[0] = dc.normalize_angle(float(truth[0]))
        z = [lc.reading_of(truth, i, tuple(0.004 * rng.standard_normal(2))) for i in list(seen) + [known + t]]
        steps.append((dth, dx, np.array(z)))
    return x, S, known, steps


def margins_ok(nis, kinds, best, gate_new=10.0, gate_update=1.0):
    """every deciding score at least MARGIN (relative) away from both gates: the minimum of each reading's row against
    gate_update and gate_new"""
    for j in range(len(kinds)):
        row = np.asarray(nis[j], dtype=np.float64)
        if row.size == 0:
            continue
        m = float(np.nanmin(row))
        for gate in (gate_new, gate_update):
            if abs(m - gate) < MARGIN * gate:
                return False
    return True
