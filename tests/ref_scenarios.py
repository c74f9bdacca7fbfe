"""Hand-built edge scenarios of rigid2d::EKF_SLAM (rigid2d/src/ekf_slam.cpp) shared by tests/test_reference_ekf.py
(live, against the reference's own class in oracle/_ref), tests/golden/make_golden.py (which records the reference
build's outputs into tests/golden/ref_edges.npz) and tests/test_gpu_reference_ekf.py (replays that fixture on the GPU).

A scenario is (n, ops) with ops applied in order to one filter:
  ("P", dtheta, dx)            prediction(Twist2D(dtheta, {dx, 0}))
  ("M", sensor[2n], vis[n])    measurement()
  ("A", meas[J, 2], known[n])  data_association() with `known` as the list passed in (copied; the filter's own
                               running list is NOT carried between A ops, so holes can be put in on purpose)
  ("S", state[N], cov[N, N])   overwrite state / covariance and set landmark_init_flag (to build exact ties)
Every filter is driven through `apply(f, op)` with the duck-typed surface of oracle.binding.OracleEKF / RefEKF."""
import math

import numpy as np

PI = 3.14159265358979323846
KINDS = "PMAS"


def polar_to_world(pose, sx, sy):
    """ekf_slam.cpp:115-120 / :204-209: where a robot-frame reading puts a landmark."""
    theta, x, y = pose
    ri = math.sqrt(sx ** 2 + sy ** 2)
    phii = math.atan2(sy, sx)
    return x + ri * math.cos(phii + theta), y + ri * math.sin(phii + theta)


def robot_frame(pose, world):
    c, s = math.cos(pose[0]), math.sin(pose[0])
    d = np.asarray(world, dtype=np.float64) - np.asarray(pose[1:], dtype=np.float64)
    return np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1)


def apply(f, op):
    """-> known list after an A op (else None)"""
    kind = op[0]
    if kind == "P":
        f.prediction(op[1], op[2])
    elif kind == "M":
        f.measurement(op[1], op[2])
    elif kind == "A":
        known = np.array(op[2], dtype=np.uint8)
        f.data_association(np.asarray(op[1], dtype=np.float64).reshape(-1, 2), known)
        return known
    elif kind == "S":
        f.state, f.cov = op[1], op[2]
        f.set_init_flag(1)
    else:
        raise ValueError(kind)
    return None


def _world(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(-2.0, 2.0, size=(n, 2))
    w[np.hypot(w[:, 0], w[:, 1]) < 0.4] += 0.7
    return w


def _all_visible_meas(n, pose, world, rng, vis=None):
    rf = robot_frame(pose, world) + rng.normal(0, 0.003, size=(n, 2))
    return ("M", rf.reshape(-1), np.ones(n, dtype=np.uint8) if vis is None else np.asarray(vis, dtype=np.uint8))


def dead_reckon(pose, dth, dx):
    """the true pose after a twist: prediction()'s own two branches (ekf_slam.cpp:79-94) on a 3-vector (theta, x, y)"""
    if abs(dth) < 1e-6:
        return np.array([pose[0], pose[1] + dx * math.cos(pose[0]), pose[2] + dx * math.sin(pose[0])])
    r = dx / dth
    return np.array([pose[0] + dth, pose[1] - r * math.sin(pose[0]) + r * math.sin(pose[0] + dth),
                     pose[2] + r * math.cos(pose[0]) - r * math.cos(pose[0] + dth)])


_dead_reckon = dead_reckon   # (the name the older tests use)


def straight_threshold():
    """dtheta values at the `fabs(dtheta) < 0.000001` branch (ekf_slam.cpp:79): the gate, one ulp inward, and 0"""
    g = 0.000001
    return [g, -g, math.nextafter(g, 0.0), -math.nextafter(g, 0.0), 0.0]


def edge_scenarios():
    """name -> (n, ops).  Deterministic."""
    sc = {}
    n = 4
    world = _world(n, 11)
    rng = np.random.default_rng(3)
    # both prediction branches exactly at the 1e-6 gate, each followed by a correction that reads the pose
    for k, dth in enumerate(straight_threshold()):
        pose = np.zeros(3)
        ops = [_all_visible_meas(n, pose, world, rng, vis=np.zeros(n))]
        for _ in range(3):
            ops.append(("P", dth, 0.2))
            pose = _dead_reckon(pose, dth, 0.2)
            ops.append(_all_visible_meas(n, pose, world, rng))
        sc[f"dtheta_gate_{k}"] = (n, ops)
    # theta driven far outside (-pi, pi]: prediction never wraps (:99), only a correction does (:187)
    pose, ops = np.zeros(3), []
    for _ in range(9):
        ops.append(("P", 1.4, 0.05))
        pose = _dead_reckon(pose, 1.4, 0.05)
    ops.append(_all_visible_meas(n, pose, world, rng, vis=[1, 0, 1, 0]))
    sc["theta_unwrapped"] = (n, ops)
    # the first measurement() initialises EVERY landmark from the reading, visible or not (:113-128)
    pose = np.array([0.0, 0.3, -0.2])
    ops = [("P", 0.0, 0.3), ("P", 0.0, 0.0), _all_visible_meas(n, np.array([0.0, 0.3, 0.0]), world, rng, vis=[0, 1, 0, 0])]
    sc["first_measurement_inits_invisible"] = (n, ops)
    # a first call with nothing visible: initialisation only, no correction
    ops = [("P", 0.3, 0.1), _all_visible_meas(n, _dead_reckon(np.zeros(3), 0.3, 0.1), world, rng, vis=[0] * n)]
    sc["first_call_nothing_visible"] = (n, ops)
    # association: known lists with holes -- known_count is the PREFIX of true entries (:281-289)
    n6 = 6
    w6 = _world(n6, 12)
    pose = np.zeros(3)
    rf = robot_frame(pose, w6)
    ops = [("A", rf[[0, 1, 3]], [0] * n6),                     # discover three landmarks into slots 0, 1, 2
           ("P", 0.05, 0.1),
           ("A", rf[[4]] + 0.001, [1, 0, 1, 1, 0, 0]),          # hole at 1: prefix count 1, a new reading lands at 1
           ("A", rf[[5, 2]], [1, 1, 0, 1, 0, 1])]               # hole at 2 with later entries set
    sc["known_with_holes"] = (n6, ops)
    # a full map: a reading beyond gate 10 has its best index at known_count == n, which is not < n (:318)
    n3 = 3
    w3 = _world(n3, 13)
    rf = robot_frame(np.zeros(3), w3)
    ops = [("A", rf, [0] * n3), ("P", 0.02, 0.05), ("A", np.array([[25.0, -30.0]]), [1] * n3),
           ("A", rf[[1]], [1] * n3)]
    sc["full_map_far_reading"] = (n3, ops)
    # J = 0 on an empty and on a partly known map
    ops = [("A", np.zeros((0, 2)), [0] * n3), ("A", rf[[0]], [0] * n3), ("P", 0.1, 0.1), ("A", np.zeros((0, 2)), [1, 0, 0])]
    sc["no_readings"] = (n3, ops)
    # n = 1 through every entry point
    ops = [("A", np.array([[0.8, 0.3]]), [0]), ("P", -0.2, 0.1), ("A", np.array([[0.75, 0.42]]), [1]),
           ("A", np.array([[0.9, 0.1]]), [1]), ("P", 0.0, 0.05), ("M", np.array([0.7, 0.45]), np.array([1], dtype=np.uint8))]
    sc["n1"] = (1, ops)
    # association never sets landmark_init_flag: a later measurement() re-initialises the whole map (:113)
    ops = [("A", rf[[0, 1]], [0] * n3), ("P", 0.1, 0.05),
           ("M", (rf + 0.01).reshape(-1), np.array([0, 1, 0], dtype=np.uint8))]
    sc["association_then_measurement"] = (n3, ops)
    # stale pose (:109-111): many landmarks corrected in ONE call after a real pose error
    n8 = 8
    w8 = _world(n8, 14)
    pose = np.array([0.15, 0.2, -0.1])
    ops = [("M", robot_frame(np.zeros(3), w8).reshape(-1), np.zeros(n8, dtype=np.uint8)), ("P", 0.1, 0.25),
           ("M", (robot_frame(pose, w8) + np.random.default_rng(5).normal(0, 0.01, (n8, 2))).reshape(-1),
            np.ones(n8, dtype=np.uint8))]
    sc["stale_pose"] = (n8, ops)
    sc.update(gate_scenarios())
    sc.update(bearing_scenarios())
    return sc


def _set_op(n, lm, pose=(0.0, 0.0, 0.0), pose_var=1e-4, lm_var=0.02):
    """an "S" op: a pose, landmarks at `lm`, a diagonal covariance"""
    N = 3 + 2 * n
    state = np.zeros(N)
    state[:3] = pose
    state[3:] = np.asarray(lm, dtype=np.float64).reshape(-1)
    cov = np.diag(np.r_[np.full(3, pose_var), np.full(2 * n, lm_var)])
    return ("S", state, cov)


def maha_closed_form(state, cov, i, sx, sy):
    """calculate_maha_dis (:217-276) for a diagonal covariance -- used only to place readings at a chosen score"""
    theta, x, y = state[:3]
    tx, ty = state[3 + 2 * i], state[4 + 2 * i]
    z = np.array([math.sqrt(sx ** 2 + sy ** 2), math.atan2(sy, sx)])
    dx, dy = tx - x, ty - y
    d = dx ** 2 + dy ** 2
    zh = np.array([math.sqrt(d), math.fmod(math.fmod(math.atan2(dy, dx) - theta, 2 * PI) + 2 * PI, 2 * PI)])
    if zh[1] > PI:
        zh[1] -= 2 * PI
    H = np.zeros((2, len(state)))
    H[:, :3] = [[0, -dx / math.sqrt(d), -dy / math.sqrt(d)], [-1, dy / d, -dx / d]]
    H[:, 3 + 2 * i:5 + 2 * i] = [[dx / math.sqrt(d), dy / math.sqrt(d)], [-dy / d, dx / d]]
    psi = H @ cov @ H.T + np.diag([0.01, 0.01])
    v = z - zh
    return float(v @ np.linalg.solve(psi, v))


def _reading_at_score(st, cov, i, target):
    """a robot-frame reading on the ray through landmark i whose score against i is ~target (bisection on range)"""
    tx, ty = st[3 + 2 * i] - st[1], st[4 + 2 * i] - st[2]
    r0, phi = math.hypot(tx, ty), math.atan2(ty, tx) - st[0]
    lo, hi = 0.0, 5.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        sx, sy = (r0 + mid) * math.cos(phi), (r0 + mid) * math.sin(phi)
        if maha_closed_form(st, cov, i, sx, sy) < target:
            lo = mid
        else:
            hi = mid
    return np.array([[sx, sy]])


def gate_scenarios():
    """the strict `<` of :305 and :330 and the lowest-index tie-break"""
    sc = {}
    n = 3
    lm = [[1.0, 0.2], [-0.5, 1.1], [0.3, -1.2]]
    set_op = _set_op(n, lm)
    st, cov = set_op[1], set_op[2]
    # scores in [1, 10): neither a new landmark nor an update -- nothing changes (:318 and :330 both fail)
    for k, target in enumerate((1.5, 4.0, 9.5)):
        sc[f"score_between_gates_{k}"] = (n, [set_op, ("A", _reading_at_score(st, cov, 0, target), [1, 1, 1])])
    # a score just below 1: the update path
    sc["score_below_1"] = (n, [set_op, ("A", _reading_at_score(st, cov, 0, 0.9), [1, 1, 1])])
    # a score in [1, 10) with free slots left: no update, and min_maha_idx != known_count so no initialisation
    sc["score_between_gates_free_slot"] = (n, [set_op, ("A", _reading_at_score(st, cov, 0, 3.0), [1, 0, 0])])
    # two landmarks at the same place with the same covariance: bit-identical scores, the LOWER index wins (:305)
    tie = _set_op(n, [[0.9, 0.4], [0.9, 0.4], [-1.0, -1.0]])
    sc["tie_lowest_index_wins"] = (n, [tie, ("A", np.array([[0.91, 0.41]]), [1, 1, 1])])
    # a score of EXACTLY 1.0 (every quantity a power of two: psi = diag(0.25, 0.25), innovation (0.5, 0)): the strict
    # `<` of :330 drops it, `<=` would update
    N = 3 + 2 * n
    state = np.zeros(N)
    state[3:] = [1.0, 0.0, -1.0, 2.0, 0.5, -2.0]
    cov = np.diag(np.r_[np.zeros(3), np.full(2 * n, 0.25 - 0.01)])   # + R (0.01) rounds to exactly 0.25
    sc["score_exactly_1"] = (n, [("S", state, cov), ("A", np.array([[1.5, 0.0]]), [1, 1, 1])])
    return sc


def bearing_scenarios():
    """a landmark behind the robot whose reading falls across the +-pi cut: measurement() wraps the bearing innovation
    (:183); without the wrap the correction would be ~2 pi off"""
    n = 3
    first = np.array([-1.0, 0.01, -1.3, -0.012, 0.2, 0.9])
    second = np.array([-1.0, -0.008, -1.3, 0.01, 0.21, 0.9])
    return {"bearing_across_pi": (n, [("M", first, np.zeros(n, dtype=np.uint8)), ("P", 0.0, 0.01),
                                      ("M", second, np.ones(n, dtype=np.uint8))])}


# ---- fixture I/O (tests/golden/ref_edges.npz) --------------------------------------------------------------

def record(make_filter, scenarios):
    """run every scenario on make_filter(n) -> {name: (n, ops, states[k], knowns{k: known}, cov)}"""
    out = {}
    for name, (n, ops) in scenarios.items():
        f = make_filter(n)
        states, knowns = [], {}
        for k, op in enumerate(ops):
            kn = apply(f, op)
            if kn is not None:
                knowns[k] = kn
            states.append(f.state.copy())
        out[name] = (n, ops, np.array(states), knowns, f.cov.copy())
    return out


def save(path, recorded):
    arrs = {"names": np.array(sorted(recorded))}
    for s, name in enumerate(sorted(recorded)):
        n, ops, states, knowns, cov = recorded[name]
        p = f"s{s}_"
        arrs[p + "n"] = np.int64(n)
        arrs[p + "kinds"] = np.array([KINDS.index(op[0]) for op in ops], dtype=np.uint8)
        for k, op in enumerate(ops):
            q = f"{p}op{k}_"
            if op[0] == "P":
                arrs[q + "x"] = np.array([op[1], op[2]], dtype=np.float64)
            elif op[0] in "MA":
                arrs[q + "x"] = np.asarray(op[1], dtype=np.float64)
                arrs[q + "v"] = np.asarray(op[2], dtype=np.uint8)
            else:
                arrs[q + "x"] = np.asarray(op[1], dtype=np.float64)
                arrs[q + "c"] = np.asarray(op[2], dtype=np.float64)
            if k in knowns:
                arrs[q + "known"] = knowns[k]
        arrs[p + "states"] = states
        arrs[p + "cov"] = cov
    np.savez_compressed(path, **arrs)


def load(path):
    """-> {name: (n, ops, states, knowns, cov)} as recorded"""
    g = np.load(path)
    out = {}
    for s, name in enumerate(g["names"]):
        p = f"s{s}_"
        n = int(g[p + "n"])
        ops, knowns = [], {}
        for k, kind in enumerate(g[p + "kinds"]):
            q = f"{p}op{k}_"
            c = KINDS[int(kind)]
            x = g[q + "x"]
            if c == "P":
                ops.append(("P", float(x[0]), float(x[1])))
            elif c == "M":
                ops.append(("M", x, g[q + "v"]))
            elif c == "A":
                ops.append(("A", x.reshape(-1, 2), g[q + "v"]))
                knowns[k] = g[q + "known"]
            else:
                ops.append(("S", x, g[q + "c"]))
        out[str(name)] = (n, ops, g[p + "states"], knowns, g[p + "cov"])
    return out
