"""Shared by tests/test_gpu_dense64_init.py and tests/test_dense64_init_host.py: the (re)initialisation of a block of
states in numpy (literally by slices, and as the dense F Sigma F^T + Q it is specified to equal), the reference's inverse
sensor model (initialize_landmark, ekf_slam.cpp:200-214) with its Jacobians, a numpy stand-in for the calls of the dense
handle that a SLAM loop uses, the reference's data_association() loop (:278-402) spelled with those calls, and the
scenarios the loop is driven through."""
import math

import numpy as np

import dense_block_cases as bc
import dense_correct_cases as dc
import dense_sparse_cases as sp

PRIOR = 100.0    # the reference's landmark prior (ekf_slam.cpp:32)
R_MEAS = 0.01    # its measurement noise (:172-175)


def np_init_block(state, Sigma, first, r, cols=None, G=None, W=None, xb=None):
    """-> state', Sigma': the three slice updates the call is specified to do, on copies; nothing else is touched.
    cols / G None: s = 0, the block's rows and columns become +0 and its corner W."""
    b = slice(first, first + r)
    N = len(Sigma)
    S = Sigma.copy()
    if cols is None or len(cols) == 0:
        rows, colsv, corner = np.zeros((r, N)), np.zeros((N, r)), np.zeros((r, r))
    else:
        cols = np.asarray(cols)
        G = np.asarray(G, dtype=np.float64)
        rows, colsv = G @ Sigma[cols, :], Sigma[:, cols] @ G.T
        corner = (G @ Sigma[np.ix_(cols, cols)]) @ G.T
    S[b, :] = rows
    S[:, b] = colsv
    S[b, b] = corner if W is None else corner + W
    x = state.copy()
    if xb is not None:
        x[b] = xb
    return x, S


def embedded_FQ(N, first, r, cols=None, G=None, W=None):
    """-> F = identity except F[b, b] = 0 and F[b, cols] = G; Q = zero except Q[b, b] = W: the dense propagation that the
    call equals"""
    F, Q = np.eye(N), np.zeros((N, N))
    F[first:first + r, first:first + r] = 0.0
    if cols is not None and len(cols):
        F[first:first + r, np.asarray(cols)] = G
    if W is not None:
        Q[first:first + r, first:first + r] = W
    return F, Q


def block_list(N, first, r, s, order, rng):
    """s distinct indices in [0, N) outside [first, first + r): 'asc', 'desc' or 'scattered'; where both sides of the block
    have room the list has members on both, and it holds the block's neighbours and the strip edges when they are free"""
    free = np.array([i for i in range(N) if not first <= i < first + r])
    want = [i for i in (first - 1, first + r, 0, N - 1, 63, 64, 127, 128) if 0 <= i < N and not first <= i < first + r]
    pick = list(dict.fromkeys(want))[:s]
    rest = np.array([i for i in free if i not in pick])
    if len(pick) < s:
        pick += list(rng.choice(rest, size=s - len(pick), replace=False))
    c = np.sort(np.array(pick))
    if order == "desc":
        c = c[::-1]
    elif order == "scattered":
        c = rng.permutation(c)
    return np.ascontiguousarray(c, dtype=np.int32)


# ---- the reference's inverse sensor model -----------------------------------------------------------------------------------

def inverse_sensor(pose, sx, sy):
    """initialize_landmark (:200-214): the landmark position the reading (sx, sy) puts on the map -> [mx, my]"""
    th, x, y = (float(v) for v in pose)
    ri = math.sqrt(sx * sx + sy * sy)
    phi = math.atan2(sy, sx)
    return np.array([x + ri * math.cos(phi + th), y + ri * math.sin(phi + th)])


def inverse_sensor_jacobians(pose, sx, sy):
    """-> G (2 x 3: d(mx, my) / d(theta, x, y)), Gz (2 x 2: d(mx, my) / d(range, bearing)), W = Gz R Gz^T"""
    th = float(pose[0])
    ri = math.sqrt(sx * sx + sy * sy)
    a = math.atan2(sy, sx) + th
    G = np.array([[-ri * math.sin(a), 1.0, 0.0], [ri * math.cos(a), 0.0, 1.0]])
    Gz = np.array([[math.cos(a), -ri * math.sin(a)], [math.sin(a), ri * math.cos(a)]])
    return G, Gz, Gz @ (R_MEAS * np.eye(2)) @ Gz.T


# ---- a numpy stand-in for the handle ------------------------------------------------------------------------------------------

class NumpyHandle:
    """The calls of DensePropagator64 that the SLAM loop uses, in numpy's spelling (bc / sp / np_init_block)."""

    def __init__(self, N):
        self.N, self.sigma, self.state = N, np.zeros((N, N)), np.zeros(N)

    def set(self, Sigma):
        self.sigma = np.array(Sigma, dtype=np.float64)

    def propagate_block(self, first, Fr, Qr=None, dx=None):
        self.state, self.sigma = bc.np_predict_slices(self.state, self.sigma, first, Fr, Qr, dx)

    def score_sparse(self, cols, Hc, R, nu):
        _, nis = sp.np_scores(self.sigma, cols, Hc, R, nu)
        return nis, None, np.zeros(len(cols), dtype=np.int32), 0.0

    def correct_sparse(self, cols, Hc, R, nu):
        self.state, self.sigma, nis = sp.np_correct(self.state, self.sigma, cols, Hc, R, nu)
        return nis, 0.0

    def init_block(self, first, G=None, cols=None, W=None, xb=None, r=None):
        r = next(len(a) for a in (G, W, xb) if a is not None) if r is None else r
        self.state, self.sigma = np_init_block(self.state, self.sigma, first, r, cols, G, W, xb)

    def state_block(self, first, count):
        return self.state[first:first + count].copy()

    def set_state_block(self, first, x):
        self.state[first:first + len(x)] = x

    def close(self):
        pass


# ---- the reference's loop with the handle's calls ---------------------------------------------------------------------------

def wrap_heading(d):
    """state(0,0) = normalize_angle(state(0,0)) (:187, :385) through the state slices: one double each way"""
    th = float(d.state_block(0, 1)[0])
    w = dc.normalize_angle(th)
    if w != th:
        d.set_state_block(0, np.array([w]))


def association_step(d, n, known, dth, dx, readings, init, scores=None):
    """prediction() and data_association() (:278-402) of one tick on the handle `d`: propagate_block, then per reading
    score_sparse over the known prefix, the reference's rule, a new landmark through `init` ('init_block': s = 0,
    W = 100 I, xb; 'state_only': set_state_block, the prior is already in Sigma) or not at all, correct_sparse on the
    winner and the heading wrap.  -> the new number of known landmarks"""
    Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), dth, dx)
    d.propagate_block(0, Fr, Qr, upd)
    for sx, sy in readings:
        x = d.state_block(0, 3 + 2 * known)
        best, win = 10.0, known
        if known:
            cols, Hc, R, nu = sp.candidate_terms(x, sx, sy, count=known)
            nis, _, flags, _ = d.score_sparse(cols, Hc, R, nu)
            assert not np.asarray(flags).any()
            if scores is not None:
                scores.append(np.array(nis))
            for i, v in enumerate(nis):                      # ascending order, strict <: the first of equals wins
                if v < best:
                    best, win = float(v), i
        if win == known and known < n:                       # :318-327
            xb = inverse_sensor(x[:3], sx, sy)
            if init == "init_block":
                d.init_block(3 + 2 * known, W=PRIOR * np.eye(2), xb=xb)
            else:
                d.set_state_block(3 + 2 * known, xb)
            known += 1
            best = 0.0
        if best < 1.0:                                       # :330-391
            x = d.state_block(0, 3 + 2 * known)
            c, h, R, _, wrapped = sp.slam_terms(x[:3], x, win, sx, sy)
            d.correct_sparse(c, h, R, wrapped)
            wrap_heading(d)
    return known


def discovery_scenario(steps=20, seed=5):
    """A seeded world of `steps` landmarks on four rings a metre apart, one every 18 degrees and the same ring every 72
    (a fresh landmark is known to 0.1 m in range and 0.1 rad in bearing, so the scores of a wrong landmark are far beyond
    the gate 10, of the right one far below 1) and a robot that turns on a small circle inside it -- the heading passes pi,
    so the wrap happens.  Step t brings one landmark never seen before and up to two seen earlier, in a seeded order:
    the map is discovered over all steps and every landmark but the last is re-observed.
    -> [(dtheta, dx, readings [k][2])]"""
    rng = np.random.default_rng(seed)
    L = steps
    ang = 2 * math.pi * np.arange(L) / L
    rad = 1.5 + 1.0 * (np.arange(L) % 4)
    world = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    pose = np.zeros(3)
    out = []
    for t in range(steps):
        dth, dx = (0.0, 0.05) if t % 7 == 3 else (0.2 + 0.01 * (t % 3), 0.06)
        _, _, upd = bc.model_operands(pose, dth, dx)
        pose = pose + upd
        seen = [t] if t == 0 else list(dict.fromkeys([t - 1, int(rng.integers(0, t)), t]))
        seen = [seen[i] for i in rng.permutation(len(seen))]
        c, s = math.cos(pose[0]), math.sin(pose[0])
        dxy = world[seen] - pose[1:] + rng.normal(0, 0.004, size=(len(seen), 2))
        out.append((dth, dx, np.stack([c * dxy[:, 0] + s * dxy[:, 1], -s * dxy[:, 0] + c * dxy[:, 1]], axis=1)))
    return out


def stale_start(n, seed=9):
    """what the handle starts from when only init_block can make the runs agree: landmark blocks 7 I instead of the prior,
    stale landmark entries in the state"""
    N = 3 + 2 * n
    S = np.zeros((N, N))
    S[3:, 3:] = 7.0 * np.eye(2 * n)
    x = np.concatenate([np.zeros(3), np.random.default_rng(seed).uniform(-4.0, 4.0, size=2 * n)])
    return x, S


def prior_start(n):
    """the reference's constructor (:27-46)"""
    N = 3 + 2 * n
    S = np.zeros((N, N))
    S[3:, 3:] = PRIOR * np.eye(2 * n)
    return np.zeros(N), S


# ---- slot recycling ------------------------------------------------------------------------------------------------------------

def recycling_scenario(n=200, seed=77):
    """A known map of n landmarks (variances ~1e-3, correlated, slightly unsymmetric), ten steps of predict / correct with
    the association given, landmark `slot` evicted (s = 0) and re-initialised correlated (s = 3) from a reading of a new
    object, ten more steps that observe the new object among others.
    -> N, Sigma0, state0, steps [(dtheta, dx, landmark, (sx, sy))], slot, world"""
    rng = np.random.default_rng(seed)
    N = 3 + 2 * n
    world = rng.uniform(-3.0, 3.0, size=(n, 2))
    world[np.hypot(world[:, 0], world[:, 1]) < 0.5] += 1.0
    A = rng.normal(size=(N, N))
    S = 1e-3 * (A @ A.T / N + np.eye(N))
    S[:3, :3] *= 0.1
    S = S + 1e-3 * np.abs(S) * rng.normal(size=S.shape)
    x0 = np.concatenate([np.zeros(3), (world + rng.normal(0, 0.02, size=(n, 2))).reshape(-1)])
    slot = 57
    world2 = world.copy()
    world2[slot] = [2.2, -1.7]                     # the new object that takes the slot
    pose = np.zeros(3)
    steps = []
    for t in range(20):
        dth, dx = (0.0, 0.04) if t % 5 == 2 else (0.1 + 0.01 * t, 0.05)
        _, _, upd = bc.model_operands(pose, dth, dx)
        pose = pose + upd
        if t < 10:
            lm = int(rng.choice([i for i in range(n) if i != slot]))
        else:
            lm = slot if t in (10, 13, 17) else int(rng.integers(0, n))
        w = world if t < 10 else world2
        c, s = math.cos(pose[0]), math.sin(pose[0])
        dxy = w[lm] - pose[1:] + rng.normal(0, 0.004, size=2)
        steps.append((dth, dx, lm, (c * dxy[0] + s * dxy[1], -s * dxy[0] + c * dxy[1])))
    return N, S, x0, steps, slot


def recycling_run(d, steps, slot, probe=None):
    """the scenario on a handle (DensePropagator64 or NumpyHandle).  Step 10 is the reading of the new object: the slot is
    evicted, re-initialised from it, and `probe(stage, d, G, W)` is called "before" and "after" the correlated call with its
    operands."""
    for t, (dth, dx, lm, (sx, sy)) in enumerate(steps):
        Fr, Qr, upd = bc.model_operands(d.state_block(0, 3), dth, dx)
        d.propagate_block(0, Fr, Qr, upd)
        if t == 10:
            first = 3 + 2 * slot
            d.init_block(first, W=PRIOR * np.eye(2))                                   # evicted: an uncorrelated prior
            pose = d.state_block(0, 3)
            G, _, W = inverse_sensor_jacobians(pose, sx, sy)
            if probe:
                probe("before", d, G, W)
            d.init_block(first, G=G, cols=[0, 1, 2], W=W, xb=inverse_sensor(pose, sx, sy))
            if probe:
                probe("after", d, G, W)
            continue
        x = d.state_block(0, d.N)
        c, h, R, _, wrapped = sp.slam_terms(x[:3], x, lm, sx, sy)
        d.correct_sparse(c, h, R, wrapped)
        wrap_heading(d)
