"""Pool logs built from HAND-CHOSEN twists (no GPU, no library): the inputs of tests/test_gpu_pool_motion.py, proved on the CPU
by tests/test_pool_motion_cases_host.py.

Every other pool test takes its twists from synth.make_known_log / make_unknown_log: one constant (v_cmd, w_cmd) plus noise,
so every prediction a pool kernel executes there takes the arc branch of prediction() (ekf_slam.cpp:88-94) with dtheta > 0 and
dx > 0, and the heading stays inside (-pi, pi].  Here each of the B = 7 filters of a pool follows another motion family, so one
launch of k_predict holds workgroups on both sides of the 1e-6 gate (:79), of both signs, with a10 = a20 = 0 exactly
(turning in place), with At = I (a zero twist) and with a heading several turns outside (-pi, pi]:

  gate        dtheta cycles through ref_scenarios.straight_threshold() and their negatives, dx = 0.2
  straight    dtheta = 0.0 / -0.0 in turn, dx of both signs
  in_place    dx = 0 with dtheta = +-0.3 (arc branch, a10 = a20 = 0 exactly), and steps of (0, 0)
  reverse     dtheta < 0, dx < 0
  spin        dtheta = +-1.4 / +-3.1 over blind steps: the heading (which prediction() never wraps, :99) leaves (-pi, pi]
              within three steps, is read from at 3 pi and beyond in both directions, and ends beyond 3 pi on a blind tail
  behind      a slow arc that only reads landmarks BEHIND the robot, nearest to the +-pi cut first: raw bearing differences
              beyond +-pi, which only measurement()'s own wrap (:187) brings back (calculate_maha_dis does not, :269)
  silent_mix  runs of 2-4 steps without readings whose predictions alternate straight / arc / negative arc / in place, then a
              step with readings: what FORM_CURRENT_COLUMNS accumulates in apred_in over the steps a filter sits out

The true pose is dead-reckoned from the twists (ref_scenarios.dead_reckon), readings are ref_scenarios.robot_frame plus seeded
noise (SENSOR_STD).  The world is seeded and shared by the filters of a pool: landmarks MIN_SPACING apart and CLEARANCE away
from every pose; for the steps at which `behind` and `spin` read, one landmark each is placed exactly behind the robot, so the
noise decides on which side of the cut its reading falls.  Visibility is by range (R_VISIBLE), nearest first, VMAX (JMAX for
unknown association) at the most.

MotionEKF is a structured O(N^2) copy of oracle/np_restatement.py's prediction / correction (rows and columns 1, 2; a rank-2
downdate) that takes one MUTANT at a time; the host test holds the unmutated copy against the checker, then shows that each
family moves under the mutant it is meant for."""
import functools
import math
from dataclasses import dataclass

import numpy as np

import ref_scenarios as rs

FAMILIES = ("gate", "straight", "in_place", "reverse", "spin", "behind", "silent_mix")
B = len(FAMILIES)
T = 18
SHAPES = (50, 130, 300)       # LDS-resident small path | N = 263 >= 256: mirrored flush and column panel | run_unknown beyond it
# on which side of the cut a reading from exactly behind falls is the noise's choice: these seeds (the first of 350000 + n +
# 1000 k) give `behind` and `spin` two or more corrections each whose raw bearing difference lies beyond +-pi; the host test
# counts them
SEEDS = {50: 350050, 130: 352130, 300: 352300}
CUTS = ((0, 4), (4, 5), (5, 11), (11, T))   # run boundaries: after a reading step, one step alone, inside a silent run
SENSOR_STD = 0.004
R_VISIBLE = 1.1
MIN_SPACING = 0.45            # at R_VISIBLE a neighbour is > 3.7 sigma of the bearing noise model away: above gate 10
CLEARANCE = 0.25              # no landmark this close to any pose (H is singular at distance 0)
VMAX, JMAX = 4, 5
BEHIND_PLACED = tuple(range(1, T))         # steps at which `behind` finds a landmark exactly on its -x axis, room permitting
MUTANTS = {"gate_le": ("gate",), "no_straight": ("straight",), "a10_sign": ("straight",), "no_wrap": ("behind", "spin"),
           "stale_apred": ("silent_mix",)}


def family_twists(family):
    """-> (twist[T, 2] as (dtheta, dx), reads[T] bool)"""
    tw, reads = np.zeros((T, 2)), np.ones(T, dtype=bool)
    if family == "gate":
        cyc = rs.straight_threshold()
        cyc = cyc + [-v for v in cyc]                 # (with -0.0 and the negated gate values a second time)
        for t in range(T):
            tw[t] = cyc[t % len(cyc)], 0.2
    elif family == "straight":
        dxs = (0.15, 0.2, -0.1, 0.25, -0.3, 0.1)
        for t in range(T):
            tw[t] = (0.0 if t % 2 == 0 else -0.0), dxs[t % len(dxs)]
    elif family == "in_place":
        dth = (0.3, -0.3, 0.0, 0.3, 0.3, 0.0, -0.3, -0.3)
        for t in range(T):
            tw[t] = dth[t % len(dth)], 0.0
    elif family == "reverse":
        for t in range(T):
            tw[t] = -0.12 - 0.01 * (t % 3), -0.15 - 0.02 * (t % 2)
    elif family == "spin":
        dth = (3.1, 3.1, 3.1, 3.1, 1.4, 1.4, -3.1, -3.1, -3.1, -1.4, -3.1, 1.4, 3.1, -1.4, -3.1, -3.1, -3.1, -3.1)
        reads[:] = False
        reads[[5, 6, 10, 11, 13]] = True              # 5 and 10: read from a heading of +15.2 / -11.2; 14 ..: the blind tail
        for t in range(T):
            # (half turns with dx of alternating sign add up: the first four carry the robot 0.9 m off the other filters' paths)
            tw[t] = dth[t], (-0.35 if t < 4 else 0.02) * (-1) ** t
    elif family == "behind":
        tw[:] = 0.15, 0.09                            # (a circle of radius 0.6: the points behind it lie off its own path)
    elif family == "silent_mix":
        seq = [(0.1, 0.1, 1), (0.1, 0.1, 1),
               (0.0, 0.15, 0), (0.25, 0.1, 0), (-0.2, 0.1, 1),
               (0.3, 0.0, 0), (-0.0, -0.1, 0), (-0.25, 0.12, 0), (0.0, 0.1, 1),
               (0.2, 0.1, 0), (0.0, 0.0, 0), (0.0, 0.2, 0), (-0.3, -0.1, 0), (0.15, 0.1, 1),
               (0.0, 0.1, 0), (-0.2, 0.1, 0), (0.1, 0.05, 1), (0.0, 0.1, 1)]
        assert len(seq) == T
        for t, (a, d, r) in enumerate(seq):
            tw[t], reads[t] = (a, d), bool(r)
    else:
        raise ValueError(family)
    return tw, reads


def branch(dtheta):
    """prediction()'s branch, restated (ekf_slam.cpp:79)"""
    return "straight" if abs(dtheta) < 0.000001 else "arc"


def predicted_bearing(state, i, theta, x, y):
    """z_hat(1) (:143-147): normalize_angle(atan2(ty - y, tx - x) - theta), restated"""
    tx, ty = state[3 + 2 * i], state[4 + 2 * i]
    a = math.fmod(math.fmod(math.atan2(ty - y, tx - x) - theta, 2 * rs.PI) + 2 * rs.PI, 2 * rs.PI)
    return a - 2 * rs.PI if a > rs.PI else a


def raw_bearing_difference(state, i, sx, sy, theta, x, y):
    """z(1) - z_hat(1) of a correction BEFORE the wrap of :187, restated"""
    return math.atan2(sy, sx) - predicted_bearing(state, i, theta, x, y)


@dataclass(frozen=True)
class Case:
    n: int
    seed: int
    world: np.ndarray      # [n, 2]
    pose: np.ndarray       # [T, B, 3] true pose after step t's prediction (theta not wrapped)
    reads: np.ndarray      # [T, B] bool
    twist: np.ndarray      # [T, B, 2]
    lm_idx: np.ndarray     # [T, B, VMAX] known log: ascending, -1 padded; step 0 only initialises (init_xy)
    z_xy: np.ndarray       # [T, B, VMAX, 2]
    init_xy: np.ndarray    # [B, 2n]
    count: np.ndarray      # [T, B] unknown log
    meas_xy: np.ndarray    # [T, B, JMAX, 2]
    truth_idx: np.ndarray  # [T, B, JMAX] generating landmark
    survey_xy: np.ndarray  # [B, 2n] the surveyed map: a first known-association call at the start pose

    def known_log(self):
        """what BatchEKF.upload_known_log takes"""
        return self.twist, self.lm_idx, self.z_xy, self.init_xy

    def unknown_log(self):
        """what BatchEKF.upload_unknown_log takes"""
        return self.twist, self.count, self.meas_xy

    def expand_step(self, t, b):
        """(sensor_reading[2n], visible[n]) of the known log's step t"""
        if t == 0:
            return self.init_xy[b].copy(), np.zeros(self.n, dtype=np.uint8)
        idx = self.lm_idx[t, b]
        k = int((idx >= 0).sum())
        sensor, vis = np.zeros(2 * self.n), np.zeros(self.n, dtype=np.uint8)
        sensor[2 * idx[:k]], sensor[2 * idx[:k] + 1] = self.z_xy[t, b, :k, 0], self.z_xy[t, b, :k, 1]
        vis[idx[:k]] = 1
        return sensor, vis


def _trajectories():
    tw = np.zeros((T, B, 2))
    reads = np.zeros((T, B), dtype=bool)
    pose = np.zeros((T, B, 3))
    for b, fam in enumerate(FAMILIES):
        tw[:, b], reads[:, b] = family_twists(fam)
        p = np.zeros(3)
        for t in range(T):
            p = rs.dead_reckon(p, tw[t, b, 0], tw[t, b, 1])
            pose[t, b] = p
    return tw, reads, pose


def _world(n, rng, pose, reads):
    """placed landmarks (exactly behind `behind` / `spin` at their reading steps), then a seeded fill"""
    flat = pose.reshape(-1, 3)[:, 1:]

    def fits(p, pts):
        if np.min(np.hypot(flat[:, 0] - p[0], flat[:, 1] - p[1])) < CLEARANCE:
            return False
        return not pts or np.min(np.hypot(*(np.array(pts) - p).T)) >= MIN_SPACING

    pts, placed = [], {"behind": 0, "spin": 0}
    for fam, steps in (("behind", BEHIND_PLACED), ("spin", np.nonzero(reads[:, FAMILIES.index("spin")])[0])):
        b = FAMILIES.index(fam)
        for t in steps:
            th, x, y = pose[t, b]
            for r in (0.6, 0.7, 0.8, 0.9, 1.0, 0.5, 0.65, 0.75, 0.85, 0.95, 1.05, 0.45, 0.4):
                p = np.array([x - r * math.cos(th), y - r * math.sin(th)])
                if fits(p, pts):
                    pts.append(p)
                    placed[fam] += 1
                    break
    if placed["behind"] < 3 or placed["spin"] < 2:   # (a step whose spot is taken, by another filter's path or by the
        #                                               landmark of a step with the same heading, goes without)
        raise ValueError(f"too few landmarks placed behind: {placed}")
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    m = 0.9
    while (hi[0] - lo[0] + 2 * m) * (hi[1] - lo[1] + 2 * m) < 0.6 * n:    # at most 1 / 0.6 landmarks per square metre
        m += 0.05
    tries = 0
    while len(pts) < n:
        p = rng.uniform(lo - m, hi + m)
        tries += 1
        if tries > 400 * n:
            raise ValueError("world too dense")
        if fits(p, pts):
            pts.append(p)
    return np.array(pts)[rng.permutation(n)]


def _select(rf, family, cap):
    """the landmarks a step reads: within R_VISIBLE, nearest first; `behind` and `spin` read behind the robot only, nearest
    to the +-pi cut first"""
    d = np.hypot(rf[:, 0], rf[:, 1])
    ok = d <= R_VISIBLE
    if family in ("behind", "spin"):
        ok &= rf[:, 0] < 0
        key = rs.PI - np.abs(np.arctan2(rf[:, 1], rf[:, 0]))
    else:
        key = d
    idx = np.nonzero(ok)[0]
    return idx[np.argsort(key[idx], kind="stable")[:cap]]


@functools.lru_cache(maxsize=None)
def make_case(n, seed=None):
    """the (B, n, T) case: deterministic, cached, read-only"""
    seed = SEEDS[n] if seed is None else seed
    rng = np.random.default_rng(seed)
    twist, reads, pose = _trajectories()
    world = _world(n, rng, pose, reads)
    lm_idx = np.full((T, B, VMAX), -1, dtype=np.int32)
    z_xy = np.zeros((T, B, VMAX, 2))
    init_xy = np.zeros((B, 2 * n))
    count = np.zeros((T, B), dtype=np.int32)
    meas = np.zeros((T, B, JMAX, 2))
    truth = np.full((T, B, JMAX), -1, dtype=np.int32)
    for t in range(T):
        for b, fam in enumerate(FAMILIES):
            rf = rs.robot_frame(pose[t, b], world)
            noisy = rf + rng.normal(0.0, SENSOR_STD, size=(n, 2))
            order = rng.permutation(JMAX)
            if t == 0:
                init_xy[b] = noisy.reshape(-1)
            if not reads[t, b]:
                continue
            if t > 0:
                sel = np.sort(_select(rf, fam, VMAX))
                lm_idx[t, b, :len(sel)] = sel
                z_xy[t, b, :len(sel)] = noisy[sel]
            sel = _select(rf, fam, JMAX)
            sel = sel[[k for k in order if k < len(sel)]]      # shuffled: the filter discovers its map in this order
            count[t, b] = len(sel)
            meas[t, b, :len(sel)] = noisy[sel]
            truth[t, b, :len(sel)] = sel
    survey = np.tile(world.reshape(-1), (B, 1)) + rng.normal(0.0, SENSOR_STD, size=(B, 2 * n))
    case = Case(n, seed, world, pose, reads, twist, lm_idx, z_xy, init_xy, count, meas, truth, survey)
    for a in (world, pose, reads, twist, lm_idx, z_xy, init_xy, count, meas, truth, survey):
        a.flags.writeable = False
    return case


# ---- replays on anything with OracleEKF's surface (OracleEKF, RefEKF, NumpyEKF, MotionEKF) --------------------------

def replay_known(f, case, b, t0=0, t1=T):
    for t in range(t0, t1):
        f.prediction(*case.twist[t, b])
        f.measurement(*case.expand_step(t, b))
    return f


def survey(f, case, b):
    """the surveyed map: one known-association call with nothing visible at the start pose -> the known list"""
    f.prediction(0.0, 0.0)
    f.measurement(case.survey_xy[b], np.zeros(case.n, dtype=np.uint8))
    return np.ones(case.n, dtype=np.uint8)


def replay_unknown(f, case, b, known, margins=None):
    """-> decisions [T, JMAX] (-2 where there is no reading; None for a filter that reports none)"""
    dec = np.full((T, JMAX), -2, dtype=np.int32)
    for t in range(T):
        J = int(case.count[t, b])
        f.prediction(*case.twist[t, b])
        d = f.data_association(case.meas_xy[t, b, :J], known) if margins is None else \
            f.data_association(case.meas_xy[t, b, :J], known, margins)
        if d is None:
            dec = None
        elif dec is not None:
            dec[t, :J] = d
    return dec


# ---- the structured restatement that takes mutants ------------------------------------------------------------------

class MotionEKF:
    """oracle/np_restatement.py's NumpyEKF with At Sigma At^T + Q written as its rows / columns 1, 2 and (I - K H) Sigma as
    Sigma - K (H Sigma): O(N^2) per call, so n = 300 replays in well under a second.  mutant: None or one of MUTANTS.
    trace: every correction appends (landmark, raw bearing difference); every prediction appends its branch."""

    def __init__(self, n, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.n, self.N, self.mutant = n, 3 + 2 * n, mutant
        self.sigma = np.zeros((self.N, self.N))
        self.sigma[3:, 3:] = np.eye(2 * n) * 100
        self._state = np.zeros(self.N)
        self.landmark_init_flag = False
        self.raw, self.branches = [], []
        self._acc = None       # stale_apred: the map of the predictions since the last correction, for the indices >= 3

    def prediction(self, dtheta, dx):  # ekf_slam.cpp:55-106
        dtheta, dx = np.float64(dtheta), np.float64(dx)
        theta = self._state[0]
        straight = abs(dtheta) <= 0.000001 if self.mutant == "gate_le" else abs(dtheta) < 0.000001
        self.branches.append("straight" if straight else "arc")
        if straight and self.mutant != "no_straight":
            u = (0.0, dx * math.cos(theta), dx * math.sin(theta))
            a10, a20 = -dx * math.sin(theta), dx * math.cos(theta)
            if self.mutant == "a10_sign":
                a10 = -a10
        else:
            with np.errstate(all="ignore"):
                r = dx / dtheta
                u = (dtheta, -r * math.sin(theta) + r * math.sin(theta + dtheta), r * math.cos(theta) - r * math.cos(theta + dtheta))
                a10 = -r * math.cos(theta) + r * math.cos(theta + dtheta)
                a20 = -r * math.sin(theta) + r * math.sin(theta + dtheta)
        self._state[:3] += u
        S = self.sigma
        with np.errstate(all="ignore"):
            if self.mutant == "stale_apred":
                # the pose block now, the long part of rows / columns 1, 2 at the next correction -- from the LAST
                # prediction's (a10, a20) alone instead of their sum (row / column 0 do not change under predictions)
                self._acc = (a10, a20)
                P = S[:3, :3].copy()
                P[1] += a10 * P[0]; P[2] += a20 * P[0]
                P[:, 1] += a10 * P[:, 0]; P[:, 2] += a20 * P[:, 0]
                S[:3, :3] = P
            else:
                S[1] += a10 * S[0]; S[2] += a20 * S[0]
                S[:, 1] += a10 * S[:, 0]; S[:, 2] += a20 * S[:, 0]
        S[0, 0] += 0.0001; S[1, 1] += 0.0001; S[2, 2] += 0.0001

    def _settle(self):
        if self._acc is not None:
            a10, a20 = self._acc
            S = self.sigma
            S[1, 3:] += a10 * S[0, 3:]; S[2, 3:] += a20 * S[0, 3:]
            S[3:, 1] += a10 * S[3:, 0]; S[3:, 2] += a20 * S[3:, 0]
            self._acc = None

    def _terms(self, i, sx, sy, theta, x, y):
        tx, ty = self._state[2 * i + 3], self._state[2 * i + 4]
        z = np.array([math.sqrt(sx ** 2 + sy ** 2), math.atan2(sy, sx)])
        dx_, dy_ = tx - x, ty - y
        d = dx_ ** 2 + dy_ ** 2
        zhat = np.array([math.sqrt(d), predicted_bearing(self._state, i, theta, x, y)])
        cols = [0, 1, 2, 3 + 2 * i, 4 + 2 * i]
        Hc = np.array([[0, -dx_ / math.sqrt(d), -dy_ / math.sqrt(d), dx_ / math.sqrt(d), dy_ / math.sqrt(d)],
                       [-1, dy_ / d, -dx_ / d, -dy_ / d, dx_ / d]])
        return z, zhat, cols, Hc

    def _correct(self, i, sx, sy, theta, x, y):  # ekf_slam.cpp:137-192 / :331-390
        self._settle()
        z, zhat, cols, Hc = self._terms(i, sx, sy, theta, x, y)
        SHt = self.sigma[:, cols] @ Hc.T
        K = SHt @ np.linalg.inv(Hc @ SHt[cols] + np.diag([0.01, 0.01]))
        zd = z - zhat
        self.raw.append((i, float(zd[1])))
        if self.mutant != "no_wrap":
            zd[1] = _normalize(zd[1])
        self._state = self._state + K @ zd
        self._state[0] = _normalize(self._state[0])
        self.sigma -= K @ (Hc @ self.sigma[cols])

    def measurement(self, sensor_xy, visible):  # ekf_slam.cpp:108-197
        theta, x, y = self._state[:3]
        if not self.landmark_init_flag:
            s = np.asarray(sensor_xy, dtype=np.float64).reshape(-1, 2)
            ri, phii = np.hypot(s[:, 0], s[:, 1]), np.arctan2(s[:, 1], s[:, 0])
            self._state[3::2] = x + ri * np.cos(phii + theta)
            self._state[4::2] = y + ri * np.sin(phii + theta)
            self.landmark_init_flag = True
        for i in np.nonzero(visible)[0]:
            self._correct(int(i), sensor_xy[2 * i], sensor_xy[2 * i + 1], theta, x, y)

    def maha(self, sx, sy, i):  # ekf_slam.cpp:217-276 (the bearing difference is NOT wrapped, :269)
        self._settle()
        z, zhat, cols, Hc = self._terms(i, sx, sy, *self._state[:3])
        psi = Hc @ self.sigma[np.ix_(cols, cols)] @ Hc.T + np.diag([0.01, 0.01])
        v = z - zhat
        return float(v @ np.linalg.inv(psi) @ v)

    def data_association(self, meas_xy, known):  # ekf_slam.cpp:278-402
        known_count = 0
        for k in known:
            if not k:
                break
            known_count += 1
        assoc = []
        for mx, my in np.asarray(meas_xy, dtype=np.float64).reshape(-1, 2):
            best, idx = 10.0, known_count
            for i in range(known_count):
                d = self.maha(mx, my, i)
                if d < best:
                    best, idx = d, i
            if idx == known_count and idx < self.n:
                theta, x, y = self._state[:3]
                ri, phii = math.sqrt(mx ** 2 + my ** 2), math.atan2(my, mx)
                self._state[2 * idx + 3] = x + ri * math.cos(phii + theta)
                self._state[2 * idx + 4] = y + ri * math.sin(phii + theta)
                known[known_count] = 1
                known_count += 1
                best = 0.0
            if best < 1.0:
                self._correct(idx, mx, my, *self._state[:3])
                assoc.append(idx)
            else:
                assoc.append(-1)
        return np.array(assoc, dtype=np.int32)

    @property
    def state(self):
        return self._state.copy()

    @property
    def cov(self):
        self._settle()
        return self.sigma.copy()


def _normalize(rad):
    """rigid2d.cpp:336-345"""
    a = math.fmod(math.fmod(rad, 2 * rs.PI) + 2 * rs.PI, 2 * rs.PI)
    return a - 2 * rs.PI if a > rs.PI else a


@functools.lru_cache(maxsize=None)
def reach(n):
    """what the families reach on the unmutated restatement's trajectory of make_case(n)'s known log ->
    {"wraps": per-family corrections with |raw difference| > pi, "corrections": per family, "final_theta": per family,
     "mixed_steps": steps whose predictions take both branches among the filters}"""
    case = make_case(n)
    out = {"wraps": {}, "corrections": {}, "final_theta": {}}
    branches = []
    for b, fam in enumerate(FAMILIES):
        f = replay_known(MotionEKF(n), case, b)
        out["wraps"][fam] = sum(abs(r) > rs.PI for _, r in f.raw)
        out["corrections"][fam] = len(f.raw)
        out["final_theta"][fam] = float(f.state[0])
        branches.append(f.branches)
    out["mixed_steps"] = sum(len({br[t] for br in branches}) == 2 for t in range(T))
    return out
