"""Shapes, worlds and references of the simulator / consistency-statistics tests (tests/test_sim_cases_host.py on the
CPU, tests/test_gpu_sim_shapes.py on the GPU).  No GPU here.

k_sim_trajectory and k_mc_stats launch (B + 127) / 128 blocks of 128 threads; k_sim_readings and k_sim_unknown_readings
pick the vmax nearest landmarks within the visibility radius by a repeated lexicographic (d2, index) minimum over 256
threads (four waves), at most 64 of them.  The cases below are the pool sizes and the selections at which that code takes
another path: a second block, a ragged last block, B = 1; a tie in d2 at the vmax cut, resolved inside one thread, inside
one wave and across waves; vmax > n (the sentinel exit); nothing in view; n <= 64 and n = 1 (three of four waves hold
sentinels only); and the bench's small-map shape.

The host twin synth.make_known_log / make_unknown_log builds its own world from the config; with_world() hands it the
world of a case instead."""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from ekf_slam_ml_amd import synth

BLOCK = 128           # threads of a k_sim_trajectory / k_mc_stats workgroup
SELECT_THREADS = 256  # threads of a k_sim_readings workgroup: landmark i is looked at by thread i % 256
WAVE = 64
CHOSEN_MAX = 64       # entries of the kernels' `chosen` array (ekf_batch_simulate_*_log refuses vmax > 64)

# ---- worlds ---------------------------------------------------------------------------------------------------------

# The duplicate world.  Pair p shares ONE position, the (3 + p)-th nearest of every pose of the case, so the pairs fill
# the distance ranks (3, 4), (5, 6), (7, 8), (9, 10) behind three single landmarks: a cap of vmax = 4, 6, 8 or 10 readings
# cuts between the two landmarks of one pair, at bit-equal d2.  Which code resolves the tie depends on where the two sit:
#   (0, n - 1)   n = 300: threads 0 and 43 of wave 0             -> the shuffle reduction
#   (3, 11)      threads 3 and 11 of wave 0                      -> the shuffle reduction
#   (20, 276)    276 = 20 + 256: both looked at by thread 20     -> the thread's own scan (`d2 == best && i < bi`)
#   (70, 200)    waves 1 and 3                                    -> thread 0's pass over the four wave minima
DUP_N = 300
DUP_PAIRS = ((0, DUP_N - 1), (3, 11), (20, 276), (70, 200))
DUP_SINGLES = (1, 2, 4)                  # the three nearest landmarks
DUP_RING0, DUP_RING_STEP = 0.30, 0.08    # distance of rank-0 position from the reference pose, and from ring to ring
DUP_FAR = 1.25                           # every other landmark is at least this far from the reference pose
DUP_VISIBLE = 3.0
DUP_CUTS = {4: (0, DUP_N - 1), 6: (3, 11), 8: (20, 276), 10: (70, 200)}   # vmax -> (taken, left out)


def random_world(cfg):
    wseed = cfg.seed if cfg.world_seed is None else cfg.world_seed
    return synth.make_world(cfg.n, cfg.half_extent, cfg.min_spacing, wseed)


def far_world(cfg):
    """a random world moved 10 m away along both axes: nothing ever within max_visible_dis"""
    return random_world(cfg) + np.array([10.0, 10.0])


def duplicate_world(cfg):
    """see DUP_PAIRS.  The reference pose is the origin: the robots of the case stay within 5 cm of it (v_cmd 0.1 m/s, 3
    steps), the rings are 8 cm apart."""
    assert cfg.n == DUP_N
    rings = len(DUP_SINGLES) + len(DUP_PAIRS)
    ang = 2.399963229728653 * np.arange(rings)    # golden angle: the ring positions point in different directions
    rad = DUP_RING0 + DUP_RING_STEP * np.arange(rings)
    ring_xy = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    pool = synth.make_world(2 * DUP_N, 6.0, 0.3, cfg.seed, use_reference_tubes=False)
    pool = pool[np.hypot(pool[:, 0], pool[:, 1]) >= DUP_FAR]
    world = np.full((DUP_N, 2), np.nan)
    for k, i in enumerate(DUP_SINGLES):
        world[i] = ring_xy[k]
    for k, (i, j) in enumerate(DUP_PAIRS):
        world[i] = world[j] = ring_xy[len(DUP_SINGLES) + k]
    rest = np.nonzero(np.isnan(world[:, 0]))[0]
    assert len(pool) >= len(rest)
    world[rest] = pool[:len(rest)]
    return world


WORLDS = {"random": random_world, "duplicate": duplicate_world, "far": far_world}


@contextlib.contextmanager
def with_world(world):
    """synth's generators with `world` in place of the one they would draw from the config"""
    orig = synth.make_world
    synth.make_world = lambda n, *a, **k: np.array(world, dtype=np.float64)
    try:
        yield
    finally:
        synth.make_world = orig


# ---- cases ----------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    world_kind: str
    cfg: synth.SimConfig = dataclasses.field(compare=False)
    reaches: str = ""

    def __str__(self):
        return self.name

    @property
    def world(self):
        return _world(self.name, self.world_kind)

    def host_known(self):
        return _host_log(self.name, False)

    def host_unknown(self):
        return _host_log(self.name, True)


def _cfg(B, n, vmax, T, seed, **kw):
    args = dict(n=n, steps=T, filters=B, seed=seed, vmax=vmax, half_extent=1.5, min_spacing=0.25, max_visible_dis=0.7)
    args.update(kw)
    return synth.SimConfig(**args)


def _bench_small_map():
    """bench.py's small_map_monte_carlo shape: synth.config1's parameters, 8192 filters, the second rank's filter ids"""
    cfg = synth.config1(steps=3)
    cfg.filters, cfg.first_filter_id = 8192, 8192
    return cfg


_ALL_VISIBLE = dict(half_extent=2.0, min_spacing=0.2, max_visible_dis=10.0)
_DUP = dict(max_visible_dis=DUP_VISIBLE, v_cmd=0.1, w_cmd=0.4)

KNOWN_CASES = (
    Case("smallest", "random", _cfg(1, 1, 1, 4, 31), "B = n = vmax = 1"),
    Case("second-block-sentinel", "random", _cfg(129, 5, 8, 3, 32, first_filter_id=7, **_ALL_VISIBLE),
         "second block of one thread; vmax > n takes the sentinel exit"),
    Case("ragged-block-chosen-full", "random", _cfg(257, 64, 64, 3, 33, **_ALL_VISIBLE),
         "ragged last block; the vmax limit; every pass of the 64-entry chosen array"),
    Case("bench-small-map", "random", _bench_small_map(), "8192 filters, vmax == n, first_filter_id = 8192"),
    Case("duplicates", "duplicate", _cfg(40, DUP_N, 6, 3, 34, **_DUP), "n > 256; the cut between landmarks 3 and 11"),
    Case("far-away", "far", _cfg(5, 12, 12, 3, 35), "nothing within the radius in any step"),
    # the other three cuts of the duplicate world (see DUP_PAIRS)
    Case("duplicates-cut-4", "duplicate", _cfg(3, DUP_N, 4, 3, 34, **_DUP), "the cut between landmarks 0 and n - 1"),
    Case("duplicates-cut-8", "duplicate", _cfg(3, DUP_N, 8, 3, 34, **_DUP), "the cut inside thread 20 (20 and 276)"),
    Case("duplicates-cut-10", "duplicate", _cfg(3, DUP_N, 10, 3, 34, **_DUP), "the cut across waves (70 and 200)"),
    # a seed at which a selection by np.argpartition alone keeps 200 and drops 70
    Case("duplicates-cut-10-seed-38", "duplicate", _cfg(3, DUP_N, 10, 3, 38, **_DUP), "the cut across waves, another world"),
)

# the duplicate cases again on other worlds and trajectories (the host test walks all of them)
DUP_SEEDS = tuple(range(34, 46))


def duplicate_seed_log(vmax, seed):
    """(cfg, world, host known log) of the duplicate world drawn from `seed`, capped at vmax readings"""
    cfg = _cfg(3, DUP_N, vmax, 3, seed, **_DUP)
    world = duplicate_world(cfg)
    with with_world(world):
        return cfg, world, synth.make_known_log(cfg)

UNKNOWN_CASES = (
    Case("u-smallest", "random", _cfg(1, 1, 1, 4, 41), "B = n = jmax = 1"),
    Case("u-second-block-sentinel", "random", _cfg(129, 5, 64, 3, 42, first_filter_id=7, **_ALL_VISIBLE),
         "second block of one thread; jmax = 64 > n takes the sentinel exit"),
    Case("u-ragged-block-chosen-full", "random", _cfg(257, 64, 64, 3, 43, **_ALL_VISIBLE),
         "ragged last block; jmax = 64 = n: every pass of the chosen array, a 64-key shuffle"),
    Case("u-one-slot", "random", _cfg(129, 40, 1, 3, 44, half_extent=2.0, min_spacing=0.2, max_visible_dis=0.8),
         "jmax = 1 of many in view"),
    Case("u-duplicates", "duplicate", _cfg(40, DUP_N, 6, 3, 34, **_DUP), "the cut between landmarks 3 and 11"),
    Case("u-duplicates-cut-4", "duplicate", _cfg(3, DUP_N, 4, 3, 34, **_DUP), "the cut between landmarks 0 and n - 1"),
    Case("u-duplicates-cut-8", "duplicate", _cfg(3, DUP_N, 8, 3, 34, **_DUP), "the cut inside thread 20"),
    Case("u-duplicates-cut-10", "duplicate", _cfg(3, DUP_N, 10, 3, 34, **_DUP), "the cut across waves"),
    Case("u-far-away", "far", _cfg(5, 12, 12, 3, 45), "nothing within the radius in any step"),
    Case("u-far-away-one-slot", "far", _cfg(257, 12, 1, 3, 46), "the same at jmax = 1, ragged last block"),
)

BY_NAME = {c.name: c for c in KNOWN_CASES + UNKNOWN_CASES}
SENTINEL_CASES = ("second-block-sentinel", "u-second-block-sentinel")
FAR_CASES = ("far-away", "u-far-away", "u-far-away-one-slot")
ALL_VISIBLE_CASES = ("second-block-sentinel", "ragged-block-chosen-full", "u-second-block-sentinel",
                     "u-ragged-block-chosen-full")


@functools.lru_cache(maxsize=None)
def _world(name, kind):
    w = WORLDS[kind](BY_NAME[name].cfg)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _host_log(name, unknown):
    """the host generator's log of a case: computed once, shared, read-only"""
    case = BY_NAME[name]
    with with_world(case.world):
        log = (synth.make_unknown_log if unknown else synth.make_known_log)(case.cfg)
    for f in dataclasses.fields(log):
        v = getattr(log, f.name)
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return log


def nearest_by_rule(world, pose, k, max_visible_dis):
    """the kernels' documented selection, spelled out: of the landmarks within the radius of pose (theta, x, y), the k
    first in ascending (d2, landmark index); returned in that order.  d2 as synth._robot_frame computes it."""
    rf = synth._robot_frame(np.asarray(world), np.asarray(pose, dtype=np.float64)[None, :])[0]
    d2 = rf[:, 0] ** 2 + rf[:, 1] ** 2
    order = np.lexsort((np.arange(len(d2)), d2))
    return order[d2[order] <= max_visible_dis ** 2][:k]


# ---- laser scans: one shape, for the grid only (one workgroup per scan) ----------------------------------------------

SCAN_S, SCAN_SEED, SCAN_FIRST_ID, SCAN_STEP = 257, 51, 8192, 3


def scan_poses():
    rng = np.random.default_rng(SCAN_SEED)
    S = SCAN_S
    return np.stack([rng.uniform(-np.pi, np.pi, S), rng.uniform(-0.7, 0.7, S), rng.uniform(-0.7, 0.7, S)], axis=1)


# ---- consistency statistics -----------------------------------------------------------------------------------------

MC_N, MC_STEPS, MC_VMAX = 20, 40, 8
MC_POOLS = (257, 1, 129)
NEES_95 = 7.815       # the threshold of ekf_batch_mc_stats' sixth output
U = 2.0 ** -53        # unit roundoff of fp64


def mc_cfg(B, seed=61, steps=MC_STEPS, **kw):
    """robots that turn through w_cmd * steps / 10 = 4 rad > pi: k_sim_trajectory never wraps the true heading, the
    filter wraps its own after every correction, so the raw heading error of the last step is about -2 pi"""
    args = dict(n=MC_N, steps=steps, filters=B, seed=seed, vmax=MC_VMAX, half_extent=1.5, min_spacing=0.25,
                max_visible_dis=0.9, v_cmd=0.1, w_cmd=1.0, sensor_std=0.15, first_filter_id=1000)
    args.update(kw)
    return synth.SimConfig(**args)


def wrap_angle(rad):
    """normalize_angle of ekf_kernels.hpp in the same fp64 operations (additions and fmod: one rounding each, so the
    result is the kernel's bit for bit)"""
    rad = float(rad)
    two_pi = 2.0 * 3.14159265358979323846
    if abs(rad) < two_pi:
        ang = rad + two_pi
        if ang >= two_pi:
            ang = ang - two_pi
    else:
        ang = float(np.fmod(np.fmod(rad, two_pi) + two_pi, two_pi))
    if ang > 3.14159265358979323846:
        ang = ang - two_pi
    return ang


def pose_error(pose, truth):
    """(wrap(theta - theta*), x - x*, y - y*) in fp64, as k_mc_stats forms it: [B, 3]"""
    pose, truth = np.asarray(pose, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    e = pose - truth
    e[:, 0] = [wrap_angle(v) for v in e[:, 0]]
    return e


def exact_nees(e, P):
    """e^T P^-1 e of fp64 inputs in exact rational arithmetic (Cramer's rule on Fractions)"""
    e = [Fraction(float(v)) for v in e]
    (a, b, c), (d, f, g), (h, i, j) = [[Fraction(float(v)) for v in row] for row in np.asarray(P)]
    det = a * (f * j - g * i) - b * (d * j - g * h) + c * (d * i - f * h)
    adj = ((f * j - g * i, c * i - b * j, b * g - c * f),
           (g * h - d * j, a * j - c * h, c * d - a * g),
           (d * i - f * h, b * h - a * i, a * f - b * d))
    x = [sum(adj[r][k] * e[k] for k in range(3)) / det for r in range(3)]
    return sum(e[r] * x[r] for r in range(3))


def adjugate_nees_fp64(e, P):
    """k_mc_stats' own expression (ekf_sim.hip), operation for operation, in numpy fp64 without fused multiply-adds;
    e [B, 3], P [B, 3, 3] -> [B]"""
    e0, e1, e2 = e[:, 0], e[:, 1], e[:, 2]
    a, bq, c = P[:, 0, 0], P[:, 0, 1], P[:, 0, 2]
    d, ee, f = P[:, 1, 0], P[:, 1, 1], P[:, 1, 2]
    g, h, i = P[:, 2, 0], P[:, 2, 1], P[:, 2, 2]
    A, Bc, Cc = ee * i - f * h, -(d * i - f * g), d * h - ee * g
    det = a * A + bq * Bc + c * Cc
    x0 = (A * e0 + (c * h - bq * i) * e1 + (bq * f - c * ee) * e2) / det
    x1 = (Bc * e0 + (a * i - c * g) * e1 + (c * d - a * f) * e2) / det
    x2 = (Cc * e0 + (bq * g - a * h) * e1 + (a * ee - bq * d) * e2) / det
    return e0 * x0 + e1 * x1 + e2 * x2


KEYS = ("nees_mean", "nees_max", "rmse_xy", "rmse_theta", "mean_trace_pose_cov", "frac_nees_below_95pct")


@dataclass
class McReference:
    stats: dict          # the six outputs, each the exact value rounded once
    bound: dict          # allowed |device - stats[k]|
    nees: list           # exact NEES per filter (Fraction)
    gap: float           # worst relative gap of the fp64 adjugate expression to the exact NEES
    nees_rtol: float     # 4 * max(gap, 2^-53)
    margin_95: float     # min over filters of |NEES - 7.815| / 7.815: must exceed nees_rtol for an exact fraction
    raw_heading: np.ndarray = None   # |theta - theta*| before the wrap


def mc_reference(pose, P, truth):
    """The six outputs of ekf_batch_mc_stats for poses [B, 3], pose covariances [B, 3, 3] and truth [B, 3]: the error is
    formed and wrapped in fp64 as the kernel does and enters as given; everything after it is exact rational arithmetic.

    Bound.  The kernel evaluates the adjugate expression in fp64; adjugate_nees_fp64 is that expression on the same
    inputs, and `gap` its worst relative distance to the exact value over the pool -- a property of the inputs and of
    fp64, not of the device.  Every output may differ from its exact value by 4 x the gap, relative (the factor covers
    multiply-adds the compiler may fuse), and nothing is added for the host reduction over the B filters.  The gap is
    taken as no less than 2^-53, the rounding of a result to fp64: at B = 1 the expression can come out closer to the
    exact value than one rounding.  The fraction below 7.815 is exact."""
    pose, P, truth = (np.asarray(v, dtype=np.float64) for v in (pose, P, truth))
    B = len(pose)
    raw = np.abs(pose[:, 0] - truth[:, 0])
    e = pose_error(pose, truth)
    nees = [exact_nees(e[b], P[b]) for b in range(B)]
    fp = adjugate_nees_fp64(e, P)
    gap = max(abs(float((Fraction(float(fp[b])) - nees[b]) / nees[b])) for b in range(B))
    rtol = 4.0 * max(gap, U)
    ef = [[Fraction(float(v)) for v in row] for row in e]
    p2 = sum(r[1] * r[1] + r[2] * r[2] for r in ef)
    a2 = sum(r[0] * r[0] for r in ef)
    tr = sum(Fraction(float(P[b, 0, 0])) + Fraction(float(P[b, 1, 1])) + Fraction(float(P[b, 2, 2])) for b in range(B))
    stats = {"nees_mean": float(sum(nees) / B), "nees_max": float(max(nees)),
             "rmse_xy": math.sqrt(float(p2 / B)), "rmse_theta": math.sqrt(float(a2 / B)),
             "mean_trace_pose_cov": float(tr / B), "frac_nees_below_95pct": sum(v < Fraction(NEES_95) for v in nees) / B}
    bound = {k: rtol * abs(stats[k]) for k in KEYS}
    bound["frac_nees_below_95pct"] = 0.0
    margin = min(abs(float(v) - NEES_95) for v in nees) / NEES_95
    return McReference(stats, bound, nees, gap, rtol, margin, raw)
