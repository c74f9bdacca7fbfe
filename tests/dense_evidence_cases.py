"""The numpy model of ekf_dense64_scan_evidence and the cases its host and GPU tests share.  np_scan_evidence is
synth.make_scans (model 0, range_std = 0) operation by operation -- the same expressions in the same order, the landmarks in
ascending index -- with the index of the standing root, the classes and the counts added; margins() lists the beams whose
integers a last-bit difference in sin, cos or sqrt could flip."""
import math

import numpy as np

MARGIN = 1e-9        # relative gap below which a beam is left out of the integer comparisons
MARGIN_CAP = 0.01    # at most this share of a case's beams may be left out


def np_scan_evidence(pose, lms, n_beams, range_max=3.5, border=2.0, radius=0.0762, obs=None, tol=None, tol_abs=0.05,
                     first_lm=0):
    """pose (3,) = (theta, x, y); lms (n, 2), landmark first_lm + i; obs (n_beams,) or None; tol (n,) or None (tol_abs).
    -> dict: expected, hit (absolute index, -1), second (the runner-up value per beam, for margins), cls, n_expected,
    n_agree, n_through, n_short, report"""
    lms = np.asarray(lms, dtype=np.float64).reshape(-1, 2)
    n = len(lms)
    ang = 2.0 * np.pi * np.arange(n_beams) / n_beams
    th = float(pose[0]) + ang
    dx, dy = np.cos(th), np.sin(th)
    ox, oy = float(pose[1]), float(pose[2])
    half = border / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(dx > 0, (half - ox) / dx, np.where(dx < 0, (-half - ox) / dx, np.inf))
        ty = np.where(dy > 0, (half - oy) / dy, np.where(dy < 0, (-half - oy) / dy, np.inf))
    r = np.minimum(np.minimum(tx, ty), range_max)
    hit = np.full(n_beams, -1, dtype=np.int32)
    second = np.full(n_beams, np.inf)      # the smallest value that did not win
    second_same = np.zeros(n_beams, dtype=bool)   # ... and it is the root of a landmark with the winner's coordinates
    graze = np.zeros(n_beams, dtype=bool)  # a disc within MARGIN of 0 on a landmark that could matter
    reach = range_max + radius
    n_cand = 0
    with np.errstate(invalid="ignore"):
        for j, (cx, cy) in enumerate(lms):
            fx, fy = ox - cx, oy - cy
            n_cand += bool(fx * fx + fy * fy <= reach * reach * (1.0 + 1e-12))
            bq = fx * dx + fy * dy
            cq = fx * fx + fy * fy - radius ** 2
            disc = bq * bq - cq
            hitj = disc > 0
            t = -bq - np.sqrt(np.where(hitj, disc, 0.0))
            win = hitj & (t > 0) & (t < r)
            lose = hitj & (t > 0) & ~win
            graze |= (np.abs(disc) <= MARGIN * np.maximum(bq * bq, np.abs(cq))) & (-bq > 0) & (-bq < r * (1 + 1e-6))
            # the value that loses: the old r where t wins, t where it does not
            loser = np.where(win, r, np.where(lose, t, np.inf))
            same = np.zeros(n_beams, dtype=bool)
            if n and np.isfinite(cx) and np.isfinite(cy):
                prev = np.where(hit >= 0, hit - first_lm, 0)
                same = (hit >= 0) & (lms[prev, 0] == cx) & (lms[prev, 1] == cy) & lose
            upd = loser < second
            second = np.where(upd, loser, second)
            second_same = np.where(upd, np.where(win, False, same), second_same)
            r = np.where(win, t, r)
            hit = np.where(win, first_lm + j, hit)
    out = dict(expected=r, hit=hit, second=second, second_same=second_same, graze=graze)
    cls = np.zeros(n_beams, dtype=np.uint8)
    cnt = np.zeros((4, n), dtype=np.int32)
    rep = dict(n_candidates=int(n_cand), n_on_tube=int((hit >= 0).sum()), n_unexplained=0, n_invalid=0)
    if obs is not None:
        obs = np.asarray(obs, dtype=np.float64)
        tl = np.full(n, float(tol_abs)) if tol is None else np.asarray(tol, dtype=np.float64)
        for b in range(n_beams):
            o, e = obs[b], r[b]
            if not o > 0.0:
                cls[b] = 4
                rep["n_invalid"] += 1
            elif hit[b] < 0:
                rep["n_unexplained"] += bool(o < e - tol_abs)
            else:
                i = hit[b] - first_lm
                d = o - e
                cls[b] = 1 if abs(d) <= tl[i] else (2 if d > tl[i] else 3)
                cnt[0, i] += 1
                cnt[cls[b], i] += 1
    out.update(cls=cls, n_expected=cnt[0], n_agree=cnt[1], n_through=cnt[2], n_short=cnt[3], report=rep)
    return out


def margins(model, obs=None, tol=None, tol_abs=0.05, first_lm=0):
    """-> bool (n_beams,): beams whose hit index or class a relative error of MARGIN could flip.  A runner-up that is the
    root of a landmark with the winner's very coordinates is equal in bits by construction and is no such beam."""
    e, s = model["expected"], model["second"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(s - e) <= MARGIN * np.maximum(np.abs(e), 1e-300)) & ~model["second_same"]
    risky = near | model["graze"]
    if obs is not None:
        obs = np.asarray(obs, dtype=np.float64)
        hit = model["hit"]
        for b in range(len(e)):
            if not obs[b] > 0.0:
                continue
            if hit[b] < 0:
                edge = e[b] - tol_abs
                risky[b] |= abs(obs[b] - edge) <= MARGIN * max(abs(edge), 1e-300)
            else:
                t = tol_abs if tol is None else tol[hit[b] - first_lm]
                if math.isfinite(t):
                    risky[b] |= abs(abs(obs[b] - e[b]) - t) <= MARGIN * max(t, abs(e[b]))
    return risky


def observed(model, through=(), short=(), invalid=(), short_wall=(), jitter=0.001):
    """a scan built from the model's expected one: +-jitter everywhere (inside any tolerance >= 10 jitter), the beams of
    `through` 0.5 m behind their tube, those of `short` 0.3 m in front, `invalid` cycling NaN, 0, -1, and the wall beams of
    `short_wall` 0.4 m short"""
    e = model["expected"]
    obs = e + jitter * np.where(np.arange(len(e)) % 2 == 0, 1.0, -1.0)
    for b in through:
        obs[b] = e[b] + 0.5
    for b in short:
        obs[b] = e[b] - 0.3
    for b in short_wall:
        obs[b] = e[b] - 0.4
    for k, b in enumerate(invalid):
        obs[b] = (np.nan, 0.0, -1.0)[k % 3]
    return obs


def disk_world(n_in, n_out, seed, reach=3.5, min_gap=0.25):
    """n_in landmarks within `reach` - 0.2 of the origin (no two closer than min_gap, none within 0.3 of it), then n_out
    beyond 2 * reach, shuffled together by the seed -> (lms (n_in + n_out, 2), in_reach bool)"""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n_in:
        p = rng.uniform(-reach, reach, 2)
        rr = math.hypot(*p)
        if 0.3 < rr < reach - 0.2 and all(math.hypot(*(p - q)) >= min_gap for q in pts):
            pts.append(p)
    far = [(2 * reach + 1.0 + k * 0.1) * np.array([math.cos(k), math.sin(k)]) for k in range(n_out)]
    lms = np.array(pts + far).reshape(-1, 2)
    order = rng.permutation(len(lms))
    return lms[order], (order < n_in)


INF = float("inf")
P, Q = (1.5, 0.3), (0.4, -1.2)

# name -> dict(pose, lms, lidar = (n_beams, range_max, border, radius), key = beams the case exists for)
CASES = {
    "exact": dict(pose=(0.0, 0.0, 0.0), lms=[(1.0, 0.0)], lidar=(4, 3.5, 2.0, 0.25), key=[0]),
    "occlusion": dict(pose=(0.0, 0.0, 0.0), lms=[(1.0, 0.0), (2.0, 0.0)], lidar=(64, 3.5, INF, 0.1), key=[0, 1, 63]),
    "occlusion_far_first": dict(pose=(0.0, 0.0, 0.0), lms=[(2.0, 0.0), (1.0, 0.0)], lidar=(64, 3.5, INF, 0.1), key=[0, 1, 63]),
    "tie_low_high": dict(pose=(0.1, 0.05, -0.02), lms=[P, Q, P], lidar=(63, 3.5, INF, 0.15), key=[]),
    "tie_adjacent": dict(pose=(0.1, 0.05, -0.02), lms=[Q, P, P], lidar=(65, 3.5, INF, 0.15), key=[]),
    "nan_landmark": dict(pose=(0.2, 0.0, 0.1), lms=[(float("nan"), float("nan")), (1.0, 0.2), (float("nan"), 1.0)],
                         lidar=(64, 3.5, 4.0, 0.2), key=[]),
    "inside_a_tube": dict(pose=(0.0, 0.05, 0.0), lms=[(0.1, 0.0), (1.5, 0.0)], lidar=(8, 3.5, INF, 0.25), key=[0]),
    "beyond_and_cut": dict(pose=(0.0, 0.0, 0.0), lms=[(5.0, 0.0), (0.0, 3.6), (-3.8, 0.0)], lidar=(360, 3.5, INF, 0.25),
                           key=[90]),
    "wall_nearer": dict(pose=(0.0, 0.0, 0.0), lms=[(1.5, 0.0), (0.0, 0.6)], lidar=(8, 3.5, 2.0, 0.1), key=[0, 2]),
    "heading_not_wrapped": dict(pose=(3.0 * math.pi + 0.3, 0.2, -0.1), lms=[(-1.2, -0.5), (0.9, 0.8), (-0.3, 1.4)],
                                lidar=(65, 3.5, 6.0, 0.2), key=[]),
}
for _n, _seed in ((1, 1), (127, 2), (128, 3), (129, 4), (130, 5)):
    _lms, _in = disk_world(_n, 100 if _n == 129 else 0, 40 + _seed)
    CASES[f"world_{_n}"] = dict(pose=(0.4, 0.1, -0.2), lms=_lms, lidar=(360, 3.5, INF, 0.0762), key=[], in_reach=_in)


def case(name):
    c = CASES[name]
    nb, rmax, border, radius = c["lidar"]
    return np.array(c["pose"], dtype=np.float64), np.asarray(c["lms"], dtype=np.float64).reshape(-1, 2), nb, rmax, border, radius


def case_model(name, **kw):
    pose, lms, nb, rmax, border, radius = case(name)
    return np_scan_evidence(pose, lms, nb, rmax, border, radius, **kw)


def classed_scan(name):
    """the observed scan of the class tests for a case: of the beams that expect a tube every 3rd goes through, every 5th
    (not a 3rd) stops short, every 7th is invalid; of the others every 4th stops short of the wall -> (obs, model with obs)"""
    m = case_model(name)
    tube = np.nonzero(m["hit"] >= 0)[0]
    wall = np.nonzero(m["hit"] < 0)[0]
    through = [b for k, b in enumerate(tube) if k % 3 == 0]
    short = [b for k, b in enumerate(tube) if k % 5 == 1 and k % 3 != 0]
    invalid = [b for k, b in enumerate(tube) if k % 7 == 2 and k % 3 != 0 and k % 5 != 1] + list(wall[1::9])
    obs = observed(m, through, short, invalid, list(wall[::4]))
    return obs, case_model(name, obs=obs)


def np_evidence_update(logodds, n_expected, n_agree, n_through, min_beams, w_hit, w_miss, l_min, l_max):
    """ekf_dense64_evidence_update restated -> (logodds, verdict)"""
    l = np.array(logodds, dtype=np.float64)
    v = np.zeros(len(l), dtype=np.int32)
    for i in range(len(l)):
        e, a, t = int(n_expected[i]), int(n_agree[i]), int(n_through[i])
        if e >= min_beams:
            if 2 * a >= e:
                l[i] = l[i] + w_hit
                v[i] = 1
            elif 2 * t > e:
                l[i] = l[i] - w_miss
                v[i] = -1
        l[i] = min(max(l[i], l_min), l_max)
    return l, v


# ---- the lifecycle: a filter at rest among tubes, one planted landmark, one true tube beyond the circle fit's reach --------
LIFE_SCANS, LIFE_SEED, LIFE_STD, LIFE_MIN_BEAMS = 15, 41, 0.0005, 3   # (at this range_std every near tube passes the circle test by > 0.08 rad)
LIFE_LIDAR = (360, 3.5, INF, 0.0762)
LIFE_PLANT_W = 0.01          # variance of the two planted landmarks (m^2)
LIFE_TOL = (0.05, 1.0)       # the tolerances of the filter's landmarks lie in this range (asserted on the GPU)


def life_world():
    """-> near (7, 2): tubes within 1 m, each more than 6 beams wide, in ascending bearing (the order the circle fit finds
    them in); distant (2,): a true tube at 1.5 m, 5 beams wide; ghost (2,): a spot at 1.4 m where nothing stands, clear of
    every tube by 0.7 m and with nothing behind it"""
    ang = np.deg2rad([20.0, 70.0, 120.0, 170.0, 220.0, 270.0, 320.0])
    rad = np.array([0.7, 0.9, 0.6, 1.0, 0.8, 0.65, 0.95])
    near = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    distant = 1.5 * np.array([math.cos(math.radians(95.0)), math.sin(math.radians(95.0))])
    ghost = 1.4 * np.array([math.cos(math.radians(40.0)), math.sin(math.radians(40.0))])
    return near, distant, ghost


def life_scans():
    """the LIFE_SCANS seeded noisy scans of the true world (near tubes and the distant one) from pose 0"""
    from ekf_slam_ml_amd import synth
    near, distant, _ = life_world()
    nb, rmax, border, radius = LIFE_LIDAR
    world = np.vstack([near, distant[None, :]])
    return np.stack([synth.make_scans(np.zeros((1, 3)), world, n_beams=nb, seed=LIFE_SEED, range_std=LIFE_STD,
                                      range_max=rmax, border=border, tube_radius=radius, step=k)[0]
                     for k in range(LIFE_SCANS)])


def life_map():
    """the filter's map in its own order: the ghost (planted first), the distant tube (planted second), the near tubes"""
    near, distant, ghost = life_world()
    return np.vstack([ghost[None, :], distant[None, :], near])


def life_counts(obs, tol):
    """the model's counters of one scan against the true map under one tolerance for all -> (n_expected, n_agree, n_through)"""
    nb, rmax, border, radius = LIFE_LIDAR
    lm = life_map()
    m = np_scan_evidence(np.zeros(3), lm, nb, rmax, border, radius, obs=obs, tol=np.full(len(lm), tol), tol_abs=LIFE_TOL[0])
    return m["n_expected"], m["n_agree"], m["n_through"]
