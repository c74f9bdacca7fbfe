"""ekf_dense64_scan_evidence on the GPU box: one 360-beam tube-world scan cast against a map of 5000 known landmarks in a
handle of N = 10003, with kappa = 0 and kappa > 0, beside fit_scan and associate_scan on the same scan in the same run, the
host route the call replaces (get_state + synth.make_scans over the 5000 landmarks), and remove_landmark beside
merge_landmarks.  Medians of `--reps` calls, wall clock and HIP-event time.  Writes profiles/r40/dense64_evidence_bench.txt.

    python tools/dense64_evidence_bench.py [--n 5000] [--reps 30]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ekf_slam_ml_amd import capi, synth  # noqa: E402


def timed(fn, reps):
    wall, ev = [], []
    for _ in range(reps + 3):
        t0 = time.perf_counter()
        ms = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ms if ms is not None else float("nan"))
    return float(np.median(wall[3:])), float(np.median(ev[3:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    n, N = a.n, 3 + 2 * a.n
    rng = np.random.default_rng(40)
    side = 0.6 * np.sqrt(n)   # the density of the project's 1000-landmark world (spacing >= 0.6)
    world = rng.uniform(-side / 2, side / 2, (n, 2))
    pose = np.array([0.3, 0.2, -0.1])
    x = np.concatenate([pose, world.reshape(-1)])
    d = capi.DensePropagator64(N)
    d.state = x
    for first in range(0, N, d.MAX_R):
        r = min(d.MAX_R, N - first)
        d.init_block(first, W=0.01 * np.eye(r))
    lp = capi.default_lidar(border_width=float("inf"), range_std=0.005)
    ranges = synth.make_scans(pose[None, :], world, n_beams=360, seed=40, range_std=0.005, border=float("inf"))[0]

    def host_route():
        xs = d.state
        synth.make_scans(xs[None, :3], xs[3:].reshape(-1, 2), n_beams=360, range_std=0.0, border=float("inf"))

    lines = [f"dense64 scan evidence: N = {N}, {n} known landmarks, 360 beams, medians of {a.reps} calls (ms)"]
    res = {}
    for name, fn in (
        ("scan_evidence kappa=0", lambda: d.scan_evidence(ranges, lp, kappa=0.0).ms),
        ("scan_evidence kappa=2", lambda: d.scan_evidence(ranges, lp, kappa=2.0).ms),
        ("fit_scan", lambda: d.fit_scan(ranges)[-1]),
        ("host: get_state + make_scans", host_route),
    ):
        res[name] = timed(fn, a.reps)
        lines.append(f"  {name:32s} wall {res[name][0]:9.4f}   events {res[name][1]:9.4f}")
    ev = d.scan_evidence(ranges, lp, kappa=2.0)
    lines.append(f"  report {ev.report}; landmarks with beams {int((ev.n_expected > 0).sum())}")
    ratio = res["scan_evidence kappa=2"][0] / res["fit_scan"][0]
    lines.append(f"  scan_evidence(kappa > 0) / fit_scan, wall clock: {ratio:.3f} (condition: <= 1.5)")
    # associate_scan changes the filter, so it runs last and five times only, on this same handle
    known = n
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        known = d.associate_scan(ranges, known, n)[0]
        t.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"  {'associate_scan':32s} wall {float(np.median(t)):9.4f}   (5 calls, known -> {known})")
    # removal and merge: on the handle as those five calls left it, eager, carry off, no live dimension to follow;
    # the merged pairs (100 + k, 200 + k) are unrelated landmarks fused with r_merge = 1.0 -- a timing, not a use
    known = n
    t_rm, t_mg = [], []
    for k in range(5):
        t0 = time.perf_counter()
        known = d.remove_landmark(7 + k, known)[0]
        t_rm.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        known = d.merge_landmarks(100 + k, 200 + k, 1.0, known)[0]
        t_mg.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"  {'remove_landmark':32s} wall {float(np.median(t_rm)):9.4f}   (5 calls, eager, a landmark in mid-map)")
    lines.append(f"  {'merge_landmarks':32s} wall {float(np.median(t_mg)):9.4f}   (5 calls, eager, unrelated pairs, r_merge = 1)")
    d.close()
    out = os.path.join(ROOT, "profiles", "r40", "dense64_evidence_bench.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    text = "\n".join(lines) + "\n"
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
