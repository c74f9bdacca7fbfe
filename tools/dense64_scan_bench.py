"""A laser scan as the dense fp64 handle's input (ekf_dense64_fit_scan, ekf_dense64_associate_scan) on the GPU box, against
what a caller had before: ekf_circle_fit_scans(S = 1), bound to no handle, and the spelled ekf_circle_fit_scans +
associate_landmarks.  One tube-world scan of 360 beams (synth.make_scans), handles of N = 69 and N = 10003 (5000 known
landmarks, the tubes among them), everything in one process, medians of 9 after 2 with the spread (max - min) of the nine:
  a  HIP-event time of k_scan_circles (fit_scan's elapsed_ms).  k_circles at S = 1 has no events around it: its time comes
     from a kernel trace of the same calls,
         rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/dense64_scan_bench.py --kernels
         python tools/dense64_scan_bench.py --trace DIR --out FILE      (appends the medians of both kernels to FILE)
  b  wall clock of fit_scan against ekf_circle_fit_scans(S = 1);
  c  wall clock of associate_scan against ekf_circle_fit_scans + associate_landmarks, eager and deferred; the pending rows
     are flushed outside the timed region before every repetition.

    python tools/dense64_scan_bench.py [--iters 9] [--warmup 2] [--out profiles/r19/dense64_scan_bench.txt]
"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def the_scan():
    import numpy as np
    from ekf_slam_ml_amd import synth
    return synth.make_scans(np.array([[0.0, 0.0, 0.0]]), seed=21)[0]


def trace_medians(directory, out, keep=9):
    """medians of the last `keep` dispatches of the two circle kernels in a rocprofv3 kernel trace"""
    import numpy as np
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {directory}"
    dur = {}
    for path in files:
        with open(path) as f:
            for row in csv.DictReader(f):
                dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = []
    for key in ("k_scan_circles", "k_circles"):
        for name, v in dur.items():
            if key in name and (key != "k_circles" or "scan" not in name):
                v = np.array(v[-keep:])
                lines.append(f"a  kernel trace, {key}: median {np.median(v):.1f} us of {len(v)} (min {v.min():.1f}, max "
                             f"{v.max():.1f}, spread {v.max() - v.min():.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "a") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", action="store_true", help="only the two circle calls, 11 times each (for a kernel trace)")
    ap.add_argument("--trace", type=str, default=None, help="append the kernel medians of a rocprofv3 trace directory to --out")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r19", "dense64_scan_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    if a.trace:
        return trace_medians(a.trace, a.out)
    import numpy as np
    from ekf_slam_ml_amd import capi, synth

    scan = the_scan()
    if a.kernels:
        d = capi.DensePropagator64(69)
        for _ in range(a.warmup + a.iters):
            d.fit_scan(scan, max_out=32)
        for _ in range(a.warmup + a.iters):
            capi.circle_fit_scans(scan, max_out=32)
        d.close()
        return

    def stats(f, before=None):
        """f() -> HIP-event ms or None; -> (wall median, wall min, wall max, event median), ms"""
        wall, ev = [], []
        for _ in range(a.warmup + a.iters):
            if before:
                before()
            t0 = time.perf_counter()
            ms = f()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(ms if ms is not None else np.nan)
        wall, ev = np.array(wall[a.warmup:]), np.array(ev[a.warmup:])
        return float(np.median(wall)), float(wall.min()), float(wall.max()), float(np.median(ev)), float(ev.max() - ev.min())

    def show(s):
        return f"wall median {s[0]:.4f} ms (min {s[1]:.4f}, max {s[2]:.4f}, spread {s[2] - s[1]:.4f})"

    circles = len(capi.circle_fit_scans(scan, max_out=64)[0][0])
    lines = [f"# python tools/dense64_scan_bench.py   (MI355X, one tube-world scan of {len(scan)} beams with {circles} circles, "
             f"medians of {a.iters} after {a.warmup}, one process)"]
    for N in (69, 10003):
        n = min(5000, (N - 3) // 2)
        rng = np.random.default_rng(8)
        A = rng.standard_normal((N, 64))
        S = A @ A.T / 64 + np.eye(N)
        del A
        x = np.concatenate([[0.0, 0.0, 0.0], rng.uniform(20.0, 40.0, size=N - 3)])
        tubes = min(len(synth.TUBE_X), n)
        x[3:3 + 2 * tubes:2], x[4:4 + 2 * tubes:2] = synth.TUBE_X[:tubes], synth.TUBE_Y[:tubes]
        d = capi.DensePropagator64(N)
        d.set(Sigma=S)
        d.state = x
        del S
        fit = stats(lambda: d.fit_scan(scan, max_out=64)[2])
        old = stats(lambda: capi.circle_fit_scans(scan, max_out=64) and None)
        lines.append(f"N = {N}, {n} known landmarks")
        lines.append(f"a  k_scan_circles, HIP events: median {fit[3] * 1e3:.1f} us (spread {fit[4] * 1e3:.1f})")
        lines.append(f"b  fit_scan: {show(fit)} | ekf_circle_fit_scans(S = 1): {show(old)} | ratio {fit[0] / old[0]:.3f}")
        for deferred in (False, True):
            def spelled():
                cen = capi.circle_fit_scans(scan, max_out=64)[0][0]
                if len(cen):
                    d.associate_landmarks(cen, n, n, deferred)

            new = stats(lambda: d.associate_scan(scan, n, n, 64, deferred) and None, d.flush)
            sp = stats(spelled, d.flush)
            lines.append(f"c  {'deferred' if deferred else 'eager'}: associate_scan {show(new)} | ekf_circle_fit_scans + "
                         f"associate_landmarks {show(sp)} | ratio {new[0] / sp[0]:.3f}")
        d.flush()
        d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
