"""The joint association of the dense fp64 handle (ekf_dense64_associate_joint) against the sequential rule
(ekf_dense64_associate_landmarks) on the GPU box: after tools/dense64_landmarks_bench.py.

At N = 10003 with 5000 known landmarks and a scan of J = 8 readings on distinct landmarks, everything in one process on one
handle, medians of >= 9 after >= 2 untimed.  Before every repetition the state and Sigma are restored (outside the timed
region), so both calls always start from the same bits.  Recorded: wall clock and HIP-event time of one call, eager and
deferred, and the ratios joint / sequential; and the HIP-event time of score_readings(J = 8) next to 8 score_landmarks, which
is the scoring leg of the two calls.

    python tools/dense64_joint_bench.py [--n 10003] [--readings 8] [--iters 9] [--warmup 2] [--out profiles/r22/dense64_joint_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--readings", type=int, default=8)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r22", "dense64_joint_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    import dense_landmark_cases as lc
    from ekf_slam_ml_amd import capi

    N, J = a.n, a.readings
    n = (N - 3) // 2
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    lms = [n * (2 * j + 1) // (2 * J) for j in range(J)]
    z = np.array([lc.reading_of(x, i, (0.002, -0.001)) for i in lms])
    d = capi.DensePropagator64(N)

    def restore():
        d.set(Sigma=S)
        d.state = x

    def stats(call):
        wall, ev = [], []
        for _ in range(a.warmup + a.iters):
            restore()
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(out[-1])
            assert (np.asarray(out[1]) >= 0).all(), out[1]   # every reading corrected a landmark: the work compared is alike
        wall, ev = np.array(wall[a.warmup:]), np.array(ev[a.warmup:])
        return float(np.median(wall)), float(wall.min()), float(wall.max()), float(np.median(ev))

    lines = [f"# python tools/dense64_joint_bench.py   (MI355X, N = {N}, known = n_max = {n}, J = {J} readings on distinct "
             f"landmarks, medians of {a.iters} after {a.warmup}, one process, one handle, state and Sigma restored before "
             f"every repetition)"]
    for deferred in (False, True):
        mode = "DEFERRED" if deferred else "eager"
        tj = stats(lambda: d.associate_joint(z, n, n, deferred=deferred))
        ts = stats(lambda: d.associate_landmarks(z, n, n, deferred=deferred))
        lines.append(f"{mode:8s} associate_joint      wall clock: median {tj[0]:.4f} ms (min {tj[1]:.4f}, max {tj[2]:.4f}); "
                     f"HIP events {tj[3]:.4f} ms")
        lines.append(f"{mode:8s} associate_landmarks  wall clock: median {ts[0]:.4f} ms (min {ts[1]:.4f}, max {ts[2]:.4f}); "
                     f"HIP events {ts[3]:.4f} ms")
        lines.append(f"{mode:8s} joint / sequential = {tj[0] / ts[0]:.3f} (wall clock), {tj[3] / ts[3]:.3f} (HIP events)")
    restore()
    ev_all, ev_one = [], []
    for _ in range(a.warmup + a.iters):
        ev_all.append(d.score_readings(z, count=n)[2])
        ev_one.append(sum(d.score_landmarks(sx, sy, count=n)[3] for sx, sy in z))
    lines.append(f"scoring, HIP events: score_readings(J = {J}) {np.median(ev_all[a.warmup:]) * 1e3:.1f} us in one call; "
                 f"{J} score_landmarks {np.median(ev_one[a.warmup:]) * 1e3:.1f} us in {J} calls")
    d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
