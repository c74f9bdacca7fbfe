"""ekf_dense64_rank_landmarks of the dense fp64 handle on the GPU box: what observing each of 5000 landmarks would gain, in
one pass over Sigma.

At N = 10003 the handle holds 5000 landmarks; everything runs in one process, medians of >= 9 after >= 2 untimed, HIP-event
time and wall clock of one call.  Beside rank_landmarks: health (it reads the same 8 Na^2 bytes once) and landmark_pairs (the
project's other all-landmarks pass).  The rate is 8 Na^2 bytes over the HIP-event time.  The spelled route -- per landmark
one clone into a second handle and one correct_sparse with nu = 0 -- is timed for --spelled landmarks (HIP events of the two
calls; reading the traces back is not included) and EXTRAPOLATED to all 5000.

    python tools/dense64_value_bench.py [--n 10003] [--iters 9] [--warmup 2] [--out profiles/r37/dense64_value_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spelled", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r37", "dense64_value_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    assert a.n % 2 == 1 and a.n >= 5
    import numpy as np
    from ekf_slam_ml_amd import capi

    N = a.n
    b = (N - 3) // 2
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    S = 0.5 * (S + S.T)
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    src, dst = capi.DensePropagator64(N), capi.DensePropagator64(N)
    src.set(Sigma=S)
    src.state = x
    dst.set(Sigma=np.zeros((N, N)))
    info = src.value_launch_info()

    def stats(call):
        wall, ev = [], []
        for _ in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            ms = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(ms)
        wall, ev = np.array(wall[a.warmup:]), np.array(ev[a.warmup:])
        return float(np.median(wall)), float(wall.min()), float(wall.max()), float(np.median(ev)), float(ev.min()), float(ev.max())

    by = 8.0 * N * N

    def line(name, t):
        return (f"{name:34s} HIP events {t[3]:.4f} ms (min {t[4]:.4f}, max {t[5]:.4f}) = {by / (t[3] * 1e-3) / 1e12:.2f} TB/s on "
                f"{by / 1e6:.1f} MB (8 Na^2); wall clock median {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})")

    lines = [f"# python tools/dense64_value_bench.py   (MI355X, N = Na = {N}, {b} landmarks, medians of {a.iters} after {a.warmup}, "
             f"one process; tile_rows {info['tile_rows']}, tile_lm {info['tile_lm']}, {info['threads']} threads)"]
    t_rank = stats(lambda: src.rank_landmarks().ms)
    t_one = stats(lambda: src.rank_landmarks(first_lm=b // 2, count=1).ms)
    t_health = stats(lambda: src.health()["ms"])
    t_pairs = stats(lambda: src.landmark_pairs(b, 0.5, 9.0)[4])
    lines.append(line(f"rank_landmarks, all {b}", t_rank))
    lines.append(f"{'rank_landmarks, one landmark':34s} HIP events {t_one[3]:.4f} ms (min {t_one[4]:.4f}, max {t_one[5]:.4f}): four "
                 f"launches on {24.0 * N / 1e6:.2f} MB, the floor of the call; wall clock median {t_one[0]:.4f} ms")
    lines.append(line("health", t_health))
    lines.append(line(f"landmark_pairs, all {b}", t_pairs))
    lines.append(f"rank_landmarks / health = {t_rank[3] / t_health[3]:.3f} (HIP events); rank_landmarks / landmark_pairs = "
                 f"{t_rank[3] / t_pairs[3]:.3f}")
    recs = 48.0 * b * -(-N // info["tile_rows"])
    lines.append(f"the pass also writes and the fold reads {recs / 1e6:.1f} MB of records ({100.0 * 2 * recs / by:.1f} % of 8 Na^2 both ways)")

    # the spelled route for a few landmarks: clone + correct_sparse(nu = 0); the traces of Sigma+ are checked, not timed
    r = src.rank_landmarks()
    picks = np.linspace(0, b - 1, a.spelled).astype(int)
    clone_ms, corr_ms, worst = [], [], 0.0
    tr0 = np.trace(S)
    for j in picks:
        clone_ms.append(dst.extract_map(src))
        corr_ms.append(dst.correct_sparse(np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j]), r.Hc[j], r.R, np.zeros(2))[1])
        if j in (picks[0], picks[-1]):
            worst = max(worst, abs((tr0 - np.trace(dst.sigma)) - r.dtrace[j]) / r.dtrace[j])
    per = float(np.median(clone_ms) + np.median(corr_ms))
    lines.append(f"the spelled route, {a.spelled} landmarks: clone {np.median(clone_ms):.4f} ms + correct_sparse {np.median(corr_ms):.4f} ms "
                 f"= {per:.4f} ms a landmark (HIP events, medians; the read-back of the traces not included)")
    lines.append(f"EXTRAPOLATED to {b} landmarks: {per * b:.0f} ms = {per * b / t_rank[3]:.0f} x rank_landmarks "
                 f"(an extrapolation from {a.spelled} landmarks, not a measurement of {b})")
    lines.append(f"dtrace against tr Sigma - tr Sigma+ read back for the first and the last of them: relative difference {worst:.2e}")
    src.close()
    dst.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
