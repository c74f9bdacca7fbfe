"""The landmark front end of the dense fp64 handle (ekf_dense64_score_landmarks, ekf_dense64_associate_landmarks) on the GPU
box: after tools/dense64_swap_bench.py.

At N = 10003 with a full map of 5000 landmarks, everything in one process, medians of >= 9 after >= 2 untimed:
  A  wall clock of one associate_landmarks reading (DEFERRED) that corrects a landmark;
  B  wall clock of the spelled loop's handle calls for the same reading -- state_block, score_sparse, state_block,
     correct_sparse_deferred, the heading read / write -- with every candidate array prebuilt outside the timed region;
and the HIP-event times of score_sparse (the scoring launch alone), score_landmarks (k_dlm_terms + the scoring launch) and a
dropped associate_landmarks reading (k_dlm_terms + the scoring launch + k_dlm_decide), whose differences are the two small
launches.

    python tools/dense64_landmarks_bench.py [--n 10003] [--iters 9] [--warmup 2] [--out profiles/r17/dense64_landmarks_bench.txt]
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
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r17", "dense64_landmarks_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    import dense_correct_cases as dc
    import dense_landmark_cases as lc
    import dense_sparse_cases as sp
    from ekf_slam_ml_amd import capi

    def stats(f, wall):
        v = []
        for _ in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            ms = f()
            v.append((time.perf_counter() - t0) * 1e3 if wall else ms)
        v = np.array(v[a.warmup:])
        return float(np.median(v)), float(v.min()), float(v.max())

    N = a.n
    n = (N - 3) // 2
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    j = n * 2 // 3
    sx, sy = lc.reading_of(x, j, (0.002, -0.001))
    d = capi.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = x
    del S
    R = 0.01 * np.eye(2)
    cols, Hc, _, nu = sp.candidate_terms(x, sx, sy)
    c, h5, _, _, wrapped = sp.slam_terms(x[:3], x, j, sx, sy)
    far = (300.0, -250.0)

    def reading_a():
        return d.associate_landmarks([(sx, sy)], n, n, deferred=True)[3]

    def reading_b():
        d.state_block(0, 3 + 2 * n)
        d.score_sparse(cols, Hc, R, nu)
        d.state_block(0, 3 + 2 * n)
        d.correct_sparse_deferred(c, h5, R, wrapped)
        th = float(d.state_block(0, 1)[0])
        d.set_state_block(0, np.array([dc.normalize_angle(th)]))

    lines = [f"# python tools/dense64_landmarks_bench.py   (MI355X, N = {N}, known = n_max = {n}, medians of {a.iters} after "
             f"{a.warmup}, one process, one handle)"]
    known, assoc, _, _ = d.associate_landmarks([(sx, sy)], n, n, deferred=True)
    assert known == n and assoc[0] == j, (known, assoc)
    ta, tb = stats(reading_a, True), stats(reading_b, True)
    lines.append(f"A  associate_landmarks, one reading, DEFERRED, wall clock: median {ta[0]:.4f} ms (min {ta[1]:.4f}, max {ta[2]:.4f})")
    lines.append(f"B  the spelled handle calls of the same reading, arrays prebuilt, wall clock: median {tb[0]:.4f} ms "
                 f"(min {tb[1]:.4f}, max {tb[2]:.4f})")
    lines.append(f"A / B = {ta[0] / tb[0]:.3f}")
    d.flush()
    e_score = stats(lambda: d.score_sparse(cols, Hc, R, nu)[3], False)
    e_lm = stats(lambda: d.score_landmarks(sx, sy)[3], False)
    e_drop = stats(lambda: d.associate_landmarks([far], n, n)[3], False)
    lines.append(f"HIP events: score_sparse(J = {n}) {e_score[0] * 1e3:.1f} us; score_landmarks (k_dlm_terms + it) "
                 f"{e_lm[0] * 1e3:.1f} us; a dropped associate_landmarks reading (+ k_dlm_decide) {e_drop[0] * 1e3:.1f} us")
    lines.append(f"k_dlm_terms + k_dlm_decide by difference: {(e_drop[0] - e_score[0]) * 1e3:.1f} us next to the scoring "
                 f"launch's {e_score[0] * 1e3:.1f} us")
    d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
