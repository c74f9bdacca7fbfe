"""The reference's prediction() and measurement() on the dense fp64 handle (ekf_dense64_predict_landmarks,
ekf_dense64_measure_landmarks) on the GPU box: after tools/dense64_landmarks_bench.py.

At N = 10003 with 5000 known landmarks, everything in one process on one handle, medians of >= 9 after >= 2 untimed:
  P  one prediction: the spelled tick (get_state_block of the heading + the host model + propagate_block with its three
     uploads) against predict_landmarks, wall clock and HIP-event time (profiles/r09/dense64_block_bench.txt has the parent's
     propagate_block(r = 3) event time at this N: 6.6 us);
  M  one measurement() call with V = 2 and V = 8 visible landmarks, eager and deferred: measure_landmarks against the same
     corrections spelled with score_landmarks(count = 1, want_terms) + correct_sparse[_deferred] + the heading read / write,
     wall clock and summed HIP-event time; the pending rows are flushed outside the timed region before every repetition.

    python tools/dense64_model_bench.py [--n 10003] [--iters 9] [--warmup 2] [--out profiles/r18/dense64_model_bench.txt]
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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r18", "dense64_model_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    import dense_correct_cases as dc
    import dense_landmark_cases as lc
    import dense_model_cases as mc
    import dense_sparse_cases as sp
    from ekf_slam_ml_amd import capi

    def stats(f, before=None):
        """f() -> HIP-event ms; -> (wall median, wall min, wall max, event median), all in ms"""
        wall, ev = [], []
        for _ in range(a.warmup + a.iters):
            if before:
                before()
            t0 = time.perf_counter()
            ms = f()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(ms)
        wall, ev = np.array(wall[a.warmup:]), np.array(ev[a.warmup:])
        return float(np.median(wall)), float(wall.min()), float(wall.max()), float(np.median(ev))

    N = a.n
    n = (N - 3) // 2
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    d = capi.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = x
    del S
    R = 0.01 * np.eye(2)
    z = np.array([lc.reading_of(x, i, (0.002, -0.001)) for i in range(n)])
    dth, dx = 0.05, 0.02
    lines = [f"# python tools/dense64_model_bench.py   (MI355X, N = {N}, {n} known landmarks, medians of {a.iters} after "
             f"{a.warmup}, one process, one handle)"]

    def predict_spelled():
        th = d.state_block(0, 1)[0]
        Fr, Qr, upd = mc.np_predict_terms(th, dth, dx)
        return d.propagate_block(0, Fr, Qr, upd)

    ps, pd = stats(predict_spelled), stats(lambda: d.predict_landmarks(dth, dx))
    lines.append(f"P  spelled (state_block + host model + propagate_block): wall median {ps[0]:.4f} ms (min {ps[1]:.4f}, max "
                 f"{ps[2]:.4f}), HIP events {ps[3] * 1e3:.1f} us")
    lines.append(f"P  predict_landmarks: wall median {pd[0]:.4f} ms (min {pd[1]:.4f}, max {pd[2]:.4f}), HIP events "
                 f"{pd[3] * 1e3:.1f} us (k_dmd_predict + the launch of propagate_block(r = 3), 6.6 us in profiles/r09); "
                 f"wall ratio {pd[0] / ps[0]:.3f}")

    for V in (2, 8):
        vis = np.zeros(n, dtype=np.uint8)
        seen = np.linspace(0, n - 1, V).astype(int)
        vis[seen] = 1
        for deferred in (False, True):
            correct = d.correct_sparse_deferred if deferred else d.correct_sparse

            def measure_spelled():
                total = 0.0
                for i in seen:
                    _, _, _, ms, (cols, Hc, nu) = d.score_landmarks(z[i, 0], z[i, 1], first_lm=int(i), count=1, want_terms=True)
                    total += ms
                    total += correct(cols[0], Hc[0], R, np.array([nu[0, 0], dc.normalize_angle(float(nu[0, 1]))]))[1]
                    lc.wrap_heading_always(d)
                return total

            ms_, md = stats(measure_spelled, d.flush), stats(lambda: d.measure_landmarks(z, vis, True, deferred)[2], d.flush)
            kind = "deferred" if deferred else "eager"
            lines.append(f"M  V = {V}, {kind}: spelled wall median {ms_[0]:.4f} ms (min {ms_[1]:.4f}, max {ms_[2]:.4f}), HIP "
                         f"events {ms_[3]:.4f} ms | measure_landmarks wall median {md[0]:.4f} ms (min {md[1]:.4f}, max "
                         f"{md[2]:.4f}), HIP events {md[3]:.4f} ms | wall ratio {md[0] / ms_[0]:.3f}")
    d.flush()
    d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
