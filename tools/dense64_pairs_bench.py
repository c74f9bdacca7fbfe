#!/usr/bin/env python3
"""ekf_dense64_score_landmark_pairs on the GPU: HIP-event time of the all-pairs scan against map size, next to
correct_sparse(m = 2, s = 5) on the same handle (which reads and writes 16 N^2 bytes where the scan reads 8 N^2), and the
merge against its spelled sequence.  Medians of 9 after 2 untimed calls.

    python tools/dense64_pairs_bench.py [--sizes 1000,2500,5000] > profiles/r21/dense64_pairs_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ekf_slam_ml_amd import capi  # noqa: E402
import dense_pairs_cases as pc  # noqa: E402
import dense_sparse_cases as sp  # noqa: E402


def median(f, iters=9, warmup=2):
    return float(np.median([f() for _ in range(warmup + iters)][warmup:]))


def wall(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,2500,5000")
    args = ap.parse_args()
    rng = np.random.default_rng(8)
    print("# n_lm  N  scan_ms  scan_wall_ms  TB/s(8 N^2)  of_8TB/s  correct_sparse(2,5)_ms  ratio")
    for n in [int(v) for v in args.sizes.split(",")]:
        N = 3 + 2 * n
        A = rng.standard_normal((N, 64))
        Sigma = A @ A.T / 64 + np.eye(N)
        Sigma += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))
        x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
        d = capi.DensePropagator64(N)
        d.set(Sigma=Sigma)
        d.state = x
        del Sigma, A
        t_scan = median(lambda: d.landmark_pairs(n, 0.5, 1.0)[4])
        w_scan = median(lambda: wall(lambda: d.landmark_pairs(n, 0.5, 1.0)))
        cols, Hc, R, nu = sp.slam_terms(x[:3], x, n // 2, 0.7, -0.4)[:4]
        t_corr = median(lambda: d.correct_sparse(cols, Hc, R, nu)[1])
        rate = 8.0 * N * N / (t_scan * 1e-3) / 1e12
        print(f"{n:6d} {N:6d} {t_scan:8.4f} {w_scan:8.4f} {rate:6.2f} {rate / 8.0:5.2f} {t_corr:8.4f} {t_corr / t_scan:5.2f}")
        if n == max(int(v) for v in args.sizes.split(",")):
            known = n
            t_merge = []
            t_spelled = []
            for k in range(5):
                a, b = 10 + k, n // 2 + k
                t_merge.append(wall(lambda: d.merge_landmarks(a, b, 0.5, known)))
                known -= 1
                a, b = 40 + k, n // 3 + k

                def spelled():
                    c4, h4, r4, v4 = pc.merge_operands(d.state, a, b, 0.5)
                    d.correct_sparse(c4, h4, r4, v4)
                    d.swap_blocks(3 + 2 * b, 3 + 2 * (known - 1), 2)
                    d.init_block(3 + 2 * (known - 1), W=100.0 * np.eye(2))
                t_spelled.append(wall(spelled))
                known -= 1
            print(f"# merge_landmarks (eager, hi in mid-map) at N={N}: {np.median(t_merge):.4f} ms of wall clock; the spelled "
                  f"sequence (state read back, correct_sparse, swap_blocks, init_block): {np.median(t_spelled):.4f} ms")
        d.close()


if __name__ == "__main__":
    main()
