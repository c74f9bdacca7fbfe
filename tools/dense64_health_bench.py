#!/usr/bin/env python3
"""ekf_dense64_health and ekf_dense64_symmetrize on the GPU: HIP-event times against the dimension, next to the flush of
two pending rows on the same handle (which reads and writes 16 N^2 bytes).  health reads 8 N^2 bytes; symmetrize reads
8 N^2 and, on a matrix whose every pair differs (set anew before every timed call), writes 8 N^2; on a symmetric matrix it
only reads.  Medians of 9 after 2 untimed calls (5 after 1 where Sigma goes up before each).

    python tools/dense64_health_bench.py [--sizes 2003,5003,10003] > profiles/r23/dense64_health_bench.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ekf_slam_ml_amd import capi  # noqa: E402


def median(f, iters=9, warmup=2):
    return float(np.median([f() for _ in range(warmup + iters)][warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2003,5003,10003")
    args = ap.parse_args()
    rng = np.random.default_rng(8)
    print("# N  flush2_ms  health_ms  TB/s(8 N^2)  health/flush  sym_all_ms  TB/s(16 N^2)  sym_all/flush  sym_clean_ms  "
          "TB/s(8 N^2)  pairs_written")
    for N in [int(v) for v in args.sizes.split(",")]:
        A = rng.standard_normal((N, 64))
        Sigma = A @ A.T / 64 + np.eye(N)
        Sigma += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))   # every pair differs
        d = capi.DensePropagator64(N)
        d.set(Sigma=Sigma)
        d.state = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
        info = d.health_launch_info()
        t_health = median(lambda: d.health()["ms"])
        written = []

        def sym_all():
            d.set(Sigma=Sigma)
            got = d.symmetrize()
            written.append(got["changed"])
            return got["ms"]

        t_all = median(sym_all, iters=5, warmup=1)
        t_clean = median(lambda: d.symmetrize()["ms"])
        j = (N - 3) // 4
        cols, Hc, R, nu = np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j]), rng.standard_normal((2, 5)), np.eye(2), np.zeros(2)

        def flush_two():
            d.correct_sparse_deferred(cols, Hc, R, nu)
            return d.flush()

        t_flush = median(flush_two)
        rep = d.health()
        d.close()
        tb = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12   # noqa: E731
        print(f"{N:6d} {t_flush:8.4f} {t_health:8.4f} {tb(8 * N * N, t_health):6.2f} {t_health / t_flush:5.2f} "
              f"{t_all:8.4f} {tb(16 * N * N, t_all):6.2f} {t_all / t_flush:5.2f} {t_clean:8.4f} {tb(8 * N * N, t_clean):6.2f} "
              f"{written[-1]:d}")
        print(f"#   tile {info['tile']} states, {info['threads']} threads; after the flush: n_asym {rep['n_asym']} "
              f"max_asym {rep['max_asym']:.3e} n_minor {rep['n_minor']} n_diag_bad {rep['n_diag_bad']}")
        del Sigma, A


if __name__ == "__main__":
    main()
