#!/usr/bin/env python3
"""A robot that dwells on a surveyed map: K sparse corrections (m = 2, s = 5) with a block prediction every eighth call,
inside a local region of the dense fp64 handle (ekf_dense64_region_begin .. ekf_dense64_region_end) and full-width on a twin
handle.  Prints the sums of the calls' own HIP-event times, the time per correction, region_end and the break-even count.

    python tools/dense64_region_bench.py [--n 10003] [--na 403] [--corrections 64] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ekf_slam_ml_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--na", type=int, default=403)
    ap.add_argument("--corrections", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, Na, K = a.n, a.na, a.corrections
    rng = np.random.default_rng(27)
    A = rng.standard_normal((N, 64))
    S0 = A @ A.T / 64 + np.eye(N)                                      # coupled everywhere, symmetric
    x0 = rng.normal(size=N)
    ops = []
    for i in range(K):
        lm = 3 + 2 * int(rng.integers(0, (Na - 3) // 2))
        ops.append(("c", np.array([0, 1, 2, lm, lm + 1], dtype=np.int32), rng.normal(size=(2, 5)), 0.5 * np.eye(2), 0.1 * rng.normal(size=2)))
        if i % 8 == 7:
            ops.append(("p", np.eye(3) + 0.01 * rng.normal(size=(3, 3)), 1e-3 * np.eye(3), 0.01 * rng.normal(size=3)))
    d, twin = capi.DensePropagator64(N), capi.DensePropagator64(N)

    def run(h, region):
        h.set(Sigma=S0)
        h.state = x0
        ms = h.region_begin(Na) if region else 0.0
        for op in ops:
            ms += h.correct_sparse(*op[1:])[1] if op[0] == "c" else h.propagate_block(0, op[1], op[2], op[3])
        end = h.region_end()["elapsed_ms"] if region else 0.0
        return ms, end

    run(d, True), run(twin, False)                                     # untimed: allocations, first launches
    inside, end = run(d, True)
    full, _ = run(twin, False)
    per_in, per_full = inside / K, full / K
    lines = [f"N = {N}, Na = {Na}, {K} correct_sparse(2, 5) + propagate_block(3) every eighth call",
             f"  region      {inside + end:9.3f} ms = in-region {inside:.3f} ms ({per_in:.4f} ms per correction) + region_end {end:.3f} ms",
             f"  full width  {full:9.3f} ms ({per_full:.4f} ms per correction)",
             f"  break-even  {end / (per_full - per_in):.1f} corrections" if per_full > per_in else "  break-even  none: the region is not faster per correction",
             f"  region_end on the Sigma_bb product's {2.0 * Na * (N - Na) ** 2:.3g} flop: {2.0 * Na * (N - Na) ** 2 / end / 1e9:.1f} TF (all six launches; the product alone is not timed)",
             f"  state against the twin: {np.abs(d.state - twin.state).max() / np.abs(twin.state).max():.3e}"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    d.close()
    twin.close()


if __name__ == "__main__":
    main()
