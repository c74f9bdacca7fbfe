"""The exchange of two blocks of the dense fp64 handle (ekf_dense64_swap_blocks) on the GPU box: after
tools/dense64_live_bench.py.

At N = 10003 with a decoupled tail, HIP-event medians of >= 9 timed repetitions after >= 2 untimed ones, everything in the
same process on the same handle, for live = Na in {2003, 10003} and r in {2, 16, 64}:
  - swap_blocks(3, Na - r, r) flush-first with nothing pending (one launch), with the time of its 64 r Na bytes at
    6.3 TB/s beside it;
  - the same carried through p = 16 pending rows (two launches, nothing flushed);
and next to them, per live width, init_block(r = 2, s = 3) and correct_sparse(2, 5).

    python tools/dense64_swap_bench.py [--n 10003] [--iters 9] [--warmup 2] [--live 2003,10003]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBS = 6.3
LIVE = [2003, 10003]
SIZES = [2, 16, 64]
PENDING = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--live", type=str, default="", help="comma-separated live dimensions instead of 2003,10003")
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    from ekf_slam_ml_amd import capi

    def stats(f):
        v = np.array([f() for _ in range(a.warmup + a.iters)][a.warmup:])
        return float(np.median(v)), float(v.min()), float(v.max())

    N = a.n
    rng = np.random.default_rng(N)
    widths = [int(v) for v in a.live.split(",")] if a.live else [n for n in LIVE if n <= N]
    low = min(widths)
    A = rng.standard_normal((low, 64))
    S = np.zeros((N, N))
    S[:low, :low] = A @ A.T / 64 + np.eye(low)                      # every correction below lists the first `low` states
    S[np.arange(low, N), np.arange(low, N)] = 100.0                 # the reference's prior: a decoupled tail at every Na
    d = capi.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = rng.standard_normal(N)
    del S
    fill = [(np.array([0, 1, 2, 3 + 2 * i, 4 + 2 * i], dtype=np.int32), rng.standard_normal((2, 5)), 0.01 * np.eye(2),
             0.1 * rng.standard_normal(2)) for i in rng.choice((low - 3) // 2, size=PENDING // 2 + 1, replace=False)]
    G, W = rng.standard_normal((2, 3)), 0.01 * np.eye(2)

    for Na in widths:
        d.live = Na
        d.carry = False
        tag = f"N={N} live={Na}"
        for r in SIZES:
            bytes_us = 64.0 * r * Na / (ACHIEVABLE_TBS * 1e12) * 1e6
            med, lo, hi = stats(lambda: d.swap_blocks(3, Na - r, r))
            print(f"{tag} swap_blocks(r = {r}) nothing pending: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max "
                  f"{hi * 1e3:.1f}; 64 r Na bytes at {ACHIEVABLE_TBS} TB/s = {bytes_us:.2f} us)", flush=True)
        d.carry = True
        for c, h, R, v in fill[:PENDING // 2]:
            d.correct_sparse_deferred(c, h, R, v)
        assert d.pending == PENDING
        for r in SIZES:
            med, lo, hi = stats(lambda: d.swap_blocks(3, Na - r, r))
            assert d.pending == PENDING
            print(f"{tag} swap_blocks(r = {r}) carried, p = {PENDING}: median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max "
                  f"{hi * 1e3:.1f})", flush=True)
        d.flush()
        d.carry = False
        med, lo, hi = stats(lambda: d.init_block(low - 2, G=G, cols=[0, 1, 2], W=W))
        print(f"{tag} init_block(r = 2, s = 3): median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
        med, lo, hi = stats(lambda: d.correct_sparse(*fill[PENDING // 2])[1])
        print(f"{tag} correct_sparse(2, 5): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})", flush=True)
    d.close()


if __name__ == "__main__":
    main()
