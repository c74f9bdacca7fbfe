"""The live dimension of the dense fp64 handle (ekf_dense64_set_live) on the GPU box: after tools/dense64_carry_bench.py.

At N = 10003 with a decoupled tail, HIP-event medians of >= 9 timed repetitions after >= 2 untimed ones, everything in the
same process on the same handle, for live = Na in {403, 2003, 5003, 10003}:
  - correct_sparse(2, 5);
  - the flush at p in {4, 16, 64} pending rows, with the time of 16 Na^2 bytes at 6.3 TB/s beside it;
  - propagate_block(0, 3) and init_block(r = 2, s = 3) with nothing pending;
  - coupling(Na).
The line of live = N is the line to hold against the same calls of the commit before the setting existed (there every
call is the live = N call): run this file there with --baseline, which leaves the setting alone and skips coupling.

    python tools/dense64_live_bench.py [--n 10003] [--iters 9] [--warmup 2] [--live 2003,10003] [--baseline]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBS = 6.3
LIVE = [403, 2003, 5003, 10003]
PENDING = [4, 16, 64]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--live", type=str, default="", help="comma-separated live dimensions instead of 403,2003,5003,10003")
    ap.add_argument("--baseline", action="store_true", help="a library without the setting: live = N only, no coupling")
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    from ekf_slam_ml_amd import capi

    def stats(f):
        v = np.array([f() for _ in range(a.warmup + a.iters)][a.warmup:])
        return float(np.median(v)), float(v.min()), float(v.max())

    N = a.n
    rng = np.random.default_rng(N)
    low = min(LIVE)
    A = rng.standard_normal((low, 64))
    S = np.zeros((N, N))
    S[:low, :low] = A @ A.T / 64 + np.eye(low)                      # every correction below lists the first `low` states
    S[np.arange(low, N), np.arange(low, N)] = 100.0                 # the reference's prior: a decoupled tail at every Na
    d = capi.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = rng.standard_normal(N)
    del S
    fill = [(np.array([0, 1, 2, 3 + 2 * i, 4 + 2 * i], dtype=np.int32), rng.standard_normal((2, 5)), 0.01 * np.eye(2),
             0.1 * rng.standard_normal(2)) for i in rng.choice((low - 3) // 2, size=33, replace=False)]
    Fr, Qr, dx = np.eye(3) + 0.005 * rng.standard_normal((3, 3)), 1e-4 * np.eye(3), 0.01 * rng.standard_normal(3)
    G, W = rng.standard_normal((2, 3)), 0.01 * np.eye(2)

    def flush_at(p):
        for c, h, r, v in fill[:p // 2]:
            d.correct_sparse_deferred(c, h, r, v)
        assert d.pending == p
        return d.flush()

    widths = [int(v) for v in a.live.split(",")] if a.live else LIVE
    for Na in ([N] if a.baseline else [n for n in widths if n <= N]):
        if not a.baseline:
            d.live = Na
        tag = f"N={N} live={Na}"
        floor_ms = 16.0 * Na * Na / (ACHIEVABLE_TBS * 1e12) * 1e3
        med, lo, hi = stats(lambda: d.correct_sparse(*fill[32])[1])
        print(f"{tag} correct_sparse(2, 5): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})", flush=True)
        for p in PENDING:
            med, lo, hi = stats(lambda: flush_at(p))
            print(f"{tag} flush at p = {p}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}; {med / floor_ms:.2f} x 16 Na^2 "
                  f"bytes at {ACHIEVABLE_TBS} TB/s = {floor_ms:.4f} ms)", flush=True)
        med, lo, hi = stats(lambda: d.propagate_block(0, Fr, Qr, dx))
        print(f"{tag} propagate_block(0, 3): median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
        med, lo, hi = stats(lambda: d.init_block(low - 2, G=G, cols=[0, 1, 2], W=W))
        print(f"{tag} init_block(r = 2, s = 3): median {med * 1e3:.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
        if not a.baseline:
            med, lo, hi = stats(lambda: d.coupling(Na)[2])
            bytes_ms = 16.0 * Na * (N - Na) / (ACHIEVABLE_TBS * 1e12) * 1e3
            print(f"{tag} coupling({Na}): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}; 16 Na (N - Na) bytes at "
                  f"{ACHIEVABLE_TBS} TB/s = {bytes_ms:.4f} ms), nonzero {d.coupling(Na)[0]}", flush=True)
    d.close()


if __name__ == "__main__":
    main()
