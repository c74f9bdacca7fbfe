"""Deferred sparse corrections (ekf_dense64_correct_sparse_deferred, ekf_dense64_flush) on the GPU box: the twin of
tools/dense64_sparse_bench.py.

For N in {2003, 10003}, HIP-event medians of >= 9 timed ticks after >= 2 untimed ones, everything in the same process on
the same handle (Sigma as the previous tick left it: the times do not depend on the values):
  - a tick of V in {2, 8, 32} corrections of (m, s) = (2, 5), distinct landmarks: eager (V x correct_sparse) against
    deferred (V x correct_sparse_deferred + one flush), with the time of 16 N^2 bytes at 6.3 TB/s beside it;
  - every deferred call's time as the pending rows p grow, and the flush at p = 2 V;
  - score_sparse over the full map (J = (N - 3) / 2, m = 2, s = 5) with 0, 16 and 62 rows pending.

    python tools/dense64_deferred_bench.py [--n 2003 10003] [--iters 9] [--warmup 2]
    rocprofv3 --kernel-trace --stats -- python tools/dense64_deferred_bench.py --trace-tick
        (one eager and one deferred tick of V = 8 at N = 10003, five times each: the per-kernel split of both)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBS = 6.3
TICKS = [2, 8, 32]
PENDING = [0, 16, 62]


def operands(N, V, rng):
    import numpy as np
    picks = rng.choice((N - 3) // 2, size=V, replace=False)
    return [(np.array([0, 1, 2, 3 + 2 * i, 4 + 2 * i], dtype=np.int32), rng.standard_normal((2, 5)), 0.01 * np.eye(2),
             0.1 * rng.standard_normal(2)) for i in picks]


def sigma(N, rng):
    import numpy as np
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    S += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))
    return S


def trace_tick(N=10003, V=8, ticks=5):
    """what a kernel trace needs and nothing else: no timing"""
    import numpy as np
    from ekf_slam_ml_amd import capi
    rng = np.random.default_rng(N)
    d = capi.DensePropagator64(N)
    d.set(Sigma=sigma(N, rng))
    tick = operands(N, V, rng)
    for _ in range(ticks):
        for c, h, R, nu in tick:
            d.correct_sparse(c, h, R, nu)
    for _ in range(ticks):
        for c, h, R, nu in tick:
            d.correct_sparse_deferred(c, h, R, nu)
        d.flush()
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2003, 10003])
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-tick", action="store_true")
    a = ap.parse_args()
    if a.trace_tick:
        return trace_tick()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed ticks after 2 untimed ones"
    import numpy as np
    from ekf_slam_ml_amd import capi

    def medians(f):
        rows = np.array([f() for _ in range(a.warmup + a.iters)][a.warmup:])
        return np.median(rows, axis=0)

    for N in a.n:
        rng = np.random.default_rng(N)
        d = capi.DensePropagator64(N)
        d.set(Sigma=sigma(N, rng))
        d.state = rng.standard_normal(N)
        floor_ms = 16.0 * N * N / (ACHIEVABLE_TBS * 1e12) * 1e3
        for V in TICKS:
            tick = operands(N, V, rng)
            eager = medians(lambda: [d.correct_sparse(c, h, R, nu)[1] for c, h, R, nu in tick])
            defer = medians(lambda: [d.correct_sparse_deferred(c, h, R, nu)[1] for c, h, R, nu in tick] + [d.flush()])
            te, td = float(eager.sum()), float(defer.sum())
            print(f"N={N} V={V} x (2, 5): eager {te:.4f} ms ({te / V:.4f} per correction) | deferred {td:.4f} ms = "
                  f"{V} calls {float(defer[:-1].sum()):.4f} ms + flush at p = {2 * V} {float(defer[-1]):.4f} ms | "
                  f"deferred / eager = {td / te:.3f} | 16 N^2 at {ACHIEVABLE_TBS} TB/s = {floor_ms:.4f} ms: the flush is "
                  f"{float(defer[-1]) / floor_ms:.2f} x that", flush=True)
            print(f"N={N} V={V} deferred calls as p grows (us): " + " ".join(f"{v * 1e3:.1f}" for v in defer[:-1]), flush=True)
        n = (N - 3) // 2
        cols = np.array([[0, 1, 2, 3 + 2 * i, 4 + 2 * i] for i in range(n)], dtype=np.int32)
        Hc, R, nu = rng.standard_normal((n, 2, 5)), 0.01 * np.eye(2), rng.standard_normal((n, 2))
        tick = operands(N, 31, rng)
        for p in PENDING:
            d.flush()
            for c, h, r, v in tick[:p // 2]:
                d.correct_sparse_deferred(c, h, r, v)
            assert d.pending == p
            med = float(medians(lambda: [d.score_sparse(cols, Hc, R, nu)[3]])[0])
            print(f"N={N} score_sparse J={n} m=2 s=5 with {p} rows pending: median {med * 1e3:.1f} us", flush=True)
        d.close()


if __name__ == "__main__":
    main()
