"""Pending rows carried across ticks (ekf_dense64_set_carry) on the GPU box: the twin of tools/dense64_deferred_bench.py.

At N = 10003, HIP-event medians of >= 9 timed repetitions after >= 2 untimed ones, everything in the same process on the
same handle (Sigma as the previous repetition left it: the times do not depend on the values):
  - the flush at p in {4, 16, 32, 64} pending rows, with the time of 16 N^2 bytes at 6.3 TB/s beside it;
  - a (2, 5) deferred correction and a 5000-candidate score_sparse with the same p rows pending;
  - propagate_block(0, 3), a correlated init_block(r = 2, s = 3) and the 3 x 3 pose readout, carried at the same p;
  - 16 ticks of propagate_block(0, 3) + V deferred (2, 5) corrections, V in {2, 8}, the policy on and a flush every
    1, 4, 8 and 16 ticks (a cadence whose rows would pass 64 flushes earlier by itself: the count of flushes is printed),
    against the same ticks with the policy off (every propagate_block flushes), per tick.

    python tools/dense64_carry_bench.py [--n 10003] [--iters 9] [--warmup 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBS = 6.3
PENDING = [4, 16, 32, 64]
CADENCE = [1, 4, 8, 16]
TICKS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    from ekf_slam_ml_amd import capi
    from tools.dense64_deferred_bench import operands, sigma

    def medians(f):
        rows = np.array([f() for _ in range(a.warmup + a.iters)][a.warmup:])
        return np.median(rows, axis=0)

    N = a.n
    rng = np.random.default_rng(N)
    d = capi.DensePropagator64(N)
    d.set(Sigma=sigma(N, rng))
    d.state = rng.standard_normal(N)
    d.carry = True
    floor_ms = 16.0 * N * N / (ACHIEVABLE_TBS * 1e12) * 1e3
    n = (N - 3) // 2
    cols = np.array([[0, 1, 2, 3 + 2 * i, 4 + 2 * i] for i in range(n)], dtype=np.int32)
    Hc, R, nu = rng.standard_normal((n, 2, 5)), 0.01 * np.eye(2), rng.standard_normal((n, 2))
    Fr, Qr, dx = np.eye(3) + 0.005 * rng.standard_normal((3, 3)), 1e-4 * np.eye(3), 0.01 * rng.standard_normal(3)
    G, W = rng.standard_normal((2, 3)), 0.01 * np.eye(2)
    pose = np.arange(3)
    fill = operands(N, 33, rng)

    def pend(p):
        d.flush()
        for c, h, r, v in fill[:p // 2]:
            d.correct_sparse_deferred(c, h, r, v)
        assert d.pending == p

    for p in PENDING:
        def flush_at_p():
            pend(p)
            return [d.flush()]
        t_flush = float(medians(flush_at_p)[0])
        print(f"N={N} flush at p = {p}: median {t_flush:.4f} ms ({t_flush / floor_ms:.2f} x 16 N^2 at {ACHIEVABLE_TBS} TB/s = "
              f"{floor_ms:.4f} ms)", flush=True)
        if p < 64:
            def one_more():
                pend(p)
                return [d.correct_sparse_deferred(*fill[32])[1]]
            print(f"N={N} deferred (2, 5) correction with {p} rows pending: median {float(medians(one_more)[0]) * 1e3:.1f} us",
                  flush=True)
        pend(p)
        t_score = float(medians(lambda: [d.score_sparse(cols, Hc, R, nu)[3]])[0])
        t_prop = float(medians(lambda: [d.propagate_block(0, Fr, Qr, dx)])[0])
        t_init = float(medians(lambda: [d.init_block(N - 2, G=G, cols=[0, 1, 2], W=W)])[0])
        assert d.pending == p
        print(f"N={N} with {p} rows pending: score_sparse J={n} {t_score * 1e3:.1f} us | carried propagate_block(0, 3) "
              f"{t_prop * 1e3:.1f} us | carried init_block(r = 2, s = 3) {t_init * 1e3:.1f} us", flush=True)
    d.flush()
    t_prop0 = float(medians(lambda: [d.propagate_block(0, Fr, Qr, dx)])[0])
    t_init0 = float(medians(lambda: [d.init_block(N - 2, G=G, cols=[0, 1, 2], W=W)])[0])
    print(f"N={N} with nothing pending: propagate_block(0, 3) {t_prop0 * 1e3:.1f} us | init_block(r = 2, s = 3) "
          f"{t_init0 * 1e3:.1f} us", flush=True)

    for V in (2, 8):
        ticks = [operands(N, V, rng) for _ in range(TICKS)]
        results = {}
        for every in [0] + CADENCE:                        # 0: the policy off
            flushes = [0]

            def run():
                d.carry = every != 0
                total, flushes[0] = 0.0, 0
                for t, tick in enumerate(ticks):
                    total += d.propagate_block(0, Fr, Qr, dx)
                    for c, h, r, v in tick:
                        before = d.pending
                        total += d.correct_sparse_deferred(c, h, r, v)[1]
                        flushes[0] += d.pending < before + 2          # the capacity forced one
                    if every and (t + 1) % every == 0:
                        total += d.flush()
                        flushes[0] += 1
                total += d.flush()
                return [total]
            results[every] = float(medians(run)[0]) / TICKS
            name = "policy off (propagate_block flushes)" if every == 0 else f"carried, flush every {every}"
            print(f"N={N} V={V}: {name}: {results[every]:.4f} ms per tick"
                  + (f", {flushes[0]} flushes in {TICKS} ticks" if every else ""), flush=True)
        best = min(CADENCE, key=lambda k: results[k])
        print(f"N={N} V={V}: best cadence {best} ({results[best] / results[0]:.3f} of the policy off)", flush=True)
    d.close()


if __name__ == "__main__":
    main()
