"""Landmark (re)initialisation and block readout of the dense fp64 handle (ekf_dense64_init_block,
ekf_dense64_get_sigma_block) on the GPU box: the twin of tools/dense64_block_bench.py and tools/dense64_sparse_bench.py.

For N in {2003, 10003}, HIP-event medians of >= 9 timed calls after >= 2 untimed ones, everything in the same process on
the same handle:
  - init_block at (r, s) = (2, 0), (2, 3), (16, 16), (64, 64), with the bytes the call touches (16 (r + s) N read and
    16 r N written, nothing read at s = 0) at 6.3 TB/s beside it;
  - propagate_block of the same r and correct_sparse(m = 2, s = 5);
  - the dense ekf_dense64_propagate with the embedded F (identity, F[b, b] = 0, F[b, cols] = G) at --dense-n only: it needs
    an N x N upload of F and Q and two N^3 products;
  - the torch float64 spelling on the same device, with index_select for the gathers:
        rows = G @ S.index_select(0, c);  colsv = S.index_select(1, c) @ G.T;  corner = G @ S[c][:, c] @ G.T + W
        S[b, :] = rows;  S[:, b] = colsv;  S[b, b] = corner
  - sigma_block of the 3 x 3 pose block against get_sigma (host wall time of the whole call: both end in a copy).

    python tools/dense64_init_bench.py [--n 2003 10003] [--dense-n 2003] [--iters 9] [--warmup 2] [--no-torch]
                                       [--out profiles/r11/dense64_init_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBS = 6.3
SHAPES = [(2, 0), (2, 3), (16, 16), (64, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2003, 10003])
    ap.add_argument("--dense-n", type=int, default=2003)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "dense64_init_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed calls after 2 untimed ones"
    torch = None
    if not a.no_torch:
        import torch   # before capi: one HIP runtime in the process (capi.load)
    import numpy as np
    from ekf_slam_ml_amd import capi

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def median(f):
        ms = [f() for _ in range(a.warmup + a.iters)][a.warmup:]
        return float(np.median(ms)), float(min(ms))

    def wall(f):
        def timed():
            t0 = time.perf_counter()
            f()
            return (time.perf_counter() - t0) * 1e3
        return median(timed)

    say(f"# tools/dense64_init_bench.py: HIP-event medians of {a.iters} after {a.warmup} in one process")
    for N in a.n:
        rng = np.random.default_rng(N)
        A = rng.standard_normal((N, 64))
        S = A @ A.T / 64 + np.eye(N)
        S += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))
        del A
        d = capi.DensePropagator64(N)
        d.set(Sigma=S)
        d.state = rng.standard_normal(N)
        if torch is not None:
            dev = torch.device("cuda:0")
            tS = torch.from_numpy(S).to(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c5 = np.array([0, 1, 2, 3 + 2 * 617, 4 + 2 * 617], dtype=np.int32)
        H5, R5 = rng.standard_normal((2, 5)), 0.01 * np.eye(2)
        cmed, cmin = median(lambda: d.correct_sparse(c5, H5, R5)[1])
        say(f"N={N} correct_sparse m=2 s=5: median {cmed * 1e3:.1f} us, min {cmin * 1e3:.1f} us")
        for r, s in SHAPES:
            first = ((N - r) // 2) | 1
            free = np.array([i for i in range(N) if not first <= i < first + r])
            cols = None
            if s:
                cols = np.ascontiguousarray(np.concatenate([[0, 1, 2], rng.choice(free[3:], size=s - 3, replace=False)]),
                                            dtype=np.int32)
            G = rng.standard_normal((r, s)) / np.sqrt(s) if s else None
            W = 0.01 * np.eye(r)
            imed, imin = median(lambda: d.init_block(first, G, cols, W))
            bmed, bmin = median(lambda: d.propagate_block(first, np.eye(r), W))
            nbytes = 16.0 * (r + s) * N + 16.0 * r * N if s else 16.0 * r * N
            floor_us = nbytes / (ACHIEVABLE_TBS * 1e12) * 1e6
            line = (f"N={N} init_block r={r} s={s}: median {imed * 1e3:.1f} us, min {imin * 1e3:.1f} us, 1 launch | "
                    f"{nbytes / 1e6:.2f} MB at {ACHIEVABLE_TBS} TB/s = {floor_us:.2f} us -> {imed * 1e3 / floor_us:.1f} x that | "
                    f"propagate_block r={r} median {bmed * 1e3:.1f} us = {imed / bmed:.2f} x | correct_sparse(2, 5) is "
                    f"{cmed / imed:.1f} x init_block")
            if N == a.dense_n:
                F, Q = np.eye(N), np.zeros((N, N))
                F[first:first + r, first:first + r] = 0.0
                if s:
                    F[first:first + r, cols] = G
                Q[first:first + r, first:first + r] = W
                d.set(F=F, Q=Q)
                dmed, dmin = median(lambda: d.propagate(1))
                line += (f" | dense propagate with the embedded F median {dmed:.3f} ms = {dmed / imed:.0f} x, plus "
                         f"{2 * 8.0 * N * N / 1e6:.0f} MB of F and Q uploaded")
                del F, Q
                d.set(Sigma=S)
            if torch is not None:
                tb = torch.arange(first, first + r, device=dev)
                tW = torch.from_numpy(W).to(dev)
                if s:
                    tc = torch.from_numpy(cols.astype(np.int64)).to(dev)
                    tG = torch.from_numpy(G).to(dev)

                def one_torch():
                    e0.record()
                    if s:
                        rows = tG @ tS.index_select(0, tc)
                        colsv = tS.index_select(1, tc) @ tG.T
                        corner = tG @ tS.index_select(0, tc).index_select(1, tc) @ tG.T + tW
                    else:
                        rows = torch.zeros((r, N), dtype=torch.float64, device=dev)
                        colsv, corner = rows.T, tW
                    tS[first:first + r, :] = rows
                    tS[:, first:first + r] = colsv
                    tS.index_put_((tb[:, None], tb[None, :]), corner)
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1)
                tmed, tmin = median(one_torch)
                line += f" | torch float64 median {tmed * 1e3:.1f} us, min {tmin * 1e3:.1f} us = {tmed / imed:.1f} x"
            say(line)
        pose = np.arange(3)
        rmed, rmin = wall(lambda: d.sigma_block(pose, pose))
        gmed, gmin = wall(lambda: d.sigma)
        say(f"N={N} readout: sigma_block of the 3 x 3 pose block median {rmed * 1e3:.1f} us (host wall time of the call), "
            f"get_sigma ({8.0 * N * N / 1e6:.0f} MB) median {gmed:.2f} ms = {gmed / rmed:.0f} x")
        smed, _ = wall(lambda: d.state_block(0, 1))
        fmed, _ = wall(lambda: d.state)
        say(f"N={N} state: state_block of one double median {smed * 1e3:.1f} us, get_state median {fmed * 1e3:.1f} us "
            f"(host wall time)")
        d.close()
        if torch is not None:
            del tS
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
