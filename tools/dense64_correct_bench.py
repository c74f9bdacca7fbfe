"""Dense fp64 measurement update (ekf_dense64_correct) on the GPU box: the twin of tools/dense64_bench.py.

For N in {10003, 2003} and m in {2, 8, 32, 64}: the HIP-event median of >= 9 timed corrections after >= 2 untimed ones,
the declared 24 N^2 bytes over that time as a fraction of 8 TB/s, 6 m N^2 / t in TF, and -- in the same process, on the
same device, as the vendor-library comparison -- the same update spelled with torch float64:
    T = H @ S; U = S @ H.T; K = U @ inv(T @ H.T + R); S.addmm_(K, T, alpha=-1)
Sigma is reloaded before every correction (repeated corrections with one H would shrink H Sigma H^T towards zero), the
copy is outside the timed region on both sides.

    python tools/dense64_correct_bench.py [--n 10003 2003] [--m 2 8 32 64] [--iters 9] [--warmup 2] [--no-torch]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10003, 2003])
    ap.add_argument("--m", type=int, nargs="+", default=[2, 8, 32, 64])
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed corrections after 2 untimed ones"
    torch = None
    if not a.no_torch:
        import torch   # before capi: one HIP runtime in the process (capi.load)
    import numpy as np
    from ekf_slam_ml_amd import capi

    for N in a.n:
        rng = np.random.default_rng(N)
        A = rng.standard_normal((N, 64))
        S = A @ A.T / 64 + np.eye(N)
        x = rng.standard_normal(N)
        d = capi.DensePropagator64(N)
        if torch is not None:
            dev = torch.device("cuda:0")
            tS0 = torch.from_numpy(S).to(dev)
            tS = torch.empty_like(tS0)
        for m in a.m:
            H = rng.standard_normal((m, N))
            R = 0.01 * np.eye(m)
            nu = rng.standard_normal(m)
            ms = []
            for it in range(a.warmup + a.iters):
                d.set(Sigma=S)
                d.state = x
                t = d.correct(H, R, nu)[1]
                if it >= a.warmup:
                    ms.append(t)
            ms = np.array(ms)
            med = float(np.median(ms))
            rows = np.sort(rng.choice(N, size=8, replace=False))
            T = H @ S
            K = (S @ H.T) @ np.linalg.inv(T @ H.T + R)
            want = S[rows] - K[rows] @ T
            err = np.abs(d.sigma[rows] - want).max() / np.abs(want).max()
            line = (f"N={N} m={m}: median {med:.3f} ms, min {ms.min():.3f} ms over {a.iters} (after {a.warmup} untimed); "
                    f"24 N^2 / t = {24.0 * N * N / (med * 1e-3) / 1e12:.2f} TB/s = "
                    f"{24.0 * N * N / (med * 1e-3) / 1e12 / HBM_TBS:.3f} of {HBM_TBS:.0f} TB/s; "
                    f"6 m N^2 / t = {6.0 * m * N * N / (med * 1e-3) / 1e12:.2f} TF; spot check (8 rows) rel err {err:.1e}")
            if torch is not None:
                tH = torch.from_numpy(H).to(dev)
                tR = torch.from_numpy(R).to(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                tt = []
                for it in range(a.warmup + a.iters):
                    tS.copy_(tS0)
                    e0.record()
                    tT = tH @ tS
                    tU = tS @ tH.T
                    tK = tU @ torch.linalg.inv(tT @ tH.T + tR)
                    tS.addmm_(tK, tT, alpha=-1)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        tt.append(e0.elapsed_time(e1))
                tmed = float(np.median(tt))
                terr = np.abs(tS[torch.from_numpy(rows).to(dev)].cpu().numpy() - want).max() / np.abs(want).max()
                line += (f" | torch float64 spelling: median {tmed:.3f} ms, min {min(tt):.3f} ms (rel err {terr:.1e}); "
                         f"correct / torch time {med / tmed:.3f}")
            print(line, flush=True)
        d.close()
        if torch is not None:
            del tS0, tS
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
