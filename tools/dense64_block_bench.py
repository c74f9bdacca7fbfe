"""Block-structured prediction (ekf_dense64_propagate_block) on the GPU box: the twin of tools/dense64_correct_bench.py.

For N in {2003, 10003} and r in {3, 16, 64} (block at an odd offset): the HIP-event median of >= 9 timed calls after >= 2
untimed ones, and in the same process, on the same handle:
  - ekf_dense64_propagate with the embedded F and Q (the only way to make this prediction without the call),
  - ekf_dense64_correct at m = 2 (once per N; Sigma reloaded before every correction, outside the timed region),
and on the same device the torch float64 spelling of the three slice updates:
    rows = Fr @ S[b, :]; cols = S[:, b] @ Fr.T; corner = (Fr @ S[b, b]) @ Fr.T + Qr; S[b, :] = rows; S[:, b] = cols; S[b, b] = corner
Printed: ms, the ratio to each, the declared 32 r N bytes over the time as a fraction of 8 TB/s, and the launch count (the
call is ONE launch, so at these sizes its time is the floor of one launch more than a stream: read the fraction with it).
Fr is orthogonal, so repeated calls keep Sigma bounded and it is not reloaded between them.

    python tools/dense64_block_bench.py [--n 2003 10003] [--r 3 16 64] [--iters 9] [--warmup 2] [--no-torch]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
LAUNCHES = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2003, 10003])
    ap.add_argument("--r", type=int, nargs="+", default=[3, 16, 64])
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed calls after 2 untimed ones"
    torch = None
    if not a.no_torch:
        import torch   # before capi: one HIP runtime in the process (capi.load)
    import numpy as np
    from ekf_slam_ml_amd import capi

    def median(f):
        ms = [f() for _ in range(a.warmup + a.iters)][a.warmup:]
        return float(np.median(ms)), float(min(ms))

    ok = True
    for N in a.n:
        rng = np.random.default_rng(N)
        A = rng.standard_normal((N, 64))
        S = A @ A.T / 64 + np.eye(N)
        S += 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))
        d = capi.DensePropagator64(N)
        d.state = rng.standard_normal(N)
        H = rng.standard_normal((2, N))
        R = 0.01 * np.eye(2)
        nu = rng.standard_normal(2)

        def one_correct():
            d.set(Sigma=S)
            return d.correct(H, R, nu)[1]
        cmed, cmin = median(one_correct)
        print(f"N={N}: ekf_dense64_correct m=2 median {cmed:.4f} ms, min {cmin:.4f} ms", flush=True)
        if torch is not None:
            dev = torch.device("cuda:0")
            tS = torch.from_numpy(S).to(dev)
        for r in a.r:
            first = ((N - r) // 2) | 1
            b = slice(first, first + r)
            Fr = np.linalg.qr(rng.standard_normal((r, r)))[0]
            Qr = 1e-4 * np.eye(r)
            dx = 1e-3 * rng.standard_normal(r)
            # one call from a fresh Sigma, checked on the block's rows and columns
            d.set(Sigma=S)
            d.propagate_block(first, Fr, Qr, dx)
            got = d.sigma
            wr, wc = Fr @ S[b, :], S[:, b] @ Fr.T
            wr[:, b] = wc[b, :] = (Fr @ S[b, b]) @ Fr.T + Qr
            err = max(np.abs(got[b, :] - wr).max() / np.abs(wr).max(), np.abs(got[:, b] - wc).max() / np.abs(wc).max())
            del got
            bmed, bmin = median(lambda: d.propagate_block(first, Fr, Qr, dx))
            F, Q = np.eye(N), np.zeros((N, N))
            F[b, b], Q[b, b] = Fr, Qr
            d.set(F=F, Sigma=S, Q=Q)
            del F, Q
            pmed, pmin = median(lambda: d.propagate(1))
            byts = 32.0 * r * N
            line = (f"N={N} r={r} first={first}: propagate_block median {bmed * 1e3:.1f} us, min {bmin * 1e3:.1f} us over "
                    f"{a.iters} (after {a.warmup} untimed), {LAUNCHES} launch; 32 r N = {byts / 1e6:.2f} MB -> "
                    f"{byts / (bmed * 1e-3) / 1e12:.3f} TB/s = {byts / (bmed * 1e-3) / 1e12 / HBM_TBS:.4f} of {HBM_TBS:.0f} TB/s; "
                    f"spot check rel err {err:.1e} | dense propagate (embedded F) median {pmed:.3f} ms = {pmed / bmed:.0f} x; "
                    f"correct m=2 {cmed:.4f} ms = {cmed / bmed:.1f} x")
            if N == 10003 and not bmed < cmed:
                ok = False
                line += "  ** NOT below correct(m = 2) **"
            if torch is not None:
                tF, tQ = torch.from_numpy(Fr).to(dev), torch.from_numpy(Qr).to(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def one_torch():
                    e0.record()
                    rows = tF @ tS[b, :]
                    cols = tS[:, b] @ tF.T
                    corner = (tF @ tS[b, b]) @ tF.T + tQ
                    tS[b, :] = rows
                    tS[:, b] = cols
                    tS[b, b] = corner
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1)
                tmed, tmin = median(one_torch)
                line += f" | torch float64 slices median {tmed * 1e3:.1f} us, min {tmin * 1e3:.1f} us = {tmed / bmed:.1f} x"
            print(line, flush=True)
        d.close()
        if torch is not None:
            del tS
            torch.cuda.empty_cache()
    if not ok:
        sys.exit("the block prediction must take less time than correct(m = 2) at N = 10003")


if __name__ == "__main__":
    main()
