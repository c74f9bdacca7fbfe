"""Dense F Sigma F^T + Q in fp64 (ekf_dense64_*) on the GPU box, N = 10003 by default.

Prints: the HIP-event time of >= 9 timed propagations after >= 2 untimed ones (median, min), the algorithmic rate 4 N^3 / t
and the rate including the zero padding (4 ld^3 / t), the share of the sustained rate of the instruction the kernel uses
(v_mfma_f64_16x16x4_f64 issued back to back: --ceiling-tf, measured by tools/micro/dense64_tile_ab.hip); in the same process, for comparison only, torch.matmul in
float64 on the same device and shapes (the vendor library), and the per-block error (tests/parity.py::cov_err) of the fp32
handle and of the fp64 handle against numpy fp64 on SLAM-shaped inputs at n = 200 and 1000.

    python tools/dense64_bench.py [--n 10003] [--iters 9] [--warmup 2] [--ceiling-tf TF] [--no-torch] [--no-precision]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_F64_CEILING_TF = 77.17   # profiles/r05/dense64_tile_ab.txt: v_mfma_f64_16x16x4_f64 back to back, 16 accumulators


def slam_inputs(n, rng, eps=0.05):
    """A SLAM-shaped covariance (pose block ~1e-4, landmark variances ~100 with correlations, small cross terms), a dense
    F = I + eps G / sqrt(N) and the motion noise on the pose block."""
    import numpy as np
    N = 3 + 2 * n
    S = np.zeros((N, N))
    P = rng.normal(size=(3, 3)) * 3e-5
    S[:3, :3] = P @ P.T + np.eye(3) * 1e-4
    L = rng.normal(size=(2 * n, max(2 * n // 4, 1)))
    S[3:, 3:] = 100.0 * (0.5 * np.eye(2 * n) + 0.5 * L @ L.T / L.shape[1])
    X = rng.normal(size=(3, 2 * n)) * 1e-3
    S[:3, 3:], S[3:, :3] = X, X.T
    F = np.eye(N) + eps * rng.normal(size=(N, N)) / np.sqrt(N)
    Q = np.zeros((N, N))
    Q[0, 0] = Q[1, 1] = Q[2, 2] = 1e-4
    return F, S, Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003, help="matrix size N")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ceiling-tf", type=float, default=MFMA_F64_CEILING_TF,
                    help="sustained v_mfma_f64_16x16x4_f64 rate the share is taken against")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-precision", action="store_true")
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed propagations after 2 untimed ones"
    torch = None
    if not a.no_torch:
        import torch   # before capi: one HIP runtime in the process (capi.load)
    import numpy as np
    from ekf_slam_ml_amd import capi
    from parity import cov_err

    N, ld = a.n, (a.n + 127) // 128 * 128
    rng = np.random.default_rng(4)
    t0 = time.time()
    F = np.eye(N) + rng.standard_normal((N, N)) * (0.05 / np.sqrt(N))
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    Q = np.zeros((N, N)); Q[0, 0] = Q[1, 1] = Q[2, 2] = 1e-4
    print(f"host inputs {time.time() - t0:.1f} s", flush=True)

    d = capi.DensePropagator64(N)
    info = d.launch_info()
    d.set(F, S, Q)
    d.propagate(1)
    rows = np.sort(rng.choice(N, size=8, replace=False))
    want = (F[rows] @ S) @ F.T + Q[rows]
    err = np.abs(d.sigma[rows] - want).max() / np.abs(want).max()
    print(f"fp64 spot check (8 rows against numpy fp64): rel err {err:.2e}", flush=True)
    d.set(Sigma=S)
    for _ in range(a.warmup):
        d.propagate(1)
    ms = np.array([d.propagate(1) for _ in range(a.iters)])
    med, mn = float(np.median(ms)), float(ms.min())
    tf = 4.0 * N ** 3 / (med * 1e-3) / 1e12
    tf_pad = 4.0 * ld ** 3 / (med * 1e-3) / 1e12
    print(f"dense64 N={N} ld={ld} {info}: median {med:.2f} ms, min {mn:.2f} ms per propagation over {a.iters} "
          f"(after {a.warmup} untimed); {tf:.2f} TF algorithmic (4 N^3), {tf_pad:.2f} TF incl. padding (4 ld^3); "
          f"{tf / a.ceiling_tf:.3f} of the {a.ceiling_tf:.2f} TF v_mfma_f64_16x16x4_f64 sustains "
          f"(min: {4.0 * N ** 3 / (mn * 1e-3) / 1e12 / a.ceiling_tf:.3f})", flush=True)
    print("  all times [ms]: " + " ".join(f"{x:.2f}" for x in ms), flush=True)
    d.close()

    if torch is not None:
        dev = torch.device("cuda:0")
        tF = torch.from_numpy(F).to(dev)
        tS = torch.from_numpy(S).to(dev)
        tQ = torch.from_numpy(Q).to(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tt = []
        for it in range(a.warmup + a.iters):
            e0.record()
            out = torch.matmul(torch.matmul(tF, tS), tF.T) + tQ
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                tt.append(e0.elapsed_time(e1))
        tt = np.array(tt)
        tmed = float(np.median(tt))
        terr = np.abs(out[torch.from_numpy(rows).to(dev)].cpu().numpy() - want).max() / np.abs(want).max()
        print(f"torch.matmul float64 (vendor library, same device, same shapes; F S F^T + Q): median {tmed:.2f} ms, "
              f"min {tt.min():.2f} ms = {4.0 * N ** 3 / (tmed * 1e-3) / 1e12:.2f} TF; dense64 / torch time "
              f"{med / tmed:.3f}; torch spot-check rel err {terr:.2e}", flush=True)
        del tF, tS, tQ, out
        torch.cuda.empty_cache()

    if not a.no_precision:
        print("per-block error (cov_err) against numpy fp64, SLAM-shaped inputs (one propagation, then 5):")
        for n in (200, 1000):
            Fs, Ss, Qs = slam_inputs(n, np.random.default_rng(n))
            Nn = Fs.shape[0]
            ref1 = Fs @ Ss @ Fs.T + Qs
            ref5 = Ss
            for _ in range(5):
                ref5 = Fs @ ref5 @ Fs.T + Qs
            for name, cls, dt in (("fp32", capi.DensePropagator, np.float32), ("fp64", capi.DensePropagator64, np.float64)):
                h = cls(Nn)
                h.set(Fs.astype(dt), Ss.astype(dt), Qs.astype(dt))
                h.propagate(1)
                e1_ = cov_err(h.sigma.astype(np.float64), ref1)
                h.propagate(4)
                e5 = cov_err(h.sigma.astype(np.float64), ref5)
                h.close()
                print(f"  n={n} N={Nn} {name}: x1 max {max(e1_.values()):.2e} "
                      + " ".join(f"{k} {v:.1e}" for k, v in e1_.items())
                      + f" | x5 max {max(e5.values()):.2e}", flush=True)


if __name__ == "__main__":
    main()
