"""Batched candidate scoring of the fp64 dense handle (ekf_dense64_score) on the GPU box: the twin of
tools/dense64_correct_bench.py.

For N in {10003, 2003} and (m, J) in {(2, 1), (2, 32), (2, 1024), (8, 8), (8, 256), (64, 1), (64, 32)}: the HIP-event
median of >= 9 timed calls after >= 2 untimed ones, 2 J m N^2 / t in TF, the bytes of Sigma read (8 N^2 per row group
of 64 rows) over that time against 8 TB/s, and in the same process on the same device
  (a) ekf_dense64_correct at the same (N, m) (Sigma reloaded before every correction, outside the timed region) -- a
      call that fits one row group (J m <= 64) does a strict subset of its work, and
  (b) the torch float64 spelling of the same scores: T = Hall @ Sigma, per-candidate blocks of T Hall^T, linalg.inv.

    python tools/dense64_score_bench.py [--n 10003 2003] [--iters 9] [--warmup 2] [--no-torch]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
SHAPES = [(2, 1), (2, 32), (2, 1024), (8, 8), (8, 256), (64, 1), (64, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10003, 2003])
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

    for N in a.n:
        rng = np.random.default_rng(N)
        A = rng.standard_normal((N, 64))
        S = A @ A.T / 64 + np.eye(N)
        x = rng.standard_normal(N)
        d = capi.DensePropagator64(N)
        if torch is not None:
            dev = torch.device("cuda:0")
            tS = torch.from_numpy(S).to(dev)
        correct_ms = {}
        for m, J in SHAPES:
            H = rng.standard_normal((J, m, N))
            R = 0.01 * np.eye(m)
            nu = rng.standard_normal((J, m))
            if m not in correct_ms:
                cm = []
                for it in range(a.warmup + a.iters):
                    d.set(Sigma=S)
                    d.state = x
                    t = d.correct(H[0], R, nu[0])[1]
                    if it >= a.warmup:
                        cm.append(t)
                correct_ms[m] = float(np.median(cm))
            d.set(Sigma=S)
            ms = []
            for it in range(a.warmup + a.iters):
                nis, _, flags, t = d.score(H, R, nu)
                if it >= a.warmup:
                    ms.append(t)
            ms = np.array(ms)
            med = float(np.median(ms))
            pick = np.unique(np.concatenate([[0, J - 1], rng.integers(0, J, size=4)]))
            want = np.array([nu[j] @ np.linalg.inv(H[j] @ S @ H[j].T + R) @ nu[j] for j in pick])
            err = float((np.abs(nis[pick] - want) / np.abs(want)).max())
            groups = -(-J // (64 // m))
            line = (f"N={N} m={m} J={J}: median {med:.3f} ms, min {ms.min():.3f} ms over {a.iters} (after {a.warmup} "
                    f"untimed); 2 J m N^2 / t = {2.0 * J * m * N * N / (med * 1e-3) / 1e12:.2f} TF; Sigma read "
                    f"{groups} x 8 N^2 / t = {groups * 8.0 * N * N / (med * 1e-3) / 1e12:.2f} TB/s = "
                    f"{groups * 8.0 * N * N / (med * 1e-3) / 1e12 / HBM_TBS:.3f} of {HBM_TBS:.0f} TB/s; flagged "
                    f"{int(flags.sum())}; spot check rel err {err:.1e} | correct at (N, m): median {correct_ms[m]:.3f} ms, "
                    f"score / correct {med / correct_ms[m]:.3f}")
            if torch is not None:
                tH = torch.from_numpy(H.reshape(J * m, N)).to(dev)
                tR = torch.from_numpy(R).to(dev)
                tnu = torch.from_numpy(nu).to(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                tt = []
                for it in range(a.warmup + a.iters):
                    e0.record()
                    tT = tH @ tS
                    tSj = torch.bmm(tT.view(J, m, N), tH.view(J, m, N).transpose(1, 2)) + tR
                    tw = torch.linalg.inv(tSj) @ tnu.unsqueeze(2)
                    tn = (tnu.unsqueeze(1) @ tw).reshape(J)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        tt.append(e0.elapsed_time(e1))
                tmed = float(np.median(tt))
                terr = float((np.abs(tn.cpu().numpy()[pick] - want) / np.abs(want)).max())
                line += (f" | torch float64 spelling: median {tmed:.3f} ms, min {min(tt):.3f} ms (rel err {terr:.1e}); "
                         f"score / torch time {med / tmed:.3f}")
                del tH, tT, tSj
            print(line, flush=True)
        d.close()
        if torch is not None:
            del tS
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
