"""Column-sparse measurement update and scoring (ekf_dense64_correct_sparse, ekf_dense64_score_sparse) on the GPU box: the
twin of tools/dense64_block_bench.py.

For N in {2003, 10003}, HIP-event medians of >= 9 timed calls after >= 2 untimed ones, everything in the same process on
the same handle:
  - correct_sparse at (m, s) = (2, 5), (8, 16), (32, 64), (64, 64), each against ekf_dense64_correct with the embedded H
    (Sigma reloaded before every correction, outside the timed region), with the time of the rank-m update's 16 N^2 bytes at
    6.3 TB/s beside it;
  - score_sparse at m = 2, s = 5 for J = 1, 32, 1024 and J = (N - 3) / 2 (the full map), against ekf_dense64_score with the
    embedded H where that call accepts the size (J * m <= 2048);
  - the torch float64 spelling of each on the same device, with index_select for the gathers:
        G = S.index_select(0, c);  T = Hc @ G;  U = S.index_select(1, c) @ Hc.T;  Sm = T.index_select(1, c) @ Hc.T + R
        K = U @ inv(Sm);  x += K @ nu;  S -= K @ T
        (scores)  G = S[c[:, :, None], c[:, None, :]];  Sm = Hc @ G @ Hc^T + R;  nis = nu^T solve(Sm, nu)

    python tools/dense64_sparse_bench.py [--n 2003 10003] [--iters 9] [--warmup 2] [--no-torch]
    rocprofv3 --kernel-trace --stats -- python tools/dense64_sparse_bench.py --trace-pair
        (only correct_sparse(2, 5) and correct(m = 2) at N = 10003, five calls each: the per-kernel split of both)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_TBS = 6.3
CORRECT_SHAPES = [(2, 5), (8, 16), (32, 64), (64, 64)]
LAUNCHES_SPARSE, LAUNCHES_DENSE = 4, 6


def trace_pair(N=10003, calls=5):
    """what a kernel trace needs and nothing else: no torch, no timing"""
    import numpy as np
    from ekf_slam_ml_amd import capi
    rng = np.random.default_rng(N)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    cols = np.array([0, 1, 2, 3 + 2 * 1234, 4 + 2 * 1234], dtype=np.int32)
    Hc, R, nu = rng.standard_normal((2, 5)), 0.01 * np.eye(2), rng.standard_normal(2)
    H = np.zeros((2, N))
    H[:, cols] = Hc
    d = capi.DensePropagator64(N)
    d.set(Sigma=S)
    for _ in range(calls):
        d.correct_sparse(cols, Hc, R, nu)
    for _ in range(calls):
        d.correct(H, R, nu)
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2003, 10003])
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace-pair", action="store_true")
    a = ap.parse_args()
    if a.trace_pair:
        return trace_pair()
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
        x0 = rng.standard_normal(N)
        d = capi.DensePropagator64(N)
        d.state = x0
        if torch is not None:
            dev = torch.device("cuda:0")
            tS0 = torch.from_numpy(S).to(dev)
            tS = tS0.clone()
            tx = torch.from_numpy(x0).to(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        floor_ms = 16.0 * N * N / (ACHIEVABLE_TBS * 1e12) * 1e3
        for m, s in CORRECT_SHAPES:
            cols = np.ascontiguousarray(np.concatenate([[0, 1, 2], 3 + rng.choice(N - 3, size=s - 3, replace=False)]),
                                        dtype=np.int32)
            Hc = rng.standard_normal((m, s))
            R = 0.01 * np.eye(m)
            nu = rng.standard_normal(m)
            H = np.zeros((m, N))
            H[:, cols] = Hc

            def one_sparse():
                d.set(Sigma=S)
                return d.correct_sparse(cols, Hc, R, nu)[1]

            def one_dense():
                d.set(Sigma=S)
                return d.correct(H, R, nu)[1]
            smed, smin = median(one_sparse)
            got = d.sigma
            dmed, dmin = median(one_dense)
            err = float(np.abs(got - d.sigma).max() / np.abs(got).max())
            del got
            line = (f"N={N} correct m={m} s={s}: correct_sparse median {smed:.4f} ms, min {smin:.4f} ms, {LAUNCHES_SPARSE} "
                    f"launches | correct (embedded H) median {dmed:.4f} ms, min {dmin:.4f} ms, {LAUNCHES_DENSE} launches = "
                    f"{dmed / smed:.2f} x | 16 N^2 = {16.0 * N * N / 1e9:.3f} GB at {ACHIEVABLE_TBS} TB/s = {floor_ms:.4f} ms "
                    f"-> correct_sparse is {smed / floor_ms:.2f} x that; Sigma' sparse vs dense rel {err:.1e}")
            if N == 10003 and (m, s) == (2, 5) and not smed < dmed:
                ok = False
                line += "  ** NOT below correct **"
            if torch is not None:
                tc = torch.from_numpy(cols.astype(np.int64)).to(dev)
                tH, tR, tnu = (torch.from_numpy(v).to(dev) for v in (Hc, R, nu))

                def one_torch():
                    tS.copy_(tS0)
                    torch.cuda.synchronize()
                    e0.record()
                    T = tH @ tS.index_select(0, tc)
                    U = tS.index_select(1, tc) @ tH.T
                    Sm = T.index_select(1, tc) @ tH.T + tR
                    K = U @ torch.linalg.inv(Sm)
                    tx.add_(K @ tnu)
                    tS.sub_(K @ T)
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1)
                tmed, tmin = median(one_torch)
                line += f" | torch float64 median {tmed:.4f} ms, min {tmin:.4f} ms = {tmed / smed:.2f} x"
            print(line, flush=True)
        # scoring: the reference's five columns per landmark
        d.set(Sigma=S)
        n = (N - 3) // 2
        m, s = 2, 5
        cols = np.array([[0, 1, 2, 3 + 2 * i, 4 + 2 * i] for i in range(n)], dtype=np.int32)
        Hc = rng.standard_normal((n, m, s))
        R = 0.01 * np.eye(m)
        nu = rng.standard_normal((n, m))
        for J in (1, 32, 1024, n):
            if J > n:
                continue
            c, h, v = cols[:J], Hc[:J], nu[:J]
            smed, smin = median(lambda: d.score_sparse(c, h, R, v)[3])
            line = f"N={N} score m={m} s={s} J={J}: score_sparse median {smed * 1e3:.1f} us, min {smin * 1e3:.1f} us, 1 launch"
            if J * m <= capi.DensePropagator64.SCORE_MAX_ROWS:
                H = np.zeros((J, m, N))
                for j in range(J):
                    H[j][:, c[j]] = h[j]
                nis_s = d.score_sparse(c, h, R, v)[0]
                nis_d = d.score(H, R, v)[0]
                dmed, dmin = median(lambda: d.score(H, R, v)[3])
                err = float((np.abs(nis_s - nis_d) / np.abs(nis_d)).max())
                line += (f" | score (embedded H, {H.nbytes / 1e6:.1f} MB of Jacobians) median {dmed:.4f} ms, min {dmin:.4f} ms "
                         f"= {dmed / smed:.0f} x; nis sparse vs dense rel {err:.1e}")
                del H
            else:
                line += f" | score does not take J * m = {J * m} > {capi.DensePropagator64.SCORE_MAX_ROWS}"
            if torch is not None:
                tc = torch.from_numpy(c.astype(np.int64)).to(dev)
                tH, tR, tv = (torch.from_numpy(np.ascontiguousarray(q)).to(dev) for q in (h, R, v))

                def one_torch_score():
                    e0.record()
                    G = tS0[tc[:, :, None], tc[:, None, :]]
                    Sm = tH @ G @ tH.transpose(1, 2) + tR
                    nis = (tv[:, None, :] @ torch.linalg.solve(Sm, tv[:, :, None])).reshape(-1)
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1)
                tmed, tmin = median(one_torch_score)
                line += f" | torch float64 median {tmed * 1e3:.1f} us, min {tmin * 1e3:.1f} us = {tmed / smed:.1f} x"
            print(line, flush=True)
        d.close()
        if torch is not None:
            del tS, tS0
            torch.cuda.empty_cache()
    if not ok:
        sys.exit("correct_sparse(2, 5) must take less time than correct(m = 2) at N = 10003")


if __name__ == "__main__":
    main()
