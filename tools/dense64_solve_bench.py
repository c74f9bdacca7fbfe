"""ekf_dense64_solve and ekf_dense64_color of the dense fp64 handle on the GPU box, against ekf_dense64_whiten timed in the
same run on the same handle.

At N = 10003, Sigma = A A^T / 64 + I (A of shape N x 64, seeded, as tests/test_gpu_dense64_factor.py's full-size test), one
factor(), then medians of >= 9 HIP-event times after >= 2 untimed calls, for 1 and for 64 right-hand sides: whiten, solve,
color, color with the state.  The conditions: solve <= 2.25 x whiten (the forward half is whiten itself, the backward half
has the same number of dependent launches), color < whiten (one launch against one per block column).  color's rate is the
4 Na^2 bytes of L it has to read over its HIP-event time.  Timed once, wall clock: the host route the calls replace --
get_factor, then a triangular solve pair / Z @ L.T on the host.  The results are checked against that host route.

    python tools/dense64_solve_bench.py [--n 10003] [--iters 9] [--warmup 2] [--out profiles/r36/dense64_solve_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r36", "dense64_solve_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    from ekf_slam_ml_amd import capi

    N = a.n
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    S = np.tril(S) + np.tril(S, -1).T
    del A
    d = capi.DensePropagator64(N)
    d.set(Sigma=S)
    d.state = rng.uniform(-20.0, 20.0, size=N)
    rep = d.factor()
    assert rep["ok"] == 1 and rep["Na"] == N
    info = d.solve_launch_info()
    V = rng.standard_normal((64, N))

    def median(call):
        ms = [call()["ms"] for _ in range(a.warmup + a.iters)][a.warmup:]
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    lines = [f"# python tools/dense64_solve_bench.py   (MI355X, N = {N}, block side {info['block']}, factor {rep['ms']:.2f} ms, "
             f"HIP-event medians of {a.iters} after {a.warmup} (min, max), one process, one handle)"]
    t, ok = {}, True
    for nrhs in (1, 64):
        M = V[:nrhs]
        t["whiten", nrhs] = median(lambda: d.whiten(M, want_Y=False))
        t["solve", nrhs] = median(lambda: d.solve(M))
        t["color", nrhs] = median(lambda: d.color(M))
        t["color + state", nrhs] = median(lambda: d.color(M, add_state=True))
        w = t["whiten", nrhs][0]
        for name in ("whiten", "solve", "color", "color + state"):
            m = t[name, nrhs]
            extra = ""
            if name.startswith("color"):
                extra = f"; {4.0 * N * N / (m[0] * 1e-3) / 1e12:.3f} TB/s on the {4.0 * N * N / 1e6:.1f} MB of L (4 Na^2)"
            lines.append(f"nrhs = {nrhs:2d}  {name:14s} {m[0]:9.4f} ms ({m[1]:.4f}, {m[2]:.4f})  = {m[0] / w:.3f} x whiten{extra}")
        c_solve, c_color = t["solve", nrhs][0] <= 2.25 * w, max(t["color", nrhs][0], t["color + state", nrhs][0]) < w
        ok = ok and c_solve and c_color
        lines.append(f"nrhs = {nrhs:2d}  solve <= 2.25 x whiten: {'met' if c_solve else 'MISSED'} (backward half alone "
                     f"{(t['solve', nrhs][0] - w) / w:.3f} x whiten); color < whiten: {'met' if c_color else 'MISSED'}")

    # the host route, timed once, and the device results against it
    got, drawn = d.solve(V[:3], want_Y=True), d.color(V[:3], add_state=True)["X"]
    state = d.state_block(0, N)
    t0 = time.perf_counter()
    L = d.get_factor()
    t_get = (time.perf_counter() - t0) * 1e3
    try:
        from scipy.linalg import solve_triangular
        how = "scipy solve_triangular"
        t0 = time.perf_counter()
        X = solve_triangular(L, solve_triangular(L, V[:3].T, lower=True), lower=True, trans="T").T
    except ImportError:
        how = "numpy.linalg.solve on L and L^T"
        t0 = time.perf_counter()
        X = np.linalg.solve(L.T, np.linalg.solve(L, V[:3].T)).T
    t_solve = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    W = V[:3] @ L.T + state
    t_color = (time.perf_counter() - t0) * 1e3
    del L
    e_solve = float(np.max(np.abs(got["X"] - X)) / np.max(np.abs(X)))
    e_color = float(np.max(np.abs(drawn - W)) / np.max(np.abs(W)))
    lines.append(f"the host route, wall clock, timed once: get_factor {t_get:.0f} ms ({8.0 * N * N / 1e6:.0f} MB), then for 3 right-hand "
                 f"sides {how} {t_solve:.0f} ms, Z @ L.T + state {t_color:.0f} ms")
    lines.append(f"against the host route: solve max |dX| / max |X| = {e_solve:.2e}, color = {e_color:.2e}")
    d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    assert e_solve < 1e-9 and e_color < 1e-12, (e_solve, e_color)
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
