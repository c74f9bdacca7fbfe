"""The joint compatibility association of the dense fp64 handle (ekf_dense64_jcbb_candidates, ekf_dense64_associate_jcbb)
against the per-reading joint rule (ekf_dense64_associate_joint) on the GPU box: after tools/dense64_joint_bench.py.

At N = 10003 with 5000 known landmarks and a scan of J = 8 readings on distinct landmarks, everything in one process on one
handle, medians of >= 9 after >= 2 untimed.  Before every repetition the state and Sigma are restored from an extract_map clone (outside the timed
region), so every call starts from the same bits.  Recorded: wall clock and HIP-event time of jcbb_candidates, of
associate_jcbb eager and deferred and of associate_joint on the same restored state; the wall clock of the search alone on
the candidates that came down; the difference jcbb - joint; and the host route for W that the device kernel replaces:
get_sigma_block of the union of the candidates' columns plus numpy products.

    python tools/dense64_jcbb_bench.py [--n 10003] [--readings 8] [--iters 9] [--warmup 2] [--out profiles/r38/dense64_jcbb_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10003)
    ap.add_argument("--readings", type=int, default=8)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r38", "dense64_jcbb_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    import numpy as np
    import dense_landmark_cases as lc
    from ekf_slam_ml_amd import capi

    N, J = a.n, a.readings
    n = (N - 3) // 2
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    lms = [n * (2 * j + 1) // (2 * J) for j in range(J)]
    z = np.array([lc.reading_of(x, i, (0.002, -0.001)) for i in lms])
    src, d = capi.DensePropagator64(N), capi.DensePropagator64(N)
    src.set(Sigma=S)
    src.state = x
    gates = np.array([float(k + 1) for k in range(J)])

    def restore():
        d.extract_map(src)   # a clone: every bit of the state and Sigma, on the device

    def stats(call, ev_of, check=None):
        wall, ev = [], []
        for _ in range(a.warmup + a.iters):
            restore()
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(ev_of(out))
            if check:
                check(out)
        wall, ev = np.array(wall[a.warmup:]), np.array(ev[a.warmup:])
        return float(np.median(wall)), float(wall.min()), float(wall.max()), float(np.median(ev))

    def all_corrected(out):
        assert (np.asarray(out[1]) >= 0).all(), out[1]   # every reading corrected a landmark: the work compared is alike

    def line(name, t):
        return f"{name:28s} wall clock: median {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f}); HIP events {t[3]:.4f} ms"

    lines = [f"# python tools/dense64_jcbb_bench.py   (MI355X, N = {N}, known = n_max = {n}, J = {J} readings on distinct "
             f"landmarks, gate_ic = 1, medians of {a.iters} after {a.warmup}, one process, one handle, state and Sigma restored "
             f"before every repetition)"]
    tc = stats(lambda: d.jcbb_candidates(z, n, 1.0), lambda o: o["elapsed_ms"])
    lines.append(line("jcbb_candidates", tc))
    t = {}
    for deferred in (False, True):
        mode = "DEFERRED" if deferred else "eager"
        t[mode, "jcbb"] = stats(lambda: d.associate_jcbb(z, n, n, 1.0, deferred=deferred), lambda o: o[-1])
        t[mode, "joint"] = stats(lambda: d.associate_joint(z, n, n, deferred=deferred), lambda o: o[-1], all_corrected)
        lines.append(line(f"{mode:8s} associate_jcbb", t[mode, "jcbb"]))
        lines.append(line(f"{mode:8s} associate_joint", t[mode, "joint"]))
        lines.append(f"{mode:8s} jcbb - joint = {t[mode, 'jcbb'][0] - t[mode, 'joint'][0]:.4f} ms (wall clock), "
                     f"{t[mode, 'jcbb'][3] - t[mode, 'joint'][3]:.4f} ms (HIP events)")
    restore()
    cand = d.jcbb_candidates(z, n, 1.0)
    search, route = [], []
    for _ in range(a.warmup + a.iters):
        t0 = time.perf_counter()
        _, rep = capi.DensePropagator64.jcbb_search(J, cand["reading_of"], cand["lm_of"], cand["nis"], cand["W"], cand["nu"],
                                                    gates)
        search.append((time.perf_counter() - t0) * 1e3)
        # the host route for W: Sigma at the union of the candidates' columns comes down, the model is repeated on the host
        t0 = time.perf_counter()
        idx = np.unique(np.concatenate([[0, 1, 2]] + [[3 + 2 * i, 4 + 2 * i] for i in cand["lm_of"]])).astype(np.int32)
        G = d.sigma_block(idx, idx)
        per = [d.score_landmarks(*z[j], first_lm=int(i), count=1, want_terms=True) for j, i in zip(cand["reading_of"], cand["lm_of"])]
        H = np.zeros((2 * len(per), len(idx)))
        for q, o in enumerate(per):
            H[2 * q:2 * q + 2, np.searchsorted(idx, o[4][0][0])] = o[4][1][0]
        Wh = H @ G @ H.T
        route.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"the search alone (P = {cand['P']}, {rep['nodes']} nodes, through ctypes): wall clock median "
                 f"{np.median(search[a.warmup:]) * 1e3:.1f} us; its share of eager associate_jcbb "
                 f"{np.median(search[a.warmup:]) / t['eager', 'jcbb'][0]:.3f}")
    lines.append(f"host route for W (get_sigma_block of {len(idx)} columns, the operands per candidate, numpy products): wall "
                 f"clock median {np.median(route[a.warmup:]):.4f} ms; max |W_host + r_meas I - W| = "
                 f"{np.abs(Wh + capi.default_params().r_meas * np.eye(2 * len(per)) - cand['W']).max():.3e}")
    d.close()
    src.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
