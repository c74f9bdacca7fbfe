"""ekf_dense64_extract_map of the dense fp64 handle on the GPU box: a map, or a submap, copied into a second handle.

At N = 10003 the source holds 5000 landmarks; everything runs in one process, medians of >= 9 after >= 2 untimed, HIP-event
time and wall clock of one call.  Cases: (a) clone (the NULL list); (b) every second landmark; (c) a seeded random permutation
of all 5000; (d) clone with 16 rows pending on the source, which are carried (the destination has none of its own: it would
apply them first, a pass over its Sigma).  Yardsticks in the same process: a device-to-device torch copy of an Nd x Nd float64
tensor (the floor for (a)), reframe(FIXED) and symmetrize at the same live dimension (the project's own one-pass kernels over
Sigma), and -- timed once -- the host route: get_sigma of the source, set on the destination, the state.  The rate is 16 Nd^2
bytes (8 read, 8 written) over the HIP-event time.

    python tools/dense64_extract_bench.py [--n 10003] [--iters 9] [--warmup 2] [--out profiles/r33/dense64_extract_bench.txt]
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
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pending", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r33", "dense64_extract_bench.txt"))
    a = ap.parse_args()
    assert a.iters >= 9 and a.warmup >= 2, "at least 9 timed repetitions after 2 untimed ones"
    assert a.n % 2 == 1 and a.pending % 2 == 0
    import numpy as np
    import torch
    from ekf_slam_ml_amd import capi

    N = a.n
    b = (N - 3) // 2
    rng = np.random.default_rng(8)
    A = rng.standard_normal((N, 64))
    S = A @ A.T / 64 + np.eye(N)
    del A
    x = np.concatenate([[0.3, 0.1, -0.2], rng.uniform(-20.0, 20.0, size=N - 3)])
    src, dst = capi.DensePropagator64(N), capi.DensePropagator64(N)
    src.set(Sigma=S)
    src.state = x
    dst.set(Sigma=np.zeros((N, N)))

    def stats(call, before=None):
        wall, ev = [], []
        for _ in range(a.warmup + a.iters):
            if before:
                before()   # (outside the timed region)
            t0 = time.perf_counter()
            ms = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(ms)
        wall, ev = np.array(wall[a.warmup:]), np.array(ev[a.warmup:])
        return float(np.median(wall)), float(wall.min()), float(wall.max()), float(np.median(ev))

    def line(name, Nd, t, extra=""):
        by = 16.0 * Nd * Nd
        return (f"{name:34s} Nd = {Nd:5d}: HIP events {t[3]:.4f} ms = {by / (t[3] * 1e-3) / 1e12:.2f} TB/s on {by / 1e6:.1f} MB "
                f"(16 Nd^2); wall clock median {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f}){extra}")

    lines = [f"# python tools/dense64_extract_bench.py   (MI355X, N = {N}, the source holds {b} landmarks, medians of {a.iters} "
             f"after {a.warmup}, one process, two handles of the same N)"]
    second, perm = np.arange(0, b, 2), rng.permutation(b)
    cases = [("(a) clone (NULL list)", None), ("(b) every second landmark", second), ("(c) random permutation of all", perm)]
    times = {}
    for name, keep in cases:
        Nd = 3 + 2 * (b if keep is None else keep.size)
        times[name] = stats(lambda: dst.extract_map(src, keep))
        lines.append(line(name, Nd, times[name]))
        rows = np.array([0, 1, 2, 3, Nd // 2, Nd - 2, Nd - 1])
        io = np.concatenate([np.arange(3), (3 + 2 * (np.arange(b) if keep is None else keep)[:, None] + np.arange(2)).reshape(-1)])
        assert np.array_equal(dst.sigma_block(rows, rows).view(np.uint64), S[np.ix_(io[rows], io[rows])].view(np.uint64)), name
    # (d) the source has rows pending: they are carried, the source keeps them
    rngd = np.random.default_rng(17)
    for i in range(a.pending // 2):
        j = (977 * i + 1) % b
        src.correct_sparse_deferred(np.array([0, 1, 2, 3 + 2 * j, 4 + 2 * j]), rngd.standard_normal((2, 5)), 0.5 * np.eye(2),
                                    0.1 * rngd.standard_normal(2))
    assert src.pending == a.pending
    name = f"(d) clone, {a.pending} rows pending"
    # (the destination applies rows of its own first -- here the ones the repetition before carried into it, a pass over
    # its Sigma that is not this case's business: they are flushed outside the timed region)
    times[name] = stats(lambda: dst.extract_map(src), before=dst.flush)
    assert src.pending == a.pending and dst.pending == a.pending
    lines.append(line(name, N, times[name], f"; + {32.0 * a.pending * N / 1e6:.1f} MB of panels"))
    src.flush()
    dst.flush()

    # the yardsticks
    dev = torch.device("cuda", 0)
    for name, Nd in (("torch copy_ (device to device)", N), ("torch copy_ (device to device)", 3 + 2 * second.size)):
        ta, tb = torch.empty((Nd, Nd), dtype=torch.float64, device=dev).normal_(), torch.empty((Nd, Nd), dtype=torch.float64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy():
            e0.record()
            tb.copy_(ta)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        times[(name, Nd)] = stats(copy)
        lines.append(line(name, Nd, times[(name, Nd)]))
        del ta, tb
    torch.cuda.empty_cache()
    t_ref = stats(lambda: src.reframe(capi.DensePropagator64.FRAME_FIXED, 0.1, 1.0, 2.0))
    lines.append(line("reframe(FIXED), in place", N, t_ref))
    t_sym = stats(lambda: src.symmetrize()["ms"])
    lines.append(line("symmetrize, in place", N, t_sym))
    t0 = time.perf_counter()
    dst.set(Sigma=src.sigma)
    dst.state = src.state
    t_host = (time.perf_counter() - t0) * 1e3
    clone, floor = times["(a) clone (NULL list)"][3], times[("torch copy_ (device to device)", N)][3]
    lines.append(f"the host route (get_sigma, set, the state), timed once: {t_host:.1f} ms wall clock = {t_host / times['(a) clone (NULL list)'][0]:.0f} x "
                 f"the clone's wall clock")
    lines.append(f"clone / torch copy = {clone / floor:.3f} (HIP events); clone / reframe(FIXED) = {clone / t_ref[3]:.3f}; "
                 f"permutation / clone = {times['(c) random permutation of all'][3] / clone:.2f}")
    src.close()
    dst.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
