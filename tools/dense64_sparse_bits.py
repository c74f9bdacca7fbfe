"""Bit fingerprints of the dense64 handle's column-sparse calls (correct_sparse, correct_sparse_deferred, score_sparse,
flush, sigma_block through pending rows) on the GPU box, for comparing two builds of the library: fixed seeds, the public
Python API only, one line per case with a SHA-256 over the raw bytes of every output of the case -- state, the full Sigma
after the flush, nis, S, flags, the pending count, block readouts.  Two builds compute the same thing bit for bit exactly
when their listings are identical (diff them).  Written when the eager and the deferred kernels became two instantiations
of one source (profiles/r14/).

The cases sit where that code takes another path:
  N in {7, 64, 65, 130}                one strip, an exact strip, a strip plus one, ld = 256 with padding
  (m, s) in {(1,1), (2,5), (16,22), (16,23), (16,31), (16,32), (17,5), (64,64)} at every N that holds them
                                       the wave and the workgroup form of the scoring kernel and both boundaries between
                                       them at m = 16: s = 31 | 32 with nothing pending, s = 22 | 23 with rows pending
  lists                                neighbouring indices 0, 1, 2, .. and scattered ones that include N - 1
  p in {0, 1, 16, 17, 62} pending      none, one, an exact fold chunk, a chunk plus one, nearly full (and with it the
                                       flush on overflow wherever p + m > 64)
  score_sparse                         J = 5 with R per candidate, nu and S; J = 4 with R shared, no nu, S; J = 1 with R
                                       shared, nu, no S
  a singular S                         eager and deferred, wave and workgroup form: the error, then state, Sigma and the
                                       pending count as they were
  sigma_block with carry on            nr * nc in {1, 255, 256, 257} and nc >= 256, with rows pending and without

    python tools/dense64_sparse_bits.py [--tree DIR] > listing.txt
        --tree: the checkout whose ekf_slam_ml_amd (and built library) is imported; default: the one this file is in
"""
import argparse
import hashlib
import os
import sys

NS = [7, 64, 65, 130]
SHAPES = [(1, 1), (2, 5), (16, 22), (16, 23), (16, 31), (16, 32), (17, 5), (64, 64)]
PENDING = [0, 1, 16, 17, 62]
READS = [(1, 1), (15, 17), (16, 16), (1, 257), (3, 300)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    from ekf_slam_ml_amd import capi

    def digest(parts):
        h = hashlib.sha256()
        for x in parts:
            h.update(np.ascontiguousarray(x).tobytes())
        return h.hexdigest()

    def sigma0(N, rng):   # well conditioned, not symmetric
        A = rng.standard_normal((N, 8))
        return A @ A.T / 8 + np.eye(N) + 1e-3 * rng.standard_normal((N, 1)) * rng.standard_normal((1, N))

    def listed(N, s, kind, rng):
        if kind == "near":
            return np.arange(s, dtype=np.int32)
        c = rng.choice(N - 1, size=s - 1, replace=False) if s > 1 else np.empty(0, dtype=np.int64)
        return rng.permutation(np.append(c, N - 1)).astype(np.int32)

    def regular_R(m, rng):
        B = rng.standard_normal((m, m))
        return 0.05 * (B @ B.T) / m + 0.1 * np.eye(m)

    def start(d, N, p, seed):
        """the handle with Sigma, a state and p rows pending, the same on every call with the same arguments"""
        rng = np.random.default_rng([seed, N, p])
        d.carry = False
        d.set(Sigma=sigma0(N, rng))
        d.state = rng.standard_normal(N)
        left = p
        while left > 0:
            mq = min(left, 16, N)
            sq = min(5, N)
            d.correct_sparse_deferred(listed(N, sq, "far", rng), rng.standard_normal((mq, sq)), regular_R(mq, rng),
                                      0.1 * rng.standard_normal(mq))
            left -= mq
        assert d.pending == p

    for N in NS:
        d = capi.DensePropagator64(N)
        for m, s in SHAPES:
            if m > N or s > N:
                continue
            for kind in ("near", "far"):
                for p in PENDING:
                    rng = np.random.default_rng([N, m, s, int(kind == "far"), p])
                    cols = listed(N, s, kind, rng)
                    Hc, R, nu = rng.standard_normal((m, s)), regular_R(m, rng), 0.1 * rng.standard_normal(m)
                    J = 5
                    cj = np.stack([cols] + [listed(N, s, "far", rng) for _ in range(J - 1)])
                    Hj, nuj = rng.standard_normal((J, m, s)), rng.standard_normal((J, m))
                    Rj = np.stack([regular_R(m, rng) for _ in range(J)])
                    out = []
                    # scores and a readout through the p pending rows, then the deferred correction and the flush
                    start(d, N, p, 1)
                    for sl, Rx, nux, want_S in ((slice(0, 5), Rj, nuj, True), (slice(0, 4), Rj[0], None, True),
                                                (slice(0, 1), Rj[0], nuj, False)):
                        nis, S, flags, _ = d.score_sparse(cj[sl], Hj[sl], Rx if Rx.ndim == 2 else Rx[sl],
                                                          None if nux is None else nux[sl], want_S=want_S)
                        out += [x for x in (nis, S, flags) if x is not None]
                    d.carry = True
                    out.append(d.sigma_block(cols, cols[::-1]))
                    assert d.pending == p
                    d.carry = False
                    nis, _ = d.correct_sparse_deferred(cols, Hc, R, nu)
                    after = d.pending
                    assert after == (p + m if p + m <= 64 else m)   # flushed first when the rows did not fit
                    nis1, S1, flags1, _ = d.score_sparse(cj[:1], Hj[:1], Rj[0], nuj[:1], want_S=True)
                    out += [np.float64(nis), np.int32(after), d.state, nis1, S1, flags1]
                    d.flush()
                    out.append(d.sigma)
                    # the eager correction on the same start (it applies the pending rows first)
                    start(d, N, p, 1)
                    nis, _ = d.correct_sparse(cols, Hc, R, nu)
                    out += [np.float64(nis), np.int32(d.pending), d.state, d.sigma]
                    start(d, N, p, 1)
                    out.append(np.float64(-1.0) if d.correct_sparse(cols, Hc, R)[0] is None else np.float64(1.0))
                    out += [d.state, d.sigma]   # without nu: the state untouched
                    print(f"N={N} m={m} s={s} {kind} p={p}: {digest(out)}", flush=True)
        # a singular S (Hc = 0, R = 0): wave form (2, 5) and workgroup form (17, 5), eager and deferred
        for m, s in ((2, 5), (17, 5)):
            if m > N:
                continue
            rng = np.random.default_rng([N, m, s, 99])
            cols = listed(N, s, "far", rng)
            for p in (0, 16):
                for name in ("correct_sparse", "correct_sparse_deferred"):
                    start(d, N, p, 2)
                    x0 = d.state
                    d.carry = True
                    b0 = d.sigma_block(np.arange(N), np.arange(N))   # Sigma_cur, the pending rows left pending
                    d.carry = False
                    try:
                        getattr(d, name)(cols, np.zeros((m, s)), np.zeros((m, m)), np.ones(m))
                        verdict = 0
                    except capi.EkfError:
                        verdict = 1
                    left = d.pending
                    assert verdict == 1 and left == (p if name.endswith("deferred") else 0)
                    x1, S1 = d.state, d.sigma
                    assert x1.tobytes() == x0.tobytes()
                    if p == 0:
                        assert S1.tobytes() == b0.tobytes()
                    print(f"N={N} m={m} s={s} singular {name} p={p}: {digest([np.int32(verdict), np.int32(left), x1, S1])}",
                          flush=True)
        # block readouts with carry on
        for p in (0, 17):
            start(d, N, p, 3)
            d.carry = True
            rng = np.random.default_rng([N, p, 7])
            out = [d.sigma_block(rng.integers(0, N, nr), np.append(rng.integers(0, N, nc - 1), N - 1)) for nr, nc in READS]
            assert d.pending == p
            d.carry = False
            out.append(d.sigma)
            print(f"N={N} sigma_block carry p={p} {READS}: {digest(out)}", flush=True)
        d.close()


if __name__ == "__main__":
    main()
