"""Writes tests/golden/dense_gemm_bits.npz: what the two dense propagations (DensePropagator, fp32, and DensePropagator64,
fp64) made of the cases of tests/dense_gemm_bits_cases.py -- launch_info(), tile_map() and, for every 128 x 128 block of the
result of set(F, S, Q), propagate(1), the first 8 bytes of the block's SHA-256 -- plus launch_info() and tile_map() alone at
two larger sizes.  Operands are not stored: the cases module rebuilds them bit for bit.
tests/test_gpu_dense_gemm_bits.py replays the cases and asks for the same numbers, so the file is recorded on the commit
whose arithmetic is to be kept, run by hand on a machine with the GPU:

    python tests/golden/make_dense_gemm_bits_golden.py

Layout, per case K = <dtype>_<N>: K_info int32 [4] = ld, tiles, n_big, n_tail; K_map uint8 [tiles][tiles] (1 = tail kernel);
K_digest uint64 [tiles][tiles].  The info-only sizes have no K_digest.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ekf_slam_ml_amd import capi  # noqa: E402
import dense_gemm_bits_cases as gc  # noqa: E402


def main():
    out = {}
    for dtype, N, ld, what in gc.CASES:
        info, tmap, dig = gc.run(capi, dtype, N)
        assert info[0] == ld and dig.shape == tmap.shape, (dtype, N, info)
        k = gc.key(dtype, N)
        out[k + "_info"], out[k + "_map"], out[k + "_digest"] = info, tmap, dig
        print(f"{k:10s} ld {info[0]:5d} tiles {info[1]:2d} n_big {info[2]:4d} n_tail {info[3]:3d}  digest[0][0] {int(dig[0, 0]):016x}  ({what})",
              flush=True)
    for N, ld in gc.INFO_ONLY:
        for dtype in ("f32", "f64"):
            d = gc.handle(capi, dtype, N)
            k = gc.key(dtype, N)
            out[k + "_info"], out[k + "_map"] = gc.info_row(d), d.tile_map().astype(np.uint8)
            d.close()
            assert out[k + "_info"][0] == ld
            print(f"{k:10s} {out[k + '_info'].tolist()} tail blocks {int(out[k + '_map'].sum())}", flush=True)
    path = os.path.join(HERE, "dense_gemm_bits.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(gc.CASES), "cases")


if __name__ == "__main__":
    main()
