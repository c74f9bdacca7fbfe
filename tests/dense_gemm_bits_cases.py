"""What tests/golden/make_dense_gemm_bits_golden.py records and tests/test_gpu_dense_gemm_bits.py replays: the cases of the
two dense propagations (the smallest shapes that reach every path of the split), their operands and the digest of a result.

Operands come from default_rng(seed).integers alone, scaled by a power of two, so they are the same bits on every machine
and are rebuilt instead of stored.  All three matrices are dense and asymmetric and the sums round, so a result's bits pin
the order of accumulation, not only the tile maps."""
import hashlib

import numpy as np

BLOCK = 128   # the unit of launch_info() / tile_map(): one digest per 128 x 128 block of the result

# (dtype, N, ld, what it reaches)
CASES = [
    ("f32", 43, 128, "one tile"),
    ("f32", 300, 384, "one main tile row plus the bottom strip on the tail kernel"),
    ("f32", 403, 512, "two main tile rows"),
    ("f32", 4700, 4736, "512 main + 345 tail"),
    ("f64", 1, 128, "one tile"),
    ("f64", 43, 128, "one tile"),
    ("f64", 129, 256, "four tiles"),
    ("f64", 300, 384, "nine tiles"),
    ("f64", 2850, 2944, "512 main + 17 tail: the smallest ld at which the fp64 tail kernel runs"),
]
# launch_info() and tile_map() alone, no propagation: (N, ld) for both handles
INFO_ONLY = [(5800, 5888), (10003, 10112)]

DTYPE = {"f32": np.float32, "f64": np.float64}
_BITS = {"f32": 11, "f64": 20}   # integers in [-2^b, 2^b) times 2^-b


def key(dtype, N):
    return f"{dtype}_{N}"


def handle(capi, dtype, N):
    return (capi.DensePropagator if dtype == "f32" else capi.DensePropagator64)(N)


def operands(dtype, N):
    """F, Sigma, Q of a case"""
    b = _BITS[dtype]
    rng = np.random.default_rng([N, b])
    return tuple((rng.integers(-2 ** b, 2 ** b, size=(N, N)) * 2.0 ** -b).astype(DTYPE[dtype]) for _ in range(3))


def info_row(d):
    i = d.launch_info()
    return np.array([i["ld"], i["tiles"], i["n_big"], i["n_tail"]], dtype=np.int32)


def digests(sigma):
    """[tiles][tiles] uint64: the first 8 bytes of the SHA-256 of every 128 x 128 block's bytes (ragged at the edge of N)"""
    N = sigma.shape[0]
    t = (N + BLOCK - 1) // BLOCK
    out = np.zeros((t, t), dtype=np.uint64)
    for i in range(t):
        for j in range(t):
            blk = np.ascontiguousarray(sigma[i * BLOCK:(i + 1) * BLOCK, j * BLOCK:(j + 1) * BLOCK])
            out[i, j] = int.from_bytes(hashlib.sha256(blk.tobytes()).digest()[:8], "little")
    return out


def run(capi, dtype, N):
    """set(F, S, Q), propagate(1): both the NN and the NT+Q product.  Returns launch_info, tile_map, digests."""
    d = handle(capi, dtype, N)
    info, tmap = info_row(d), d.tile_map().astype(np.uint8)
    d.set(*operands(dtype, N))
    d.propagate(1)
    dig = digests(d.sigma)
    d.close()
    return info, tmap, dig
