"""GPU: the two dense propagations against their own recorded bits.  tests/golden/dense_gemm_bits.npz holds, for the cases of
dense_gemm_bits_cases.py, what DensePropagator (fp32) and DensePropagator64 (fp64) returned on the commit before the two
GEMMs became one template in ekf_dense_gemm.hpp (tests/golden/make_dense_gemm_bits_golden.py): launch_info(), tile_map()
and a digest of every 128 x 128 block of Sigma after set(F, S, Q), propagate(1).  The operands are dense, asymmetric and
make every sum round, the kernels are compiled with -ffp-contract=off and accumulate along k in a fixed order, so the answer
to a change of the shared source that is meant to keep the arithmetic is the same bits, not a tolerance.  No CPU product here:
test_gpu_dense.py and test_gpu_dense64.py hold the values."""
import os

import numpy as np
import pytest

import dense_gemm_bits_cases as gc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rec():
    z = np.load(os.path.join(HERE, "golden", "dense_gemm_bits.npz"))
    return {k: z[k] for k in z.files}


def _same_cut(rec, k, info, tmap):
    want = rec[k + "_info"]
    assert info.tolist() == want.tolist(), f"{k}: launch_info (ld, tiles, n_big, n_tail) {info.tolist()}, recorded {want.tolist()}"
    assert tmap.shape == rec[k + "_map"].shape and np.array_equal(tmap, rec[k + "_map"]), \
        f"{k}: tile map differs at blocks {np.argwhere(tmap != rec[k + '_map'])[:4].tolist()}"
    assert int(tmap.sum()) == int(info[3])


@pytest.mark.parametrize("dtype,N,ld", [c[:3] for c in gc.CASES], ids=[gc.key(c[0], c[1]) for c in gc.CASES])
def test_same_bits(hip, rec, dtype, N, ld):
    k = gc.key(dtype, N)
    info, tmap, dig = gc.run(hip, dtype, N)
    assert info[0] == ld
    _same_cut(rec, k, info, tmap)
    want = rec[k + "_digest"]
    assert dig.dtype == want.dtype == np.uint64 and dig.shape == want.shape
    bad = np.argwhere(dig != want)
    if len(bad):
        i, j = bad[0]
        raise AssertionError(f"{k}: {len(bad)} of {dig.size} blocks differ, first ({i},{j}) = rows {i * gc.BLOCK}.., columns "
                             f"{j * gc.BLOCK}.., owned by the {'tail' if tmap[i, j] else 'main'} kernel: digest "
                             f"{int(dig[i, j]):016x}, recorded {int(want[i, j]):016x}")


@pytest.mark.parametrize("N,ld", gc.INFO_ONLY)
def test_same_cut_at_large_sizes(hip, rec, N, ld):
    for dtype in ("f32", "f64"):
        d = gc.handle(hip, dtype, N)
        info, tmap = gc.info_row(d), d.tile_map().astype(np.uint8)
        d.close()
        assert info[0] == ld
        _same_cut(rec, gc.key(dtype, N), info, tmap)
