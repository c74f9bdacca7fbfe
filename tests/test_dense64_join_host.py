"""CPU (not gpu): the ground under tests/test_gpu_dense64_join.py.  1. the op-by-op numpy model of dense_join_cases equals the
exact int64 model of J blockdiag(Sigma_A, Sigma_B) J^T on every integer family, and a transposed Sigma_A or Sigma_B shows;
2. G and E of join_terms agree with central differences of the composition g; 3. the block formulas equal J S J^T in long
double within the header's bound; 4. an empty local map is the identity by value; 5. two slam_like corners join into a positive
definite covariance; 6. NULL handles and NULL arguments are refused through the built library; 7. the header states the rules
the GPU test holds."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_join_cases as jn
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()


@pytest.mark.parametrize("Nb", [3, 5, 7, 131])
@pytest.mark.parametrize("Na", [3, 5, 13, 65])
@pytest.mark.parametrize("family", sorted(jn.GS))
def test_model_equals_exact_arithmetic_on_the_integer_families(family, Na, Nb):
    SA, SB, G, E = jn.integer_corner(Na), jn.integer_corner(Nb, seed=1), jn.GS[family], jn.integer_E(Nb)
    assert np.abs(E).max() <= 8 and np.abs(E).min() >= 1 and not np.array_equal(SB, SB.T)
    want = jn.exact_join(SA, SB, G, E)
    got = jn.np_join(SA, SB, G, E)
    assert got.shape == (Na + Nb - 3,) * 2 and jn.same_bits(got, want)
    assert np.abs(want).max() < 2 ** 24                           # far below 2^53: exact in any order
    assert jn.same_bits(got[3:Na, 3:Na], SA[3:Na, 3:Na])          # the untouched corner
    assert not jn.same_bits(jn.np_join(SA.T.copy(), SB, G, E), want)      # a transposed access of either operand shows
    assert not jn.same_bits(jn.np_join(SA, SB.T.copy(), G, E), want)
    assert not np.array_equal(want, want.T)                       # never symmetrised


@pytest.mark.parametrize("a,b", [(0, 0), (1, 2), (3, 4)])
def test_terms_agree_with_central_differences(a, b):
    Na, Nb = 3 + 2 * a, 3 + 2 * b
    xa, xb = jn.slam_state(Na), jn.slam_state(Nb, seed=1)
    xb[:3] = [0.4, 2.0, -1.0]
    G, E = jn.join_terms(xa, xb)
    J = jn.jacobian(Na, Nb, G, E)
    h = 1e-6
    num = np.empty_like(J)
    for j in range(Na + Nb):
        e = np.zeros(Na + Nb)
        e[j] = h
        num[:, j] = (jn.g(xa + e[:Na], xb + e[Na:]) - jn.g(xa - e[:Na], xb - e[Na:])) / (2 * h)
    err = jn.row_scale_err(num, J)
    print(f"a={a} b={b}: the join's Jacobian against central differences {err:.3e}")
    assert err <= 1e-7


@pytest.mark.parametrize("Na,Nb", [(3, 3), (3, 7), (7, 3), (5, 5), (13, 7), (7, 13)])
def test_block_formulas_equal_the_full_product_within_the_bound(Na, Nb):
    SA, SB = jn.slam_like(Na), jn.slam_like(Nb, seed=1)
    G, E = jn.join_terms(jn.slam_state(Na), jn.slam_state(Nb, seed=1))
    ratio = jn.bound_ratio(jn.np_join(SA, SB, G, E), SA, SB, G, E)
    print(f"Na={Na} Nb={Nb}: max |err| / (gamma_{jn.OPS} |J||S||J|^T) = {ratio:.4f}")
    assert ratio <= 1.0
    for fast, full in zip(jn.reference(SA, SB, G, E), jn.reference_full(SA, SB, G, E)):   # the reference, block by block
        assert np.all(np.abs(fast - full) <= 8 * np.finfo(np.longdouble).eps * np.abs(jn.reference_full(SA, SB, G, E)[1]))
    rng = np.random.default_rng(Na + Nb)                          # ... and a general E
    E2 = rng.standard_normal((Nb, 3))
    got = jn.np_join(SA, SB, G, E2)
    assert jn.bound_ratio(got, SA, SB, G, E2) <= 1.0
    Nj = Na + Nb - 3
    rows, cols = rng.integers(0, Nj, size=64), rng.integers(0, Nj, size=64)
    assert jn.sampled_bound_ratio(got[rows, cols], SA, Na, SB, Nb, G, E2, rows, cols) <= 1.0   # the sampled form agrees


@pytest.mark.parametrize("Na", [3, 7, 13])
def test_an_empty_local_map_is_the_identity_by_value(Na):
    SA, xa = jn.slam_like(Na), jn.slam_state(Na)
    xb, SB = np.zeros(3), np.zeros((3, 3))
    G, E = jn.join_terms(xa, xb)
    assert np.array_equal(E, [[1, 0, 0], [0, 1, 0], [0, 0, 1]])   # (M' 0 = 0: -0.0 compares equal)
    assert np.array_equal(jn.np_join(SA, SB, G, E), SA) and np.array_equal(jn.g(xa, xb), xa)
    out, Ed = jn.state_model(xa, xb, G[0, 0], G[1, 0])
    assert np.array_equal(out, xa) and np.array_equal(Ed, E)


@pytest.mark.parametrize("Na,Nb", [(7, 5), (13, 13), (65, 31)])
def test_joined_slam_like_corners_are_positive_definite(Na, Nb):
    SA, SB = jn.slam_like(Na), jn.slam_like(Nb, seed=1)
    G, E = jn.join_terms(jn.slam_state(Na), jn.slam_state(Nb, seed=1))
    out = jn.np_join(SA, SB, G, E)
    assert not np.array_equal(out, out.T)                         # slam_like carries an antisymmetric part of 1e-6, kept
    np.linalg.cholesky(0.5 * (out + out.T))                       # definiteness is a property of the symmetric part


def test_null_handles_and_arguments_are_refused_without_a_device():
    lib = capi.load()
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    buf = np.full(13, 7.0)
    fake = ctypes.c_void_p(1)                                     # never dereferenced: the NULL partner is checked first
    for call in (lambda d, s: lib.ekf_dense64_join_congruence(d, s, capi._d(buf), capi._d(buf), None),
                 lambda d, s: lib.ekf_dense64_join_map(d, s, capi._d(buf), None)):
        assert call(None, None) == 1 and b"null destination handle" in lib.ekf_last_error()
        assert call(None, fake) == 1 and b"null destination handle" in lib.ekf_last_error()
        assert call(fake, None) == 1 and b"null source handle" in lib.ekf_last_error()
    assert lib.ekf_dense64_join_launch_info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 1
    assert lib.ekf_dense64_join_launch_info(fake, None, ctypes.byref(b), ctypes.byref(c)) == 1
    assert lib.ekf_dense64_join_launch_info(fake, ctypes.byref(a), None, ctypes.byref(c)) == 1
    assert lib.ekf_dense64_join_launch_info(fake, ctypes.byref(a), ctypes.byref(b), None) == 1
    assert (a.value, b.value, c.value) == (7, 7, 7) and np.array_equal(buf, np.full(13, 7.0))


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with a closed handle")


def test_wrapper_checks_come_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 7, _NoLibrary(), None
    for call in (lambda: d.join_congruence(d, np.eye(2), np.zeros((3, 3))), lambda: d.join_map(d), d.join_launch_info):
        with pytest.raises(ValueError):
            call()
    d._lib = None
    assert callable(capi.DenseEKFSLAM.join)


def test_calls_are_declared_bound_and_documented():
    for name in ("ekf_dense64_join_launch_info", "ekf_dense64_join_congruence", "ekf_dense64_join_map"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS
    text = " ".join(re.sub(r"\n \*", "\n", HDR).split())          # (the comment's own line starts are not part of a rule)
    block = text[text.index("/* Map joining"):text.index("ekf_status ekf_dense64_join_launch_info")]
    for rule in ("SIGMA'[3:Na, 3:Na] IS NOT TOUCHED: NOT READ, NOT WRITTEN", "SIGMA IS NEVER SYMMETRISED",
                 "THE CHECKS COME IN THIS ORDER: (1) NULL dst; (2) NULL src; (3) dst == src; (4) the handles live on different "
                 "devices; (5) dst's live and src's live both odd and >= 3; (6) Na + 2 b <= dst's N; (7) NULL G or E",
                 "AN ENTRY OF Y SEES 14 ROUNDED OPERATIONS", "A CROSS ENTRY 3", "gamma_14 (|J| |Sigma| |J|^T)_ij",
                 "E IS A GENERAL OPERAND", "THETA' IS NOT WRAPPED", "THIS IS THE CALLER'S DUTY AND IS NOT CHECKED",
                 "TOUCHES NEITHER STATE VECTOR", "BIT FOR BIT, ekf_dense64_join_congruence WITH THOSE OPERANDS",
                 "FLUSHES ITS PENDING ROWS FIRST, carry or not", "OTHERWISE SRC IS READ-ONLY", "ORIGINS SIT ON ODD INDICES",
                 "NO ATOMICS, NO REDUCTIONS: A RUN REPEATS BIT FOR BIT", "EKF_ERR_NOMEM", "b = 0 is legal",
                 "acc = fma(W[i][l], E[j][l], acc) for l = 0, 1, 2",
                 "gamma_3 on the two rectangles and on the pose rows and columns below Na",
                 "the uploads of G and E are queued in front of it and are not"):
        assert rule in block, rule
    assert jn.OPS == 14 and jn.CROSS_OPS == 3
    assert "joining two handles" not in text.replace("(Joining two handles is ekf_dense64_join_map, below.)", "")
    assert "Joining two handles is ekf_dense64_join_map" in text
    for doc, words in (("DESIGN.md", "4.8.22"), ("DESIGN.md", "k_jn_corner"), ("README.md", "ekf_dense64_join.hip"),
                       ("INTEGRATION.md", "join(")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
