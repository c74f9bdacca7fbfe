"""CPU: the numpy models of ekf_dense64_solve / ekf_dense64_color (dense_solve_cases) against exact rational arithmetic on the
integer family, exactness of that family at every size the GPU test uses for every block side the library may report, the
derived componentwise bounds on slam_like for the model itself, and what the library and the wrapper refuse without a device."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dense_solve_cases as sc
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
ALL_SIZES = sorted({Na for nb in sc.BLOCK_SIDES for Na in sc.sizes(nb)})


def _fraction_back(L, y):
    Na = L.shape[0]
    x = [Fraction(0)] * Na
    for i in range(Na - 1, -1, -1):
        x[i] = (Fraction(y[i]) - sum(Fraction(L[k, i]) * x[k] for k in range(i + 1, Na))) / Fraction(L[i, i])
    return x


def _fraction_color(L, z, state=None):
    Na = L.shape[0]
    x = [sum(Fraction(L[i, k]) * Fraction(z[k]) for k in range(i + 1)) for i in range(Na)]
    return x if state is None else [a + Fraction(s) for a, s in zip(x, state)]


@pytest.mark.parametrize("Na", [1, 2, 3, 15, 17, 33, 50])
def test_models_equal_exact_arithmetic_on_the_integer_family(Na):
    C, L0 = sc.integer_factor(Na)
    rng = np.random.default_rng(Na)
    Y = rng.integers(-3, 4, size=(2, Na)).astype(np.float64)
    state = rng.integers(-9, 10, size=Na).astype(np.float64)
    junk = L0 + np.triu(np.full((Na, Na), np.nan), 1)        # the models read nothing above the diagonal
    colored, shifted = sc.np_color(junk, Y), sc.np_color(junk, Y, state)
    back = sc.np_back(junk, Y @ L0)                          # L0^T x = y' has the integer solution x = Y for y' = Y L0
    for r in range(2):
        assert [Fraction(v) for v in colored[r]] == _fraction_color(L0, Y[r])
        assert [Fraction(v) for v in shifted[r]] == _fraction_color(L0, Y[r], state)
        assert [Fraction(v) for v in back[r]] == _fraction_back(L0, (Y @ L0)[r]) == [Fraction(v) for v in Y[r]]


@pytest.mark.parametrize("Na", ALL_SIZES)
def test_integer_family_is_exact_at_every_gpu_size(Na):
    C, L0 = sc.integer_factor(Na)
    X0 = np.random.default_rng(50 + Na).integers(-3, 4, size=(3, Na)).astype(np.float64)
    B = X0 @ C
    assert np.array_equal(B, np.rint(B)) and np.abs(B).max() < 2 ** 20      # every partial sum is an integer far below 2^53
    Y, _ = sc.np_whiten(L0, B)
    assert sc.same_bits(Y, X0 @ L0)
    assert sc.same_bits(sc.np_back(L0, Y), X0)
    assert sc.same_bits(sc.np_color(L0, X0), X0 @ L0.T)
    assert sc.same_bits(sc.np_color(L0, Y), B)                               # colouring undoes whitening


@pytest.mark.parametrize("Na", ALL_SIZES)
def test_derived_bounds_hold_for_the_model_on_slam_like(Na):
    A = sc.slam_like(Na)
    rep, L = sc.np_factor(sc.slam_like_input(Na))
    assert rep["ok"] == 1
    rng = np.random.default_rng(Na + 9)
    B, Z, state = rng.standard_normal((3, Na)), rng.standard_normal((3, Na)), rng.standard_normal(Na)
    Y, _ = sc.np_whiten(L, B)
    X = sc.np_back(L, Y)
    V, Vs = sc.np_color(L, Z), sc.np_color(L, Z, state)
    back = max(sc.back_residual_ratio(L, X[r], Y[r]) for r in range(3))
    col = max(max(sc.color_residual_ratio(L, V[r], Z[r]), sc.color_residual_ratio(L, Vs[r], Z[r], state)) for r in range(3))
    whole = max(sc.solve_residual_ratio(A, L, X[r], B[r]) for r in range(3))
    print(f"Na={Na}: backward {back:.3f}, colour {col:.3f}, end to end {whole:.4f} of their bounds")
    assert back <= 1.0 and col <= 1.0 and whole <= 1.0
    assert sc.same_bits(Vs, V + state)                                       # the addition comes last


def test_zero_sign_is_the_only_thing_forgiven():
    assert sc.same_up_to_zero_sign([0.0, 1.0], [-0.0, 1.0]) and not sc.same_bits([0.0], [-0.0])
    assert not sc.same_up_to_zero_sign([1.0], [np.nextafter(1.0, 2.0)])


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_checks_come_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 30, _NoLibrary(), None   # a closed handle
    for call in (d.solve_launch_info, lambda: d.solve(np.zeros(30)), lambda: d.color(np.zeros(30))):
        with pytest.raises(ValueError):
            call()
    d._lib = None
    assert callable(capi.DenseEKFSLAM.sample_maps) and callable(capi.DenseEKFSLAM.map_solve)


def test_null_handles_and_arguments_are_refused_without_a_device():
    lib = capi.load()
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    buf = np.full(4, 7.0)
    p = capi._d(buf)
    assert lib.ekf_dense64_solve_launch_info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 1
    assert (a.value, b.value, c.value) == (7, 7, 7)
    assert lib.ekf_dense64_solve(None, 1, p, p, p, p, None) == 1 and b"ekf_dense64_solve: null handle" in lib.ekf_last_error()
    assert lib.ekf_dense64_color(None, 1, p, 1, p, None) == 1 and b"ekf_dense64_color: null handle" in lib.ekf_last_error()
    assert lib.ekf_dense64_solve(None, 0, None, None, None, None, None) == 1 and b"null handle" in lib.ekf_last_error()
    assert lib.ekf_dense64_color(None, 0, None, 0, None, None) == 1 and b"null handle" in lib.ekf_last_error()
    assert np.array_equal(buf, np.full(4, 7.0))


def test_calls_are_declared_bound_and_documented():
    for name in ("ekf_dense64_solve", "ekf_dense64_color", "ekf_dense64_solve_launch_info"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS
    text = " ".join(HDR.split())
    for rule in ("no reciprocal and no inverse of a diagonal block", "THE FORWARD HALF IS ekf_dense64_whiten's launches",
                 "THE FACTOR IS A SNAPSHOT, THE STATE IS THE CURRENT ONE", "IS NOT WRAPPED",
                 "neither flushes the pending rows, neither ends an open region"):
        assert rule in text, rule
    for doc, words in (("DESIGN.md", "ekf_dense64_solve"), ("DESIGN.md", "k_dc_color"), ("INTEGRATION.md", "sample_maps"),
                       ("README.md", "ekf_dense64_color")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
