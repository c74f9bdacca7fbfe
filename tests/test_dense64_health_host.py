"""CPU (not gpu): the definitions behind ekf_dense64_health and ekf_dense64_symmetrize.  The op-by-op numpy models of
dense_health_cases against exact rational arithmetic on the integer families, the properties symmetrize promises, the
conditions on the inputs that the GPU test relies on (for every size it uses), the hand-counted defects of the degenerate
family, the wrappers' checks and the header."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dense_health_cases as hc
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()


def _tile():
    """the tile side in states: kDense64HealthTile of ekf_dense.hpp (the GPU test asks the library)"""
    src = open(os.path.join(ROOT, "ekf_slam_ml_amd", "csrc", "ekf_dense.hpp")).read()
    return int(re.search(r"constexpr int kDense64HealthTile = (\d+);", src).group(1))


SIZES = hc.sizes(_tile())


def _fraction_health(C):
    """the report on a finite corner in exact arithmetic (integers: every fl() is exact)"""
    Na = C.shape[0]
    F = [[Fraction(float(C[i, j])) for j in range(Na)] for i in range(Na)]
    rep = {"n_nonfinite": 0, "n_asym": 0, "n_minor": 0, "max_asym": 0.0, "asym_i": -1, "asym_j": -1}
    best = None
    for i in range(Na):
        for j in range(i + 1, Na):
            rep["n_asym"] += F[i][j] != F[j][i]
            rep["n_minor"] += F[i][j] * F[j][i] > F[i][i] * F[j][j]
            d = abs(F[i][j] - F[j][i])
            if best is None or d > best:
                best, rep["asym_i"], rep["asym_j"] = d, i, j
    rep["max_asym"] = float(best) if best is not None else 0.0
    dg = [F[i][i] for i in range(Na)]
    rep["min_diag"] = float(min(dg))
    rep["min_diag_i"] = dg.index(min(dg))
    rep["n_diag_bad"] = sum(v <= 0 for v in dg)
    return rep


@pytest.mark.parametrize("family", ["symmetric_integers", "asymmetric_integers"])
@pytest.mark.parametrize("Na", [1, 2, 3, 17, 40])
def test_models_equal_exact_arithmetic_on_integers(family, Na):
    C = hc.corner(family, Na)
    assert np.array_equal(C, np.round(C)) and np.abs(C).max() <= 9
    got, want = hc.np_health(C, Na), _fraction_health(C)
    assert hc.same_report(got, want), (got, want)
    out, changed, most = hc.np_symmetrize(C, Na)
    assert changed == want["n_asym"] and most == want["max_asym"]
    for i in range(Na):
        for j in range(Na):
            exact = Fraction(float(C[i, j])) if i == j else (Fraction(float(C[i, j])) + Fraction(float(C[j, i]))) / 2
            assert Fraction(float(out[i, j])) == exact, (i, j)
    if family == "symmetric_integers":
        assert changed == 0 and most == 0.0 and (Na == 1 or (got["asym_i"], got["asym_j"]) == (0, 1))


@pytest.mark.parametrize("family", hc.FAMILIES)
@pytest.mark.parametrize("Na", SIZES)
def test_symmetrize_model_properties(family, Na):
    N = Na + 5
    S = np.full((N, N), 7.25)
    S[:Na, :Na] = hc.corner(family, Na)
    out, changed, most = hc.np_symmetrize(S, Na)
    before = hc.np_health(S, Na)
    assert changed == before["n_asym"] and hc.same_bits(most, before["max_asym"])
    assert hc.same_bits(out[:Na, :Na], out[:Na, :Na].T)                          # symmetric in bits
    assert hc.same_bits(np.diagonal(out), np.diagonal(S))                        # the diagonal is not written
    assert hc.same_bits(out[Na:], S[Na:]) and hc.same_bits(out[:, Na:], S[:, Na:])   # nor anything outside the corner
    again, changed2, most2 = hc.np_symmetrize(out, Na)
    assert changed2 == 0 and (most2 == 0.0 or family == "degenerate")             # (a NaN pair keeps d a NaN)
    assert hc.same_bits(again, out)                                              # twice is once
    after = hc.np_health(out, Na)
    assert after["n_asym"] == 0
    if family == "symmetric_integers":
        assert changed == 0 and hc.same_bits(out, S)                             # a symmetric input comes back bit for bit


@pytest.mark.parametrize("Na", SIZES)
def test_random_spd_is_healthy_at_every_size_of_the_gpu_test(Na):
    """the condition on the inputs the GPU test relies on: no minor violation, no bad diagonal entry, nothing non-finite,
    |correlation| <= 0.9; and (from 2 on) the perturbation did make it asymmetric"""
    C = hc.corner("random_spd", Na)
    rep = hc.np_health(C, Na)
    assert rep["n_minor"] == 0 and rep["n_diag_bad"] == 0 and rep["n_nonfinite"] == 0, rep
    dg = np.sqrt(np.diagonal(C))
    corr = np.abs(C / np.outer(dg, dg) - np.eye(Na))
    assert corr.max() <= 0.9
    if Na >= 3:
        assert rep["n_asym"] > 0 and 0.0 < rep["max_asym"] < 1e-14 * np.abs(C).max()


def test_degenerate_defects_are_each_counted_once():
    for Na in (hc.DEGENERATE_FULL, 16, _tile() + 1):
        C = hc.corner("degenerate", Na)
        rep, want = hc.np_health(C, Na), hc.degenerate_counts(Na)
        assert hc.same_report(rep, want), (Na, rep, want)
        out, changed, most = hc.np_symmetrize(C, Na)
        assert changed == 5 and hc.same_bits(most, hc.NAN_LONE)
        assert hc.same_bits(out[0, 1], hc.NAN_PAIR) and hc.same_bits(out[1, 0], hc.NAN_PAIR)   # the payload survives
        assert np.isnan(out[0, 2]) and np.isnan(out[2, 0]) and hc.same_bits(out[0, 2], out[2, 0])
        assert out[1, 3] == out[3, 1] == np.inf
        assert hc.same_bits(out[2, 4], 0.0) and hc.same_bits(out[4, 2], 0.0)                    # -0.0 + 0.0 = +0.0
        assert int(hc.bits(out[3, 5])[0]) == 5 and int(hc.bits(out[5, 3])[0]) == 5              # (3 + 7) / 2 subnormal units
        assert out[4, 6] == out[6, 4] == np.inf                                                  # the sum overflowed
        assert out[7, 7] == -4.0 and hc.same_bits(out[8, 8], 0.0)
        after = hc.np_health(out, Na)
        assert after["n_asym"] == 0 and after["n_nonfinite"] == 2 + 2 + 2 + 2


def test_ties_and_empty_cases():
    one = hc.np_health(np.array([[np.nan]]), 1)
    assert (one["max_asym"], one["asym_i"], one["asym_j"]) == (0.0, -1, -1)
    assert one["min_diag"] == np.inf and one["min_diag_i"] == -1 and one["n_diag_bad"] == 1 and one["n_nonfinite"] == 1
    S = np.array([[0.0, 1.0, 5.0, 2.0], [3.0, -0.0, 4.0, 8.0], [3.0, 4.0, 2.0, 1.0], [2.0, 6.0, 1.0, np.nan]])
    rep = hc.np_health(S, 4)
    assert (rep["max_asym"], rep["asym_i"], rep["asym_j"]) == (2.0, 0, 1)        # (0, 1), (0, 2) and (1, 3) all differ by 2
    assert rep["min_diag_i"] == 0 and hc.same_bits(rep["min_diag"], 0.0)         # +0.0 at 0 before -0.0 at 1
    assert rep["n_diag_bad"] == 3 and rep["n_asym"] == 3
    assert hc.np_health(S, 2)["n_asym"] == 1                                     # the corner only


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_checks_come_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 30, _NoLibrary(), None   # a closed handle
    for call in (d.health, d.symmetrize, d.health_launch_info):
        with pytest.raises(ValueError):
            call()
    d._lib = None
    assert callable(capi.DenseEKFSLAM.health) and callable(capi.DenseEKFSLAM.symmetrize)


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()
    rep, n, most = capi.HealthReport(), ctypes.c_longlong(7), ctypes.c_double(7.0)
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.ekf_dense64_health(None, ctypes.byref(rep), None) == 1
    assert lib.ekf_dense64_symmetrize(None, ctypes.byref(n), ctypes.byref(most), None) == 1
    assert lib.ekf_dense64_health_launch_info(None, ctypes.byref(a), ctypes.byref(b)) == 1
    assert n.value == 7 and most.value == 7.0


def test_calls_are_declared_bound_and_documented():
    for name in ("ekf_dense64_health", "ekf_dense64_symmetrize", "ekf_dense64_health_launch_info"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS
    body = re.search(r"typedef struct ekf_dense64_health_report \{(.*?)\} ekf_dense64_health_report;", HDR, re.S).group(1)
    declared = re.findall(r"(long long|double|int)\s+([a-z_, ]+);", body)
    names = [(t, n.strip()) for t, group in declared for n in group.split(",")]
    ctype = {ctypes.c_longlong: "long long", ctypes.c_double: "double", ctypes.c_int: "int"}
    assert names == [(ctype[t], n) for n, t in capi.HealthReport._fields_]       # the same fields in the same order
    for doc, words in (("README.md", "ekf_dense64_symmetrize"), ("DESIGN.md", "4.8.17"), ("INTEGRATION.md", "ekf_dense64_symmetrize")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
