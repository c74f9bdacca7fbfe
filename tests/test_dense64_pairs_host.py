"""CPU (not gpu): the definition behind ekf_dense64_score_landmark_pairs and ekf_dense64_merge_landmarks.  The op-by-op numpy
model of a pair's score (dense_pairs_cases) builds the S that dense_sparse_cases' model of score_sparse builds, bit for
bit, and through the same elimination the same nis; d2(a, b) = d2(b, a) in bits; on the integer family S is exact; the
random family is conditioned and separated well enough that the model stays within FP64_TOL of a long-double evaluation
and no argmin can flip; the wrapper's argument checks fire before the library is called."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dense_invert_cases as di
import dense_pairs_cases as pc
import dense_sparse_cases as sp
from parity import FP64_TOL
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(5, 13), (9, 26)]   # (n_lm, N): a full corner, and one with a tail


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _families(n_lm, N):
    yield "integers", pc.integer_family(n_lm, N, 11 + n_lm)
    yield "random", pc.random_family(n_lm, N, 23 + n_lm)
    yield "degenerate", pc.degenerate_family(n_lm, N, 37 + n_lm)[:2]


@pytest.mark.parametrize("n_lm,N", CASES)
def test_model_is_the_sparse_model_in_bits(n_lm, N):
    """S: the bits of dense_sparse_cases.np_scores (the embedded H has two non-zero entries a row, so each of its sums
    rounds once whatever the order).  nis: np_scores inverts with LAPACK, the device eliminates; the model of score_sparse's
    nis is that S through dense_invert_cases.eliminate, and the pair model has its bits; LAPACK's value agrees to FP64_TOL
    where S is regular."""
    for name, (state, Sigma) in _families(n_lm, N):
        for r_merge in pc.R_MERGES:
            for a, b in pc.all_pairs(n_lm):
                cols, Hc, R, nu = pc.pair_operands(state, a, b, r_merge)
                d2, flag, S = pc.model_score(Sigma, state, a, b, r_merge)
                G, own = Sigma[np.ix_(cols, cols)], np.arange(4)[None]   # (the 4 x 4 block: a NaN elsewhere in Sigma is not the pair's)
                with np.errstate(all="ignore"):
                    try:
                        S_ref, nis_ref = sp.np_scores(G, own, Hc[None], R, nu[None])
                    except np.linalg.LinAlgError:
                        S_ref, nis_ref = sp.np_scores(G, own, Hc[None], R)[0], None
                if np.isfinite(S).all():
                    assert np.array_equal(_bits(S + 0.0), _bits(S_ref[0] + 0.0)), (name, a, b)   # (+ 0.0: -0 and +0 are one)
                e = di.eliminate(S_ref[0], nu)
                assert flag == e["verdict"]
                if not flag:
                    assert _bits(d2) == _bits(e["nis"])
                    if name != "degenerate" and nis_ref is not None:
                        assert abs(d2 - nis_ref[0]) <= FP64_TOL * max(abs(nis_ref[0]), 1e-3)


@pytest.mark.parametrize("n_lm,N", CASES)
def test_score_is_symmetric_in_bits(n_lm, N):
    for name, (state, Sigma) in _families(n_lm, N):
        for r_merge in pc.R_MERGES:
            for a, b in pc.all_pairs(n_lm):
                d_ab, f_ab, _ = pc.model_score(Sigma, state, a, b, r_merge)
                d_ba, f_ba, _ = pc.model_score(Sigma, state, b, a, r_merge)
                assert f_ab == f_ba and (f_ab or _bits(d_ab) == _bits(d_ba)), (name, a, b, r_merge)


@pytest.mark.parametrize("n_lm,N", CASES)
def test_integer_family_S_is_exact(n_lm, N):
    state, Sigma = pc.integer_family(n_lm, N, 11 + n_lm)
    asym = 0
    for r_merge in pc.R_MERGES:
        for a, b in pc.all_pairs(n_lm):
            cols, Hc, R, _ = pc.pair_operands(state, a, b, r_merge)
            S = pc.model_S(Sigma, cols, Hc, R)
            G = [[Fraction(float(Sigma[i, j])) for j in cols] for i in cols]
            h = [[Fraction(int(v)) for v in row] for row in Hc]
            for i in range(2):
                for j in range(2):
                    want = sum(h[i][k] * G[k][l] * h[j][l] for k in range(4) for l in range(4)) + Fraction(float(R[i, j]))
                    assert Fraction(float(S[i, j])) == want
            asym += int(S[0, 1] != S[1, 0])
    assert asym > 0, "the family must exercise Sigma_ab != Sigma_ba^T"


@pytest.mark.parametrize("n_lm,N", [(9, 26), (33, 69), (66, 140)])
def test_random_family_is_conditioned_and_separated(n_lm, N):
    """kappa_2(S) <= 1e4 for every pair and every winner >= 1e-6 (relative) ahead of its runner-up; so the float64 model is
    within FP64_TOL of the elimination in long double (kappa * 2^-52 ~ 2e-12 per operation) and no argmin can flip"""
    state, Sigma = pc.random_family(n_lm, N, 23 + n_lm)
    worst = 0.0
    for r_merge in (0.5, 4.0):
        pairs = pc.all_pairs(n_lm)
        scores = np.empty(len(pairs))
        for q, (a, b) in enumerate(pairs):
            d2, flag, S = pc.model_score(Sigma, state, a, b, r_merge)
            assert not flag and np.linalg.cond(S) <= 1e4
            wide = pc.model_score(Sigma, state, a, b, r_merge, number=np.longdouble)[0]
            worst = max(worst, abs(float(wide) - d2) / max(abs(d2), 1e-3))
            scores[q] = d2
        table = np.full((n_lm, n_lm), np.inf)
        for (a, b), d in zip(pairs, scores):
            table[a, b] = table[b, a] = d
        two = np.sort(table, axis=1)[:, :2]
        assert np.all(two[:, 1] - two[:, 0] >= 1e-6 * np.abs(two[:, 1]))
    assert worst <= FP64_TOL


def test_degenerate_family_holds_its_cases():
    state, Sigma, what = pc.degenerate_family(9, 26, 46)
    assert what == ["copy", "nan", "tie"]
    assert pc.model_score(Sigma, state, 0, 1, 0.0)[1] == 1 and pc.model_score(Sigma, state, 0, 1, 0.5)[:2] == (0.0, 0)
    assert all(pc.model_score(Sigma, state, min(2, o), max(2, o), 0.5)[1] == 1 for o in range(9) if o != 2)
    d34, d35 = pc.model_score(Sigma, state, 3, 4, 0.5)[0], pc.model_score(Sigma, state, 3, 5, 0.5)[0]
    assert _bits(d34) == _bits(d35)
    nearest, d2, below, flagged = pc.model_scan(Sigma, state, 9, 0.5, 1.0)
    assert nearest[3] == 4 and _bits(d2[3]) == _bits(d34) and flagged == 8 and nearest[2] == -1 and d2[2] == np.inf
    nearest0 = pc.model_scan(Sigma, state, 9, 0.0, 1.0)
    assert nearest0[3] == 9 and nearest0[0][0] != 1   # the copy is flagged at r_merge = 0 and never wins


def test_merge_model_fuses_and_deletes():
    state, Sigma = pc.random_family(6, 15, 5)
    s1, S1, known, moved, d2 = pc.np_merge(state, Sigma, 6, 1, 0, 0.5)
    assert known == 5 and moved == 5 and d2 == pytest.approx(pc.model_score(Sigma, state, 0, 1, 0.5)[0], rel=1e-9)
    assert np.all(np.abs(s1[3:5] - state[3:5]) <= np.abs(state[5:7] - state[3:5]) + 1e-12)   # between the two copies
    assert np.array_equal(S1[13:15, 13:15], 100.0 * np.eye(2)) and not S1[13:15, :13].any() and not S1[:13, 13:15].any()
    assert np.trace(S1[3:5, 3:5]) < np.trace(Sigma[3:5, 3:5])
    assert pc.np_merge(state, Sigma, 6, 2, 5, 0.5)[3] == -1


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_checks_come_before_the_library():
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = 30, _NoLibrary(), None
    bad = [lambda: d.landmark_pairs(0, 0.5), lambda: d.landmark_pairs(14, 0.5), lambda: d.landmark_pairs(5, -1.0),
           lambda: d.landmark_pairs(5, float("inf")), lambda: d.landmark_pairs(5, float("nan")),
           lambda: d.landmark_pairs(5, 0.5, float("nan")),
           lambda: d.merge_landmarks(1, 1, 0.5, 4), lambda: d.merge_landmarks(0, 4, 0.5, 4),
           lambda: d.merge_landmarks(-1, 2, 0.5, 4), lambda: d.merge_landmarks(0, 1, -0.5, 4),
           lambda: d.merge_landmarks(0, 1, 0.5, 14), lambda: d.merge_landmarks(0, 1, 0.5, 4, flags=4)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    d._lib, d._h = None, None   # (close() of the object must not reach for a library either)


def test_calls_are_declared_bound_and_documented():
    hdr = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
    for name in ("ekf_dense64_score_landmark_pairs", "ekf_dense64_merge_landmarks", "ekf_dense64_pairs_launch_info"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", hdr, re.M) and name in capi.SYMBOLS
    assert "FLUSHES THE PENDING ROWS FIRST" in hdr
    for doc, words in (("README.md", "landmark_pairs"), ("DESIGN.md", "4.8.15"), ("INTEGRATION.md", "Duplicate landmarks")):
        assert words in open(os.path.join(ROOT, doc)).read(), doc
