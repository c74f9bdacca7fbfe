"""CPU (not gpu): what tests/test_gpu_dense64_invert.py takes for granted about tests/dense_invert_cases.py -- the door
identities in numpy, the restatement of the elimination against numpy.linalg.inv and mpmath at 50 digits, the self-check
that every exact family really is exact in fp64 (so a family that needs rounding fails here, not silently on the GPU), the
tie matrices' power to tell the tie rule, and the preconditions of the accuracy families (a row swap happens, nothing
overflows, the long-double truth is three orders inside the bound)."""
from fractions import Fraction

import numpy as np
import pytest

import dense_correct_cases as dc
import dense_invert_cases as ic
import dense_score_cases as ds


# ---- 1: the door -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,N", [(1, 2), (3, 6), (5, 300), (17, 34), (64, 128), (64, 300)])
def test_door_identities_in_numpy(m, N):
    rng = np.random.default_rng(m + N)
    R = rng.normal(size=(m, m))
    nu = rng.normal(size=m)
    H, Sigma = ic.door(N, m)
    assert np.array_equal(H @ Sigma @ H.T + R, R)                      # S == R bit for bit
    x1, S1, nis = dc.np_correct(np.zeros(N), Sigma, H, R, nu)
    X, w, untouched = ic.through_the_door(Sigma, S1, x1, m)
    Ri = np.linalg.inv(R)
    assert untouched and np.array_equal(X, Ri)                          # the inverse itself, bit for bit
    # state' and nis are sums of the same terms in whatever order the BLAS takes them
    scale = np.abs(Ri) @ np.abs(nu)
    assert (np.abs(w - Ri @ nu) <= 1e-14 * scale).all() and abs(nis - nu @ Ri @ nu) <= 1e-14 * (np.abs(nu) @ scale)
    S, snis = ds.np_scores(Sigma, H[None], R, nu[None])
    assert np.array_equal(S[0], R) and abs(snis[0] - nis) <= 1e-14 * (np.abs(nu) @ scale)
    S, _ = ds.np_scores(np.zeros((N, N)), H[None], R)
    assert np.array_equal(S[0], R)


# ---- 2: the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("number", [np.float64, np.longdouble])
def test_restatement_against_numpy(number):
    for m in (1, 2, 3, 7, 16, 33, 64):
        rng = np.random.default_rng(m)
        R = rng.normal(size=(m, m))
        nu = rng.normal(size=m)
        r = ic.eliminate(R, nu, number)
        Ri = np.linalg.inv(R)
        assert r["verdict"] == 0 and len(r["pivots"]) == m
        assert ic.rel_err(r["X"], Ri) <= np.linalg.cond(R) * 2.0 ** -48, m
        assert abs(float(r["nis"]) - float(nu @ Ri @ nu)) <= 1e-9 * float(np.abs(nu) @ np.abs(Ri) @ np.abs(nu))
        # the pivot rule: the largest magnitude at or below the diagonal, on the matrix of that step
        assert r["pivots"][0][1] == int(np.argmax(np.abs(R[:, 0])))


def test_restatement_in_fractions_is_the_inverse():
    for m in (1, 2, 5, 9):
        R = np.random.default_rng(m).integers(-4, 5, size=(m, m)).astype(np.float64) + 7.0 * np.eye(m)
        nu = np.arange(1.0, m + 1.0)
        r = ic.eliminate(R, nu, Fraction)
        X = r["X"]
        prod = [[sum(Fraction(R[i, k]) * X[k, j] for k in range(m)) for j in range(m)] for i in range(m)]
        assert r["verdict"] == 0 and prod == [[Fraction(int(i == j)) for j in range(m)] for i in range(m)]
        assert r["nis"] == sum(Fraction(nu[k]) * X[k, l] * Fraction(nu[l]) for k in range(m) for l in range(m))
        f = ic.eliminate(R, nu, np.float64)
        assert f["pivots"] == r["pivots"]


def _mp_inverse(R):
    import mpmath
    with mpmath.workdps(50):
        Xi = mpmath.matrix(R.tolist()) ** -1
        return np.array([[np.longdouble(mpmath.nstr(Xi[i, j], 30)) for j in range(len(R))] for i in range(len(R))])


def test_restatement_and_truth_against_mpmath():
    """the long-double run that serves as truth sits at kappa * 2^-60 or closer to the 50-digit inverse: 256 times inside
    the kappa * 2^-52 it judges (64 significand bits against 53, and a constant of 16 for the elimination itself -- the
    fp64 run of the same code stays below 1 in that unit)"""
    cases = [c for c in ic.accuracy_cases() if c[1] <= 17 and c[3] == 0]
    cases.append(("general", 64, 1e10, 0, ic.svd_matrix(64, 1e10, 0, False)))
    worst = 0.0
    for fam, m, kappa, seed, R in cases:
        Xmp = _mp_inverse(R)
        k2 = float(np.linalg.cond(R, 2))
        e_ld = ic.rel_err(ic.truth(R)["X"], Xmp)
        e_f64 = ic.rel_err(ic.eliminate(R, None, np.float64)["X"], Xmp)
        worst = max(worst, e_ld / (k2 * 2.0 ** -60))
        assert e_ld <= k2 * 2.0 ** -60, (fam, m, kappa, e_ld)
        assert e_f64 <= k2 * ic.U52, (fam, m, kappa, e_f64)
    print(f"long-double truth vs mpmath: worst err / (kappa 2^-60) = {worst:.3f}")


# ---- 2: the exact families ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ic.SIZES)
def test_exact_families_are_exact(m):
    """every value the elimination produces (products included) is a double, the fp64 run of the restatement gives the
    same pivots and the same bits, state' and nis are exact in any order of summation, and every column of a permutation
    family needs a swap"""
    rng = np.random.default_rng(m)
    negative = 0
    for name, R in ic.exact_families(m, 0):
        nu = ic.exact_nu(m, rng)
        r = ic.eliminate(R, nu, Fraction)
        assert r["verdict"] == 0 and r["inexact"] == 0, (name, r["inexact"])
        assert ic.sums_exact(r["X"], nu), name
        f = ic.eliminate(R, nu, np.float64)
        assert f["pivots"] == r["pivots"]
        assert np.array_equal(f["X"], ic.as_float(r["X"])) and float(f["nis"]) == float(r["nis"])
        if m >= 2:
            assert r["swaps"] >= 1, name
            negative += sum(R[pr, p] < 0 for p, pr in r["pivots"] if np.count_nonzero(R[:, p]) == 1)
        if name == "cyclic" and m >= 2:
            assert not np.diag(R).any() and r["swaps"] == m - 1
        if name.startswith("perm_nilpotent") and m >= 4:
            assert (np.count_nonzero(R, axis=0) > 1).any()                       # the update does real work
    assert negative >= 1 or m < 3                                                # some pivots are negative


@pytest.mark.parametrize("m", [m for m in ic.SIZES if m >= 2])
def test_tie_matrices_tell_the_tie_rule(m):
    for name, R, rows in ic.tie_cases(m):
        c0 = rows[0]
        r = ic.eliminate(R, None, Fraction)
        assert r["verdict"] == 0 and r["inexact"] == 0 and r["pivots"][c0] == (c0, c0), name
        col = np.abs(R[c0:, c0])
        assert (col == col.max()).sum() == len(rows)                             # an exact tie among these rows
        f = ic.eliminate(R, None, np.float64)
        assert f["verdict"] == 0 and np.array_equal(f["X"], ic.as_float(r["X"]))
        assert ic.eliminate(R, None, np.float64, tie_highest=True)["verdict"] == 1, name


@pytest.mark.parametrize("how", ["equal_rows", "sum_of_two"])
@pytest.mark.parametrize("m", [5, 16, 17, 40])
def test_rank_deficient_matrices_fail_late_and_exactly(m, how):
    R = ic.rank_deficient(m, 0, how)
    r = ic.eliminate(R, None, Fraction)
    f = ic.eliminate(R, None, np.float64)
    assert r["verdict"] == 1 and r["step"] is not None and r["step"] > 0 and r["inexact"] == 0
    assert f["verdict"] == 1 and f["step"] == r["step"] and f["pivots"] == r["pivots"]
    assert np.linalg.matrix_rank(R) == m - 1


# ---- 4: preconditions of the accuracy families -------------------------------------------------------------------------

def test_accuracy_families_swap_and_stay_finite():
    """for every m >= 5 and kappa >= 1e6 the elimination swaps rows at least once and its largest intermediate is finite;
    kappa_2 of the svd families is what was asked for"""
    seen = {}
    for fam, m, kappa, seed, R in ic.accuracy_cases():
        r = ic.eliminate(R, None, np.float64)
        assert r["verdict"] == 0 and np.isfinite(r["big"]), (fam, m, kappa, seed)
        if kappa is not None:
            assert abs(np.linalg.cond(R, 2) / kappa - 1.0) < 1e-3 or m == 1 or kappa >= 1e10, (fam, m, kappa)
            if m >= 5 and kappa >= 1e6:
                assert r["swaps"] >= 1, (fam, m, kappa, seed)
        key = (fam, m, kappa)
        seen[key] = max(seen.get(key, 0), r["swaps"])
    for key in sorted(seen, key=str):
        print(f"swaps {key}: {seen[key]}")


def test_verdict_matrices():
    for m in (5, 17):
        assert ic.eliminate(np.eye(m) * 2.0 ** -1060, None, np.float64)["step"] == m     # 1 / pivot overflows
        o = ic.eliminate(ic.overflow_one_entry(m), None, np.float64)
        assert o["verdict"] == 1 and o["step"] == m and [pr for _, pr in o["pivots"]] == list(range(m))
        X = ic.eliminate(ic.overflow_one_entry(m), None, Fraction)["X"]
        assert sum(abs(v) >= 2 ** 1024 for v in X.reshape(-1)) == 1
        for e in (-1000, -1023):
            P = ic.permutation(m, 0)
            r = ic.eliminate(P * 2.0 ** e, None, np.float64)
            assert r["verdict"] == 0 and np.array_equal(r["X"], P.T * 2.0 ** -e)
