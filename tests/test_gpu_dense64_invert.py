"""-m gpu: the one numerically delicate routine of the fp64 dense handle, gj_invert / gj_quadratic
(ekf_dense64_invert.hpp: Gauss-Jordan with partial pivoting on [S | I] in LDS), looked at directly through all three of
its callers -- k_dc_invert (correct, a workgroup), k_ds_invert<256, 64> (score, m > 16) and k_ds_invert<64, 16> (score, a
wave per candidate, four per workgroup).  tests/dense_invert_cases.py builds operands for which S is exactly R and S^-1
comes back bit for bit (its docstring has the identities; test_door_* asserts them on the device first), restates the
elimination over Fraction / float64 / long double, and supplies the matrices; tests/test_dense64_invert_host.py holds all
of that to numpy and mpmath without a GPU.

Here: matrices on which every step is exact (signed scaled permutations, the same with a nilpotent E so that the update
does real work above and below the diagonal, a zero diagonal, exact ties whose wrong winner overflows) must give the
Fraction run's inverse, state' and nis bit for bit at m = 1 .. 64 including 31 / 32 / 33 and 63; the three callers must
give the same bits on general matrices, at every fill of the wave path's last workgroup and every slot, next to flagged
neighbours; the error against a long-double inverse must stay below max(8 * LAPACK's error, kappa_2 * 2^-52) for
kappa = 1e2 .. 1e12 (and below FP64_TOL up to 1e6); and the verdict must be 1 for an exactly rank-deficient S that fails
late, +-Inf / NaN in R, an inverse that overflows (wholly or in one entry), and 0 with exact results for 2^-1000 P and the
subnormal 2^-1023 P.  Equality is numpy's ==: a zero's sign is not compared (the door returns 0 - x).

Worst values seen on the MI355X (printed by test_zz_report): NOT YET RECORDED -- this file has not been run on the device.
What is recorded (profiles/r08/dense64_invert_accuracy.txt) is the fp64 run of the restatement standing in for the handle
on the same matrices: worst err / (kappa_2 * 2^-52) general 0.171 | spd 0.158 | graded 0.153, LAPACK 0.159 | 0.143 |
0.153, 0 .. 61 row swaps (none for spd at kappa = 1e2, m = 33 and 64; at least one for every m >= 5, kappa >= 1e6)."""
import numpy as np
import pytest

import dense_invert_cases as ic
from fractions import Fraction
from parity import FP64_TOL

pytestmark = pytest.mark.gpu
WORST = {}
RATIO = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))
    print(f"{key}: {v:.3e}")


class Door:
    """a handle of size N with the door's Sigma: correct() and score() of an m x m matrix R"""

    def __init__(self, hip, N, m):
        self.hip, self.N, self.m = hip, N, m
        self.H, self.Sigma = ic.door(N, m)
        self.d = hip.DensePropagator64(N)

    def correct(self, R, nu):
        """-> X, w, nis; asserts that nothing but the S^-1 block and its part of the state moved"""
        self.d.set(Sigma=self.Sigma)
        self.d.state = np.zeros(self.N)
        nis, _ = self.d.correct(self.H, R, nu)
        X, w, untouched = ic.through_the_door(self.Sigma, self.d.sigma, self.d.state, self.m)
        assert untouched, "correct() through the door moved something outside Sigma[m:2m, m:2m] / state[m:2m]"
        return X, w, nis

    def correct_refused(self, R, nu):
        """status 5, Sigma and state (set to something nonzero) untouched"""
        x = np.arange(1.0, self.N + 1.0)
        self.d.set(Sigma=self.Sigma)
        self.d.state = x
        with pytest.raises(self.hip.EkfError) as e:
            self.d.correct(self.H, R, nu)
        assert e.value.status == 5                                 # EKF_ERR_STATE
        assert np.array_equal(self.d.sigma, self.Sigma) and np.array_equal(self.d.state, x)

    def score(self, Rs, nus):
        """Rs (J, m, m), nus (J, m) -> nis (J,), flags (J,); asserts S_out == R wherever R is finite"""
        Rs, nus = np.asarray(Rs), np.asarray(nus)
        self.d.set(Sigma=self.Sigma)
        nis, S, flags, _ = self.d.score(np.stack([self.H] * len(Rs)), Rs, nus, want_S=True)
        fin = np.isfinite(Rs)
        assert np.array_equal(S[fin], Rs[fin]) and not np.isfinite(S[~fin]).any()
        return nis, flags

    def close(self):
        self.d.close()


def _sizes_N(m):
    return [2 * m, ic.BIG_N]


# ---- 1: the door on the device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", sorted(set(ic.SIZES) | set(ic.ACC_SIZES) | {7, 40}))
def test_door_identities_on_the_device(hip, m):
    """S_out == R bitwise from score (with the door's Sigma and with Sigma = 0), the untouched parts of Sigma and of the
    state bitwise from correct, for a general R"""
    R = ic.svd_matrix(m, 1e2, 3, False)
    nu = ic.accuracy_nu(m, 3)
    for N in _sizes_N(m):
        g = Door(hip, N, m)
        X, w, nis = g.correct(R, nu)                                 # asserts the untouched parts
        snis, flags = g.score([R, R.T], [nu, nu])                    # asserts S_out == R
        g.d.set(Sigma=np.zeros((N, N)))
        _, S, f0, _ = g.d.score(g.H[None], R, nu[None], want_S=True)
        g.close()
        assert np.array_equal(S[0], R) and not flags.any() and not f0.any()
        assert np.isfinite(X).all() and np.isfinite(w).all() and np.isfinite(nis) and np.isfinite(snis).all()


# ---- 2: the elimination in exact arithmetic ----------------------------------------------------------------------------

def _check_exact(g, name, R, nu, want=None):
    r = want if want is not None else ic.eliminate(R, nu, Fraction)
    assert r["verdict"] == 0 and r["inexact"] == 0 and ic.sums_exact(r["X"], nu), name   # (also held on the CPU side)
    wX, ww, wn = ic.as_float(r["X"]), ic.as_float(r["w"]), float(r["nis"])
    X, w, nis = g.correct(R, nu)
    bad = X != wX
    assert not bad.any(), f"{name} m={g.m} N={g.N}: {bad.sum()} wrong elements of S^-1, first at {np.argwhere(bad)[0]}"
    assert np.array_equal(w, ww), f"{name} m={g.m} N={g.N}: state'"
    assert nis == wn, f"{name} m={g.m} N={g.N}: nis {nis} != {wn} (correct)"
    snis, flags = g.score([R], [nu])
    assert flags[0] == 0 and snis[0] == wn, f"{name} m={g.m} N={g.N}: nis {snis[0]} != {wn} (score)"
    return r


@pytest.mark.parametrize("m", ic.SIZES)
def test_exact_families_bit_for_bit(hip, m):
    """-S^-1, state' and nis (correct and score) equal the Fraction run's, bit for bit"""
    rng = np.random.default_rng(m)
    cases = [(name, R, ic.exact_nu(m, rng)) for name, R in ic.exact_families(m, 0)]
    want = [ic.eliminate(R, nu, Fraction) for _, R, nu in cases]
    for N in _sizes_N(m):
        g = Door(hip, N, m)
        for (name, R, nu), r in zip(cases, want):
            _check_exact(g, name, R, nu, r)
        g.close()


@pytest.mark.parametrize("m", [m for m in ic.SIZES if m >= 2])
def test_exact_ties_lowest_row_wins(hip, m):
    """+a and -a in two rows, a in three rows of one pivot column: the Fraction run's pivot list says the lowest row wins;
    any other winner's scaled row holds 2^1040 = Inf, so the device's verdict and bits show which row it took.  nu is a
    multiple of one unit vector per call (the inverse spans 2^-520 .. 2^520, so only single-term sums are exact)."""
    g = Door(hip, 2 * m, m)
    for name, R, rows in ic.tie_cases(m):
        for j, k in zip(rows, (3.0, -2.0, 5.0)):
            nu = np.zeros(m)
            nu[j] = k
            r = _check_exact(g, name, R, nu)
            assert r["pivots"][rows[0]] == (rows[0], rows[0])
    g.close()


# ---- 3: the three callers give the same bits ---------------------------------------------------------------------------

def _general(m, seed, kappa=1e6):
    return ic.svd_matrix(m, kappa, seed, False), ic.accuracy_nu(m, seed)


@pytest.mark.parametrize("m", [1, 2, 7, 16, 17, 40, 64])
def test_correct_and_score_give_the_same_nis_bits(hip, m):
    """k_dc_invert (256 threads) against k_ds_invert (a wave up to m = 16, a workgroup above) on a general R: S = R on both
    sides, so the order in which S was summed is no excuse"""
    for N in _sizes_N(m):
        g = Door(hip, N, m)
        for seed in (10, 11):
            R, nu = _general(m, seed)
            _, _, nis = g.correct(R, nu)
            snis, flags = g.score([R], [nu])
            assert flags[0] == 0 and snis[0] == nis, (m, N, seed, snis[0], nis)
        g.close()


@pytest.mark.parametrize("m", [1, 2, 7, 16])
def test_wave_path_every_fill_and_every_slot(hip, m):
    """J = 1, 2, 3, 4, 5, 7 leave 3, 2, 1, 0, 3, 1 of the last workgroup's four slots empty; rolling the batch puts every
    candidate at every cand % 4"""
    g = Door(hip, 2 * m, m)
    Rs, nus = map(np.stack, zip(*[_general(m, 20 + j) for j in range(7)]))
    alone = np.array([g.score(Rs[j:j + 1], nus[j:j + 1])[0][0] for j in range(7)])
    assert np.isfinite(alone).all()
    for J in (1, 2, 3, 4, 5, 7):
        nis, flags = g.score(Rs[:J], nus[:J])
        assert not flags.any() and np.array_equal(nis, alone[:J]), J
    for shift in (1, 2, 3):
        nis, flags = g.score(np.roll(Rs, shift, axis=0), np.roll(nus, shift, axis=0))
        assert not flags.any() and np.array_equal(nis, np.roll(alone, shift)), shift
    g.close()


def _bad_R(m, why):
    R = ic.svd_matrix(m, 1e2, 40, False)
    if why == "singular":
        return ic.rank_deficient(m, 0, "equal_rows") if m >= 3 else np.zeros((m, m))
    R[0, m - 1] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[why]     # off the diagonal for m >= 2
    return R


@pytest.mark.parametrize("m", [2, 7, 16, 17])
def test_flagged_candidates_share_a_workgroup_with_a_good_one(hip, m):
    """a singular, a NaN and an Inf candidate in three of the four slots of the first workgroup, the good one in each slot
    in turn: its nis is the bits it has alone, the three have flag 1 and NaN, the next workgroup is unaffected"""
    g = Door(hip, 2 * m, m)
    Rs, nus = map(np.stack, zip(*[_general(m, 30 + j) for j in range(5)]))
    alone = np.array([g.score(Rs[j:j + 1], nus[j:j + 1])[0][0] for j in range(5)])
    bad = [_bad_R(m, w) for w in ("singular", "nan", "inf")]
    for slot in range(4):
        first = bad[:slot] + [Rs[0]] + bad[slot:]
        nis, flags = g.score(np.stack(first + list(Rs[1:])), np.concatenate([np.stack([nus[0]] * 4), nus[1:]]))
        want = np.ones(8, dtype=bool)
        want[slot] = False
        want[4:] = False
        assert np.array_equal(flags.astype(bool), want), (slot, flags)
        assert np.isnan(nis[want]).all() and nis[slot] == alone[0] and np.array_equal(nis[4:], alone[1:]), slot
    g.close()


# ---- 4: accuracy against a long-double inverse -------------------------------------------------------------------------

@pytest.mark.parametrize("m", ic.ACC_SIZES)
def test_accuracy_against_long_double(hip, m):
    """err = max |X - X_true| / max |X_true| <= max(8 err_lapack, kappa_2 2^-52); state' against X_true nu relative to
    max |X_true| max |nu| with one factor m; nis relative to |nu|^T |X_true| |nu| (nis itself can cancel); through correct
    and, for nis, through score.  Up to kappa = 1e6 also err <= FP64_TOL.  Truth: the long-double run of the restatement
    (held to mpmath on the CPU side)."""
    g = Door(hip, 2 * m, m)
    for fam, mm, kappa, seed, R in ic.accuracy_cases():
        if mm != m:
            continue
        nu = ic.accuracy_nu(m, seed)
        t = ic.truth(R, nu)
        Xt = t["X"]
        bound, e_lapack, k2 = ic.accuracy_bound(R, Xt)
        swaps = ic.eliminate(R, None, np.float64)["swaps"]
        X, w, nis = g.correct(R, nu)
        snis, flags = g.score([R], [nu])
        assert flags[0] == 0 and snis[0] == nis
        ld = np.longdouble
        e_X = ic.rel_err(X, Xt)
        e_w = float(np.abs(w.astype(ld) - t["w"]).max() / (np.abs(Xt).max() * np.abs(nu).max()))
        e_n = float(abs(ld(nis) - t["nis"]) / (np.abs(nu).astype(ld) @ np.abs(Xt) @ np.abs(nu).astype(ld)))
        key = f"{fam} m={m} kappa={kappa:g}" if kappa else f"{fam} m={m}"
        print(f"{key} seed={seed} kappa2={k2:.2e}: device err/(kappa u) {e_X / (k2 * ic.U52):.3f}  LAPACK "
              f"{e_lapack / (k2 * ic.U52):.3f}  state {e_w / (k2 * ic.U52):.3f}  nis {e_n / (k2 * ic.U52):.3f}  "
              f"swaps {swaps}")
        rec = RATIO.setdefault(key, [0.0, 0.0, 0])
        rec[0], rec[1], rec[2] = max(rec[0], e_X / (k2 * ic.U52)), max(rec[1], e_lapack / (k2 * ic.U52)), max(rec[2], swaps)
        assert e_X <= bound, (key, seed, e_X, bound)
        assert e_w <= m * bound, (key, seed, e_w, m * bound)
        assert e_n <= bound, (key, seed, e_n, bound)
        if kappa is not None and kappa <= 1e6:
            _note("contract_inverse", e_X); _note("contract_state", e_w / m); _note("contract_nis", e_n)
            assert e_X <= FP64_TOL and e_w <= m * FP64_TOL and e_n <= FP64_TOL, (key, seed, e_X, e_w, e_n)
    g.close()


# ---- 5: the verdict ----------------------------------------------------------------------------------------------------

def _refused_everywhere(g, R, nu):
    """correct: status 5 with Sigma and state untouched, and the handle works on the next call; score: flag 1 and NaN
    between two good neighbours whose bits do not change"""
    m = g.m
    good, gnu = _general(m, 50)
    X0, w0, n0 = g.correct(good, gnu)
    g.correct_refused(R, nu)
    X1, w1, n1 = g.correct(good, gnu)
    assert np.array_equal(X0, X1) and np.array_equal(w0, w1) and n0 == n1
    nis, flags = g.score([good, R, good], [gnu, nu, gnu])
    assert list(flags) == [0, 1, 0] and np.isnan(nis[1]) and nis[0] == n0 and nis[2] == n0


VERDICT_M = [5, 16, 17, 40]


@pytest.mark.parametrize("how", ["equal_rows", "sum_of_two"])
@pytest.mark.parametrize("m", VERDICT_M)
def test_rank_deficient_late_is_flagged(hip, m, how):
    """an exact zero column that only appears at step p > 0 (the Fraction run says where; every step before it is exact)"""
    R = ic.rank_deficient(m, 0, how)
    r = ic.eliminate(R, None, Fraction)
    assert r["verdict"] == 1 and r["step"] > 0 and r["inexact"] == 0
    g = Door(hip, 2 * m, m)
    _refused_everywhere(g, R, np.ones(m))
    g.close()


@pytest.mark.parametrize("what", ["inf", "-inf", "nan"])
@pytest.mark.parametrize("m", VERDICT_M)
def test_nonfinite_R_is_flagged(hip, m, what):
    g = Door(hip, 2 * m, m)
    _refused_everywhere(g, _bad_R(m, what), np.ones(m))
    g.close()


@pytest.mark.parametrize("m", VERDICT_M)
def test_overflowed_inverse_is_flagged(hip, m):
    """2^-1060 I: subnormal and nonzero, the pivot test passes and 1 / pivot is Inf; and a matrix whose pivots are all 1
    and whose inverse overflows in one entry only"""
    g = Door(hip, 2 * m, m)
    for R in (np.eye(m) * 2.0 ** -1060, ic.overflow_one_entry(m)):
        assert ic.eliminate(R, None, np.float64)["step"] == m      # every pivot passes, the inverse is not finite
        _refused_everywhere(g, R, np.ones(m))
    g.close()


@pytest.mark.parametrize("e", [-1000, -1023])
@pytest.mark.parametrize("m", VERDICT_M)
def test_finite_neighbours_are_not_flagged(hip, m, e):
    """2^-1000 P has the finite inverse 2^1000 P^T: flag 0 and exact; the same for 2^-1023 P, whose pivots are subnormal.
    nu = 2^-520 x small integers keeps nis (about 2^-1040 2^1000) finite; with an oversized nu an infinite nis with flag 0
    is the documented behaviour (the flag speaks of S alone)."""
    P = ic.permutation(m, 1)
    R = P * 2.0 ** e
    nu = np.random.default_rng(m).integers(1, 4, size=m) * 2.0 ** -520
    g = Door(hip, 2 * m, m)
    X, w, nis = g.correct(R, nu)
    snis, flags = g.score([R], [nu])
    g.close()
    Xw = P.T * 2.0 ** -e
    assert np.array_equal(X, Xw) and np.array_equal(w, Xw @ nu) and flags[0] == 0
    assert nis == float(nu @ (Xw @ nu)) == snis[0] and np.isfinite(nis)     # one term per row, small integers: exact


@pytest.mark.parametrize("m", VERDICT_M)
def test_nearly_singular_is_the_same_everywhere(hip, m):
    """kappa ~ 1e15, not exactly singular: the header promises a flag only for zero or non-finite pivots, so no verdict is
    asserted -- only that verdict and nis are the same bits on all three callers and from run to run"""
    R, nu = _general(m, 60, kappa=1e15)
    g = Door(hip, 2 * m, m)
    runs = []
    for _ in range(2):
        try:
            _, _, nis = g.correct(R, nu)
            c = (0, nis)
        except hip.EkfError as e:
            assert e.value.status == 5
            c = (1, float("nan"))
        nis1, f1 = g.score([R], [nu])
        nis4, f4 = g.score([R] * 4, [nu] * 4)
        runs.append([c, (int(f1[0]), float(nis1[0]))] + [(int(f), float(v)) for f, v in zip(f4, nis4)])
    g.close()
    flat = runs[0] + runs[1]
    assert all(f == flat[0][0] for f, _ in flat), flat
    assert all(np.array([v]).view(np.uint64)[0] == np.array([flat[0][1]]).view(np.uint64)[0] or
               (np.isnan(v) and np.isnan(flat[0][1])) for _, v in flat), flat


def test_zz_report():
    for k in sorted(WORST):
        print(f"dense64 invert worst {k}: {WORST[k]:.3e}")
    print("dense64 invert  family / m / kappa : device err/(kappa_2 2^-52) | LAPACK | most swaps")
    for k in RATIO:
        print(f"dense64 invert  {k:28s}: {RATIO[k][0]:8.3f} | {RATIO[k][1]:8.3f} | {RATIO[k][2]}")
    fams = sorted({k.split()[0] for k in RATIO})
    for f in fams:
        v = [RATIO[k] for k in RATIO if k.split()[0] == f]
        print(f"dense64 invert worst {f}: device {max(x[0] for x in v):.3f}  LAPACK {max(x[1] for x in v):.3f}")
    assert all(v <= FP64_TOL for v in WORST.values())
