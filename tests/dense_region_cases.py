"""Shared by tests/test_dense64_region_host.py and tests/test_gpu_dense64_region.py: the numpy model of a local region of
the dense fp64 handle (ekf_dense64_region_begin .. ekf_dense64_region_end: the accumulators Phi, Psi, theta of the compressed
EKF and the global update), the plain full-width numpy sequence it is compared with, and the chains both run.

A chain is a list of ops in the format of tests/dense_live_cases.py ("eager", "deferred", "propagate", "init", "flush"),
every index below Na.  Two kinds:
  live_ops(Na, order, m, s)   the ops of lc.live_chain -- the chains the live dimension is tested on.  Their corner is NOT
                              symmetric (integers drawn entry by entry), so on them the region and the full-width sequence
                              differ by more than rounding OUTSIDE the corner (Sigma_ba Gamma against Sigma_ba Phi^T, the
                              note of DESIGN.md 4.8.21); they serve where only the corner is looked at.
  exact_chain(N, Na, seed)    a SYMMETRIC integer Sigma of dimension N with a coupled tail and corrections with m = 1 whose
                              R makes S a power of two: the gain is exact, and every product the model and the plain
                              sequence form goes through cc.exact_product, which refuses (Inexact) a product whose terms
                              are not integers over one power of two with the sum of their absolute values below 2^52.  On
                              these every number is exact in float64 in any order of summation, the region and the
                              full-width sequence are EQUAL, and the device has to give the same bits.
  float_chain(N, Na, seed)    an SPD Sigma with a coupled tail and general corrections: agreement within parity.FP64_TOL."""
import functools

import numpy as np

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_init_cases as ic
import dense_live_cases as lc
import dense_sparse_cases as sp

GRID_N = lc.GRID_N
GRID_NA = [3, 5, 63, 64, 65, 127, 128, 129, 191]


def pairs():
    """every (N, Na) of the grid with Na < N, and N - Na in {1, 2} once each"""
    out = [(N, Na) for N in GRID_N for Na in GRID_NA if Na < N]
    return out + [(65, 64), (66, 64), (130, 129), (131, 129), (129, 127)]


def live_ops(Na, order, m, s):
    return lc.live_chain(Na, order, m, s)


def coupled(corner, x_corner, N, seed, integer):
    """(Sigma0, x0) of dimension N around the given corner: a dense tail and NON-ZERO rectangles; symmetric outside the corner"""
    Na = len(corner)
    rng = np.random.default_rng(seed)
    S = np.zeros((N, N))
    if integer:
        B = rng.integers(-2, 3, size=(N - Na, N - Na)).astype(np.float64)
        S[Na:, Na:] = B + B.T + 64.0 * np.eye(N - Na)
        C = rng.integers(-2, 3, size=(Na, N - Na)).astype(np.float64)
        xt = rng.integers(-9, 10, size=N - Na).astype(np.float64)
    else:
        A = rng.normal(size=(N, N))
        S = A @ A.T / N + np.eye(N)
        C = S[:Na, Na:].copy()
        xt = rng.normal(size=N - Na)
    S[:Na, Na:], S[Na:, :Na] = C, C.T
    S[:Na, :Na] = corner
    return S, np.concatenate([x_corner, xt])


# ---- the two models --------------------------------------------------------------------------------------------------------

def _mm(exact):
    return cc.exact_product if exact else (lambda A, B, C=None: A @ B if C is None else A @ B + C)


def _gain(S, cols, Hc, R, exact):
    """T, S^-1 and K of a sparse correction on S (any dimension), the way the handle forms them"""
    mm = _mm(exact)
    T = mm(Hc, S[cols, :])
    U = mm(S[:, cols], Hc.T)
    Sm = mm(T[:, cols], Hc.T, R)
    if exact:
        assert Sm.shape == (1, 1) and np.log2(Sm[0, 0]) == np.floor(np.log2(Sm[0, 0])), "S must be a power of two"
        Sinv = 1.0 / Sm
    else:
        Sinv = np.linalg.inv(Sm)
    return T, Sinv, mm(U, Sinv)


def _step(x, S, op, exact):
    """one op of the plain sequence on (x, S) of any dimension -> (x, S); a flush is nothing to an eager model"""
    mm, k = _mm(exact), op["op"]
    if k in ("eager", "deferred"):
        T, Sinv, K = _gain(S, op["cols"], op["Hc"], op["R"], exact)
        return x + mm(K, op["nu"].reshape(-1, 1)).ravel(), mm(-K, T, S)
    if k == "propagate":
        if exact:
            r = len(op["Fr"])
            b = slice(op["first"], op["first"] + r)
            mm(op["Fr"], S[b, :]), mm(S[:, b], op["Fr"].T), mm(mm(op["Fr"], S[b, b]), op["Fr"].T, op["Qr"])
        return bc.np_predict_slices(x, S, op["first"], op["Fr"], op["Qr"], op["dx"])
    if k == "init":
        if exact and op["cols"] is not None:
            c = op["cols"]
            mm(op["G"], S[c, :]), mm(S[:, c], op["G"].T), mm(mm(op["G"], S[np.ix_(c, c)]), op["G"].T, op["W"])
        return ic.np_init_block(x, S, op["first"], op["r"], op["cols"], op["G"], op["W"], op["xb"])
    return x, S


def run_full(S0, x0, ops, exact=False):
    """the plain full-width numpy sequence"""
    x, S = x0.copy(), S0.copy()
    for op in ops:
        x, S = _step(x, S, op, exact)
    return x, S


class RegionModel:
    """the region: the corner runs the plain sequence at dimension Na, the accumulators take what include/ekfslam.h says
    (every update with the Phi from before the call), end() is the global update in the handle's order"""

    def __init__(self, S0, x0, Na, exact=False):
        self.S0, self.x0, self.Na, self.exact = S0.copy(), x0.copy(), Na, exact
        self.Saa, self.xa = S0[:Na, :Na].copy(), x0[:Na].copy()
        self.Phi, self.Psi, self.theta = np.eye(Na), np.zeros((Na, Na)), np.zeros(Na)
        self.corrections = self.row_maps = 0

    def apply(self, op):
        mm, k = _mm(self.exact), op["op"]
        if k in ("eager", "deferred"):
            _, Sinv, K = _gain(self.Saa, op["cols"], op["Hc"], op["R"], self.exact)
            W = mm(op["Hc"], self.Phi[op["cols"], :])
            Z = mm(Sinv, W)
            self.theta = mm(Z.T, op["nu"].reshape(-1, 1), self.theta.reshape(-1, 1)).ravel()
            self.Psi = mm(W.T, Z, self.Psi)
            self.Phi = mm(-K, W, self.Phi)
            self.corrections += 1
        elif k == "propagate":
            b = slice(op["first"], op["first"] + len(op["Fr"]))
            self.Phi[b, :] = mm(op["Fr"], self.Phi[b, :])
            self.row_maps += 1
        elif k == "init":
            b = slice(op["first"], op["first"] + op["r"])
            self.Phi[b, :] = 0.0 if op["cols"] is None else mm(op["G"], self.Phi[op["cols"], :])
            self.row_maps += 1
        self.xa, self.Saa = _step(self.xa, self.Saa, op, self.exact)

    def end(self):
        mm, Na = _mm(self.exact), self.Na
        S, x = self.S0.copy(), self.x0.copy()
        ab, ba = self.S0[:Na, Na:], self.S0[Na:, :Na]
        x[:Na], S[:Na, :Na] = self.xa, self.Saa
        x[Na:] = mm(ba, self.theta.reshape(-1, 1), self.x0[Na:].reshape(-1, 1)).ravel()
        Y = -mm(self.Psi, ab)
        S[Na:, Na:] = mm(ba, Y, self.S0[Na:, Na:])
        S[Na:, :Na] = mm(ba, self.Phi.T)
        S[:Na, Na:] = mm(self.Phi, ab)
        return x, S


def run_region(S0, x0, Na, ops, exact=False):
    model = RegionModel(S0, x0, Na, exact)
    for op in ops:
        model.apply(op)
    return model.end()


# ---- the chains ------------------------------------------------------------------------------------------------------------

def _exact_correction(S, Na, rng, s, kind):
    """m = 1, s listed columns below Na, small integer Hc, R > 0 such that S = Hc Sigma[cols, cols] Hc^T + R is 2^k"""
    cols = np.sort(rng.permutation(Na)[:s]).astype(np.int32)
    Hc = rng.choice([-1.0, 1.0], size=(1, s))
    q = float((Hc @ S[np.ix_(cols, cols)] @ Hc.T)[0, 0])
    k = max(3, int(np.floor(np.log2(max(abs(q), 1.0)))) + 2)
    return {"op": kind, "cols": cols, "Hc": Hc, "R": np.array([[2.0 ** k - q]]), "nu": rng.integers(-3, 4, size=1).astype(np.float64)}


def _build_exact(N, Na, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-1, 2, size=(Na, Na)).astype(np.float64)
    corner = A + A.T + 16.0 * np.eye(Na)
    S0, x0 = coupled(corner, rng.integers(-9, 10, size=Na).astype(np.float64), N, seed + 1, integer=True)
    ops, x, S = [], x0.copy(), S0.copy()

    def done(op):
        nonlocal x, S
        x, S = _step(x, S, op, True)
        ops.append(op)

    done(_exact_correction(S, Na, rng, min(3, Na), "eager"))
    r = min(3, Na)
    F = np.eye(r)
    F[0, r - 1] = 2.0                                             # an integer Jacobian that is not the identity
    Q = rng.integers(0, 2, size=(r, r)).astype(np.float64)
    done({"op": "propagate", "first": 0, "Fr": F, "Qr": Q + Q.T, "dx": rng.integers(-2, 3, size=r).astype(np.float64)})
    done(_exact_correction(S, Na, rng, min(2, Na), "eager"))
    if Na >= 5:                                                   # the last block of the region, from two listed states
        first = Na - 2
        src = np.sort(rng.permutation(first)[:2]).astype(np.int32)
        done({"op": "init", "first": first, "r": 2, "cols": src, "G": rng.integers(-1, 2, size=(2, 2)).astype(np.float64),
              "W": 4.0 * np.eye(2), "xb": rng.integers(-9, 10, size=2).astype(np.float64)})
    x2, S2 = run_region(S0, x0, Na, ops, exact=True)              # raises Inexact too
    assert np.array_equal(S, S.T)                                 # (symmetric throughout: the condition of the identity)
    return {"N": N, "Na": Na, "Sigma0": S0, "x0": x0, "ops": ops, "Sigma": S, "x": x, "region": (x2, S2)}


@functools.lru_cache(maxsize=None)
def exact_chain(N, Na, seed=0):
    """a seed on which a product leaves float64's exact range is replaced by the next"""
    for attempt in range(40):
        try:
            return _build_exact(N, Na, 1000 * N + 10 * Na + 97 * seed + 7919 * attempt)
        except (cc.Inexact, AssertionError):
            continue
    raise cc.Inexact(f"no exact chain for N = {N}, Na = {Na}")


def float_chain(N, Na, seed=0, shapes=None):
    """an SPD Sigma with a coupled tail; per (m, s) of lc.shapes(Na) a correction, with a prediction and an init between"""
    rng = np.random.default_rng(50000 + 1000 * N + Na + seed)
    A = rng.normal(size=(N, N))
    S0, x0 = A @ A.T / N + np.eye(N), rng.normal(size=N)          # one SPD matrix: corner, rectangles and tail together
    ops = []
    for i, (m, s) in enumerate(shapes or lc.shapes(Na)):
        cols = np.sort(rng.permutation(Na)[:s]).astype(np.int32)
        ops.append({"op": "deferred" if i % 2 else "eager", "cols": cols, "Hc": rng.normal(size=(m, s)),
                    "R": 0.5 * np.eye(m), "nu": rng.normal(size=m)})
        if i == 0:
            r = min(3, Na)
            Q = rng.normal(size=(r, r))
            ops.append({"op": "propagate", "first": 0, "Fr": np.eye(r) + 0.1 * rng.normal(size=(r, r)), "Qr": Q @ Q.T,
                        "dx": rng.normal(size=r)})
        if i == 1 and Na >= 5:
            src = np.sort(rng.permutation(Na - 2)[:2]).astype(np.int32)
            ops.append({"op": "init", "first": Na - 2, "r": 2, "cols": src, "G": rng.normal(size=(2, 2)),
                        "W": np.eye(2), "xb": rng.normal(size=2)})
    ops.append({"op": "flush"})
    return {"N": N, "Na": Na, "Sigma0": S0, "x0": x0, "ops": ops}


# ---- the plan, as ekf_dense64_region.hpp cuts it -------------------------------------------------------------------------------

def plan(Na, N, ld):
    up = lambda a, b: (a + b - 1) // b
    pitch = up(Na, 128) * 128
    acc = 8 * (2 * Na * pitch + pitch + 2 * 64 * pitch)
    scratch = 8 * 2 * Na * ld
    tile0 = Na // 128
    return {"pitch": pitch, "update_tiles": up(Na, 32) * up(Na, 64), "gemm_tiles": (up(N, 128) - tile0) ** 2,
            "gemm_k": up(Na, 16) * 16, "acc_bytes": acc, "scratch_bytes": scratch, "group_bytes": acc + scratch,
            "tile_rows": 32, "tile_cols": 64, "threads": 256}
