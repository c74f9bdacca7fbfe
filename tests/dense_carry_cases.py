"""Shared by tests/test_gpu_dense64_carry.py and tests/test_dense64_carry_host.py: a numpy model of the CARRIED
representation of the dense fp64 handle (Sigma_base and the two pending panels, mapped by propagate_block / init_block and
read through by the block readout) on top of dense_deferred_cases.DeferredModel, with every product it forms checked to be
exact in float64; the integer chains that interleave deferred corrections with the three carried calls; and the grid of
shapes the chains are run on."""
import itertools

import numpy as np

import dense_block_cases as bc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_sparse_cases as sp

LIMIT = 2.0 ** 52

GRID_N = [1, 5, 63, 64, 65, 200]
GRID_R = [1, 3, 16, 17, 64]
GRID_PLACE = ["zero", "straddle", "end"]
GRID_P = [1, 2, 17, 64]
GRID_S = [0, 3, 64]
RECIPE = {1: [(1, 1)], 2: [(2, 5)], 17: [(17, 5)], 64: [(17, 5), (17, 5), (17, 5), (13, 5)]}   # (m, s) that make p rows


class Inexact(AssertionError):
    pass


def frac_bits(A):
    """the smallest e >= 0 with A * 2^e integral: every entry of A is an integer over 2^e"""
    A = np.asarray(A, dtype=np.float64)
    for e in range(0, 200):
        B = A * 2.0 ** e
        if np.array_equal(B, np.round(B)):
            return e
    raise Inexact("not a dyadic rational of fewer than 200 fractional bits")


def exact_product(A, B, plus=None):
    """A @ B (+ plus), after checking that it is exact in ANY order of summation: all terms are integers over one power of
    two, and the sum of their absolute values (times that power) stays below 2^52, so every partial sum is an integer below
    2^53 over that power.  The bound itself is a float64 sum of non-negative terms: good to 1e-13, against a margin of 2."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    e = frac_bits(A) + frac_bits(B)
    bound = np.abs(A) @ np.abs(B)
    if plus is not None:
        e = max(e, frac_bits(plus))
        bound = bound + np.abs(plus)
    if bound.size and float(bound.max()) * 2.0 ** e >= LIMIT:
        raise Inexact(f"a product reaches {float(bound.max()):.3g} at {e} fractional bits")
    out = A @ B
    return out if plus is None else out + plus


class CarriedModel(dd.DeferredModel):
    """DeferredModel with every product exact-checked, plus the three calls that the handle can carry the pending rows
    through.  carry = False is the flush-first sequence (what the handle does with the policy off)."""

    def __init__(self, Sigma, state, carry=True):
        super().__init__(Sigma, state)
        self.carry = carry

    # -- the deferred calls, guarded ----------------------------------------------------------------------------------
    def read(self, rows, cols):
        rows, cols = np.asarray(rows), np.asarray(cols)
        exact_product(-self.Kt[:, rows].T, self.Tp[:, cols], self.base[np.ix_(rows, cols)])   # the check; then the fold
        return super().read(rows, cols)

    def gather(self, cols, Hc):
        every = np.arange(self.N)
        return exact_product(Hc, self.read(cols, every)), exact_product(Hc, self.read(every, cols).T)

    def scores(self, cols, Hc, R, nu=None):
        J, m = Hc.shape[0], Hc.shape[1]
        S, nis = np.empty((J, m, m)), None if nu is None else np.empty(J)
        for j in range(J):
            S[j] = exact_product(exact_product(Hc[j], self.read(cols[j], cols[j])), Hc[j].T, R if R.ndim == 2 else R[j])
            if nu is not None:
                nis[j] = float(nu[j] @ np.linalg.inv(S[j]) @ nu[j])
        return S, nis

    def correct_deferred(self, cols, Hc, R, nu):
        if self.pending + len(Hc) > dd.MAX_ROWS:
            self.flush()
        T, Ut = self.gather(cols, Hc)
        S = exact_product(T[:, cols], Hc.T, R)
        d = np.diag(S).copy()
        if not (np.array_equal(S, np.diag(d)) and (d > 0).all() and np.array_equal(np.log2(d), np.round(np.log2(d)))):
            raise Inexact("S is not a diagonal of powers of two")
        Kt = Ut / d[:, None]                                        # U S^-1: a scaling by powers of two
        self.state = exact_product(Kt.T, nu[:, None], self.state[:, None])[:, 0]
        self.Kt, self.Tp = np.vstack([self.Kt, Kt]), np.vstack([self.Tp, T])
        return float(np.sum(nu * nu / d))

    def flush(self):
        self.base = exact_product(-self.Kt.T, self.Tp, self.base)
        self.Kt, self.Tp = np.zeros((0, self.N)), np.zeros((0, self.N))

    @property
    def sigma_cur(self):
        return exact_product(-self.Kt.T, self.Tp, self.base)

    # -- the carried calls ------------------------------------------------------------------------------------------------
    def propagate_block(self, first, Fr, Qr=None, dx=None):
        """k_d64_block on Sigma_base; every pending row v of both panels: v[b] <- Fr v[b]"""
        if not self.carry:
            self.flush()
        r = len(Fr)
        b = slice(first, first + r)
        S = self.base
        exact_product(Fr, S[b, :])
        exact_product(S[:, b], Fr.T)
        exact_product(exact_product(Fr, S[b, b]), Fr.T, Qr)
        self.state, self.base = bc.np_predict_slices(self.state, S, first, Fr, Qr, dx)
        self.Kt[:, b], self.Tp[:, b] = exact_product(self.Kt[:, b], Fr.T), exact_product(self.Tp[:, b], Fr.T)

    def init_block(self, first, r, cols=None, G=None, W=None, xb=None):
        """k_d64_init on Sigma_base; every pending row v of both panels: v[b] <- G v[cols], +0 with s = 0"""
        if not self.carry:
            self.flush()
        b = slice(first, first + r)
        S = self.base
        if cols is not None:
            exact_product(G, S[cols, :])
            exact_product(S[:, cols], G.T)
            exact_product(exact_product(G, S[np.ix_(cols, cols)]), G.T, W)
        self.state, self.base = ic.np_init_block(self.state, S, first, r, cols, G, W, xb)
        if cols is None:
            self.Kt[:, b], self.Tp[:, b] = 0.0, 0.0
        else:
            self.Kt[:, b], self.Tp[:, b] = exact_product(self.Kt[:, cols], G.T), exact_product(self.Tp[:, cols], G.T)

    def sigma_block(self, rows, cols):
        if not self.carry:
            self.flush()
        return self.read(rows, cols)


# ---- the grid ------------------------------------------------------------------------------------------------------------------

def first_of(N, r, place):
    """the block's first index, or None when N cannot hold the placement"""
    if r > N:
        return None
    if place == "zero":
        return 0
    if place == "end":
        return N - r
    first = 60 if r >= 5 else 64 - (r + 1) // 2       # covers columns 63 and 64
    return first if r >= 2 and first + r <= N else None


def holds(N, r, place, p, s):
    """whether a chain of these sizes exists at this N (carry_chain builds it)"""
    if first_of(N, r, place) is None or s > min(N - r, 64):
        return False
    if any(m > N for m, _ in RECIPE[p]):
        return False
    return p != 64 or N - r >= 20                      # four lists of five outside the block (see carry_chain)


def grid():
    """-> [(N, r, place, p, s)] that hold, and the cells (r, place, p, s) that no N holds"""
    cells = list(itertools.product(GRID_R, GRID_PLACE, GRID_P, GRID_S))
    run = [(N,) + c for N in GRID_N for c in cells if holds(N, *c)]
    nowhere = [c for c in cells if not any(holds(N, *c) for N in GRID_N)]
    return run, cells, nowhere


# ---- integer chains ----------------------------------------------------------------------------------------------------------

def _thin(rng, rows, cols, nonzero=3):
    return dd.sparse_rows(rng, rows, cols, nonzero) if cols else np.zeros((rows, 0))


def _start(N, first, r, p, rng):
    """Sigma0 and the lists of the corrections that make the p rows.  One correction (p <= 17): a dense Sigma0 in
    {-1, 0, 1} and a scattered list anywhere.  Four (p = 64): they must not compound (four levels of K T on a dense
    Sigma pass 2^52), so Sigma0 is dense in the block's rows and columns only and otherwise zero outside four groups of five
    free indices, one per correction: K and T of each are then dense on the block, which is what the maps act on, and zero
    on the other groups."""
    shapes = [(m, min(s, N)) for m, s in RECIPE[p]]
    if len(shapes) == 1:
        return rng.integers(-1, 2, size=(N, N)).astype(np.float64), shapes, [sp.index_list(N, shapes[0][1], "scattered", rng)]
    free = rng.permutation([i for i in range(N) if not first <= i < first + r])[:20]
    S = np.zeros((N, N))
    S[first:first + r, :] = rng.integers(-1, 2, size=(r, N))
    S[:, first:first + r] = rng.integers(-1, 2, size=(N, r))
    lists = []
    for g in range(4):
        idx = free[5 * g:5 * g + 5]
        S[np.ix_(idx, idx)] = rng.integers(-1, 2, size=(5, 5))
        lists.append(np.ascontiguousarray(idx, dtype=np.int32))
    return S, shapes, lists


def carry_chain(N, r, place, p, s, seed=None):
    """The chain of one grid point: the corrections that make p rows, propagate_block on [first, first + r) with p rows
    pending, init_block of the same block from s scattered columns (among them columns the corrections listed) with p rows
    pending, one more correction whose list crosses the block, a second propagate_block, the flush.  After every call the
    model's state, count, a readout through the pending rows and the S / nis of three candidates are recorded.
    -> dict; raises Inexact when a value leaves float64's integers (the seed must then be replaced)."""
    first = first_of(N, r, place)
    assert holds(N, r, place, p, s)
    rng = np.random.default_rng(
        (100000 * N + 1000 * r + 100 * GRID_PLACE.index(place) + 10 * GRID_P.index(p) + GRID_S.index(s)) if seed is None else seed)
    Sigma0, shapes, lists = _start(N, first, r, p, rng)
    x0 = rng.integers(-9, 10, size=N).astype(np.float64)
    model = CarriedModel(Sigma0, x0)
    chain = {"N": N, "first": first, "r": r, "p": p, "s": s, "Sigma0": Sigma0.copy(), "x0": x0.copy(), "ops": []}
    block = list(range(first, first + r))
    listed = [int(v) for c in lists for v in c]

    def correction(m, sc, lst):
        cols, Hc, R, nu, _ = dd.exact_candidates(model.sigma_cur, 1, m, sc, "scattered", rng, first=lst)
        return {"op": "correct", "cols": cols[0], "Hc": Hc[0], "R": R[0], "nu": nu[0]}

    def apply(op):
        if op["op"] == "correct":
            op["nis"] = model.correct_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
        elif op["op"] == "propagate":
            model.propagate_block(first, op["Fr"], op["Qr"], op["dx"])
        else:
            model.init_block(first, r, op["cols"], op["G"], op["W"], op["xb"])
        # what the handle must show after the call
        pick = [first, first + r - 1, 0, N - 1] + listed[:4] + [int(v) for v in rng.integers(0, N, size=4)]
        rows = np.array(pick, dtype=np.int32)
        cols = np.array(pick[::-1] + block[:3], dtype=np.int32)
        m, sc = min(2, N), min(5, N)
        lst = np.array((block + [i for i in rng.permutation(N) if i not in block])[:sc], dtype=np.int32)   # crosses the block
        cc, Hc, R, nu, _ = dd.exact_candidates(model.sigma_cur, 3, m, sc, "scattered", rng, first=rng.permutation(lst))
        S, nis = model.scores(cc, Hc, R, nu)
        op["check"] = {"state": model.state.copy(), "pending": model.pending, "rows": rows, "cols": cols,
                       "block": model.read(rows, cols), "cand": (cc, Hc, R, nu), "S": S, "nis": nis}
        chain["ops"].append(op)

    for (m, sc), lst in zip(shapes, lists):
        apply(correction(m, sc, lst))
    assert model.pending == p
    ints = lambda shape, lo=-2, hi=3: rng.integers(lo, hi, size=shape).astype(np.float64)
    for _ in range(1):
        apply({"op": "propagate", "Fr": _thin(rng, r, r), "Qr": ints((r, r)), "dx": ints(r)})
    cols = None
    if s:
        outside = [i for i in range(N) if i not in block]
        seen = [i for i in dict.fromkeys(listed) if i not in block][:max(1, s // 2)]
        rest = [i for i in rng.permutation(outside) if i not in seen]
        cols = np.array(rng.permutation((seen + rest)[:s]), dtype=np.int32)
    apply({"op": "init", "cols": cols, "G": _thin(rng, r, s) if s else None, "W": ints((r, r)), "xb": ints(r, -9, 10)})
    sc = min(3, N)
    lst = np.array(([first] + [i for i in rng.permutation(N) if i != first])[:sc], dtype=np.int32)
    apply(correction(1, sc, lst))
    apply({"op": "propagate", "Fr": _thin(rng, r, r), "Qr": None, "dx": None})
    chain["pending_end"] = model.pending
    model.flush()
    chain["Sigma"] = model.base.copy()
    return chain


def run_model(chain, carry):
    """the chain's calls on a fresh model -> per call (state, Sigma_cur, readout, S, nis, pending), and Sigma after the flush"""
    model = CarriedModel(chain["Sigma0"], chain["x0"], carry=carry)
    first, r = chain["first"], chain["r"]
    out = []
    for op in chain["ops"]:
        nis0 = None
        if op["op"] == "correct":
            nis0 = model.correct_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
        elif op["op"] == "propagate":
            model.propagate_block(first, op["Fr"], op["Qr"], op["dx"])
        else:
            model.init_block(first, r, op["cols"], op["G"], op["W"], op["xb"])
        ck = op["check"]
        S, nis = model.scores(*ck["cand"])
        pending = model.pending
        out.append({"nis0": nis0, "state": model.state.copy(), "pending": pending, "S": S, "nis": nis,
                    "Sigma_cur": model.sigma_cur, "block": CarriedModel.read(model, ck["rows"], ck["cols"])})
    model.flush()
    return out, model.base.copy()
