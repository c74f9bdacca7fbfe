"""Shared by tests/test_gpu_dense64_session.py and tests/test_dense64_session_host.py: ONE model of the whole dense fp64
handle and the named sessions that drive it through a map's lifetime -- discover, correct, move, prune, re-discover.

HandleModel is dense_carry_cases.CarriedModel (Sigma_base and the two pending panels, every product checked to be exact in
float64) plus what that model lacks: the live dimension, swap_blocks, the dense-operand calls, set, the state slices and the
refusals.  PlainModel has none of the machinery: a full N x N Sigma on which every call is its embedded dense matrices
(F Sigma F^T + Q, Sigma - K (H Sigma), an explicit permutation, an explicit G-embedding); nothing is ever pending in it.  A
structured call with live = Na acts on Sigma[:Na, :Na] with matrices of dimension Na -- the header's "filter of dimension Na
that lives in the corner" -- so the two models agree on a coupled tail too; the dense-operand calls act on all N.
PlainModel is generic in its element type: float64 for the comparison, np.longdouble for the margins.

A session is a name, a fixed list of ops built from a fixed seed and the start (Sigma0, x0).  The integer form uses small
integers throughout (a seed on which a value leaves float64's integers raises Inexact and is replaced by the next, twelve
at most; none left is an error); the random form keeps the op list -- the same calls, indices and shapes -- with an SPD
Sigma0, Gaussian operands and a well-conditioned R.  Outside the largest live corner a session reaches, Sigma and the state
hold dense_swap_cases.unique_data (every entry different, -0.0 and NaN payloads): an entry written there is seen."""
import functools

import numpy as np

import dense_block_cases as bc
import dense_carry_cases as cc
import dense_deferred_cases as dd
import dense_init_cases as ic
import dense_swap_cases as sc

OK, INVALID = 0, 1                                         # EKF_OK, EKF_ERR_INVALID
MAX_R = MAX_S = MAX_M = 64
SIZES = [67, 131, 203]
PRIOR = 100.0                                              # the reference's landmark prior, an integer


def bad_block(first, r, live):
    return r < 1 or r > MAX_R or r > live or first < 0 or first > live - r


def bad_list(cols, live):
    c = np.asarray(cols)
    return len(c) < 1 or len(c) > min(MAX_S, live) or c.min() < 0 or c.max() >= live or len(np.unique(c)) != len(c)


def bad_swap(a, b, r, live):
    return bad_block(a, r, live) or bad_block(b, r, live) or abs(a - b) < r


def bad_init(first, r, cols, live):
    if bad_block(first, r, live):
        return True
    if cols is None:
        return False
    c = np.asarray(cols)
    return len(c) > live - r or bad_list(c, live) or bool(((c >= first) & (c < first + r)).any())


def rectangles(S, Na):
    """-> (how many entries with exactly one index >= Na are != 0, their largest absolute value): ekf_dense64_coupling"""
    both = np.concatenate([np.asarray(S[:Na, Na:], dtype=np.float64).ravel(), np.asarray(S[Na:, :Na], dtype=np.float64).ravel()])
    return int(np.count_nonzero(both != 0.0)), float(np.abs(both).max()) if both.size else 0.0


# ---- the handle, on the carried model ------------------------------------------------------------------------------------------

class HandleModel(cc.CarriedModel):
    """Every entry point of DensePropagator64 on the carried representation.  The pending rows are zero from `live` on at
    all times (asserted); a structured call runs CarriedModel at dimension `live` on the corner and pastes the result."""

    def __init__(self, Sigma, state, carry=False, live=None):
        super().__init__(Sigma, state, carry)
        self.live = self.N if live is None else int(live)
        self.F, self.Q = np.zeros((self.N, self.N)), np.zeros((self.N, self.N))

    # -- the corner as a CarriedModel of dimension live ---------------------------------------------------------------------
    def _corner(self):
        Na = self.live
        assert not self.Kt[:, Na:].any() and not self.Tp[:, Na:].any()
        sub = cc.CarriedModel(self.base[:Na, :Na], self.state[:Na], self.carry)
        sub.Kt, sub.Tp = self.Kt[:, :Na].copy(), self.Tp[:, :Na].copy()
        return sub

    def _paste(self, sub):
        Na = self.live
        self.base[:Na, :Na], self.state[:Na] = sub.base, sub.state
        self.Kt, self.Tp = np.zeros((sub.pending, self.N)), np.zeros((sub.pending, self.N))
        self.Kt[:, :Na], self.Tp[:, :Na] = sub.Kt, sub.Tp

    @property
    def sigma_cur(self):
        S = self.base.copy()
        S[:self.live, :self.live] = self._corner().sigma_cur
        return S

    # -- the structured calls -------------------------------------------------------------------------------------------------
    def flush(self):
        if self.pending == 0:                                # a no-op that does not look at Sigma
            return OK, None
        sub = self._corner()
        sub.flush()
        self._paste(sub)
        return OK, None

    def correct_sparse(self, cols, Hc, R, nu, deferred):
        if len(Hc) > min(self.live, MAX_M) or bad_list(cols, self.live):
            return INVALID, None
        sub = self._corner()
        if not deferred:
            sub.flush()
        nis = sub.correct_deferred(cols, Hc, R, nu)          # flushes by itself when pending + m > 64
        if not deferred:
            sub.flush()
        self._paste(sub)
        return OK, nis

    def scores(self, cols, Hc, R, nu):
        if Hc.shape[1] > min(self.live, MAX_M) or any(bad_list(c, self.live) for c in cols):
            return INVALID, None
        return OK, self._corner().scores(cols, Hc, R, nu)

    def propagate_block(self, first, Fr, Qr=None, dx=None):
        if bad_block(first, len(Fr), self.live):
            return INVALID, None
        sub = self._corner()
        sub.propagate_block(first, Fr, Qr, dx)
        self._paste(sub)
        return OK, None

    def init_block(self, first, r, cols=None, G=None, W=None, xb=None):
        if bad_init(first, r, cols, self.live):
            return INVALID, None
        sub = self._corner()
        sub.init_block(first, r, cols, G, W, xb)
        self._paste(sub)
        return OK, None

    def swap_blocks(self, a, b, r):
        if bad_swap(a, b, r, self.live):
            return INVALID, None
        sub = self._corner()
        if not (self.carry and sub.pending):
            sub.flush()
        sub.base, sub.state = sc.swap_model(sub.base, sub.state, a, b, r)
        if sub.pending:
            sub.Kt, sub.Tp = sc.swap_panels(sub.Kt, sub.Tp, a, b, r)
        self._paste(sub)
        return OK, None

    def sigma_block(self, rows, cols):
        """Sigma_cur[rows][cols] over [0, N): with the policy off it flushes; an index >= live is returned as stored"""
        rows, cols = np.asarray(rows), np.asarray(cols)
        if not self.carry:
            self.flush()
        out = self.base[np.ix_(rows, cols)].copy()
        ri, ci = rows < self.live, cols < self.live
        if ri.any() and ci.any():
            out[np.ix_(ri, ci)] = self._corner().read(rows[ri], cols[ci])
        return OK, out

    def set_live(self, Na):
        if Na < 1 or Na > self.N:
            return INVALID, None
        if Na < self.live:
            self.flush()                                     # at the old width
        else:
            self.Kt[:, self.live:Na], self.Tp[:, self.live:Na] = 0.0, 0.0
        self.live = int(Na)
        return OK, None

    def set_carry(self, on):
        self.carry = bool(on)
        return OK, None

    # -- the dense-operand calls: flush at the live width, then all N states ---------------------------------------------------
    def set(self, F=None, Sigma=None, Q=None):
        if F is not None:
            self.F = np.array(F, dtype=np.float64)
        if Q is not None:
            self.Q = np.array(Q, dtype=np.float64)
        if Sigma is not None:
            self.base = np.array(Sigma, dtype=np.float64)
            self.Kt, self.Tp = np.zeros((0, self.N)), np.zeros((0, self.N))
        return OK, None

    def dense_propagate(self, iterations=1):
        self.flush()
        for _ in range(iterations):
            self.base = cc.exact_product(cc.exact_product(self.F, self.base), self.F.T, self.Q)
        return OK, None

    def dense_correct(self, H, R, nu):
        self.flush()
        T, U = cc.exact_product(H, self.base), cc.exact_product(self.base, H.T)
        S = cc.exact_product(T, H.T, R)
        d = np.diag(S).copy()
        if not (np.array_equal(S, np.diag(d)) and (d > 0).all() and np.array_equal(np.log2(d), np.round(np.log2(d)))):
            raise cc.Inexact("S is not a diagonal of powers of two")
        K = U / d[None, :]
        self.state = cc.exact_product(K, nu[:, None], self.state[:, None])[:, 0]
        self.base = cc.exact_product(-K, T, self.base)
        return OK, float(np.sum(nu * nu / d))

    def dense_score(self, H, R, nu):
        self.flush()
        J, m = H.shape[0], H.shape[1]
        S, nis = np.empty((J, m, m)), np.empty(J)
        for j in range(J):
            S[j] = cc.exact_product(cc.exact_product(H[j], self.base), H[j].T, R if R.ndim == 2 else R[j])
            nis[j] = float(nu[j] @ np.linalg.inv(S[j]) @ nu[j])
        return OK, (S, nis)

    def sigma(self):
        self.flush()
        return OK, self.base.copy()

    def coupling(self, Na):
        if Na < 1 or Na > self.N:
            return INVALID, None
        self.flush()
        return OK, rectangles(self.base, Na)

    # -- the state slices: [0, N), never stale, never flush -----------------------------------------------------------------------
    def state_block(self, first, count):
        if count < 1 or first < 0 or first + count > self.N:
            return INVALID, None
        return OK, self.state[first:first + count].copy()

    def set_state_block(self, first, x):
        if len(x) < 1 or first < 0 or first + len(x) > self.N:
            return INVALID, None
        self.state[first:first + len(x)] = x
        return OK, None


# ---- the plain dense model --------------------------------------------------------------------------------------------------------

def inverse(S):
    """S^-1: numpy's for float64 (the spelling of the other models), Gauss-Jordan with row pivoting for wider types"""
    if S.dtype == np.float64:
        return np.linalg.inv(S)
    n = len(S)
    A = np.concatenate([S.copy(), np.eye(n, dtype=S.dtype)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
        A[k] = A[k] / A[k, k]
        f = A[:, k].copy()
        f[k] = 0
        A = A - np.outer(f, A[k])
    return A[:, n:]


class PlainModel:
    """A full N x N Sigma and the state; every call is its embedded dense matrices.  check = True: every product goes
    through exact_product and S must be a diagonal of powers of two (the integer sessions); otherwise plain products in
    `dtype`.  Nothing is ever pending; carry has no effect; live decides the corner the structured calls act on and what
    they refuse."""

    def __init__(self, Sigma, state, carry=False, live=None, dtype=np.float64, check=False):
        self.t, self.check = dtype, check
        self.S, self.state = np.array(Sigma, dtype=dtype), np.array(state, dtype=dtype)
        self.N = len(self.state)
        self.live = self.N if live is None else int(live)
        self.F, self.Q = np.zeros((self.N, self.N), dtype=dtype), np.zeros((self.N, self.N), dtype=dtype)
        self.carry, self.pending = bool(carry), 0

    def _a(self, A):
        return None if A is None else np.asarray(A, dtype=self.t)

    def mm(self, A, B, plus=None):
        if self.check:
            return cc.exact_product(A, B, plus)
        return A @ B if plus is None else A @ B + plus

    def _gain(self, U, S, nu):
        """-> K = U S^-1, nis"""
        if self.check:
            d = np.diag(S).copy()
            if not (np.array_equal(S, np.diag(d)) and (d > 0).all() and np.array_equal(np.log2(d), np.round(np.log2(d)))):
                raise cc.Inexact("S is not a diagonal of powers of two")
            return U / d[None, :], float(np.sum(nu * nu / d))
        Si = inverse(S)
        return U @ Si, nu @ Si @ nu

    def _congruence(self, Na, F, Q=None):
        C = self.S[:Na, :Na]
        self.S[:Na, :Na] = self.mm(self.mm(self._a(F), C), self._a(F).T, self._a(Q))

    def _update(self, Na, H, R, nu):
        """Sigma - K (H Sigma), state + K nu on the leading Na states -> nis"""
        C = self.S[:Na, :Na]
        T, U = self.mm(H, C), self.mm(C, H.T)
        K, nis = self._gain(U, self.mm(T, H.T, R), nu)
        self.state[:Na] = self.mm(K, nu[:, None], self.state[:Na, None])[:, 0]
        self.S[:Na, :Na] = self.mm(-K, T, C)
        return nis

    @property
    def sigma_cur(self):
        return self.S.copy()

    def flush(self):
        return OK, None

    def correct_sparse(self, cols, Hc, R, nu, deferred):
        if len(Hc) > min(self.live, MAX_M) or bad_list(cols, self.live):
            return INVALID, None
        H = np.zeros((len(Hc), self.live), dtype=self.t)
        H[:, cols] = Hc
        return OK, self._update(self.live, H, self._a(R), self._a(nu))

    def scores(self, cols, Hc, R, nu):
        if Hc.shape[1] > min(self.live, MAX_M) or any(bad_list(c, self.live) for c in cols):
            return INVALID, None
        J, m = Hc.shape[0], Hc.shape[1]
        S, nis = np.empty((J, m, m), dtype=self.t), np.empty(J, dtype=self.t)
        for j in range(J):
            h, Rj = self._a(Hc[j]), self._a(R if R.ndim == 2 else R[j])
            S[j] = self.mm(self.mm(h, self.S[np.ix_(cols[j], cols[j])]), h.T, Rj)
            nis[j] = self._a(nu[j]) @ inverse(S[j]) @ self._a(nu[j])
        return OK, (S, nis)

    def propagate_block(self, first, Fr, Qr=None, dx=None):
        if bad_block(first, len(Fr), self.live):
            return INVALID, None
        self._congruence(self.live, *bc.embed(self.live, first, Fr, Qr))
        if dx is not None:
            self.state[first:first + len(Fr)] += self._a(dx)
        return OK, None

    def init_block(self, first, r, cols=None, G=None, W=None, xb=None):
        if bad_init(first, r, cols, self.live):
            return INVALID, None
        self._congruence(self.live, *ic.embedded_FQ(self.live, first, r, cols, G, W))
        if xb is not None:
            self.state[first:first + r] = self._a(xb)
        return OK, None

    def swap_blocks(self, a, b, r):
        if bad_swap(a, b, r, self.live):
            return INVALID, None
        P = sc.explicit_P(self.live, a, b, r)
        self._congruence(self.live, P)
        self.state[:self.live] = self.mm(self._a(P), self.state[:self.live, None])[:, 0]
        return OK, None

    def sigma_block(self, rows, cols):
        return OK, self.S[np.ix_(rows, cols)].copy()

    def set_live(self, Na):
        if Na < 1 or Na > self.N:
            return INVALID, None
        self.live = int(Na)
        return OK, None

    def set_carry(self, on):
        self.carry = bool(on)
        return OK, None

    def set(self, F=None, Sigma=None, Q=None):
        if F is not None:
            self.F = np.array(F, dtype=self.t)
        if Q is not None:
            self.Q = np.array(Q, dtype=self.t)
        if Sigma is not None:
            self.S = np.array(Sigma, dtype=self.t)
        return OK, None

    def dense_propagate(self, iterations=1):
        for _ in range(iterations):
            self._congruence(self.N, self.F, self.Q)
        return OK, None

    def dense_correct(self, H, R, nu):
        return OK, self._update(self.N, self._a(H), self._a(R), self._a(nu))

    def dense_score(self, H, R, nu):
        J, m = H.shape[0], H.shape[1]
        S, nis = np.empty((J, m, m), dtype=self.t), np.empty(J, dtype=self.t)
        for j in range(J):
            h, Rj = self._a(H[j]), self._a(R if R.ndim == 2 else R[j])
            S[j] = self.mm(self.mm(h, self.S), h.T, Rj)
            nis[j] = self._a(nu[j]) @ inverse(S[j]) @ self._a(nu[j])
        return OK, (S, nis)

    def sigma(self):
        return OK, self.S.copy()

    def coupling(self, Na):
        if Na < 1 or Na > self.N:
            return INVALID, None
        return OK, rectangles(self.S, Na)

    def state_block(self, first, count):
        if count < 1 or first < 0 or first + count > self.N:
            return INVALID, None
        return OK, self.state[first:first + count].copy()

    def set_state_block(self, first, x):
        if len(x) < 1 or first < 0 or first + len(x) > self.N:
            return INVALID, None
        self.state[first:first + len(x)] = self._a(x)
        return OK, None


# ---- the op language -----------------------------------------------------------------------------------------------------------

def apply(model, op):
    """one call of a session on a HandleModel or a PlainModel -> (status, value): nis of a correction, (S, nis) of a
    scoring, the block of a readout, Sigma, (count, max) of coupling, a state slice, else None"""
    k = op["op"]
    if k in ("eager", "deferred"):
        return model.correct_sparse(op["cols"], op["Hc"], op["R"], op["nu"], k == "deferred")
    if k == "score_sparse":
        return model.scores(op["cols"], op["Hc"], op["R"], op["nu"])
    if k == "propagate":
        return model.propagate_block(op["first"], op["Fr"], op["Qr"], op["dx"])
    if k == "init":
        return model.init_block(op["first"], op["r"], op["cols"], op["G"], op["W"], op["xb"])
    if k == "swap":
        return model.swap_blocks(op["a"], op["b"], op["r"])
    if k == "flush":
        return model.flush()
    if k == "live":
        return model.set_live(op["Na"])
    if k == "carry":
        return model.set_carry(op["on"])
    if k == "sigma_block":
        return model.sigma_block(op["rows"], op["cols"])
    if k == "set":
        return model.set(op["F"], op["Sigma"], op["Q"])
    if k == "dense_propagate":
        return model.dense_propagate(1)
    if k == "dense_correct":
        return model.dense_correct(op["H"], op["R"], op["nu"])
    if k == "dense_score":
        return model.dense_score(op["H"], op["R"], op["nu"])
    if k == "sigma":
        return model.sigma()
    if k == "coupling":
        return model.coupling(op["Na"])
    if k == "state_block":
        return model.state_block(op["first"], op["count"])
    if k == "set_state_block":
        return model.set_state_block(op["first"], op["x"])
    raise KeyError(k)


def reads_block(carry, pending):
    """whether the probe readout runs after a call: where it would not flush (the policy on, or nothing pending)"""
    return bool(carry) or pending == 0


def run(session, carry, model=HandleModel, **kw):
    """the session's calls on a fresh model -> per call {status, value, pending, live, carry, state, Sigma_cur, S, nis,
    block}: S, nis of the probe candidates through whatever is pending, block of the probe readout (None where it would
    flush).  Sigma_cur is the model's own view of all of Sigma, for the host tests."""
    m = model(session["Sigma0"], session["x0"], carry=carry, **kw)
    out = []
    for op in session["ops"]:
        status, value = apply(m, op)
        assert status == (INVALID if op.get("refused") else OK), (session["name"], len(out), op["op"], status)
        rec = {"status": status, "value": value, "pending": m.pending, "live": m.live, "carry": m.carry,
               "state": m.state.copy(), "Sigma_cur": m.sigma_cur}
        st, (rec["S"], rec["nis"]) = m.scores(*op["cand"])
        assert st == OK
        rec["block"] = m.sigma_block(op["rows"], op["cols_rd"])[1] if reads_block(m.carry, m.pending) else None
        assert m.pending == rec["pending"]
        out.append(rec)
    return out


def describe(session, i):
    """the text of a failure message: session, N, step index and op"""
    op = session["ops"][i]
    extra = {k: op[k] for k in ("first", "r", "a", "b", "Na", "on") if k in op}
    return f"{session['name']} N={session['N']} step {i} {op['op']}{' (refused)' if op.get('refused') else ''} {extra}"


# ---- writing a script ------------------------------------------------------------------------------------------------------------

class Script:
    """Collects the ops of one session.  form = 'int': a HandleModel (carry on unless the script switches it) follows the
    script, and every operand is small integers with R = D - H Sigma_cur H^T so that S = D = diag(2^k); form = 'random': the
    same calls with Gaussian operands.  After every op the probes are chosen: two candidates for score_sparse in the live
    corner, and a readout whose rows and columns straddle the block just touched and the edge of the live corner."""

    def __init__(self, name, N, form, rng, Sigma0, x0, top, carry=True):
        self.name, self.N, self.form, self.rng, self.top = name, N, form, rng, top
        self.Sigma0, self.x0 = np.array(Sigma0, dtype=np.float64), np.array(x0, dtype=np.float64)
        self.model = (HandleModel if form == "int" else PlainModel)(self.Sigma0, self.x0, carry=carry)
        self.ops = []

    @property
    def live(self):
        return self.model.live

    # -- operands ---------------------------------------------------------------------------------------------------------------
    def ints(self, shape, lo=-2, hi=3):
        if self.form == "int":
            return self.rng.integers(lo, hi, size=shape).astype(np.float64)
        return self.rng.normal(size=shape)

    def thin(self, rows, cols, nonzero=3):
        """rows x cols, at most `nonzero` entries of +-1 per row (int) / the same pattern times Gaussians (random)"""
        if cols == 0:
            return np.zeros((rows, 0))
        A = dd.sparse_rows(self.rng, rows, cols, nonzero)
        return A if self.form == "int" else A * self.rng.normal(size=A.shape)

    def noise(self, m, scale=1.0):
        """a well-conditioned m x m R (random form)"""
        A = self.rng.normal(size=(m, m))
        return scale * (np.eye(m) + 0.2 * A @ A.T / m)

    def corner(self):
        Na = self.live
        return self.model.sigma_cur[:Na, :Na]

    def candidates(self, J, m, s, first=None, nonzero=2):
        """cols (J, s), Hc (J, m, s), R (J, m, m), nu (J, m) in the live corner; candidate 0 lists `first` when given"""
        Na = self.live
        if self.form == "int":
            C = self.corner()
            cols = np.stack([np.array(self.rng.permutation(Na)[:s], dtype=np.int32) for _ in range(J)])
            if first is not None:
                cols[0] = first
            Hc = np.stack([dd.sparse_rows(self.rng, m, s, nonzero) for _ in range(J)])
            nu = self.rng.integers(-2, 3, size=(J, m)).astype(np.float64)
            R = np.stack([np.diag(2.0 ** self.rng.integers(0, 3, size=m)) - Hc[j] @ C[np.ix_(cols[j], cols[j])] @ Hc[j].T
                          for j in range(J)])                  # S_j = diag(2^k) exactly
            return cols, Hc, R, nu
        cols = np.stack([np.array(self.rng.permutation(Na)[:s], dtype=np.int32) for _ in range(J)])
        if first is not None:
            cols[0] = first
        return cols, self.rng.normal(size=(J, m, s)), np.stack([self.noise(m) for _ in range(J)]), self.rng.normal(size=(J, m))

    # -- ops ---------------------------------------------------------------------------------------------------------------------
    def do(self, op, touched=None, refused=False):
        if refused:
            op["refused"] = True
        status, value = apply(self.model, op)
        assert status == (INVALID if refused else OK), (self.name, self.N, len(self.ops), op["op"], status)
        Na, N = self.live, self.N
        op["cand"] = self.candidates(2, min(2, Na), min(5, Na))
        first, r = touched if touched is not None else (0, 1)
        near = [first - 1, first, first + r - 1, first + r, Na - 2, Na - 1, Na, Na + 1, 0, N - 1, int(self.rng.integers(0, N))]
        pick = [i for i in dict.fromkeys(near) if 0 <= i < N]
        op["rows"], op["cols_rd"] = np.array(pick, dtype=np.int32), np.array(pick[::-1], dtype=np.int32)
        self.ops.append(op)
        return value

    def correction(self, kind, m, cols, refused=False):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        if refused:                                        # a list the handle refuses: the operands are never looked at
            s = len(cols)
            return self.do({"op": kind, "cols": cols, "Hc": np.ones((m, s)), "R": np.eye(m), "nu": np.ones(m)}, refused=True)
        c, Hc, R, nu = self.candidates(1, m, len(cols), first=cols, nonzero=1)
        return self.do({"op": kind, "cols": c[0], "Hc": Hc[0], "R": R[0], "nu": nu[0]}, touched=(int(cols[0]), 1))

    def listing(self, must, s):
        """s distinct live indices in a seeded order that contain `must`"""
        rest = [int(i) for i in self.rng.permutation(self.live) if i not in must]
        return np.array(self.rng.permutation((list(must) + rest)[:s]), dtype=np.int32)

    def propagate(self, first, r, refused=False):
        Fr = self.thin(r, r) if self.form == "int" else np.eye(r) + 0.1 * self.rng.normal(size=(r, r))
        Qr = self.ints((r, r)) if self.form == "int" else 0.01 * self.noise(r)
        return self.do({"op": "propagate", "first": first, "Fr": Fr, "Qr": Qr, "dx": self.ints(r)}, (first, r), refused)

    def init(self, first, r, cols=None, W=None, refused=False):
        cols = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        G = None if cols is None else self.thin(r, len(cols))
        if W is None:
            W = self.ints((r, r)) if self.form == "int" else self.noise(r)
        return self.do({"op": "init", "first": first, "r": r, "cols": cols, "G": G, "W": W, "xb": self.ints(r, -9, 10)},
                       (first, r), refused)

    def swap(self, a, b, r, refused=False):
        return self.do({"op": "swap", "a": a, "b": b, "r": r}, (min(a, b), r), refused)

    def set_live(self, Na):
        return self.do({"op": "live", "Na": Na}, (max(0, min(Na, self.live) - 1), 1))

    def set_carry(self, on):
        return self.do({"op": "carry", "on": bool(on)})

    def flush(self):
        return self.do({"op": "flush"})

    def read(self, rows, cols):
        return self.do({"op": "sigma_block", "rows": np.array(rows, dtype=np.int32), "cols": np.array(cols, dtype=np.int32)},
                       (int(rows[0]), 1))

    def reset(self, corner):
        """set(Sigma): a fresh corner in front of the tail the session started with; drops what is pending"""
        S = self.Sigma0.copy()
        S[:self.top, :self.top] = corner
        return self.do({"op": "set", "F": None, "Sigma": S, "Q": None})

    def fresh(self, n):
        """an n x n covariance: integers in {-1, 0, 1} (int) / SPD (random)"""
        return self.rng.integers(-1, 2, size=(n, n)).astype(np.float64) if self.form == "int" else sc.spd(n, self.rng)

    def finish(self):
        return {"name": self.name, "N": self.N, "form": self.form, "top": self.top, "Sigma0": self.Sigma0, "x0": self.x0,
                "ops": self.ops}


def start(N, top, corner, x, seed=0):
    """(Sigma0, x0) of dimension N: `corner` (top x top) and x in front, unique_data everywhere else"""
    S, xs = sc.unique_data(N, seed)
    S[:top, :top] = corner
    xs[:top] = x
    return S, xs


def known_corner(form, rng, top, known):
    """the corner of a map whose first `known` states are known -- small integers in diagonal blocks of five over the pose
    block's rows and columns (int) / SPD (random) -- and the reference's prior on the states behind them"""
    C = PRIOR * np.eye(top)
    if form == "int":
        C[:known, :known] = dd.block_sigma(known, 5, rng) if known >= 5 else 0.0
        C[:3, :known], C[:known, :3] = rng.integers(-1, 2, size=(3, known)), rng.integers(-1, 2, size=(known, 3))
        x = np.concatenate([rng.integers(-9, 10, size=known), np.zeros(top - known)]).astype(np.float64)
    else:
        C[:known, :known] = sc.spd(known, rng)
        x = np.concatenate([rng.normal(size=known), np.zeros(top - known)])
    return C, x


# ---- the sessions -------------------------------------------------------------------------------------------------------------

def _grow_prune(N, form, rng, top, name="grow_prune"):
    """The INTEGRATION.md removal recipe inside a lifetime.  The map holds the pose, (top - 11) / 2 known landmarks and room
    for four more; live starts at top - 8.  Four landmarks are discovered one at a time: live += 2 with rows pending,
    init_block with s = 3 at the new end, a deferred correction that lists the new block.  propagate_block on the pose.
    Landmark 1 is removed from mid-map: swap_blocks with the last live block, init_block(s = 0) there, live -= 2 with rows
    pending (the flush at the old width); a row is appended; the freed slot is discovered again.  Then the stale-column case
    without the recipe's zeroing: a correction lists the last block, live -= 2 flushes it, two rows are appended at the
    narrow width, live += 2 grows over columns of the panels that still hold the flushed rows, and a correction and a readout
    look at them.  Three calls are refused on the way.  An exact rank update doubles the length of the numbers, so the
    integers last for about five corrections that build on each other: twice the script relocalises with set(Sigma) (a
    fresh corner, the rows dropped), each time followed by a correction so that rows are pending again."""
    known = top - 8
    assert known >= 3 and (known - 3) % 2 == 0 and top <= N
    C, x = known_corner(form, rng, top, known)
    S0, x0 = start(N, top, C, x, seed=1)
    s = Script(name, N, form, rng, S0, x0, top)
    s.set_live(known)
    s.correction("deferred", 1, s.listing([known - 1], min(3, known)))
    for k in range(4):
        assert s.form != "int" or (s.model.pending > 0)
        s.set_live(s.live + 2)
        first = s.live - 2
        s.init(first, 2, cols=[0, 1, 2])
        s.correction("deferred", 1 + k % 2, s.listing([first, first + 1, 0], 5))
    s.propagate(0, 3)
    s.propagate(s.live - 1, 2, refused=True)                  # a block past the live edge
    C2 = PRIOR * np.eye(top)
    C2[:s.live, :s.live] = s.fresh(s.live)
    s.reset(C2)
    lm1, last = known + 2, s.live - 2                          # landmark 1 of the four, the last live block
    s.correction("deferred", 2, s.listing([lm1, last], 5))
    s.swap(lm1, lm1 + 1, 2, refused=True)                      # overlapping blocks
    s.swap(lm1, last, 2)
    s.init(last, 2, cols=None, W=PRIOR * np.eye(2))
    assert s.form != "int" or (s.model.pending > 0 or not s.model.carry)
    s.set_live(s.live - 2)
    s.correction("deferred", 1, s.listing([0, lm1], 3))        # a row appended before the re-grow
    s.correction("deferred", 1, s.listing([s.live, 0], 3), refused=True)   # an index at the live dimension
    s.set_live(s.live + 2)
    first = s.live - 2
    s.init(first, 2, cols=[0, 1, 2])
    s.correction("deferred", 2, s.listing([first, first + 1, 1], 5))
    s.reset(s.fresh(top))
    s.correction("deferred", 2, s.listing([s.live - 1, s.live - 2, 0], 4))
    s.set_live(s.live - 2)                                     # not the recipe: the block stays coupled; flush at the old width
    s.correction("deferred", 2, s.listing([0, s.live - 1], 4))
    s.set_live(s.live + 2)
    s.read([s.live - 2, s.live - 1, 0, 3], [s.live - 1, s.live - 2, 1, 4])
    s.correction("deferred", 1, s.listing([s.live - 2, s.live - 1], 3))
    s.flush()
    return s.finish()


def _high(N):
    return N if (N - 11) % 2 == 0 else N - 1


def _recipe_start(N, first, r, form, rng, width=None):
    """(Sigma, lists) for the four corrections that make 64 rows (dense_carry_cases._start): they must not build on each
    other, so Sigma is dense in the rows and columns of the block [first, first + r) and otherwise zero outside four groups
    of five free indices below `width`, one per correction.  random: an SPD Sigma and four such lists."""
    W = N if width is None else width
    if form == "int":
        S, _, lists = cc._start(W, first, r, 64, rng)
        if W < N:
            S = np.pad(S, ((0, N - W), (0, N - W)))
            S[W:, :], S[:, W:] = rng.integers(-1, 2, size=(N - W, N)), rng.integers(-1, 2, size=(N, N - W))
        return S, lists
    free = rng.permutation([i for i in range(W) if not first <= i < first + r])[:20]
    return sc.spd(N, rng), [np.array(free[5 * g:5 * g + 5], dtype=np.int32) for g in range(4)]


def _policy_flips(N, form, rng):
    """Carry toggled with 1, 17 and 64 rows pending.  Every phase starts from set(Sigma) (which drops what is pending and
    leaves live and carry alone) on the Sigma of dense_carry_cases._start: dense in the rows and columns of the block
    [62, 65), four groups of five free indices for the four corrections of the 64 rows.  Per phase: the rows are made, then
    carry on, propagate_block (carried), carry off, carry on (two flips, rows pending), swap_blocks (carried), a readout
    through the rows, carry off, init_block (flushes first), sigma_block (nothing left)."""
    first, r, other = 62, 3, 10
    x0 = rng.integers(-9, 10, size=N).astype(np.float64) if form == "int" else rng.normal(size=N)
    s = Script("policy_flips", N, form, rng, np.zeros((N, N)), x0, N, carry=False)
    for p in (1, 17, 64):
        Sp, lists = _recipe_start(N, first, r, form, rng)
        s.do({"op": "set", "F": None, "Sigma": Sp, "Q": None})
        if p == 64:
            for (m, _), lst in zip(cc.RECIPE[64], lists):
                s.correction("deferred", m, lst)
        else:
            s.correction("deferred", p, s.listing([first + 1, int(lists[0][0])], 5))
        assert s.form != "int" or (s.model.pending == p)
        s.set_carry(True)
        s.propagate(first, r)
        s.set_carry(False)
        s.set_carry(True)
        s.swap(first, other, r)
        assert s.form != "int" or (s.model.pending == p)
        s.read([first, first + 1, other, other + 1, 0, N - 1], [other + 2, first + 2, 2, first, N - 1])
        s.set_carry(False)
        assert s.form != "int" or (s.model.pending == p)
        s.init(first, r, cols=[int(c) for c in lists[0][:3]])
        assert s.form != "int" or (s.model.pending == 0)
        s.read([first, 0, N - 1], [first, first + 2, N - 1])
    return s.finish()


def without_flips(session):
    """the same script with the carry switches removed (the indices of the kept ops come along)"""
    keep = [i for i, op in enumerate(session["ops"]) if op["op"] != "carry"]
    return dict(session, ops=[session["ops"][i] for i in keep]), keep


def _capacity(N, form, rng):
    """64 rows by the recipe dense_carry_cases.RECIPE[64] at live = N - 1; swap_blocks with r = 64 where two such blocks fit
    (else r = 3); live grows by one (the new row and column of Sigma are not zero); a deferred correction with m = 2 that
    lists the new index and forces the automatic flush; sigma_block; flush (2 rows); flush with nothing pending."""
    r = 64 if N - 1 >= 128 else 3
    a = 0 if r == 64 else 60
    b = N - 1 - r
    S0, lists = _recipe_start(N, a, r, form, rng, width=N - 1)
    x0 = rng.integers(-9, 10, size=N).astype(np.float64) if form == "int" else rng.normal(size=N)
    s = Script("capacity", N, form, rng, S0, x0, N)
    s.set_live(N - 1)
    for (m, _), lst in zip(cc.RECIPE[64], lists):
        s.correction("deferred", m, lst)
    assert s.form != "int" or (s.model.pending == 64)
    s.swap(a, b, r)
    s.set_live(N)
    s.correction("deferred", 2, s.listing([N - 1, a], 5))
    assert s.form != "int" or (s.model.pending == 2)
    s.read([N - 1, N - 2, a, b], [N - 1, 0, b + r - 1, a])
    s.flush()
    s.flush()
    return s.finish()


def _general_rows(s, J, m, low, high):
    """H (J, m, N): every row has one entry at a column < live (from `low`) and one at a column >= live (from `high`)"""
    H = np.zeros((J, m, s.N))
    for j in range(J):
        for a in range(m):
            cols = [int(s.rng.choice(low)), int(s.rng.choice(high))]
            H[j, a, cols] = s.rng.choice([-1.0, 1.0], size=2) if s.form == "int" else s.rng.normal(size=2)
    return H


def _dense_R(s, H):
    """R (J, m, m) that makes S_j = diag(2^k) on the current covariance (int) / well-conditioned (random)"""
    J, m = H.shape[0], H.shape[1]
    if s.form != "int":
        return np.stack([s.noise(m) for _ in range(J)])
    Sig = s.model.sigma_cur
    return np.stack([np.diag(2.0 ** s.rng.integers(0, 3, size=m)) - H[j] @ Sig @ H[j].T for j in range(J)])


def _dense_between(N, form, rng):
    """The dense-operand calls between structured ones, with live < N, rows pending and a COUPLED tail: Sigma0 is small
    integers in diagonal blocks of five and live = 5 k + 2 cuts one of them, which coupling(live) records.  The script:
    a deferred correction; score (general H with columns >= live); a deferred correction; correct (general H, S a diagonal of
    powers of two); a deferred correction; set(F, Q) with the row pending; propagate(1) with an integer F; a deferred
    correction; set(F) alone (the rows stay); set(Sigma) with rows pending (they are dropped, live and carry stay); a refused
    list; a live deferred correction; flush; sigma.  No NaNs here: the dense calls read all of Sigma."""
    Na = 5 * ((N - 6) // 5) + 2
    blocks = lambda k: np.array(rng.permutation(np.arange(5 * k, 5 * k + 5)), dtype=np.int32)
    if form == "int":
        S0, x0 = dd.block_sigma(N, 5, rng), rng.integers(-9, 10, size=N).astype(np.float64)
    else:
        S0, x0 = sc.spd(N, rng), rng.normal(size=N)
    s = Script("dense_between", N, form, rng, S0, x0, N)
    s.set_live(Na)
    count, most = s.do({"op": "coupling", "Na": Na})
    assert count > 0 and most > 0.0, "the tail must be coupled"
    low, high = np.arange(Na - 2, Na), np.arange(Na, min(N, Na + 3))        # both sides of the cut, inside the cut block
    s.correction("deferred", 2, blocks(0))
    H = _general_rows(s, 2, 2, low, high)
    nu = s.ints((2, 2))
    s.do({"op": "dense_score", "H": H, "R": _dense_R(s, H), "nu": nu}, (Na - 1, 2))
    s.correction("deferred", 2, blocks(1))
    H = _general_rows(s, 1, 2, np.arange(10, 15), high)
    s.do({"op": "dense_correct", "H": H[0], "R": _dense_R(s, H)[0], "nu": s.ints(2)}, (Na - 1, 2))
    s.correction("deferred", 1, blocks(3))
    F = np.eye(N)
    for i, j in ((0, Na), (Na, 1), (Na - 1, N - 1), (N - 1, 16), (17, 18), (N - 2, Na + 1)):
        F[i, j] = 1.0 if form == "int" else 0.3
    Q = np.diag(s.ints(N, 0, 3)) if form == "int" else 0.01 * np.eye(N)
    s.do({"op": "set", "F": F, "Sigma": None, "Q": Q})
    assert s.form != "int" or (s.model.pending == 1)
    s.do({"op": "dense_propagate"}, (Na - 1, 2))
    s.correction("deferred", 2, blocks(4))
    s.do({"op": "set", "F": np.eye(N) + np.diag(np.ones(N - 1), 1) * (1.0 if form == "int" else 0.1), "Sigma": None, "Q": None})
    assert s.form != "int" or (s.model.pending == 2)
    S1 = dd.block_sigma(N, 5, rng) if form == "int" else sc.spd(N, rng)
    s.do({"op": "set", "F": None, "Sigma": S1, "Q": None})
    assert s.form != "int" or (s.model.pending == 0 and s.live == Na)
    s.correction("deferred", 1, [0, Na, 2], refused=True)
    s.correction("deferred", 2, blocks(2))
    s.flush()
    s.do({"op": "sigma"})
    return s.finish()


WALK = [63, 64, 65, 127, 128, 129, 65, 1, 129]


def _edges_walk(N, form, rng):
    """N = 203.  Live goes through 63, 64, 65, 127, 128, 129, 65, 1, 129; at each stop an eager correct_sparse, a deferred
    one whose list ends at Na - 1, and a swap_blocks of r = 1 blocks that include index Na - 1 (refused at Na = 1, where no
    two blocks exist).  The deferred rows are pending at every change of live: the shrinks 129 -> 65 -> 1 flush at the old
    width, the grows zero the new columns; the last grow, 1 -> 129, crosses both strip edges with a row pending."""
    assert N == 203
    top = max(WALK)
    if form == "int":
        C, x = dd.block_sigma(top, 5, rng), rng.integers(-9, 10, size=top).astype(np.float64)
        C[top - 4:, top - 4:] = rng.integers(-1, 2, size=(4, 4))
    else:
        C, x = sc.spd(top, rng), rng.normal(size=top)
    S0, x0 = start(N, top, C, x, seed=2)
    s = Script("edges_walk", N, form, rng, S0, x0, top)
    for k, Na in enumerate(WALK):
        s.set_live(Na)
        if Na == 1:
            s.correction("eager", 1, [0])
            s.correction("deferred", 1, [0])
            s.swap(0, 0, 1, refused=True)
            continue
        s.correction("eager", 1, np.arange(5 * k, 5 * k + 3)[::-1])           # block k: the eager ones do not build on each other
        s.correction("deferred", 1, [Na - 1, Na - 2, Na - 3])
        s.swap(Na - 1, 50 + k, 1)
    s.flush()
    return s.finish()


BUILDERS = {"grow_prune": lambda N, form, rng: _grow_prune(N, form, rng, 11),
            "grow_prune_high": lambda N, form, rng: _grow_prune(N, form, rng, _high(N), "grow_prune_high"),
            "policy_flips": _policy_flips, "capacity": _capacity, "dense_between": _dense_between, "edges_walk": _edges_walk}
LISTED = {name: ([203] if name == "edges_walk" else SIZES) for name in BUILDERS}      # none drops 203
CASES = [(name, N) for name in BUILDERS for N in LISTED[name]]
TWO_HANDLES = [("two_a", 67, 35), ("two_b", 131, 131), ("two_c", 67, 11)]              # (name, N, the corner's final size)


def _seed(name, N, form):
    return 100000 * (1 + sorted(BUILDERS).index(name) if name in BUILDERS else 50 + len(name)) + 100 * N + (form == "random")


def _checked(session):
    """an integer session must be exact on every model it is run on, not only on the one that wrote it"""
    for carry in (True, False):
        run(session, carry)
        run(session, carry, PlainModel, check=True)
    return session


@functools.lru_cache(maxsize=None)
def session(name, N, form="int"):
    """the named session at dimension N; a seed on which a value leaves float64's integers is replaced by the next"""
    build = BUILDERS.get(name) or (lambda n, f, rng: _grow_prune(n, f, rng, dict((a, c) for a, _, c in TWO_HANDLES)[name], name))
    if form != "int":
        return build(N, form, np.random.default_rng(_seed(name, N, form)))
    for attempt in range(12):
        try:
            return _checked(build(N, form, np.random.default_rng(_seed(name, N, form) + 7 * attempt)))
        except cc.Inexact:
            continue
    raise cc.Inexact(f"no exact session {name} at N = {N}")


# ---- the long-double margins -------------------------------------------------------------------------------------------------

def finite_part(session):
    """the index range [0, top) outside which Sigma and the state hold unique_data (NaNs among it)"""
    return session["top"]


def margin(name, N):
    """how far the float64 plain model is from the same replay in np.longdouble on the random form: the largest per-block
    relative covariance error (parity.cov_err) and the largest absolute state error over all steps -> (cov, state)"""
    from parity import cov_err
    ses = session(name, N, "random")
    top = finite_part(ses)
    a, b = run(ses, True, PlainModel), run(ses, True, PlainModel, dtype=np.longdouble)
    cov = max(max(cov_err(ra["Sigma_cur"][:top, :top], np.asarray(rb["Sigma_cur"][:top, :top], dtype=np.float64)).values())
              for ra, rb in zip(a, b))
    st = max(float(np.abs(ra["state"][:top] - np.asarray(rb["state"][:top], dtype=np.float64)).max()) for ra, rb in zip(a, b))
    return cov, st
