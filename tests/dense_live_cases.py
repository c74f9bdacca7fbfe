"""Shared by tests/test_gpu_dense64_live.py and tests/test_dense64_live_host.py: the grid of (N, Na) on which the live
dimension of the dense fp64 handle (ekf_dense64_set_live) is run, and the integer chains of width Na -- an eager sparse
correction, a deferred one, propagate_block, init_block, a deferred correction that lists the new block, the flush -- on the
carried model of tests/dense_carry_cases.py, which checks every product it forms to be exact in float64.  run_model replays
a chain at its own width or EMBEDDED in a larger N with a decoupled tail, which is how the host test shows that the
full-width call leaves the tail and both rectangles alone and equals the filter of dimension Na in the corner."""
import functools

import numpy as np

import dense_carry_cases as cc
import dense_deferred_cases as dd

GRID_N = [65, 200, 403]
GRID_NA = [1, 3, 5, 17, 63, 64, 65, 127, 128, 129, 191]
ORDERS = dd.ORDERS
PAIRS = dd.PAIRS                                           # (m, s): (1, 1), (2, 5), (16, 16), (17, 5), (2, 64)


def pairs():
    """the grid: every (N, Na) with Na < N; none is skipped"""
    return [(N, Na) for N in GRID_N for Na in GRID_NA if Na < N]


def shapes(Na):
    """the (m, s) a filter of dimension Na can take"""
    return [(m, s) for m, s in PAIRS if m <= Na and s <= Na]


def apply(model, op):
    """one call of a chain on a CarriedModel -> nis of a correction, else None"""
    k = op["op"]
    if k == "eager":                                       # correct_sparse: flushes first, applies at once
        model.flush()
        nis = model.correct_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
        model.flush()
        return nis
    if k == "deferred":
        return model.correct_deferred(op["cols"], op["Hc"], op["R"], op["nu"])
    if k == "propagate":
        model.propagate_block(op["first"], op["Fr"], op["Qr"], op["dx"])
    elif k == "init":
        model.init_block(op["first"], op["r"], op["cols"], op["G"], op["W"], op["xb"])
    else:
        model.flush()
    return None


def _build(Na, order, m, s, seed):
    rng = np.random.default_rng(seed)
    Sigma0 = rng.integers(-1, 2, size=(Na, Na)).astype(np.float64)
    x0 = rng.integers(-9, 10, size=Na).astype(np.float64)
    model = cc.CarriedModel(Sigma0, x0)
    ops = []
    ints = lambda shape, lo=-2, hi=3: rng.integers(lo, hi, size=shape).astype(np.float64)

    def done(op):
        apply(model, op)
        cols, Hc, R, nu, _ = dd.exact_candidates(model.sigma_cur, 2, min(2, Na), min(5, Na), "scattered", rng)
        op["cand"] = (cols, Hc, R, nu)                      # scored after the call, through whatever is pending
        ops.append(op)

    def correction(kind, mm, ss, how, first=None):
        cols, Hc, R, nu, _ = dd.exact_candidates(model.sigma_cur, 1, mm, ss, how, rng, first=first)
        done({"op": kind, "cols": cols[0], "Hc": Hc[0], "R": R[0], "nu": nu[0]})

    correction("eager", m, s, order)
    correction("deferred", m, s, "scattered")
    r = min(3, Na)
    done({"op": "propagate", "first": 0, "Fr": dd.sparse_rows(rng, r, r, 3), "Qr": ints((r, r)), "dx": ints(r)})
    r2 = 2 if Na >= 4 else 1
    first2, si = Na - r2, min(3, Na - r2)                  # the last block of the live corner: it touches column Na - 1
    outside = rng.permutation(first2)
    done({"op": "init", "first": first2, "r": r2, "cols": np.array(outside[:si], dtype=np.int32) if si else None,
          "G": dd.sparse_rows(rng, r2, si, 3) if si else None, "W": ints((r2, r2)), "xb": ints(r2, -9, 10)})
    ss = min(5, Na)
    lst = np.array([first2] + [int(i) for i in rng.permutation(Na) if i != first2][:ss - 1], dtype=np.int32)
    correction("deferred", min(2, Na), ss, "scattered", first=lst)
    done({"op": "flush"})
    return {"Na": Na, "Sigma0": Sigma0, "x0": x0, "ops": ops}


@functools.lru_cache(maxsize=None)
def live_chain(Na, order, m, s):
    """the chain of one (Na, order, (m, s)); a seed on which a value leaves float64's integers is replaced by the next"""
    base = 1000 * Na + 100 * ORDERS.index(order) + PAIRS.index((m, s))
    for attempt in range(12):
        try:
            return _build(Na, order, m, s, 7 * base + attempt)
        except cc.Inexact:
            continue
    raise cc.Inexact(f"no exact chain for Na = {Na}, {order}, ({m}, {s})")


def run_model(chain, carry, Sigma0=None, x0=None):
    """the chain's calls on a fresh CarriedModel -- at width Na, or on the (Sigma0, x0) of a larger N that embeds it ->
    per call {nis0, state, pending, Sigma_cur, S, nis}"""
    model = cc.CarriedModel(chain["Sigma0"] if Sigma0 is None else Sigma0, chain["x0"] if x0 is None else x0, carry=carry)
    out = []
    for op in chain["ops"]:
        nis0 = apply(model, op)
        S, nis = model.scores(*op["cand"])
        out.append({"nis0": nis0, "state": model.state.copy(), "pending": model.pending, "Sigma_cur": model.sigma_cur,
                    "S": S, "nis": nis})
    return out


def tail_block(k, seed):
    """a dense, non-trivial k x k tail in small integers (not symmetric) and a tail state"""
    rng = np.random.default_rng(seed)
    B = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=(k, k)) + 100.0 * np.eye(k)      # no entry is zero
    return B, rng.integers(-9, 10, size=k).astype(np.float64)


def embed(chain, N, seed=0):
    """(Sigma0, x0) of dimension N: the chain's corner, a decoupled tail that holds tail_block"""
    Na = chain["Na"]
    B, xt = tail_block(N - Na, seed)
    S = np.zeros((N, N))
    S[:Na, :Na], S[Na:, Na:] = chain["Sigma0"], B
    return S, np.concatenate([chain["x0"], xt])
