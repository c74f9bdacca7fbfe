"""No GPU: the model that tests/test_gpu_dense64_session.py holds the dense fp64 handle to is right.  Every named session
of tests/dense_session_cases.py builds at every N it is listed for (none is dropped, which is asserted here so that the GPU
test cannot hide a case); on the integer sessions HandleModel -- the carried representation with the live dimension, the
swap, the dense-operand calls and set -- equals, after every call and in every number, a plain dense model that holds one
N x N Sigma and applies each call as its embedded dense matrices; the carried and the flush-first model agree; the scripts
hold the situations the issue names (a row pending at a shrink and one appended before the re-grow, the policy switched with
1, 17 and 64 rows pending, the automatic flush, a coupled tail under the dense calls, every refusal).  For the random forms
the float64 plain model is replayed in np.longdouble: its distance is the reference's own error, the number the measured
device error is set against in profiles/r17/dense64_sessions.txt."""
import numpy as np
import pytest

import dense_carry_cases as cc
import dense_session_cases as ss
from parity import FP64_TOL

CASE_IDS = [f"{name}-N{N}" for name, N in ss.CASES]
ALL = ss.CASES + [(name, N) for name, N, _ in ss.TWO_HANDLES]


def _eq(a, b):
    """the same numbers (a NaN equals a NaN: the tail's unique data)"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_every_named_session_builds_at_every_size_it_is_listed_for():
    assert set(ss.BUILDERS) == {"grow_prune", "grow_prune_high", "policy_flips", "capacity", "dense_between", "edges_walk"}
    for name in ss.BUILDERS:
        assert ss.LISTED[name] == ([203] if name == "edges_walk" else [67, 131, 203])
    assert len(ss.CASES) == 5 * 3 + 1 and [(n, N) for n, N, _ in ss.TWO_HANDLES] == [("two_a", 67), ("two_b", 131), ("two_c", 67)]
    for name, N in ALL:                                               # Inexact (no exact seed) is an error here, never a skip
        for form in ("int", "random"):
            ses = ss.session(name, N, form)
            assert ses["N"] == N and len(ses["ops"]) >= 10 and ses["Sigma0"].shape == (N, N)
        a, b = ss.session(name, N), ss.session(name, N, "random")     # the random form keeps the op list
        assert [o["op"] for o in a["ops"]] == [o["op"] for o in b["ops"]]
        for oa, ob in zip(a["ops"], b["ops"]):
            assert oa.get("refused") == ob.get("refused")
            for k in ("first", "r", "a", "b", "Na", "on"):
                assert oa.get(k) == ob.get(k)
            for k in ("Hc", "H", "Fr", "G"):
                assert np.shape(oa.get(k)) == np.shape(ob.get(k))


@pytest.mark.parametrize("name,N", ALL, ids=[f"{n}-N{N}" for n, N in ALL])
def test_handle_model_equals_the_plain_dense_model_and_carry_on_equals_carry_off(name, N):
    ses = ss.session(name, N)
    on, off = ss.run(ses, True), ss.run(ses, False)
    plain = ss.run(ses, True, ss.PlainModel, check=True)
    top = ses["top"]
    for i, (a, b, p) in enumerate(zip(on, off, plain)):
        at = ss.describe(ses, i)
        for r in (a, b):
            assert r["status"] == p["status"] and r["live"] == p["live"], at
            assert _eq(r["Sigma_cur"], p["Sigma_cur"]), (at, np.argwhere(r["Sigma_cur"] != p["Sigma_cur"])[:3])
            assert _eq(r["state"], p["state"]) and _eq(r["S"], p["S"]) and _eq(r["nis"], p["nis"]), at
            if r["block"] is not None:
                assert _eq(r["block"], p["Sigma_cur"][np.ix_(ses["ops"][i]["rows"], ses["ops"][i]["cols_rd"])]), at
            va, vp = r["value"], p["value"]
            if isinstance(vp, tuple) and isinstance(vp[0], np.ndarray):
                assert _eq(va[0], vp[0]) and _eq(va[1], vp[1]), at
            elif vp is not None:
                assert _eq(va, vp), at
            else:
                assert va is None, at
        # outside the largest corner nothing is ever written: the bits of the start
        S0 = ses["Sigma0"]
        if top < N and not any(o["op"] == "set" for o in ses["ops"][:i + 1]):
            out = np.ones((N, N), dtype=bool)
            out[:top, :top] = False
            assert np.array_equal(a["Sigma_cur"].view(np.uint64)[out], S0.view(np.uint64)[out]), at
            assert np.array_equal(a["state"][top:].view(np.uint64), ses["x0"][top:].view(np.uint64)), at
    assert on[-1]["pending"] == off[-1]["pending"] == 0
    assert any(r["pending"] > 0 for r in on)


def test_the_scripts_hold_the_situations_they_are_written_for():
    for N in ss.SIZES:
        ses = ss.session("grow_prune", N)
        recs, ops = ss.run(ses, True), ses["ops"]
        lives = [r["live"] for r in recs]
        assert lives[0] == 3 and max(lives) == 11
        shrinks = [i for i in range(1, len(ops)) if ops[i]["op"] == "live" and lives[i] < lives[i - 1]]
        grows = [i for i in range(1, len(ops)) if ops[i]["op"] == "live" and lives[i] > lives[i - 1]]
        assert len(shrinks) == 2 and len(grows) == 6
        for i in shrinks:                                             # a row pending at the shrink: it flushes
            assert recs[i - 1]["pending"] > 0 and recs[i]["pending"] == 0
            g = min(j for j in grows if j > i)                        # rows appended before the re-grow: it does not flush
            assert recs[g - 1]["pending"] > 0 and recs[g]["pending"] == recs[g - 1]["pending"]
        assert all(recs[i]["pending"] == recs[i - 1]["pending"] > 0 for i in grows)
        assert [o["op"] for o in ops if o.get("refused")] == ["propagate", "swap", "deferred"]
        kinds = [o["op"] for o in ops]
        assert kinds.count("init") == 6 and kinds.count("swap") == 2 and "propagate" in kinds
        assert sum(1 for o in ops if o["op"] == "init" and o["cols"] is None) == 1

        ses = ss.session("policy_flips", N)
        recs, ops = ss.run(ses, False), ses["ops"]
        flips = [recs[i - 1]["pending"] for i, o in enumerate(ops) if o["op"] == "carry"]
        assert sorted(set(flips)) == [1, 17, 64] and len(flips) == 12
        between = {o["op"] for o in ops}
        assert {"propagate", "init", "swap", "sigma_block"} <= between
        plainer, keep = ss.without_flips(ses)                        # the flips removed, flush-first: the same Sigma
        flat = ss.run(plainer, False)
        assert len(flat) == len(ops) - 12
        for r, i in zip(flat, keep):
            assert _eq(r["Sigma_cur"], recs[i]["Sigma_cur"]) and _eq(r["state"], recs[i]["state"]), ss.describe(ses, i)
        assert any(r["pending"] != recs[i]["pending"] for r, i in zip(flat, keep))   # the flips did change what was carried

        ses = ss.session("capacity", N)
        recs, ops = ss.run(ses, True), ses["ops"]
        assert [o["op"] for o in ops] == ["live"] + ["deferred"] * 4 + ["swap", "live", "deferred", "sigma_block", "flush", "flush"]
        assert [r["pending"] for r in recs] == [0, 17, 34, 51, 64, 64, 64, 2, 2, 0, 0]
        assert ops[5]["r"] == (64 if N >= 129 else 3) and recs[6]["live"] == N and N - 1 in ops[7]["cols"]

        ses = ss.session("dense_between", N)
        recs, ops = ss.run(ses, True), ses["ops"]
        kinds = [o["op"] for o in ops]
        assert recs[1]["value"][0] > 0 and all(r["live"] < N for r in recs)          # a coupled tail, live < N throughout
        for k in ("dense_score", "dense_correct", "dense_propagate"):                # each flushes rows that were pending
            i = kinds.index(k)
            assert recs[i - 1]["pending"] > 0 and recs[i]["pending"] == 0, k
        i = kinds.index("dense_correct")
        assert ops[i]["H"][:, recs[i]["live"]:].any()
        sets = [i for i, k in enumerate(kinds) if k == "set"]
        assert [recs[i - 1]["pending"] for i in sets] == [1, 2, 2] and [recs[i]["pending"] for i in sets] == [1, 2, 0]
        assert all(recs[i]["live"] == recs[i - 1]["live"] and recs[i]["carry"] for i in sets)
        assert kinds[-3:] == ["deferred", "flush", "sigma"] and sum(1 for o in ops if o.get("refused")) == 1

    ses = ss.session("edges_walk", 203)
    recs, ops = ss.run(ses, True), ses["ops"]
    assert [o["Na"] for o in ops if o["op"] == "live"] == ss.WALK == [63, 64, 65, 127, 128, 129, 65, 1, 129]
    for i, o in enumerate(ops):
        if o["op"] == "live" and i:
            assert recs[i - 1]["pending"] > 0                         # a row waits at every change of live
            assert recs[i]["pending"] == (0 if o["Na"] < recs[i - 1]["live"] else recs[i - 1]["pending"])
        if o["op"] == "swap" and not o.get("refused"):
            assert o["r"] == 1 and recs[i]["live"] - 1 in (o["a"], o["b"])
    kinds = [o["op"] for o in ops]
    assert kinds.count("eager") == kinds.count("deferred") == 9 and kinds.count("swap") == 9
    assert [o["op"] for o in ops if o.get("refused")] == ["swap"]


def test_a_wrong_model_is_noticed():
    """the three defects the sessions are meant to catch, planted in the model: each changes a recorded number"""
    ses = ss.session("grow_prune", 67)
    want = ss.run(ses, True)

    class NarrowFlush(ss.HandleModel):                                # the flush on shrink cut for the new width
        def set_live(self, Na):
            if Na < self.live:
                self.Kt[:, Na:], self.Tp[:, Na:] = 0.0, 0.0
            return super().set_live(Na)

    class HalfSwap(ss.HandleModel):                                   # the T panel left behind by the swap
        def swap_blocks(self, a, b, r):
            T = self.Tp.copy()
            out = super().swap_blocks(a, b, r)
            if out[0] == ss.OK and self.pending:
                self.Tp = T
            return out

    for wrong in (NarrowFlush, HalfSwap):
        try:
            got = ss.run(ses, True, wrong)
        except (cc.Inexact, np.linalg.LinAlgError):                                            # a later correction no longer meets its own S: noticed
            continue
        assert any(not _eq(g["Sigma_cur"], w["Sigma_cur"]) for g, w in zip(got, want)), wrong.__name__


LONG = np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.skipif(not LONG, reason="np.longdouble is no wider than float64 on this platform")
@pytest.mark.parametrize("name", list(ss.BUILDERS))
def test_long_double_margins_of_the_random_forms(name):
    """the float64 plain model against the same replay in long double, at the session's smallest size (the replay runs
    numpy's unblocked long-double products): far inside the contract, and printed for profiles/r17/dense64_sessions.txt"""
    N = ss.LISTED[name][0]
    cov, st = ss.margin(name, N)
    print(f"margin {name} N={N}: cov {cov:.3e} state {st:.3e}")
    assert np.isfinite(cov) and np.isfinite(st) and 0.0 < cov < FP64_TOL / 100 and st < FP64_TOL / 100


def test_inverse_in_long_double():
    rng = np.random.default_rng(4)
    A = (rng.normal(size=(17, 17)) + 17 * np.eye(17)).astype(np.longdouble)
    assert np.abs(ss.inverse(A) @ A - np.eye(17)).max() < 64 * np.finfo(np.longdouble).eps
    with pytest.raises(cc.Inexact):
        cc.exact_product(np.array([[2.0 ** 30]]), np.array([[2.0 ** 30]]))
