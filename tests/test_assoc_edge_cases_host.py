"""tests/assoc_edge_cases.py on the CPU: the stated decisions, known counts and scores hold on the checker (OracleEKF,
DENSE) and, where oracle/_ref/libekf_slam_ref.so is built, the reference's own EKF_SLAM agrees on the decisions; the
case table covers every pair kind each form's layout has."""
from fractions import Fraction

import numpy as np
import pytest

import assoc_edge_cases as ec

FORMS = list(ec.FORMS)


DENSE_MAX_N = 130   # the DENSE checker multiplies full N x N matrices per landmark: minutes beyond this; STRUCTURED there


def _oracle_run(oracle, c):
    f = oracle.OracleEKF(c.n, oracle.DENSE if c.n <= DENSE_MAX_N else oracle.STRUCTURED, params=ec.PARAMS)
    ec.init_by_measurement(f, c)
    return f


def _unique_cases():
    """cases by content: the forms share shapes, and the checker does not know forms"""
    seen, out = set(), []
    for form in FORMS:
        for cid, c in ec.cases_for(form):
            key = (c.n, c.M, c.name, c.J)
            if key not in seen:
                seen.add(key)
                out.append((f"{form}-{cid}", c))
    return out


UNIQUE = _unique_cases()


@pytest.mark.parametrize("n", sorted({c.n for _, c in UNIQUE}))
def test_checker_returns_the_stated_decisions(oracle, n):
    for cid, c in UNIQUE:
        if c.n != n:
            continue
        f = _oracle_run(oracle, c)
        s0, c0 = f.state, f.cov
        w, nanmask = ec.masked(c.world.reshape(-1))
        assert np.array_equal(ec.masked(s0[3:])[0], w) and np.array_equal(np.isnan(s0[3:]), nanmask), f"{cid}: world not exact"
        assert np.array_equal(c0, np.diag(np.r_[np.zeros(3), np.full(2 * c.n, ec.PARAMS[0])])), cid
        # the stated scores, as exact fractions, of the case's first edge reading
        m = c.readings[c.first]
        got = {i: Fraction(f.maha(m[0], m[1], i)) for i in c.scores}
        assert got == c.scores, f"{cid}: scores {got} vs stated {c.scores}"
        if c.kind == "tie":
            lo, hi = sorted(c.scores)
            assert np.float64(f.maha(m[0], m[1], lo)).tobytes() == np.float64(f.maha(m[0], m[1], hi)).tobytes(), cid
        near = {i for i in range(c.n) if c.world[i, 0] < ec.FAR0 or np.isnan(c.world[i, 0])}
        far = [i for i in (0, 1, c.M // 2, c.M - 1) if i not in near]
        assert far and all(f.maha(m[0], m[1], i) > 16.0 for i in far), cid
        known = ec.known_list(c)
        dec = f.data_association(c.readings, known)
        assert tuple(int(d) for d in dec) == tuple(c.decisions), f"{cid}: decisions {dec} vs stated {c.decisions}"
        assert int(known.sum()) == c.known_after and known[:c.known_after].all(), cid
        s1, c1 = f.state, f.cov
        if c.dropped:
            assert s1.tobytes() == s0.tobytes() and c1.tobytes() == c0.tobytes(), f"{cid}: a dropped reading changed something"
        for i in c.unchanged:
            r = ec.rows_of(i)
            assert s1[r].tobytes() == s0[r].tobytes() and c1[r].tobytes() == c0[r].tobytes() \
                and c1[:, r].tobytes() == c0[:, r].tobytes(), f"{cid}: the loser {i} changed"
        if c.new_slot >= 0:
            assert tuple(s1[ec.rows_of(c.new_slot)]) == tuple(c.readings[-1]), cid
        for j, d in enumerate(c.decisions):   # every winner moved towards its reading
            if d >= 0 and d != c.new_slot:
                assert s0[3 + 2 * d] < s1[3 + 2 * d] < c.readings[j, 0], f"{cid}: winner {d} did not move"


def test_every_far_landmark_scores_above_gate_new(oracle):
    """all of them, once per map size (the per-case test samples)"""
    for n in sorted({c.n for _, c in UNIQUE}):
        c = ec.tie(n, 0, n - 1)
        f = _oracle_run(oracle, c)
        sc = np.array([f.maha(1.25, 0.0, i) for i in range(1, n - 1)])
        assert sc.min() > 16.0 and sc.min() == 4.0 * (65.0 - 1.25) ** 2, n
        if n > 101:
            assert f.maha(1.5, 0.0, 100) == 105625.0   # the issue's far row: far landmark 100


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.RefEKF._load()
    except FileNotFoundError:
        pytest.skip("oracle/_ref/libekf_slam_ref.so not built (reference sources absent at build time)")
    return oracle.RefEKF


REF_MAX_N = 300   # calculate_maha_dis is a dense 2 x N by N x N product per landmark: a second per reading beyond this


def test_reference_build_agrees_on_the_decisions(ref):
    """The reference takes no parameters (R = 0.01, gates 10 and 1): the world is set through state and Sigma with landmark
    variance 0.25 - 0.01, so that S00 = 0.25 again and every score that decides is the same exact fraction.  What it
    cannot express is left out: gate_new = 16 (both gate_new cases) and maps beyond REF_MAX_N (cost).  It reports no
    decision; the winner is the landmark that moved."""
    ran = 0
    for cid, c in UNIQUE:
        if c.kind.startswith("gate_new") or c.n > REF_MAX_N or c.J > ec.STAGED_FILLERS:
            continue
        r = ref(c.n)
        N = 3 + 2 * c.n
        state = np.zeros(N)
        state[3:] = c.world.reshape(-1)
        r.state, r.cov = state, np.diag(np.r_[np.zeros(3), np.full(2 * c.n, 0.25 - 0.01)])
        r.set_init_flag(1)
        m = c.readings[0]
        for i, want in c.scores.items():
            assert Fraction(r.maha(m[0], m[1], i)) == want, f"{cid}: reference score of {i}"
        known = ec.known_list(c)
        r.data_association(c.readings, known)
        s1 = r.state
        moved = {i for i in range(c.n) if not np.isnan(state[3 + 2 * i]) and s1[3 + 2 * i] != state[3 + 2 * i]}
        assert moved == {d for d in c.decisions if d >= 0}, f"{cid}: the reference moved {sorted(moved)}, stated {c.decisions}"
        assert int(known.sum()) == c.known_after, cid
        ran += 1
    assert ran >= 40


@pytest.mark.parametrize("form", FORMS)
def test_case_table_covers_the_layout(form):
    f = ec.FORMS[form]
    need = ec.required_pair_kinds(f["layout"])
    # the list of the issue, restated: which kinds a layout with these properties must have
    want = {"neighbour", "first_last"} | ({"wave"} if f["layout"]["waves"] > 1 else set()) \
        | ({"own_scan", "decisive"} if f["layout"]["T"] else set()) | ({"outer"} if f["layout"]["outer"] else set())
    assert need == want
    cases = [c for _, c in ec.cases_for(form)]
    T, outer = f["layout"]["T"], f["layout"]["outer"]
    if f.get("sequence_only"):
        c = cases[0]
        pairs = list(zip(c.decisions, c.unchanged))
        have = set()
        for lo, hi in pairs:
            have |= _classify(lo, hi, c.M, T, outer)
    else:
        have = set()
        for c in cases:
            if c.kind in ("tie", "near_tie"):
                lo, hi = sorted(c.scores)
                kinds = _classify(lo, hi, c.M, T, outer)
                assert c.pair_kind in kinds, f"{c.name}: labelled {c.pair_kind}, is {kinds}"
                have.add(c.pair_kind)
        kinds_of = {c.kind for c in cases}
        assert {"tie", "near_tie", "gate_update_exact", "gate_update_below", "nan_low", "sequence"} <= kinds_of, form
        assert "gate_new_exact_full" in kinds_of or any("full-map drop" in s for s in f["notes"]), form
        assert "gate_new_exact_append" in kinds_of or any("no append case" in s for s in f["notes"]), form
    assert need <= have, f"{form}: the table lacks {need - have}"
    if T:
        assert "decisive" in have, f"{form}: no (a + 1, a + T) pair"


def _classify(lo, hi, top, T, outer):
    """what a pair crosses, from the indices alone (thread of index i: i mod T, or i where threads do not stride)"""
    tl, th = (lo % T, hi % T) if T else (lo, hi)
    k = set()
    if hi == lo + 1:
        k.add("neighbour")
    if tl // 64 != th // 64:
        k.add("wave")
    if T and tl == th:
        k.add("own_scan")
    if T and hi >= T and th < tl and (not outer or hi < outer):
        k.add("decisive")
    if outer and hi >= outer and th < tl:
        k.add("outer")
    if lo == 0 and hi == top - 1:
        k.add("first_last")
    return k
