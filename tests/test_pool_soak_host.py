"""CPU: the scenarios of the four pool soaks (pool_soak_cases.py).  Seed s of each soak is the scenario it was when the
construction lived in tools/soak_*.py (SHA-256 per scenario, golden/pool_soak_scenarios.txt), and the seed lists that run
under -m gpu (test_gpu_pool_soak.py) hold, between them, what the soaks exist for -- conditions on the descriptors, checked
here so that a change of a list cannot quietly drop one."""
import os

import pytest

import pool_soak_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_soak_scenarios.txt")
MAX_SIGMA_BYTES = 700 * 1000 * 1000
MAX_STEPS = 30


def _golden():
    want = {}
    with open(GOLDEN) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                soak, seed, sha = line.split()
                want[soak, int(seed)] = sha
    return want


@pytest.mark.parametrize("soak", cases.SOAKS)
def test_seeds_give_the_scenarios_they_always_gave(soak):
    want = _golden()
    assert sorted(s for k, s in want if k == soak) == list(range(40))
    got = {seed: cases.SCENARIO[soak](seed).digest() for seed in range(40)}
    bad = [seed for seed in range(40) if got[seed] != want[soak, seed]]
    assert not bad, f"{soak}: seeds {bad} no longer give the scenario of the golden file (a draw was reordered, added or removed)"


def _scenarios(soak):
    return [cases.scenario(soak, s) for s in cases.SEEDS[soak]]


@pytest.mark.parametrize("soak", cases.SOAKS)
def test_seed_lists_are_small_and_bounded(soak):
    seeds = cases.SEEDS[soak]
    assert len(seeds) == 12 and len(set(seeds)) == 12
    assert [s for b in cases.seed_blocks(seeds) for s in b] == list(seeds)
    for sc in _scenarios(soak):
        assert cases.sigma_bytes(sc.B, sc.n) <= MAX_SIGMA_BYTES, sc
        assert sc.T <= MAX_STEPS, sc


def test_pick_ld_is_the_library_rule():
    """(csrc/ekf_rank2_plan.hpp: rows on 2-KB boundaries where that costs <= 1/32 of a row, else on 128-B lines)"""
    assert [cases.pick_ld(N) for N in (7, 255, 257, 259, 683, 2003, 2047, 2048, 2049)] == [16, 256, 272, 272, 688, 2048, 2048, 2048, 2064]
    assert cases.sigma_bytes(19, 1000) == 19 * 2003 * 2048 * 8 <= MAX_SIGMA_BYTES


def test_panel_seeds_cover_what_the_soak_is_for():
    sc = _scenarios("panel")
    assert {126, 127, 128} <= {s.n for s in sc}                       # N = 255, 257, 259 around the panel's minimum 256
    assert {255, 257, 259} <= {s.N for s in sc} and cases.PANEL_MIN_DIM == 256
    ks = {s.k for s in sc}
    assert 1 in ks and ks & {2, 3, 4} and 17 in ks and 64 in ks
    assert {s.strip for s in sc} == {True, False}
    # (a forced strip flush holds 80 pending vectors: a strip scenario whose every flush is a strip flush)
    assert any(s.strip and 2 * s.k <= cases.STRIP_MAX_VECTORS for s in sc)
    assert sum(1 for s in sc if s.blind_run_ends()) >= 2
    assert sum(1 for s in sc if s.getters_between_runs()) >= 2
    # a whole run of blind steps that starts with a panel and that nothing heals afterwards: the panel repair alone
    assert sum(1 for s in sc if s.N >= cases.PANEL_MIN_DIM and s.k >= 2 and s.blind_runs_left_to_the_repair()) >= 2
    assert sum(1 for s in sc if s.sit_outs()) >= 2
    vs = {s.vmax for s in sc}
    assert 1 in vs and max(vs) >= 5
    # where the panel can be on at all (N >= 256, room for a pair: k >= 2): most of the list
    assert sum(1 for s in sc if s.N >= cases.PANEL_MIN_DIM and s.k >= 2) >= 8


def test_delayed_pool_seeds_cover_what_the_soak_is_for():
    sc = _scenarios("delayed_pools")
    kinds = {s.kind for s in sc}
    # (the soak's surveyed share is 1.0, 0.7 or 0.3 and filter 0 is surveyed at every one of them: no seed gives a pool
    # of discovering filters only -- they come inside the mixed pools, as the majority at share 0.3)
    assert {"surveyed", "mixed"} <= kinds
    assert any(int((s.known0 == 0).sum()) > s.B // 2 for s in sc)
    assert all(0 < s.cut < s.T for s in sc)                           # a run boundary, in every one
    assert sum(1 for s in sc if s.sit_out_steps()) >= 2
    ks = {s.k for s in sc}
    assert 8 in ks and max(ks) >= 32


def test_symmetric_seeds_cover_what_the_soak_is_for():
    sc = _scenarios("symmetric")
    assert any(s.N < cases.MIRROR_MIN_DIM for s in sc) and any(s.N >= cases.MIRROR_MIN_DIM for s in sc)
    assert {255, 257} <= {s.N for s in sc}                            # on both sides of the threshold, next to it
    assert sum(1 for s in sc if s.blind_steps()) >= 2
    assert sum(1 for s in sc if len(s.cuts) > 2) >= 2
    assert any(len(s.cuts) > 2 and s.N >= cases.MIRROR_MIN_DIM for s in sc)
    Bs = {s.B for s in sc}
    assert 1 in Bs and max(Bs) >= 8


def test_batch_seeds_cover_what_the_soak_is_for():
    sc = _scenarios("batch")
    # big prefixes (a surveyed map of >= 300 landmarks: N >= 603) on a pool whose known counts are read back every step
    # (B >= 64), the automatic step form: the two-launch step; and such a pool with four launches per slot
    assert any(s.heavy and s.surveyed and s.step_fused == 1 and s.B >= 64 and s.n >= 300 for s in sc)
    assert any(s.heavy and s.surveyed and s.step_fused == 0 for s in sc)
    assert 1 in {s.B for s in sc}
    assert {s.step_fused for s in sc} == {0, 1, 2} and {s.small_map for s in sc} == {True, False}
    assert any(s.cut == 0 for s in sc) and any(s.cut == s.T for s in sc)   # an empty first run, an empty second run
