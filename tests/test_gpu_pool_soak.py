"""-m gpu: seeded slices of the four pool soaks (tools/soak_panel.py, soak_delayed_pools.py, soak_symmetric.py,
soak_batch.py; scenarios and runs in pool_soak_cases.py) at the soaks' own tolerances -- random cuts, getters between runs,
blind steps at the end of a run, filters that sit steps out, strip / plain / mirrored flush, the per-filter prefix: the
combinations the fixed shapes of test_gpu_delayed.py, test_gpu_batch_unknown.py, test_gpu_dense_sigma.py and
test_gpu_parity.py do not hold.  What the seed lists cover is asserted on the CPU (test_pool_soak_host.py).

Two things the soaks themselves lack: the eager run of the smallest scenarios against the CPU checker (every other
comparison here is between two GPU runs, blind to an error they share), and proof through form_counts() that the form
under test ran."""
import numpy as np
import pytest

import pool_soak_cases as cases
from parity import FP64_TOL, assert_parity, state_err

pytestmark = pytest.mark.gpu

_results = {}   # (soak, seed) -> result: the counting tests below read what the slices ran, they run nothing again


def _run(hip, soak, seed, **kw):
    if (soak, seed) not in _results:
        sc = cases.scenario(soak, seed)
        _results[soak, seed] = {"panel": cases.run_panel, "delayed_pools": cases.run_delayed_pool,
                                "symmetric": cases.run_symmetric, "batch": cases.run_batch}[soak](hip, sc, **kw)
    return _results[soak, seed]


def _ids(blocks):
    return ["seeds_" + "_".join(str(s) for s in b) for b in blocks]


PANEL_BLOCKS = cases.seed_blocks(cases.PANEL_SEEDS)
DELAYED_BLOCKS = cases.seed_blocks(cases.DELAYED_POOL_SEEDS)
SYMMETRIC_BLOCKS = cases.seed_blocks(cases.SYMMETRIC_SEEDS)
BATCH_BLOCKS = cases.seed_blocks(cases.BATCH_SEEDS)


def _panel_counts_hold(r):
    """what form_counts() can show of a panel scenario's variants (it counts flushes per kind and the delayed gain launches
    that read the panel; it has no counter of its own for the one-slot plan: that variant is told from the panel-less one by
    gain_from_panel > 0, not from the full plan)"""
    sc, c = r.sc, r.counts
    what = r.fail_line() + f" counts={c}"
    assert c["off"]["gain_from_panel"] == 0 and c["eager"]["gain_from_panel"] == 0, what
    if sc.N < cases.PANEL_MIN_DIM or sc.k < 2:          # no panel below its minimum dimension or without room for a pair
        assert all(c[v]["gain_from_panel"] == 0 for v in ("panel", "one_slot", "current")), what
    # the plan only moves where the gain launches read from: every delayed variant appends and flushes alike
    for v in ("one_slot", "off", "current"):
        assert all(c[v][key] == c["panel"][key] for key in ("flush_plain", "flush_strip", "gain_pairs")), what
    for v in ("one_slot", "current"):
        assert (c[v]["gain_from_panel"] > 0) == (c["panel"]["gain_from_panel"] > 0), what
    corrections = int((sc.log.lm_idx >= 0).any(axis=1).sum())     # (step, slot) pairs with a reading: the launches' work
    for v in ("panel", "one_slot", "off", "current"):
        assert c[v]["rank2_streams"] == 0 and c[v]["flush_mirrored"] == 0, what
        if corrections:
            assert c[v]["flush_plain"] + c[v]["flush_strip"] > 0, what
            if sc.strip and 2 * sc.k <= cases.STRIP_MAX_VECTORS:  # forced, and never more pending than the strip form holds
                assert c[v]["flush_strip"] > 0 and c[v]["flush_plain"] == 0, what
            elif sc.strip:
                assert c[v]["flush_strip"] + c[v]["flush_plain"] > 0, what
    assert all(c["eager"][key] == 0 for key in ("flush_plain", "flush_strip", "flush_mirrored", "gain_pairs")), what


@pytest.mark.parametrize("block", PANEL_BLOCKS, ids=_ids(PANEL_BLOCKS))
def test_panel_slice(hip, block):
    """panel on / one-slot plan / panel off bit-identical; the default (current columns kept) within 1e-10 of them; all
    within 1e-9 of the eager run"""
    for seed in block:
        r = _run(hip, "panel", seed)
        print(f"panel seed {seed}: identical={r.identical} dcur={r.dcur:.2e} dstate={r.dstate:.2e} dcov={r.dcov:.2e} "
              f"from_panel={r.counts['panel']['gain_from_panel']}")
        assert r.identical, r.fail_line()
        assert r.dcur < 1e-10, r.fail_line() + f" dcur={r.dcur:.2e}"
        assert r.dstate < 1e-9 and r.dcov < 1e-9, r.fail_line()
        _panel_counts_hold(r)


def test_panel_slices_read_the_panel(hip):
    """over the panel seeds: the gain launches read the panel in at least half of the scenarios that can have one"""
    rs = [_run(hip, "panel", s) for s in cases.PANEL_SEEDS]
    big = [r for r in rs if r.sc.N >= cases.PANEL_MIN_DIM]
    hit = [r.sc.seed for r in big if r.counts["panel"]["gain_from_panel"] > 0]
    assert len(big) >= 8 and 2 * len(hit) >= len(big), (hit, [r.sc.seed for r in big])
    strips = [r for r in rs if r.sc.strip and 2 * r.sc.k <= cases.STRIP_MAX_VECTORS]
    assert strips and all(r.counts["panel"]["flush_strip"] > 0 for r in strips)


def _smallest(soak):
    return cases.smallest([cases.scenario(soak, s) for s in cases.SEEDS[soak]], 3)


@pytest.mark.parametrize("soak,run", [("panel", cases.run_panel), ("symmetric", cases.run_symmetric)])
def test_eager_run_against_the_cpu_checker(hip, oracle, soak, run):
    """the three smallest scenarios (B * n * T): the eager run every other variant is held to, against the CPU checker"""
    for sc in _smallest(soak):
        r = run(hip, sc, oracle)
        assert r.ok, r.fail_line()
        for b in range(sc.B):
            e = state_err(r.eager_state[b], r.checker_state[b])
            assert max(e.values()) <= FP64_TOL, f"{soak} seed {sc.seed} state of filter {b} vs checker {e}: {r.fail_line()}"
        for b, c, ref in zip(r.cov_filters, r.eager_cov, r.checker_cov):
            w = assert_parity(r.eager_state[b], c, r.checker_state[b], ref, FP64_TOL, f"{soak} seed {sc.seed} filter {b} vs checker")
            print(f"{soak} seed {sc.seed} filter {b}: worst per-block error against the checker {w:.2e}")


@pytest.mark.parametrize("block", DELAYED_BLOCKS, ids=_ids(DELAYED_BLOCKS))
def test_delayed_pool_slice(hip, block):
    """pools' delayed data_association() against the eager run of the same pool: decisions and known counts identical,
    state and Sigma within 1e-9"""
    for seed in block:
        r = _run(hip, "delayed_pools", seed)
        print(f"delayed pool seed {seed}: decisions_equal={r.decisions_equal} dstate={r.dstate:.2e} dcov={r.dcov:.2e} spec={r.spec}")
        assert r.decisions_equal, r.fail_line()
        assert r.dstate < 1e-9 and r.dcov < 1e-9, r.fail_line()
        # the delayed step kernel ran (its launches are counted with the steps that leave the pass to a later launch),
        # and what it left pending was folded in by flushes
        assert r.counts["step_split_passes"] > 0 and r.counts["flush_plain"] + r.counts["flush_strip"] > 0, r.fail_line() + f" {r.counts}"


def test_delayed_pool_eager_run_against_the_cpu_checker(hip, oracle):
    """two filters of the smallest scenario on the dense-literal checker, reading by reading"""
    sc = _smallest("delayed_pools")[0]
    filters = (0, sc.B - 1)
    r = cases.run_delayed_pool(hip, sc, cov_filters=filters)
    assert r.ok, r.fail_line()
    for b in filters:
        dec, state, cov = cases.checker_delayed_pool(oracle, sc, b)
        for t in range(sc.T):
            assert np.array_equal(r.eager_decisions[t, b, :sc.count[t, b]], dec[t]), f"{r.fail_line()} filter {b} step {t}"
        assert_parity(r.eager_state[b], r.eager_cov[b], state, cov, FP64_TOL, f"delayed pools seed {sc.seed} filter {b} vs checker")


def test_delayed_pool_slices_speculate(hip):
    """spec_counts() over the slices: the delayed step compared readings with the guesses of the launch in front, and some
    continued from them (the speculating form ran; it is on by default)"""
    rs = [_run(hip, "delayed_pools", s) for s in cases.DELAYED_POOL_SEEDS]
    eligible, hits = sum(r.spec[0] for r in rs), sum(r.spec[1] for r in rs)
    assert 0 < hits <= eligible, (eligible, hits)


@pytest.mark.parametrize("block", SYMMETRIC_BLOCKS, ids=_ids(SYMMETRIC_BLOCKS))
def test_symmetric_slice(hip, block):
    """the symmetric option within 1e-9 of the eager run; Sigma handed back equal to its transpose to the bit outside the
    32 x 32 diagonal squares; the mirrored flush is the one that ran from its threshold on, and never below it"""
    for seed in block:
        r = _run(hip, "symmetric", seed)
        sc = r.sc
        print(f"symmetric seed {seed}: dstate={r.dstate:.2e} dcov={r.dcov:.2e} mirror={r.mirror_ok} mirrored={r.mirrored} checks={r.mirror_checks}")
        assert r.dstate < 1e-9 and r.dcov < 1e-9, r.fail_line()
        assert r.mirror_ok, r.fail_line()
        corrections = int((sc.log.lm_idx >= 0).sum())
        if sc.N >= cases.MIRROR_MIN_DIM and corrections:
            assert r.mirrored > 0 and r.mirror_checks > 0, r.fail_line() + f" mirrored={r.mirrored}"
        if sc.N < cases.MIRROR_MIN_DIM:
            assert r.mirrored == 0, r.fail_line() + f" mirrored={r.mirrored}"


@pytest.mark.parametrize("block", BATCH_BLOCKS, ids=_ids(BATCH_BLOCKS))
def test_batch_slice(hip, block):
    """the pool against the single-filter API: decisions, known counts, state and Sigma bit for bit"""
    for seed in block:
        r = _run(hip, "batch", seed)
        sc = r.sc
        print(f"batch seed {seed}: ok={r.ok} counts={r.counts}")
        assert r.ok, r.fail_line() + f" first differing filter {r.first_bad} small_map={sc.small_map} step_fused={sc.step_fused} " \
                                     f"active_prefix={sc.active_prefix} surveyed={sc.surveyed} cut={sc.cut}"
        if sc.heavy and sc.step_fused == 1 and sc.surveyed:
            # big prefixes (N >= 603), known counts read back every step (B >= 64), the automatic form: steps ran as two
            # launches (the separate pass is counted)
            assert r.counts["step_split_passes"] > 0, r.fail_line() + f" counts={r.counts}"
        if sc.step_fused == 2 or sc.step_fused == 0:
            assert r.counts["step_split_passes"] == 0, r.fail_line() + f" counts={r.counts}"
