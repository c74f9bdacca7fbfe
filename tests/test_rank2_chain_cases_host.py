"""CPU only: the inputs of the chained pass's full-covariance tests (tests/rank2_chain_cases.py), checked in the checker
alone -- OracleEKF(STRUCTURED), never the kernel.

Every log reaches a covariance without a zero entry before its first step under test, and every step under test changes
>= CHANGE_SHARE (0.99) of all entries by more than 1e-9 of sqrt(S_ii S_jj).  On the uneven logs that holds per filter and per
step wherever the filter has a correction; a filter without one changes nothing outside the pose rows and columns (its
prediction).  That is what lets a skipped tile, a dropped batch or a wrong row of a ragged tile show in the GPU tests."""
import numpy as np
import pytest

import dense_sigma_cases as cases
import rank2_chain_cases as chain_cases

_CASES = chain_cases.host_cases()


@pytest.mark.parametrize("idx", range(len(_CASES)), ids=[c[0] for c in _CASES])
def test_every_chain_case_corrects_a_full_covariance(oracle, idx):
    name, log, filters, keep = _CASES[idx]
    lm, n, S = log.lm_idx, log.cfg.n, log.survey_steps
    pad = np.where(lm < 0, 1 << 30, lm)
    assert ((np.diff(pad, axis=2) > 0) | (pad[:, :, 1:] == 1 << 30)).all()          # ascending, -1 pads last (what the pool accepts)
    assert sorted(lm[:S, 0][lm[:S, 0] >= 0].tolist()) == list(range(n))              # the survey shows every landmark once
    assert log.steps - S == (4 if name in ("uneven", "narrow-ld-switch") else cases.STEPS_UNDER_TEST)
    traces, _ = cases.checker_pool(oracle, log, filters)
    for b in filters:
        covs = [c for _, c in traces[b]]
        assert len(covs) == log.steps - S + 1
        if keep is None:
            zero, share = cases.require_preconditions(covs, f"{name} filter {b}")
            print(f"preconditions {name} filter {b}: zero share {zero:g}, smallest changed share {share:.4f}")
            continue
        assert (covs[0] != 0.0).all(), f"{name} filter {b}: Sigma still has zero entries behind the survey"
        for t, (before, after) in enumerate(zip(covs[:-1], covs[1:])):
            count = int((lm[S + t, b] >= 0).sum())
            assert count == keep[t, b]
            if count:
                share = float((cases.entry_map(before, after) > cases.CHANGE_EPS).mean())
                print(f"preconditions {name} filter {b} step {t}: {count} corrections change {share:.4f}")
                assert share >= cases.CHANGE_SHARE, f"{name} filter {b} step {t}: {count} corrections change only {share:.4f}"
            else:   # the prediction alone: rows and columns 0 .. 2
                assert np.array_equal(before[3:, 3:], after[3:, 3:]), f"{name} filter {b} step {t}: changed without a correction"
                assert not np.array_equal(before[:3], after[:3])


def test_the_case_lists_cover_what_they_claim():
    by = chain_cases.BY_NAME
    assert [s.chunks for s in chain_cases.SHAPES] == [1, 2, 2, 3, 4, 2] and by["one-row"].last_rows == 1
    assert by["narrow-ld"].ld % 256 and by["three-chunk"].ld % 256 and not by["three-chunk"].packing
    assert (by["narrow-ld"].N + 1) // 2 == by["narrow-ld"].ld // 2                     # ld / 2 = the active double2 columns
    assert by["one-chunk"].chunks * 256 - (by["one-chunk"].N + 1) // 2 == 4            # four idle lanes
    for name in chain_cases.BATCH_SHAPES:   # a short last batch at m = 5 and 63 (8 divides both tile counts)
        assert all(by[name].tiles % m for m in (5, 63)) and by[name].tiles % 8 == 0, name
    assert by["one-chunk"].tiles % 5 == 2
    # long call: launches of C = 8 and C = 1 in every step; its uneven twin: cnt = 0 and cnt = 1 side by side in the C = 1 launch
    log = by["long-call"].log()
    S = log.survey_steps
    assert all(chain_cases.active_slots(log, t) == 9 for t in range(S, log.steps))
    assert chain_cases.expected_counts(log, S) == (2 * 3, 9 * 3, 9 * 3)
    ulog, keep = chain_cases.long_uneven_log()
    assert all(sorted(set(keep[t].tolist())) == list(chain_cases.LONG_UNEVEN_COUNTS) for t in range(keep.shape[0]))
    assert all(chain_cases.active_slots(ulog, S + t) == 9 for t in range(keep.shape[0]))
    assert {tuple(keep[:, b]) for b in chain_cases.LONG_UNEVEN_FILTERS} == {tuple(keep[:, b]) for b in range(ulog.cfg.filters)}
    # the uneven log: the existing test's slot counts, and one filter of each activity pattern
    ulog, keep = chain_cases.uneven_log()
    S = ulog.survey_steps
    assert [chain_cases.active_slots(ulog, t) for t in range(S, ulog.steps)] == [3, 3, 1, 3]
    assert {tuple(keep[:, b]) for b in chain_cases.UNEVEN_FILTERS} == {tuple(keep[:, b]) for b in range(ulog.cfg.filters)}
    assert len({tuple(keep[:, b]) for b in chain_cases.UNEVEN_FILTERS}) == len(chain_cases.UNEVEN_FILTERS)
    assert chain_cases.expected_counts(ulog, S) == (3, 9, 10)
