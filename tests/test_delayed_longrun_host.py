"""No GPU: the logs of tests/test_gpu_delayed_longrun.py are fit for their purpose -- shown with the CPU checker alone.

These conditions say which inputs are admissible for the long-horizon parity tests of the delayed update; none of them
is there to be loosened when a GPU test fails.

* Reference floor: at every probe the strict checker and its FMA / AVX2 build -- two correct fp64 implementations of the
  same recurrences -- differ by at most 1e-10 per block (parity.worst), a tenth of the 1e-9 contract, so two correct
  implementations cannot trip the GPU tests.  (Not true of every log: synth.config5(filters=1, steps=300) shows 1.9e-10
  in theta between the two builds at step 250, which is why it is not among them.)
* Re-observation: the logs correct the SAME landmarks hundreds of times, which is what a kept current row / column, a
  recycled plan slot or a stale version counter needs to show.
* LOG_UNKNOWN: both checker builds decide identically at every step, and no score sits within 1e-6 (relative) of a gate
  or of the runner-up, so a decision that differs on the GPU is a fault and not a coin toss."""
import numpy as np
import pytest

import delayed_longrun_cases as lc


@pytest.mark.parametrize("name,min_corrections,min_landmarks_50x", [
    (lc.LOG_N1000, 550, 6),      # found: 586-588 corrections; 6, 6 and 7 landmarks with >= 50
    (lc.LOG_N200, 0, 50),        # found: 61 landmarks with >= 50 corrections
    (lc.LOG_N5000, 96, 0),       # two full flush periods at k = 32 and the closing flush
])
def test_known_log_is_fit_for_purpose(oracle, name, min_corrections, min_landmarks_50x):
    case = lc.known_case(name)
    for b in case.filters:
        assert case.corrections(b) >= min_corrections, (name, b, case.corrections(b))
        assert case.landmarks_corrected_at_least(b, 50) >= min_landmarks_50x, (name, b)
    seen = []
    for P, per in lc.iter_known_reference(oracle, case):
        for b, (s, c, floor, blocks) in per.items():
            print(f"{name} filter {b} probe {P}: strict vs FMA checker {floor:.2e}")
            assert np.isfinite(floor) and floor <= lc.FLOOR_MAX, f"{name} filter {b} probe {P}: floor {blocks}"
        seen.append(P)
        del per
    assert tuple(seen) == case.probes and seen[-1] == case.log.cfg.steps


def test_n1000_edits_are_in_the_uploaded_log():
    case = lc.known_case(lc.LOG_N1000)
    lm, raw = case.lm, case.log.lm_idx
    assert (lm[120:126] == -1).all() and (raw[120:126] >= 0).all()        # the blind stretch blinds readings that were there
    assert (lm[200, ::3] == -1).all() and (lm[200, 1::3] >= 0).all() and (lm[200, 2::3] >= 0).all()
    assert ((lm[1:120] >= 0).sum(axis=2) == 2).all()                       # V = 2: every other step is one paired launch
    # the two nearest landmarks change along the circle and come back: landmarks leave and re-enter the panel plan
    for b in case.filters:
        first = {int(i): t for t in range(300, 0, -1) for i in lm[t, b] if i >= 0}
        last = {int(i): t for t in range(1, 301) for i in lm[t, b] if i >= 0}
        gaps = [i for i in first if any((lm[t, b] != i).all() for t in range(first[i], last[i]))]
        assert 15 <= len(first) <= 18 and len(gaps) >= 6, (b, len(first), len(gaps))


def test_unknown_log_is_fit_for_purpose(oracle):
    case = lc.unknown_case()
    assert (case.count[90:94] == 0).all() and (case.log.count[90:94] > 0).any()
    assert (case.count[140, ::2] == 0).all() and (case.count[140, 1::2] > 0).all()
    P = None
    for P, dec, kc, margins, dec_fma, per in lc.iter_unknown_reference(oracle, case):
        assert np.array_equal(dec, dec_fma), f"the two checker builds decide differently before step {P}"
        assert (kc == case.n).all()
        for b, (s, c, floor, blocks) in per.items():
            print(f"{case.name} filter {b} probe {P}: strict vs FMA checker {floor:.2e}")
            assert np.isfinite(floor) and floor <= lc.FLOOR_MAX, f"filter {b} probe {P}: floor {blocks}"
    assert P == case.log.cfg.steps == case.probes[-1]
    m = dict(zip(oracle.MARGIN_KEYS, margins))
    print(f"{case.name}: margins {m}")
    assert m["decision_relevant"] >= lc.MIN_DECISION_MARGIN, m
    corrected = [(dec[:, b] >= 0).sum() for b in range(case.B)]
    print(f"{case.name}: corrections per filter {corrected}")
    assert min(corrected) >= 400, corrected
