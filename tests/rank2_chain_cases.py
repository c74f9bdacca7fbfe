"""Shapes and logs of the chained pass's tests on a FULL covariance (tests/test_rank2_chain_cases_host.py on the CPU,
tests/test_gpu_rank2_chain.py on the GPU).  No GPU here.

A config5 log corrects two or four landmarks per filter: a whole run changes (3 + 2 * 4)^2 entries of Sigma, all of them in
the first tile of a filter, and everything else is v - (0 * g + 0 * g).  The logs below are dense_sigma_cases.survey_log's:
every landmark is shown once before the steps under test, so every tile of every filter is CORRECTED by every step.

Every shape is a small pool that still takes the tile queue on 256 compute units (rows of 256 lanes, N >= 385, and at
least 16 x 256 tiles of 32 rows x 512 columns): 0.5 to 0.8 GB each.  The plan facts of the table (ld, column
chunks, 16-row tiles, rows of the last one) are asserted from ekf_rank2_plan.hpp by tests/cpp/rank2_chain_check.cpp, and
tests/test_rank2_chain_host.py holds that program's table against this one."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

import dense_sigma_cases as cases

CALL_V = 8          # ekf::kCallV: corrections per chained launch; a step with more active slots takes ceil(a / 8) launches


@dataclass(frozen=True)
class Shape:
    name: str
    n: int
    B: int
    ld: int            # pick_ld(3 + 2n)
    chunks: int        # 512-column chunks of a row
    row_blocks: int    # 16-row tiles down a filter
    last_rows: int     # rows of the last of them
    packing: bool      # set_row_packing: off where the pool would otherwise take the row-packed kernel and not the queue
    vmax: int
    seed: int
    extra_steps: int = cases.STEPS_UNDER_TEST

    @property
    def N(self):
        return 3 + 2 * self.n

    @property
    def tiles(self):
        return self.chunks * self.row_blocks

    def log(self):
        return cases.survey_log(self.n, self.vmax, B=self.B, seed=self.seed, extra_steps=self.extra_steps)


SHAPES = (
    # chunks == 1: t % chunks == 0 and t / chunks == t for every tile, lanes 252 .. 255 idle; strips full: no packing
    Shape("one-chunk", 250, 256, 512, 1, 32, 7, True, 2, 1250),
    # ld = 960 is the 16-double rounding: rows not on 2-KB boundaries, ld / 2 = 480 = the active double2 columns; strips
    # filled to 0.9375 >= 0.93: no packing
    Shape("narrow-ld", 478, 72, 960, 2, 60, 15, True, 2, 1478),
    # N = 1009 = 63 * 16 + 1: the last tile has ONE row, min(u, rows - 1) is 0 for all 16 registers
    Shape("one-row", 503, 64, 1024, 2, 64, 1, True, 2, 1503),
    # ld = 1408, three chunks (an odd count); row packing would take P = 4, so the pool chains with packing off only
    # (seed 1700 puts a landmark within 3 cm of the robot: survey_log refuses it)
    Shape("three-chunk", 700, 32, 1408, 3, 88, 11, False, 2, 1701),
    # the shape of the config5 tests, on test_pool_tile_queue's own log
    Shape("four-chunk", 1000, 24, 2048, 4, 126, 3, True, 2, 1600),
    # nine active slots: launches of C = 8 and C = 1 in every step
    Shape("long-call", 500, 80, 1024, 2, 63, 11, True, 9, 1509),
)
BY_NAME = {s.name: s for s in SHAPES}
CHECKER_SHAPES = ("one-chunk", "narrow-ld", "one-row", "long-call")   # chained run against OracleEKF(STRUCTURED)
BATCH_SHAPES = ("one-row", "one-chunk")


def batch_sizes(shape):
    """m of test_chain_batch_sizes_on_a_full_sigma: 5 and 63 divide neither tile count (one-chunk: 32 tiles, m = 5 ends on
    a batch of 2; one-row: 128 tiles, 3 at m = 5, 2 at m = 63), 1, 2 and 8 divide both, m = tiles is one item per filter,
    m = tiles + 1 is clamped to it"""
    return (1, 2, 5, 8, 63, shape.tiles, shape.tiles + 1)


def masked(log, keep, tag):
    """the log with filter b keeping its first keep[t - S, b] corrections in step under test t (a known log is -1 padded:
    a filter's corrections are its leading slots); the survey is untouched.  `tag` tells the checker's trace cache apart."""
    S = log.survey_steps
    keep = np.asarray(keep)
    assert keep.shape == (log.steps - S, log.cfg.filters)
    lm = log.lm_idx.copy()
    for t in range(keep.shape[0]):
        for b in range(keep.shape[1]):
            lm[S + t, b, keep[t, b]:] = -1
    lm.setflags(write=False)
    return dataclasses.replace(log, lm_idx=lm, key=log.key + (tag,)), keep


UNEVEN_N, UNEVEN_B, UNEVEN_VMAX, UNEVEN_SEED, UNEVEN_STEPS = 500, 80, 3, 1653, 4


def uneven_log():
    """test_chain_uneven_activity's masks on a full Sigma: 3 corrections everywhere; b % 4; one active slot pool-wide
    (that step must not chain); 3 - b % 4.  Returns (log, keep[4, B])."""
    log = cases.survey_log(UNEVEN_N, UNEVEN_VMAX, B=UNEVEN_B, seed=UNEVEN_SEED, extra_steps=UNEVEN_STEPS)
    b = np.arange(UNEVEN_B)
    return masked(log, np.stack([np.full(UNEVEN_B, 3), b % 4, (b % 3 == 0).astype(int), 3 - b % 4]), "uneven")


# one filter of each activity pattern (b % 4, b % 3 == 0) of uneven_log
UNEVEN_FILTERS = (0, 1, 2, 3, 4, 6, 7, 9)
LONG_UNEVEN_COUNTS = (0, 1, 5, 8, 9)


def long_uneven_log():
    """long-call's log with 0, 1, 5, 8 and 9 corrections side by side in every step under test (filter b, step t:
    LONG_UNEVEN_COUNTS[(b + t) % 5]): in the C = 1 launch of a step a fifth of the filters have cnt = 1, the rest 0"""
    log = BY_NAME["long-call"].log()
    b = np.arange(log.cfg.filters)
    pat = np.array(LONG_UNEVEN_COUNTS)
    return masked(log, np.stack([pat[(b + t) % 5] for t in range(log.steps - log.survey_steps)]), "long-uneven")


LONG_UNEVEN_FILTERS = (0, 1, 2, 3, 4)


def switch_log():
    """narrow-ld's log with a fourth step under test: chained, per-correction, call-fused, and chained again on one pool"""
    s = BY_NAME["narrow-ld"]
    return cases.survey_log(s.n, s.vmax, B=s.B, seed=s.seed, extra_steps=4)


def active_slots(log, t):
    """slots of step t that hold a correction in at least one filter"""
    return int((log.lm_idx[t] >= 0).any(axis=0).sum())


def expected_counts(log, t0=0, t1=None):
    """(chained launches, corrections they apply, correction passes of steps t0 .. t1 - 1): a step chains when two or more
    of its slots hold a correction in some filter -- the plan is asked with the step's slot count, so a last launch of one
    slot chains too -- and takes ceil(a / 8) launches"""
    slots = [active_slots(log, t) for t in range(t0, log.lm_idx.shape[0] if t1 is None else t1)]
    return sum(-(-a // CALL_V) for a in slots if a >= 2), sum(a for a in slots if a >= 2), sum(slots)


def host_cases():
    """(name, log, filters, keep or None) of everything the GPU file replays: what the host test checks in the checker"""
    out = [(s.name, s.log(), (0,), None) for s in SHAPES]
    out.append(("narrow-ld-switch", switch_log(), (0,), None))
    log, keep = uneven_log()
    out.append(("uneven", log, UNEVEN_FILTERS, keep))
    log, keep = long_uneven_log()
    out.append(("long-uneven", log, LONG_UNEVEN_FILTERS, keep))
    return out
