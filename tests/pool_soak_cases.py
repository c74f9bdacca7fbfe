"""The scenarios of the four pool soaks (tools/soak_panel.py, soak_delayed_pools.py, soak_symmetric.py, soak_batch.py) and
the runs that compare their variants: one source for the command-line soaks and for the seeded slices of them that run
under -m gpu (test_gpu_pool_soak.py).  Shared-cases code, not a conftest.

Each soak has
  *_scenario(seed) -> a dataclass of descriptors and input arrays, built on the CPU (no GPU, no library call);
  run_*(hip, scenario[, oracle]) -> a result dataclass with the comparison figures the soak asserts on, `ok` (the soak's
      own verdict at the soak's own tolerances) and `fail_line()` (the soak's FAIL text).

The order of the random draws is part of the contract: seed s of a soak gives the scenario it gave when the construction
lived in the script (tests/golden/pool_soak_scenarios.txt holds a SHA-256 per scenario of seeds 0..39 of each soak, taken
from the scripts before the move; test_pool_soak_host.py compares).  Do not reorder, add or remove a draw."""
from __future__ import annotations

import dataclasses
import functools
import hashlib
from dataclasses import dataclass, field

import numpy as np

from ekf_slam_ml_amd import synth

PANEL_MIN_DIM = 256      # ekf_batch_run_known: panel_capable needs N >= 256
MIRROR_MIN_DIM = 256     # the mirrored flush's threshold (sym_flush_applies)
STRIP_MAX_VECTORS = 80   # kStripMaxVec: a forced strip flush holds at most 80 pending vectors (2 per correction)
SOAKS = ("panel", "delayed_pools", "symmetric", "batch")

# The seeds that run under -m gpu (test_gpu_pool_soak.py); test_pool_soak_host.py asserts what they cover between them.
PANEL_SEEDS = (2, 3, 10, 17, 24, 25, 38, 40, 60, 63, 217, 1051)
DELAYED_POOL_SEEDS = (1, 6, 11, 14, 18, 22, 28, 32, 34, 49, 50, 65)
SYMMETRIC_SEEDS = (0, 5, 7, 12, 16, 19, 35, 39, 58, 65, 71, 77)
BATCH_SEEDS = (0, 2, 3, 6, 7, 12, 13, 19, 29, 30, 36, 359)
SEEDS = {"panel": PANEL_SEEDS, "delayed_pools": DELAYED_POOL_SEEDS, "symmetric": SYMMETRIC_SEEDS, "batch": BATCH_SEEDS}


def seed_blocks(seeds, size=3):
    return [tuple(seeds[i:i + size]) for i in range(0, len(seeds), size)]


def smallest(scenarios, count):
    """the `count` scenarios with the smallest B * n * T"""
    return sorted(scenarios, key=lambda s: (s.B * s.n * s.T, s.seed))[:count]


def pick_ld(N):
    """leading dimension of Sigma as the library pads it (csrc/ekf_rank2_plan.hpp, pick_ld; layout: csrc/ekf_kernels.hpp)"""
    wide = (N + 255) // 256 * 256
    return wide if (wide - N) * 32 <= N else (N + 15) // 16 * 16


def sigma_bytes(B, n):
    N = 3 + 2 * n
    return B * N * pick_ld(N) * 8


def digest(desc, arrays):
    """SHA-256 over a descriptor tuple (its repr) and input arrays (dtype, shape, bytes)"""
    h = hashlib.sha256()
    h.update(repr(desc).encode())
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"|{a.dtype.str}{a.shape}|".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _rel(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


# ---- the column panel of delayed known-association runs (tools/soak_panel.py) ----------------------------------------

@dataclass
class PanelScenario:
    seed: int
    B: int
    n: int
    T: int
    k: int
    vmax: int
    cuts: tuple          # run boundaries, 0 ... T
    getter: tuple        # per run: a getter behind it (drops the panel: the next run starts without one)
    strip: bool          # FORM_STRIP_FLUSH_ALWAYS
    log: synth.KnownLog = field(repr=False)   # lm_idx: with the blind steps and the sit-outs

    @property
    def N(self):
        return 3 + 2 * self.n

    def descriptors(self):
        return ("panel", self.seed, self.B, self.n, self.T, self.k, self.vmax, self.strip, self.cuts, self.getter)

    def digest(self):
        g = self.log
        return digest(self.descriptors(), [g.twist, g.lm_idx.astype(np.int32), g.z_xy, g.init_xy])

    def steps_with_readings(self):
        return (self.log.lm_idx >= 0).any(axis=(1, 2))

    def blind_run_ends(self):
        """runs whose last step has no reading in any filter (step 0, which only brings the map in, does not count)"""
        any_ = self.steps_with_readings()
        return sum(1 for b in self.cuts[1:] if b > 1 and not any_[b - 1])

    def blind_runs_left_to_the_repair(self):
        """runs of blind steps only, behind a run with corrections and no getter in between (its closing flush hands the
        panel over: nothing is pending when the blind run ends, so only the repair brings the matrix's columns 1, 2 up to
        date), that end the log or have a getter behind them (nothing later would heal the matrix)"""
        any_, runs = self.steps_with_readings(), list(zip(self.cuts[:-1], self.cuts[1:]))
        return sum(1 for i in range(1, len(runs))
                   if not any_[runs[i][0]:runs[i][1]].any() and any_[runs[i - 1][0]:runs[i - 1][1]].any()
                   and not self.getter[i - 1] and (i == len(runs) - 1 or self.getter[i]))

    def getters_between_runs(self):
        return sum(1 for g in self.getter[:-1] if g)

    def sit_outs(self):
        """(step, filter) pairs without a reading in a step where another filter has one"""
        row = (self.log.lm_idx >= 0).any(axis=2)
        return int((~row & row.any(axis=1)[:, None])[1:].sum())


def panel_scenario(seed):
    rng = np.random.default_rng(81000 + seed)
    B, n, T = int(rng.integers(1, 20)), int(rng.choice([100, 126, 127, 128, 200, 333, 500, 1000])), int(rng.integers(6, 30))
    k, vmax = int(rng.choice([1, 2, 3, 4, 8, 16, 17, 32, 64])), int(rng.choice([1, 2, 2, 3, 5, 6]))
    cfg = synth.SimConfig(n=n, steps=T, filters=B, seed=5000 + seed, half_extent=float(rng.uniform(2.0, 6.0)) * max(1.0, (n / 150.0) ** 0.5),
                          min_spacing=0.15, max_visible_dis=1e9 if vmax <= 2 else float(rng.uniform(0.8, 2.0)), vmax=vmax,
                          v_cmd=float(rng.uniform(0.1, 1.0)), w_cmd=float(rng.uniform(0.05, 0.6)))
    log = synth.make_known_log(cfg)
    lm = log.lm_idx.copy()
    lm[rng.random(T) < 0.12] = -1                                  # blind steps (the repair path when a run ends on them)
    for _ in range(int(rng.integers(0, 4))):
        lm[int(rng.integers(0, T)), int(rng.integers(0, B))] = -1  # a filter sits a step out
    cuts = sorted(set([0, T] + [int(c) for c in rng.integers(1, T, size=int(rng.integers(0, 4)))]))
    getter = rng.random(len(cuts)) < 0.3
    strip = bool(rng.integers(0, 2))
    return PanelScenario(seed, B, n, T, k, vmax, tuple(cuts), tuple(bool(g) for g in getter[:len(cuts) - 1]), strip,
                         dataclasses.replace(log, lm_idx=lm))


PANEL_VARIANTS = ("panel", "one_slot", "off", "current", "eager")


@dataclass
class PanelResult:
    sc: PanelScenario
    identical: bool      # panel on / one-slot plan / panel off: state and Sigma bit for bit
    dcur: float          # the kept current rows / columns (the default) against the panel-less run
    dstate: float        # panel and current against the eager run
    dcov: float
    counts: dict         # variant -> form_counts()
    cov_filters: tuple
    eager_state: np.ndarray = field(repr=False)
    eager_cov: list = field(repr=False)
    checker_state: np.ndarray = field(repr=False, default=None)   # with an oracle: the CPU checker's run of the log
    checker_cov: list = field(repr=False, default=None)

    @property
    def ok(self):
        return self.identical and self.dcur < 1e-10 and self.dstate < 1e-9 and self.dcov < 1e-9

    def fail_line(self):
        s = self.sc
        return (f"FAIL seed {s.seed}: B={s.B} n={s.n} T={s.T} k={s.k} vmax={s.vmax} cuts={list(s.cuts)} strip={s.strip} "
                f"identical={self.identical and self.dcur < 1e-10} dstate={self.dstate:.2e} dcov={self.dcov:.2e}")


def _checker_known(oracle, log, filters):
    st, cv, _ = oracle.batch_run_known(log, oracle.STRUCTURED, want_cov=True, fast=False)
    return st, [cv[b] for b in filters]


def run_panel(hip, sc, oracle=None):
    log, B = sc.log, sc.B
    base = hip.FORMS_DEFAULT | (hip.FORM_STRIP_FLUSH_ALWAYS if sc.strip else 0)
    outs = {}
    nocur = base & ~hip.FORM_CURRENT_COLUMNS
    filters = tuple(sorted({0, B // 2, B - 1}))
    for name, forms, mode in (("panel", nocur, sc.k), ("one_slot", nocur | hip.FORM_COLUMN_PANEL_ONE_SLOT, sc.k),
                              ("off", base & ~hip.FORM_COLUMN_PANEL, sc.k), ("current", base, sc.k), ("eager", base, 0)):
        bt = hip.BatchEKF(B, sc.n)
        bt.set_forms(forms)
        bt.set_update_mode(mode)
        bt.upload_known_log(log.twist, log.lm_idx, log.z_xy, log.init_xy)
        for i, (a, b) in enumerate(zip(sc.cuts[:-1], sc.cuts[1:])):
            bt.run_known(a, b)
            if sc.getter[i]:
                bt.state(0)                                        # (drops the panel: the next run starts without one)
        outs[name] = (np.stack([bt.state(b) for b in range(B)]), [bt.cov(b) for b in filters], bt.form_counts())
        bt.close()
    same = all(np.array_equal(outs[v][0], outs["off"][0]) and all(np.array_equal(x, y) for x, y in zip(outs[v][1], outs["off"][1]))
               for v in ("panel", "one_slot"))
    ds = max(float(np.abs(outs[v][0] - outs["eager"][0]).max()) for v in ("panel", "current"))
    dc = max(_rel(x, y) for v in ("panel", "current") for x, y in zip(outs[v][1], outs["eager"][1]))
    # the kept current rows / columns (the default): another association of the same sums -- 1e-10 from the rebuilt form
    dcur = max(float(np.abs(outs["current"][0] - outs["off"][0]).max()),
               max(_rel(x, y) for x, y in zip(outs["current"][1], outs["off"][1])))
    res = PanelResult(sc, same, dcur, ds, dc, {v: outs[v][2] for v in outs}, filters, outs["eager"][0], outs["eager"][1])
    if oracle is not None:
        res.checker_state, res.checker_cov = _checker_known(oracle, log, filters)
    return res


# ---- pools' delayed data_association() (tools/soak_delayed_pools.py) -------------------------------------------------

@dataclass
class DelayedPoolScenario:
    seed: int
    B: int
    n: int
    T: int
    k: int
    share: float         # share of the filters that start from a surveyed map
    cut: int             # the run boundary
    known0: np.ndarray = field(repr=False)    # [B] known counts at the start: n (surveyed) or 0 (discovering)
    init: np.ndarray = field(repr=False)      # [B, 2n] the survey
    twist: np.ndarray = field(repr=False)
    count: np.ndarray = field(repr=False)     # [T, B] readings per step, 0 where a filter sits the step out
    meas_xy: np.ndarray = field(repr=False)

    @property
    def kind(self):
        s = int((self.known0 > 0).sum())
        return "surveyed" if s == self.B else "discovering" if s == 0 else "mixed"

    def descriptors(self):
        return ("delayed_pools", self.seed, self.B, self.n, self.T, self.k, self.cut)

    def digest(self):
        return digest(self.descriptors(), [self.known0.astype(np.int32), self.init, self.twist, self.count.astype(np.int32),
                                           self.meas_xy])

    def sit_out_steps(self):
        """steps in which some filter has no reading while another has"""
        return int(((self.count == 0).any(axis=1) & (self.count > 0).any(axis=1)).sum())


def delayed_pool_scenario(seed):
    rng = np.random.default_rng(90000 + seed)
    B, n, T = int(rng.integers(3, 20)), int(rng.integers(110, 340)), int(rng.integers(5, 15))
    k = int(rng.choice([8, 16, 24, 32, 40, 64]))
    share = float(rng.choice([1.0, 1.0, 0.7, 0.3]))
    cfg = synth.SimConfig(n=n, steps=T, filters=B, seed=1000 + seed, half_extent=float(rng.uniform(4.0, 7.0)), min_spacing=0.3,
                          max_visible_dis=float(rng.uniform(1.0, 1.6)), vmax=8, v_cmd=1.0, w_cmd=0.6)
    log = synth.make_unknown_log(cfg)
    cnt = log.count.copy()
    cnt[rng.random(cnt.shape) < 0.08] = 0          # filters that sit a step out
    init = (log.world[None] + rng.normal(0.0, 0.005, size=(B, n, 2))).reshape(B, 2 * n)
    known0 = np.where(np.arange(B) < share * B, n, 0).astype(np.int32)
    cut = int(rng.integers(1, T))
    return DelayedPoolScenario(seed, B, n, T, k, share, cut, known0, init, log.twist, cnt, log.meas_xy)


@dataclass
class DelayedPoolResult:
    sc: DelayedPoolScenario
    decisions_equal: bool    # decisions and known counts: delayed against eager
    dstate: float
    dcov: float
    eager_decisions: np.ndarray = field(repr=False)
    eager_state: np.ndarray = field(repr=False)
    eager_cov: dict = field(repr=False)         # filter -> Sigma of the eager run (filter 0, + those asked for)
    spec: tuple = (0, 0)                        # spec_counts() of the delayed run
    counts: dict = None                         # form_counts() of the delayed run

    @property
    def ok(self):
        return self.decisions_equal and self.dstate < 1e-9 and self.dcov < 1e-9

    def fail_line(self):
        s = self.sc
        return (f"FAIL seed {s.seed}: B={s.B} n={s.n} T={s.T} k={s.k} share={s.share} decisions_equal={self.decisions_equal} "
                f"dstate={self.dstate:.2e} dcov={self.dcov:.2e}")


def run_delayed_pool(hip, sc, cov_filters=()):
    B, n = sc.B, sc.n
    lm0 = np.full((2, B, 1), -1, dtype=np.int32)
    res, extra, spec, counts = [], {}, (0, 0), None
    for mode in (0, sc.k):
        bt = hip.BatchEKF(B, n)
        bt.upload_known_log(np.zeros((2, B, 2)), lm0, np.zeros((2, B, 1, 2)), sc.init)
        bt.run_known()
        bt.set_known_counts(sc.known0)
        bt.set_update_mode(mode)
        bt.upload_unknown_log(sc.twist, sc.count, sc.meas_xy)
        bt.run_unknown(0, sc.cut)
        bt.run_unknown(sc.cut, sc.T)
        res.append((bt.decisions().copy(), bt.known_counts().copy(), np.stack([bt.state(b) for b in range(B)]), bt.cov(0)))
        if mode == 0:
            extra = {0: res[0][3], **{b: bt.cov(b) for b in cov_filters if b != 0}}
        else:
            spec, counts = bt.spec_counts(), bt.form_counts()
        bt.close()
    ok = np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    ds = float(np.abs(res[0][2] - res[1][2]).max())
    dc = float(np.abs(res[0][3] - res[1][3]).max() / np.abs(res[0][3]).max())
    return DelayedPoolResult(sc, bool(ok), ds, dc, res[0][0], res[0][2], extra, spec, counts)


def checker_delayed_pool(oracle, sc, b):
    """filter b of the scenario on the CPU checker (dense-literal data_association): (decisions per step, state, Sigma)"""
    o, known = oracle.OracleEKF(sc.n, oracle.DENSE), np.zeros(sc.n, dtype=np.uint8)
    for _ in range(2):                               # the two blind steps that bring the survey in
        o.prediction(0.0, 0.0)
        o.measurement(sc.init[b], np.zeros(sc.n, dtype=np.uint8))
    known[:int(sc.known0[b])] = 1
    dec = []
    for t in range(sc.T):
        o.prediction(*sc.twist[t, b])
        dec.append(o.data_association(sc.meas_xy[t, b, :sc.count[t, b]], known))
    return dec, o.state, o.cov


# ---- the symmetric option of the delayed mode (tools/soak_symmetric.py) ----------------------------------------------

@dataclass
class SymmetricScenario:
    seed: int
    B: int
    n: int
    T: int
    k: int
    vmax: int
    cuts: tuple
    picks: tuple         # per run: the filter whose Sigma is read back behind it where the flush mirrored
    log: synth.KnownLog = field(repr=False)   # lm_idx: with the blind steps

    @property
    def N(self):
        return 3 + 2 * self.n

    def descriptors(self):
        return ("symmetric", self.seed, self.B, self.n, self.T, self.k, self.vmax, self.cuts, self.picks)

    def digest(self):
        g = self.log
        return digest(self.descriptors(), [g.twist, g.lm_idx.astype(np.int32), g.z_xy, g.init_xy])

    def blind_steps(self):
        return int((~(self.log.lm_idx >= 0).any(axis=(1, 2)))[1:].sum())


def symmetric_scenario(seed):
    rng = np.random.default_rng(70000 + seed)
    B, n, T = int(rng.integers(1, 20)), int(rng.choice([40, 100, 126, 127, 128, 200, 333, 500, 700, 1000])), int(rng.integers(6, 30))
    k, vmax = int(rng.choice([1, 2, 3, 8, 16, 17, 32, 48, 64])), int(rng.choice([1, 2, 3, 5]))
    cfg = synth.SimConfig(n=n, steps=T, filters=B, seed=3000 + seed, half_extent=float(rng.uniform(2.0, 6.0)) * max(1.0, (n / 150.0) ** 0.5), min_spacing=0.15,
                          max_visible_dis=1e9 if vmax == 1 else float(rng.uniform(0.8, 2.0)), vmax=vmax)
    log = synth.make_known_log(cfg)
    blind = rng.random(T) < 0.15
    log.lm_idx[blind] = -1
    cuts = sorted(set([0, T] + [int(c) for c in rng.integers(1, T, size=int(rng.integers(0, 3)))]))
    # (one draw per run, as the soak draws them where every run's flush mirrored)
    picks = tuple(int(rng.integers(0, B)) for _ in cuts[1:])
    return SymmetricScenario(seed, B, n, T, k, vmax, tuple(cuts), picks, log)


@dataclass
class SymmetricResult:
    sc: SymmetricScenario
    dstate: float
    dcov: float
    mirror_ok: bool      # every Sigma read back behind a mirrored flush equals its transpose outside the diagonal squares
    mirrored: int        # form_counts()["flush_mirrored"] of the symmetric run
    mirror_checks: int   # how many Sigma were held against their transpose
    cov_filters: tuple
    eager_state: np.ndarray = field(repr=False)
    eager_cov: list = field(repr=False)
    checker_state: np.ndarray = field(repr=False, default=None)
    checker_cov: list = field(repr=False, default=None)

    @property
    def ok(self):
        return self.dstate < 1e-9 and self.dcov < 1e-9 and self.mirror_ok

    def fail_line(self):
        s = self.sc
        return (f"FAIL seed {s.seed}: B={s.B} n={s.n} T={s.T} k={s.k} vmax={s.vmax} cuts={list(s.cuts)} dstate={self.dstate:.2e} "
                f"dcov={self.dcov:.2e} mirror={self.mirror_ok}")


def symmetric_outside_squares(c):
    """Sigma equals its transpose to the bit outside the 32 x 32 diagonal squares"""
    tile = np.arange(c.shape[0]) // 32
    above = tile[:, None] < tile[None, :]
    return bool(np.array_equal(c.T[above], c[above]))


def run_symmetric(hip, sc, oracle=None):
    log, B = sc.log, sc.B
    res, mirrored, checks = [], 0, 0
    for mode in (0, sc.k):
        bt = hip.BatchEKF(B, sc.n)
        bt.set_update_mode(mode, symmetric_gather=bool(mode))
        bt.upload_known_log(log.twist, log.lm_idx, log.z_xy, log.init_xy)
        sym_ok = True
        for i, (a, b) in enumerate(zip(sc.cuts[:-1], sc.cuts[1:])):
            bt.run_known(a, b)
            if mode and bt.form_counts()["flush_mirrored"]:
                sym_ok = symmetric_outside_squares(bt.cov(sc.picks[i])) and sym_ok
                checks += 1
        if mode:
            mirrored = bt.form_counts()["flush_mirrored"]
        res.append((np.stack([bt.state(b) for b in range(B)]), bt.cov(0), bt.cov(B - 1), sym_ok))
        bt.close()
    ds = float(np.abs(res[0][0] - res[1][0]).max())
    dc = max(_rel(res[1][i], res[0][i]) for i in (1, 2))
    out = SymmetricResult(sc, ds, dc, res[1][3], mirrored, checks, (0, B - 1), res[0][0], [res[0][1], res[0][2]])
    if oracle is not None:
        out.checker_state, out.checker_cov = _checker_known(oracle, log, out.cov_filters)
    return out


# ---- batched unknown association against the single-filter API (tools/soak_batch.py) ---------------------------------

@dataclass
class BatchScenario:
    seed: int
    B: int
    n: int
    T: int
    J: int
    heavy: bool          # big prefixes on a pool with fresh known counts: the two-launch step (k_rank2v, K in LDS)
    small_map: bool
    step_fused: int      # four launches per slot / automatic / always one launch per step
    active_prefix: bool
    surveyed: bool       # known_list all true from the start: the map comes from a first known-association call
    cut: int
    call_fused: tuple    # per filter: the single-filter object's call-fused form
    twist: np.ndarray = field(repr=False)
    count: np.ndarray = field(repr=False)
    meas: np.ndarray = field(repr=False)
    init: np.ndarray = field(repr=False, default=None)

    def descriptors(self):
        return ("batch", self.seed, self.B, self.n, self.T, self.J, self.heavy, self.small_map, self.step_fused,
                self.active_prefix, self.surveyed, self.cut, self.call_fused)

    def digest(self):
        return digest(self.descriptors(), [self.twist, self.count.astype(np.int32), self.meas,
                                           self.init if self.init is not None else np.zeros((0, 0))])


def batch_scenario(seed):
    rng = np.random.default_rng(70000 + seed)
    B, n, T, J = int(rng.integers(1, 7)), int(rng.integers(3, 91)), int(rng.integers(4, 26)), int(rng.integers(1, 7))
    heavy = seed % 20 == 19   # big prefixes on a pool with fresh known counts: the two-launch step (k_rank2v, K in LDS)
    if heavy:
        B, n, T, J = int(rng.integers(64, 72)), int(rng.integers(300, 340)), int(rng.integers(3, 6)), int(rng.integers(2, 9))
    world = rng.uniform(-2.5, 2.5, size=(max(n, 8), 2)) * (3.0 if heavy else 1.0)
    twist = np.stack([rng.normal(0, 0.2, (T, B)), rng.normal(0.05, 0.03, (T, B))], axis=2)
    count = rng.integers(0, J + 1, size=(T, B)).astype(np.int32)
    meas = np.zeros((T, B, J, 2))
    pose = np.zeros((B, 3))
    for t in range(T):
        pose[:, 1] += twist[t, :, 1] * np.cos(pose[:, 0]); pose[:, 2] += twist[t, :, 1] * np.sin(pose[:, 0]); pose[:, 0] += twist[t, :, 0]
        for b in range(B):
            pick = rng.choice(len(world), size=J, replace=False)
            d = world[pick] - pose[b, 1:]
            c, s = np.cos(pose[b, 0]), np.sin(pose[b, 0])
            meas[t, b] = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], axis=1) + rng.normal(0, 0.004, (J, 2))
    small_map = bool(rng.integers(0, 2))
    step_fused = int(rng.integers(0, 3))   # four launches per slot / automatic / always one launch per step
    active_prefix = bool(rng.integers(0, 2))
    surveyed = heavy and bool(rng.integers(0, 2))
    init = (world[:n][None] + rng.normal(0, 0.004, (B, n, 2))).reshape(B, 2 * n) if surveyed else None
    cut = int(rng.integers(0, T + 1))
    call_fused = tuple(bool(rng.integers(0, 2)) for _ in range(B))
    return BatchScenario(seed, B, n, T, J, heavy, small_map, step_fused, active_prefix, surveyed, cut, call_fused, twist, count,
                         meas, init)


@dataclass
class BatchResult:
    sc: BatchScenario
    ok: bool             # decisions, known counts, state and Sigma of every filter: pool against single-filter API, bit for bit
    first_bad: int       # the first filter that differs (-1: none)
    counts: dict         # form_counts() of the pool

    def fail_line(self):
        s = self.sc
        return f"FAIL scenario {s.seed}: B={s.B} n={s.n} T={s.T} J={s.J}"


def run_batch(hip, sc):
    B, n, T = sc.B, sc.n, sc.T
    bt = hip.BatchEKF(B, n)
    bt.set_small_map_path(sc.small_map)
    bt.set_step_fused(sc.step_fused)
    bt.set_active_prefix(sc.active_prefix)
    if sc.surveyed:   # known_list all true from the start: the map comes from a first known-association call
        bt.upload_known_log(np.zeros((1, B, 2)), np.full((1, B, 1), -1, dtype=np.int32), np.zeros((1, B, 1, 2)), sc.init)
        bt.run_known()
        bt.set_known_counts(n)
    bt.upload_unknown_log(sc.twist, sc.count, sc.meas)
    bt.run_unknown(0, sc.cut); bt.run_unknown(sc.cut, T)
    dec, kc = bt.decisions(), bt.known_counts()
    ok, first_bad = True, -1
    for b in range(B):
        f = hip.EKF_SLAM(n)
        f.set_call_fused(sc.call_fused[b])
        k = np.zeros(n, dtype=np.uint8)
        okb = True
        if sc.surveyed:
            f.prediction((0.0, 0.0)); f.measurement(sc.init[b], np.zeros(n, dtype=np.uint8))
            k[:] = 1
        for t in range(T):
            f.prediction(sc.twist[t, b])
            a = f.data_association(sc.meas[t, b, :sc.count[t, b]], k)
            okb &= bool(np.array_equal(a, dec[t, b, :sc.count[t, b]]))
        okb &= int(k.sum()) == int(kc[b]) and np.array_equal(f.state, bt.state(b)) and np.array_equal(f.cov, bt.cov(b))
        f.close()
        if not okb and first_bad < 0:
            first_bad = b
        ok = ok and bool(okb)
    counts = bt.form_counts()
    bt.close()
    return BatchResult(sc, ok, first_bad, counts)


SCENARIO = {"panel": panel_scenario, "delayed_pools": delayed_pool_scenario, "symmetric": symmetric_scenario,
            "batch": batch_scenario}


@functools.lru_cache(maxsize=None)
def scenario(soak, seed):
    """the scenario of a seed, built once per process (the tests read it, nobody writes to it)"""
    return SCENARIO[soak](seed)
