"""Association decisions at ties and exact gates (ekf_slam.cpp:293-330), shared by tests/test_assoc_edge_cases_host.py
(CPU checker and the reference build) and tests/test_gpu_assoc_edges.py (every kernel form).  No GPU, no library.

THE EXACT WORLD.  Every score is an exact binary fraction in any summation order, so the expected decisions are written
down by construction and are not taken from a checker:
  PARAMS   sigma0_landmark 0.1875, q_pose 0, r_meas 0.0625, gate_new 16, gate_update 1
  pose (0, 0, 0), every twist (0, 0); every landmark and every reading on the +x axis (bearing 0: atan2 and fmod exact)
  "far" landmark i at x = 64 + i; "near" landmarks at small dyadic x
A reading at (m, 0) against a landmark at (x, 0): H = [[0, -1, -0, 1, 0], [-1, 0, -1/x, -0, 1/x]], S01 = 0,
S00 = 0.1875 + 0.0625 = 0.25, inv2 divides S11 / (0.25 S11) = 4, the bearing innovation is 0 -> score = 4 (m - x)^2.
The pose block of Sigma is zero and q_pose = 0, so no correction moves the pose, and a correction of one landmark leaves
every other landmark's 5 x 5 block at its prior: a later reading of the same call is an exact tie again (sequence()).

The rule every form promises: the winner is the lexicographic (d, i) minimum = the sequential scan's first strict minimum;
a score equal to gate_new is no match, a score equal to gate_update is no update, a NaN score never wins."""
from dataclasses import dataclass, field, replace
from fractions import Fraction

import numpy as np

PARAMS = (0.1875, 0.0, 0.0625, 16.0, 1.0, 1e-6)   # sigma0_landmark, q_pose, r_meas, gate_new, gate_update, straight_eps
FAR0 = 64.0
TIE_X = 1.0
STAGED_FILLERS = 32   # J = 33 is the first call the staged small form takes (kSmallInlineJ = 32)


def score(m, x):
    """4 (m - x)^2 in double arithmetic: m - x and the product by 4 are exact, the square rounds once (exact for every
    case but the 2^-30 near-tie, where the IEEE result is still strictly below 0.25)"""
    v0 = float(m) - float(x)
    assert Fraction(v0) == Fraction(m) - Fraction(x)
    return Fraction((v0 * 4.0) * v0)


@dataclass
class Case:
    name: str
    kind: str
    n: int
    M: int                      # known count in front of the call (the leading M entries of `known` are set)
    world: np.ndarray           # [n, 2] landmark positions the map is initialised with (NaN allowed)
    readings: np.ndarray        # [J, 2]
    decisions: tuple            # stated, by construction
    known_after: int
    scores: dict = field(default_factory=dict)   # of readings[0]: landmark -> Fraction, stated
    unchanged: tuple = ()       # landmarks whose state entries and rows / columns of Sigma stay bit-unchanged
    dropped: bool = False       # nothing changes at all
    new_slot: int = -1          # a landmark is initialised here, at exactly readings[-1]
    pair_kind: str = ""

    @property
    def J(self):
        return len(self.readings)

    @property
    def first(self):
        """index of the first edge reading (behind the staged form's fillers)"""
        return STAGED_FILLERS if self.J > STAGED_FILLERS else 0


def make_world(n, near):
    w = np.zeros((n, 2))
    w[:, 0] = FAR0 + np.arange(n)
    for i, x in near.items():
        w[i, 0] = x
    return w


def _r(*xs):
    return np.array([[x, 0.0] for x in xs], dtype=np.float64)


def tie(n, lo, hi, M=None, pair_kind=""):
    assert lo < hi
    M = n if M is None else M
    return Case(f"tie_{lo}_{hi}", "tie", n, M, make_world(n, {lo: TIE_X, hi: TIE_X}), _r(1.25), (lo,), M,
                scores={lo: Fraction(1, 4), hi: Fraction(1, 4)}, unchanged=(hi,), pair_kind=pair_kind)


def near_tie(n, lo, hi, bits=20, M=None, pair_kind=""):
    """the HIGHER index has the strictly smaller score; at bits = 30 the gap is below single precision's step"""
    assert lo < hi
    M = n if M is None else M
    xh = 1.0 + 2.0 ** -bits
    sc = {lo: Fraction(1, 4), hi: score(1.25, xh)}
    assert sc[hi] < sc[lo] and (bits != 20 or sc[hi] == Fraction(68718952449, 2 ** 38))
    assert bits < 24 or np.float32(float(sc[hi])) == np.float32(0.25)
    return Case(f"near_tie{bits}_{lo}_{hi}", "near_tie", n, M, make_world(n, {lo: TIE_X, hi: xh}), _r(1.25), (hi,), M,
                scores=sc, unchanged=(lo,), pair_kind=pair_kind)


def gate_update_exact(n, i, M=None):
    M = n if M is None else M
    return Case(f"gate_update_exact_{i}", "gate_update_exact", n, M, make_world(n, {i: 1.0}), _r(1.5), (-1,), M,
                scores={i: Fraction(1)}, dropped=True)


def gate_update_below(n, i, M=None):
    M = n if M is None else M
    m = 1.5 - 2.0 ** -20
    sc = score(m, 1.0)
    assert sc == 1 - Fraction(1, 2 ** 18) + Fraction(1, 2 ** 38)
    return Case(f"gate_update_below_{i}", "gate_update_below", n, M, make_world(n, {i: 1.0}), _r(m), (i,), M,
                scores={i: sc})


def gate_new_exact(n, i, M=None):
    """score exactly 16 = gate_new: no match.  Full map: dropped.  M < n: a new landmark at slot M, at exactly (3, 0)"""
    M = n if M is None else M
    assert i < M
    if M == n:
        return Case(f"gate_new_exact_{i}_full", "gate_new_exact_full", n, M, make_world(n, {i: 1.0}), _r(3.0), (-1,), M,
                    scores={i: Fraction(16)}, dropped=True)
    return Case(f"gate_new_exact_{i}_M{M}", "gate_new_exact_append", n, M, make_world(n, {i: 1.0}), _r(3.0), (M,), M + 1,
                scores={i: Fraction(16)}, new_slot=M)


def nan_low(n, a, i, M=None):
    """landmark a < i has a NaN position (its score is NaN and never wins); i is near with score 0.25"""
    assert a < i
    M = n if M is None else M
    w = make_world(n, {i: 1.0})
    w[a] = np.nan   # (initialisation from a NaN reading leaves both coordinates NaN)
    return Case(f"nan_low_{a}_{i}", "nan_low", n, M, w, _r(1.25), (i,), M, scores={i: Fraction(1, 4)})


def sequence(n, pairs, M=None):
    """one call / one pool step of 4..8 readings, each an exact tie of its own pair (pair p at x = 1 + 4p): from the second
    reading on the tie is scored against a state and a Sigma that earlier readings of the same call have changed"""
    M = n if M is None else M
    assert 4 <= len(pairs) <= 8
    idx = [i for p in pairs for i in p]
    assert len(set(idx)) == len(idx), "sequence pairs must be disjoint"
    near, xs = {}, []
    for p, (lo, hi) in enumerate(pairs):
        assert lo < hi
        near[lo] = near[hi] = 1.0 + 4.0 * p
        xs.append(near[lo] + 0.25)
    return Case("sequence", "sequence", n, M, make_world(n, near), _r(*xs), tuple(lo for lo, _ in pairs), M,
                scores={pairs[0][0]: Fraction(1, 4), pairs[0][1]: Fraction(1, 4)}, unchanged=tuple(hi for _, hi in pairs))


def with_fillers(c):
    """the staged small form: STAGED_FILLERS readings far off the map in front (dropped against a full map), J > 32"""
    assert c.M == c.n, "a far-off reading is dropped only against a full map"
    fill = _r(*[4096.0 + k for k in range(STAGED_FILLERS)])
    return replace(c, readings=np.concatenate([fill, c.readings]), decisions=(-1,) * STAGED_FILLERS + tuple(c.decisions))


# ---- the form table ---------------------------------------------------------------------------------------------------
# layout: what the form's reduction crosses.  waves > 1: an LDS stage between waves; T: the workgroup's stride (one thread
# scans i, i + T, ...); outer: k_assoc_reading's second stride (index tid + 256 u + 1024 k).
# shapes: (n, M0, pairs, gate indices, append counts M).  M0 = known count of the non-append cases (n: a full map).
# notes: what had to be left out of a form, and why.

def _pairs(n, T=None, outer=None, waves=True, top=None):
    top = n if top is None else top
    p = [(7, 8, "neighbour")]
    if waves and top > 64:
        p += [(63, 64, "wave"), (9, 73, "wave")]
    if T and top > T + 8:
        # decisive: the lower index in the higher lane of the same wave (the shuffle loop), and in a higher WAVE than the
        # thread that holds the higher index (the sh_d[w] stage)
        p += [(3, 3 + T, "own_scan"), (5, 4 + T, "decisive"), (70, 2 + T, "decisive")]
    if outer and top > outer + 8:
        p += [(11, 11 + outer, "own_scan"), (13, 12 + outer, "outer"), (78, 14 + outer, "outer")]
    p.append((0, top - 1, "first_last"))
    return p


LDS = dict(waves=1, T=None, outer=None)       # one landmark per lane of wave 0
CALL = dict(waves=7, T=None, outer=None)      # one landmark per thread, up to 448
T256 = dict(waves=4, T=256, outer=None)
READ = dict(waves=4, T=256, outer=1024)
T512 = dict(waves=8, T=512, outer=None)

FORMS = {
    # ---- single filter ----
    "single_inline": dict(pool=False, layout=LDS, kernel="k_small_associate_inline",
                          shapes=[(50, 50, _pairs(50, waves=False), (2, 49), (49,))], notes=[]),
    "single_staged": dict(pool=False, layout=LDS, kernel="k_small_associate",
                          shapes=[(50, 50, _pairs(50, waves=False), (2, 49), ())],
                          notes=["no append case: the 32 readings in front are dropped only against a full map"]),
    "single_prefix": dict(pool=False, layout=LDS, kernel="k_pool_associate",
                          shapes=[(270, 40, _pairs(270, waves=False, top=40), (2, 39), (40,))],
                          notes=["known count 40 of n = 270 (the form needs 3 + 2 (known + J) <= 104): first_last is (0, 39), "
                                 "the append slot is 40, and a full-map drop at gate_new cannot be reached"]),
    "single_call": dict(pool=False, layout=CALL, kernel="k_assoc_call",
                        shapes=[(130, 130, _pairs(130), (2, 129), (63, 64, 129)),
                                (270, 270, _pairs(270), (2, 269), (63, 64, 255, 256, 269)),
                                (440, 440, _pairs(440) + [(383, 384, "wave"), (370, 434, "wave")], (2, 439), (439,))],
                        notes=["one landmark per thread: no stride, so no own_scan / decisive pair exists in this layout"]),
    "single_reading": dict(pool=False, layout=READ, kernel="k_assoc_score + k_assoc_reading",
                           shapes=[(460, 460, _pairs(460, T=256), (2, 459), (459,)),
                                   (1040, 1040, _pairs(1040, T=256, outer=1024), (2, 1039), (1023, 1024, 1039))],
                           notes=["append counts start where known + J > 448: below it the call is k_assoc_call's"]),
    "single_chain": dict(pool=False, layout=T256, kernel="k_maha + k_assoc_decide",
                         shapes=[(270, 270, _pairs(270, T=256), (2, 269), (63, 64, 255, 256, 269))], notes=[]),
    "single_delayed": dict(pool=False, layout=T256, kernel="k_maha (pending pairs) + k_assoc_decide", sequence_only=True,
                           shapes=[(270, 270, _pairs(270, T=256), (), ())],
                           notes=["the sequence case only: ties scored against pending pairs"]),
    # ---- pools (B = 3, the edge filter is filter 1) ----
    "pool_small": dict(pool=True, layout=LDS, kernel="k_pool_associate",
                       shapes=[(50, 50, _pairs(50, waves=False), (2, 49), (49,))], notes=[]),
    "pool_fused_off": dict(pool=True, layout=T256, kernel="k_maha + k_assoc_decide",
                           shapes=[(270, 270, _pairs(270, T=256), (2, 269), (63, 64, 255, 256, 269))], notes=[]),
    "pool_fused_auto": dict(pool=True, layout=T512, kernel="k_pool_step_unknown<false> + k_rank2v (split pass)",
                            shapes=[(300, 300, _pairs(300), (2, 299), (299,)),
                                    (530, 530, _pairs(530, T=512), (2, 529), (511, 512, 529))],
                            notes=["append counts near n only: the split pass needs 70 % of the launch bound to be real work"]),
    "pool_fused_always": dict(pool=True, layout=T512, kernel="k_pool_step_unknown<false>",
                              shapes=[(530, 530, _pairs(530, T=512), (2, 529), (63, 64, 255, 256, 511, 512, 529))], notes=[]),
    "pool_delayed_spec": dict(pool=True, layout=T512, kernel="k_pool_step_spec + k_pool_step_unknown<true>",
                              shapes=[(530, 530, _pairs(530, T=512), (2, 529), (512, 529))], notes=[]),
    "pool_delayed_nospec": dict(pool=True, layout=T512, kernel="k_pool_step_unknown<true>",
                                shapes=[(530, 530, _pairs(530, T=512), (2, 529), (512, 529))], notes=[]),
}


def required_pair_kinds(layout):
    """the pair kinds a layout has (the list of the issue): neighbouring lanes and first-against-last always; a wave
    boundary where there is more than one wave; one thread's own scan and THE DECISIVE ONE -- the lower index in the higher
    lane -- where threads stride; the outer stride where there is one"""
    k = {"neighbour", "first_last"}
    if layout["waves"] > 1:
        k.add("wave")
    if layout["T"]:
        k |= {"own_scan", "decisive"}
    if layout["outer"]:
        k.add("outer")
    return k


def _sequence_pairs(pairs):
    out, used = [], set()
    for lo, hi, _ in pairs:
        if lo in used or hi in used:
            continue
        out.append((lo, hi))
        used |= {lo, hi}
    k = 20
    while len(out) < 4:   # layouts with few pair kinds: neighbours elsewhere in the wave
        if not {k, k + 1} & used:
            out.append((k, k + 1))
            used |= {k, k + 1}
        k += 2
    return out[:8]


def cases_for(form):
    """[(case id, Case)] of a form, over all its shapes"""
    f = FORMS[form]
    out = []
    for n, M0, pairs, gates, appends in f["shapes"]:
        cs = []
        if not f.get("sequence_only"):
            first30 = True
            for lo, hi, kind in pairs:
                cs.append(tie(n, lo, hi, M0, kind))
                cs.append(near_tie(n, lo, hi, 20, M0, kind))
                if kind == "decisive" or (first30 and not f["layout"]["T"]):
                    cs.append(near_tie(n, lo, hi, 30, M0, kind))
                    first30 = False
            for i in gates:
                cs += [gate_update_exact(n, i, M0), gate_update_below(n, i, M0)]
                if M0 == n:
                    cs.append(gate_new_exact(n, i, n))
            for M in appends:
                cs.append(gate_new_exact(n, 2, M))
            # the NaN landmark in the winner's own thread where threads stride, else in the lane next to it
            T = f["layout"]["T"]
            top = M0
            cs.append(nan_low(n, 5, 5 + T, M0) if T and top > T + 8 else nan_low(n, 5, 6, M0))
            if top > 64:
                cs.append(nan_low(n, 1, 65, M0))
        cs.append(sequence(n, _sequence_pairs(pairs), M0))
        if form == "single_staged":
            cs = [with_fillers(c) for c in cs]
        out += [(f"n{n}-{c.name}", c) for c in cs]
    return out


def all_case_ids():
    return [(form, cid) for form in FORMS for cid, _ in cases_for(form)]


_CACHE = {}


def get_case(form, cid):
    if form not in _CACHE:
        _CACHE[form] = dict(cases_for(form))
    return _CACHE[form][cid]


# ---- running a case on a filter with OracleEKF's surface ------------------------------------------------------------

def init_by_measurement(f, c):
    """one measurement() with nothing visible: every landmark initialised from the sensor vector (:113-128) -- exact
    here (pose 0: r = |x|, bearing 0) -- and Sigma left at the constructor's prior"""
    f.measurement(c.world.reshape(-1), np.zeros(c.n, dtype=np.uint8))


def known_list(c):
    k = np.zeros(c.n, dtype=np.uint8)
    k[:c.M] = 1
    return k


def masked(state):
    """(state with NaN -> 0, NaN mask): the parity metric wants finite numbers; the mask is compared on its own"""
    s = np.array(state, dtype=np.float64)
    m = np.isnan(s)
    s[m] = 0.0
    return s, m


def rows_of(i):
    return [3 + 2 * i, 4 + 2 * i]
