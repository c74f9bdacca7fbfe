"""CPU (not gpu): what the GPU checks of ekf_dense64_scan_evidence rest on, and the host surface of the feature.  1. the
numpy model (tests/dense_evidence_cases.py) reproduces synth.make_scans (model 0, range_std = 0) bit for bit on every case;
2. the preconditions of the cases: the beams a last-bit difference could flip are at most 1 % of a case and never a beam
the case exists for, and the cases are what they claim; 3. ekf_dense64_evidence_update against a Python restatement, and
as a stand-alone C++ program, plain and under AddressSanitizer + UBSan (nothing is preloaded); 4. DenseEKFSLAM.logodds
follows the landmarks through merge, remove, prune, join, clone and submap (a handle double that tracks landmark ids);
5. the header, capi.SYMBOLS and the library agree and the checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_evidence_cases as ev
from ekf_slam_ml_amd import capi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
NAMES = ("ekf_dense64_evidence_launch_info", "ekf_dense64_scan_evidence", "ekf_dense64_evidence_update",
         "ekf_dense64_remove_landmark")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- 1. the model is make_scans ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ev.CASES))
def test_model_reproduces_make_scans_bit_for_bit(name):
    pose, lms, nb, rmax, border, radius = ev.case(name)
    want = synth.make_scans(pose[None, :], lms, n_beams=nb, range_std=0.0, range_max=rmax, border=border,
                            tube_radius=radius, model=0)[0]
    got = ev.case_model(name)
    assert np.array_equal(_bits(got["expected"]), _bits(want))
    # the index is that of the landmark which alone gives the range
    for b in np.nonzero(got["hit"] >= 0)[0][:40]:
        alone = synth.make_scans(pose[None, :], lms[got["hit"][b]][None, :], n_beams=nb, range_std=0.0, range_max=rmax,
                                 border=border, tube_radius=radius, model=0)[0]
        assert _bits(alone[b]) == _bits(want[b])


# ---- 2. preconditions ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ev.CASES))
def test_margins_stay_under_the_cap(name):
    m = ev.case_model(name)
    obs, mc = ev.classed_scan(name)
    for risky in (ev.margins(m), ev.margins(mc, obs)):
        assert risky.sum() <= ev.MARGIN_CAP * len(risky), (name, np.nonzero(risky)[0])
        assert not risky[ev.CASES[name]["key"]].any()


def test_cases_are_what_they_claim():
    m = ev.case_model("exact")
    assert m["expected"][0] == 0.75 and list(m["hit"]) == [0, -1, -1, -1]
    for name, near, far in (("occlusion", 0, 1), ("occlusion_far_first", 1, 0)):
        m = ev.case_model(name)
        assert (m["hit"] == near).sum() >= 3 and not (m["hit"] == far).any()
    for name, low, high in (("tie_low_high", 0, 2), ("tie_adjacent", 1, 2)):
        m = ev.case_model(name)
        assert (m["hit"] == low).sum() >= 2 and not (m["hit"] == high).any()
    m = ev.case_model("nan_landmark")
    assert set(m["hit"]) == {-1, 1} and m["report"]["n_candidates"] == 1
    m = ev.case_model("inside_a_tube")
    assert not (m["hit"] == 0).any() and m["hit"][0] == 1
    m = ev.case_model("beyond_and_cut")
    assert m["report"]["n_candidates"] == 1 and not (m["hit"] == 0).any() and not (m["hit"] == 2).any()
    assert m["hit"][90] == 1 and m["hit"][180] == -1 and 0 < (m["hit"] == 1).sum() < 9   # the cut tube: its centre beams only
    m = ev.case_model("wall_nearer")
    assert m["hit"][0] == -1 and m["expected"][0] == 1.0 and m["hit"][2] == 1
    info = capi_consts()
    for n in (1, 127, 128, 129, 130):
        m = ev.case_model(f"world_{n}")
        assert m["report"]["n_candidates"] == n and m["report"]["n_on_tube"] > 0
    assert {info["lm_chunk"] - 1, info["lm_chunk"], info["lm_chunk"] + 1} <= {127, 128, 129, 130}
    assert {info["beam_tile"] - 1, info["beam_tile"], info["beam_tile"] + 1} <= {c["lidar"][0] for c in ev.CASES.values()}
    obs, mc = ev.classed_scan("world_129")
    assert all((mc["cls"] == c).any() for c in range(5)) and mc["report"]["n_unexplained"] > 0
    assert np.array_equal(mc["n_expected"], mc["n_agree"] + mc["n_through"] + mc["n_short"])


def capi_consts():
    hpp = open(os.path.join(ROOT, "ekf_slam_ml_amd", "csrc", "ekf_dense.hpp")).read()
    get = lambda k: int(re.search(r"constexpr int " + k + r" = (\d+);", hpp).group(1))
    return {"beam_tile": get("kDense64EvidenceBeamTile"), "lm_chunk": get("kDense64EvidenceLmChunk"),
            "threads": get("kDense64EvidenceThreads")}


# ---- 3. the bookkeeping ----------------------------------------------------------------------------------------------------------

def test_evidence_update_against_the_restatement():
    rng = np.random.default_rng(3)
    for trial in range(20):
        n = int(rng.integers(1, 300))
        e = rng.integers(0, 15, n).astype(np.int32)
        a = (rng.random(n) * (e + 1)).astype(np.int32)
        t = (rng.random(n) * (e - a + 1)).astype(np.int32)
        l0 = rng.uniform(-5.0, 5.0, n)
        mb, wh, wm = int(rng.integers(1, 6)), float(rng.uniform(0, 1)), float(rng.uniform(0, 2))
        want_l, want_v = ev.np_evidence_update(l0, e, a, t, mb, wh, wm, -4.0, 4.0)
        l = l0.copy()
        v = capi.evidence_update(l, e, a, t, mb, wh, wm, -4.0, 4.0)
        assert np.array_equal(v, want_v) and np.array_equal(_bits(l), _bits(want_l)), trial
    l = np.zeros(3)
    for bad in (dict(min_beams=0), dict(w_hit=-1.0), dict(w_miss=float("nan")), dict(l_min=1.0, l_max=0.0)):
        with pytest.raises(capi.EkfError):
            capi.evidence_update(l, [5, 5, 5], [5, 0, 0], [0, 5, 0], **bad)
    assert not l.any()


@pytest.mark.parametrize("sanitize", [False, True])
def test_update_as_a_standalone_program(tmp_path, sanitize):
    exe = str(tmp_path / "evidence_update_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe,
                    os.path.join(HERE, "cpp", "evidence_update_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.split("\n")[:-1]
    assert lines[-1] == "ok"
    state = [12345]

    def nxt():
        state[0] = (state[0] * 1664525 + 1013904223) % (1 << 32)
        return (state[0] >> 16) & 0x7FFF
    e, a, t, l = [], [], [], []
    for i in range(200):
        ex = nxt() % 12
        ag = nxt() % (ex + 1) if ex else 0
        th = nxt() % (ex - ag + 1) if ex - ag else 0
        e.append(ex), a.append(ag), t.append(th), l.append(-4.5 + 0.045 * i)
    e += [2147483647, 2147483647]
    a += [1073741824, 0]
    t += [1073741823, 2147483647]
    l += [0.0, 0.0]
    want_l, want_v = ev.np_evidence_update(l, e, a, t, 3, 0.4, 0.85, -4.0, 4.0)
    assert len(lines) == len(l) + 1
    for i, line in enumerate(lines[:-1]):
        k, v, x = line.split()
        assert (int(k), int(v)) == (i, want_v[i]) and _bits(float(x)) == _bits(want_l[i]), line
    assert list(want_v[-2:]) == [1, -1] and {-1, 0, 1} == set(want_v)


# ---- 4. the log-odds follow the landmarks ------------------------------------------------------------------------------------------

class _Handle:
    """what DenseEKFSLAM's bookkeeping needs of a DensePropagator64, in numpy: the landmark ids slot by slot"""
    LM_DEFERRED, LM_GROW_LIVE, LM_JOSEPH = 1, 2, 4

    def __init__(self, cap):
        self.N = self.live = 3 + 2 * cap
        self.carry = False
        self.ids = []

    def _lm_flags(self, *a, **k):
        return 0

    def _drop(self, slot, known):
        assert known == len(self.ids) and 0 <= slot < known
        last = known - 1
        moved = last if slot != last else -1
        if moved >= 0:
            self.ids[slot] = self.ids[last]
        self.ids.pop()
        return last, moved

    def merge_landmarks(self, a, b, r_merge, known, flags, params):
        return self._drop(max(a, b), known) + (0.0, 0.0)

    def remove_landmark(self, i, known, flags, params):
        return self._drop(i, known) + (0.0,)

    def extract_map(self, src, keep=None):
        self.ids = list(src.ids) if keep is None else [src.ids[int(k)] for k in keep]

    def join_map(self, src):
        self.ids += src.ids
        return 0.0

    def coupling(self, W):
        return (0, 0.0, 0.0)

    def init_block(self, first, W=None, xb=None):
        assert first == 3 + 2 * len(self.ids) and W.shape == (2, 2) and xb.shape == (2,)
        self.ids.append(max(self.ids, default=-1) + 1)


def _filter(cap, ids, logodds):
    f = capi.DenseEKFSLAM.__new__(capi.DenseEKFSLAM)
    f.n, f.deferred, f.grow_live, f.params, f.joseph, f._device = cap, False, False, None, False, -1
    f.handle = _Handle(cap)
    f.handle.ids = list(ids)
    f._known, f._init_flag, f.jcbb_report, f.evidence = len(ids), False, None, None
    f._logodds = np.array(logodds, dtype=np.float64)
    return f


def _tagged(f):
    """every landmark's log-odds are still its own: the value is 0.25 * id"""
    return len(f.logodds) == f.known == len(f.handle.ids) and list(f.logodds) == [0.25 * i for i in f.handle.ids]


def test_logodds_follow_merge_remove_prune_join_clone_submap():
    ids = list(range(8))
    f = _filter(10, ids, [0.25 * i for i in ids])
    assert f.merge(1, 5, 0.5)[0] == 7 and f.handle.ids == [0, 1, 2, 3, 4, 7, 6] and _tagged(f)
    assert f.remove(6) == -1 and _tagged(f)                 # the last: nothing moves
    assert f.remove(0) == 5 and f.handle.ids == [7, 1, 2, 3, 4] and _tagged(f)
    g = _filter(10, [20, 21], [5.0, 5.25])
    f.join(g)
    assert f.handle.ids == [7, 1, 2, 3, 4, 20, 21] and _tagged(f)
    snap = f.clone(into=_filter(10, [], []))
    sub = f.submap([6, 0, 3], into=_filter(10, [], []))
    assert sub.handle.ids == [21, 7, 3] and _tagged(sub)
    removed = f.prune(0.6)                                     # ids 1 and 2 (0.25, 0.5), highest index first
    assert removed == [2, 1] and sorted(f.handle.ids) == [3, 4, 7, 20, 21] and _tagged(f)
    assert f.prune(0.6) == []
    f.restore(snap)
    assert f.handle.ids == [7, 1, 2, 3, 4, 20, 21] and _tagged(f) and _tagged(snap)
    # a planted landmark is the next known one and starts at 0
    f.logodds[:] = 1.0
    assert f.add_landmark([1.0, 2.0], 0.01 * np.eye(2)) == 7 and f.known == 8 and list(f.logodds) == [1.0] * 7 + [0.0]
    f.logodds[:] = [0.25 * i for i in f.handle.ids]
    # a landmark the map gained since the last look starts at 0
    f.handle.ids.append(0)
    f._known += 1
    assert f.logodds[-1] == 0.0 and _tagged(f)


# ---- 5. the host surface -----------------------------------------------------------------------------------------------------------

def test_header_symbols_and_library_agree():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS and hasattr(lib, name)
    assert "typedef struct ekf_dense64_evidence_report" in HDR and C.sizeof(capi.EvidenceReport) == 16
    mk = open(os.path.join(ROOT, "ekf_slam_ml_amd", "csrc", "Makefile")).read()
    assert "ekf_dense64_evidence.hip" in mk and "ekf_dense64_evidence.hpp" in mk
    hpp = open(os.path.join(ROOT, "ekf_slam_ml_amd", "csrc", "ekf_dense64_evidence.hpp")).read()
    assert "hip_runtime" not in hpp and "#include <hip" not in hpp and "ekf_dense.hpp" not in hpp
    assert "Nothing above says WHICH landmark is spurious" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_refusals_need_no_device():
    lib = capi.load()
    lp = capi.default_lidar()
    rep = capi.EvidenceReport()
    assert lib.ekf_dense64_scan_evidence(None, None, C.byref(lp), None, -1, 0, -1.0, -1.0, None, None, None, None, None, None,
                                         None, None, None, None) == 1
    assert b"ekf_dense64_scan_evidence: null handle or lidar" in lib.ekf_last_error()
    known = C.c_int(3)
    assert lib.ekf_dense64_remove_landmark(None, None, 0, C.byref(known), 0, None, None) == 1 and known.value == 3
    assert b"ekf_dense64_remove_landmark: null handle" in lib.ekf_last_error()
    assert lib.ekf_dense64_evidence_launch_info(None, None, None, None) == 1
    assert lib.ekf_dense64_evidence_update(0, None, None, None, 3, 0.4, 0.85, -4.0, 4.0, None, None) == 1
    assert rep.n_candidates == 0


# ---- 6. the lifecycle's preconditions, on the model ------------------------------------------------------------------------------

def test_lifecycle_margins_on_the_model():
    """the circle list is the seven near tubes on every scan (the distant tube and the planted spot never appear in it), and
    every counter of every landmark keeps >= 2 beams from the threshold that decides it, the same for any tolerance the
    filter's landmarks can have -- so the outcome of the GPU test does not hang on one beam"""
    import sys
    sys.path.insert(0, ROOT)
    from oracle import np_restatement as npr
    near, distant, ghost = ev.life_world()
    assert 1.25 < np.hypot(*distant) < ev.LIFE_LIDAR[1] and np.all(np.hypot(*near.T) <= 1.0)
    assert min(np.hypot(*(near - ghost).T).min(), np.hypot(*(distant - ghost))) >= 0.7
    for k, obs in enumerate(ev.life_scans()):
        centres = npr.np_approx_circle_positions(obs)[0]
        assert len(centres) == len(near), k
        assert np.all(np.hypot(*(centres - near).T) < 0.02), k          # in the order of the near tubes, each on its tube
        lo, hi = ev.life_counts(obs, ev.LIFE_TOL[0]), ev.life_counts(obs, ev.LIFE_TOL[1])
        assert all(np.array_equal(a, b) for a, b in zip(lo, hi)), k
        e, a, t = (c.astype(int) for c in lo)
        assert np.all(e - ev.LIFE_MIN_BEAMS >= 2), (k, e)
        assert t[0] - (e[0] // 2 + 1) >= 2 and a[0] == 0, (k, e[0], t[0])   # the planted landmark: a miss
        assert np.all(a[1:] - (e[1:] + 1) // 2 >= 2) and not t[1:].any(), (k, e, a)   # every true tube: a hit
        assert e[1] <= 6                                                    # the distant tube: too few beams for a cluster
