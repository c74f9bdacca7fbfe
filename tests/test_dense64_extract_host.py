"""CPU: the numpy model of ekf_dense64_extract_map (dense_extract_cases) against the definition spelled as a double loop, the
preconditions of the keep-list families for the tile sides the kernel has (read from ekf_dense.hpp), the refusals that need
no device, the Python layer's checks, and that the calls are declared, bound and documented."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_extract_cases as ex
from ekf_slam_ml_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "ekfslam.h")).read()
DENSE_HPP = open(os.path.join(ROOT, "ekf_slam_ml_amd", "csrc", "ekf_dense.hpp")).read()


def _tiles():
    """the hot kernel's tile sides in states, as the source declares them (the GPU test reads them from the library)"""
    tr = int(re.search(r"kDense64ExtractTileRows = (\d+);", DENSE_HPP).group(1))
    tc = int(re.search(r"kDense64ExtractTileCols = (\d+);", DENSE_HPP).group(1))
    assert int(re.search(r"kDense64ExtractThreads = (\d+);", DENSE_HPP).group(1)) == 256
    return tr, tc


def test_model_is_the_definition():
    Tr, Tc = _tiles()
    for Nb in (3, 5, 7, 21, 67):
        b = (Nb - 3) // 2
        S, x = ex.source_corner(Nb), ex.source_state(Nb)
        assert not ex.same_bits(S, S.T) and not ex.same_bits(S[:3, :3], S[:3, :3].T)
        assert np.isnan(S).any() and (np.signbit(S) & (S == 0)).any()
        for name, keep in ex.families(b, Tr // 2, Tc // 2).items():
            lst = ex.as_list(keep, b)
            want = ex.brute_corner(S, lst)
            got = ex.expected_corner(S, lst)
            assert got.shape == (3 + 2 * lst.size,) * 2 and ex.same_bits(got, want), (Nb, name)
            assert not ex.same_bits(ex.transposed_corner(S, lst), want), (Nb, name)
            io = ex.iota(lst)
            assert ex.same_bits(ex.expected_state(x, lst), [x[i] for i in io])
            P = np.arange(1.0, 2 * Nb + 1).reshape(2, Nb)
            pg = ex.panel_gather(P, lst, width=io.size + 3)
            assert ex.same_bits(pg[:, :io.size], [[P[q][i] for i in io] for q in range(2)]) and not pg[:, io.size:].any()
    assert ex.same_bits(ex.expected_corner(S, ex.as_list(None, b)), S)   # the identity list is a clone


def test_families_are_lists_of_distinct_landmarks_in_range():
    Tr, Tc = _tiles()
    lr, lc = Tr // 2, Tc // 2
    assert ex.sizes(Tr, Tc) == sorted({ex.odd_near(v) for T in (Tr, Tc) for v in (3, 5, 7, T - 1, T, T + 1, 2 * T + 1, 3 * T + 2)})
    assert max(ex.sizes(Tr, Tc)) <= 3 * max(Tr, Tc) + 3
    seen = set()
    for Nb in ex.sizes(Tr, Tc):
        b = (Nb - 3) // 2
        fam = ex.families(b, lr, lc)
        assert {"identity", "identity_list", "reversed", "every_second", "random", "k0"} <= set(fam)
        assert ("one" in fam) == (b > 0) and fam["identity"] is None and fam["k0"].size == 0
        for name, keep in fam.items():
            lst = ex.as_list(keep, b)
            assert lst.ndim == 1 and np.unique(lst).size == lst.size and (lst.size == 0 or (lst.min() >= 0 and lst.max() < b)), (Nb, name)
            seen.add(name)
        if b > 2:
            assert 0 < fam["random"].size < b
        if b > 20:
            assert not np.array_equal(fam["random"], np.sort(fam["random"]))
        assert np.array_equal(fam["every_second"], np.arange(b)[::2]) and np.array_equal(fam["reversed"], np.arange(b)[::-1])
    assert seen == {"identity", "identity_list", "reversed", "every_second", "random", "k0", "one", "two_runs_inside",
                    "two_runs_on_edge"}


def test_two_runs_have_their_boundary_inside_a_tile_and_on_a_tile_edge():
    """for the reported sides: the `inside` list breaks a run inside a row tile and inside a column tile, so that tile takes
    the scattered path and its neighbours the run path; the `on_edge` list breaks on a tile edge, so every tile is a run"""
    Tr, Tc = _tiles()
    lr, lc = Tr // 2, Tc // 2
    inside = on_edge = 0
    for Nb in ex.sizes(Tr, Tc):
        b = (Nb - 3) // 2
        fam = ex.families(b, lr, lc)
        if "two_runs_inside" in fam:
            keep = fam["two_runs_inside"]
            cut = int(np.flatnonzero(np.diff(keep) != 1)[0]) + 1          # the first entry of the second run
            assert np.flatnonzero(np.diff(keep) != 1).size == 1 and keep[cut] == 0 and keep[0] == b - cut
            assert cut % lr != 0 and cut % lc != 0
            flags = ex.run_flags(keep, lc)
            assert flags[cut // lc] is False and sum(flags) == len(flags) - 1
            inside += 1
        if "two_runs_on_edge" in fam:
            keep = fam["two_runs_on_edge"]
            cut = int(np.flatnonzero(np.diff(keep) != 1)[0]) + 1
            assert cut == lc and cut % lr == 0 and keep[cut] == 0
            assert all(ex.run_flags(keep, lc)) and len(ex.run_flags(keep, lc)) >= 2
            on_edge += 1
        assert all(ex.run_flags(np.arange(b), lc))
        if b > 1:
            assert not any(ex.run_flags(np.arange(b)[::-1], lc)[:-1]) or b <= lc + 1
    assert inside >= 6 and on_edge >= 3
    b = (max(ex.sizes(Tr, Tc)) - 3) // 2                                  # the largest size has both kinds of tile at once
    assert sorted(set(ex.run_flags(ex.families(b, lr, lc)["two_runs_inside"], lc))) == [False, True]


def test_null_handles_are_refused_in_order_without_a_device():
    lib = capi.load()
    fake = ctypes.c_void_p(0x1000)
    keep = (ctypes.c_int * 2)(0, 1)
    ms = ctypes.c_double(7.0)
    call = lib.ekf_dense64_extract_map
    assert call(None, None, 2, keep, ctypes.byref(ms)) == 1 and b"null destination handle" in lib.ekf_last_error()
    assert call(None, fake, 2, keep, ctypes.byref(ms)) == 1 and b"null destination handle" in lib.ekf_last_error()
    assert call(fake, None, 2, keep, ctypes.byref(ms)) == 1 and b"null source handle" in lib.ekf_last_error()
    assert call(fake, fake, 2, keep, ctypes.byref(ms)) == 1 and b"same handle" in lib.ekf_last_error()
    assert ms.value == 7.0
    a, b, c = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7)
    info = lib.ekf_dense64_extract_launch_info
    assert info(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 1
    assert info(fake, None, ctypes.byref(b), ctypes.byref(c)) == 1
    assert info(fake, ctypes.byref(a), None, ctypes.byref(c)) == 1
    assert info(fake, ctypes.byref(a), ctypes.byref(b), None) == 1
    assert (a.value, b.value, c.value) == (7, 7, 7)
    assert info(fake, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0       # (reads nothing of the handle)
    assert (a.value, b.value, c.value) == _tiles() + (256,)


class _NoLibrary:
    def __getattr__(self, name):
        if name.endswith("_destroy"):                                     # (a handle that goes away may say so)
            return lambda h: 0
        raise AssertionError(f"the wrapper reached the library ({name})")


def _fake_handle(N):
    d = capi.DensePropagator64.__new__(capi.DensePropagator64)
    d.N, d._lib, d._h = N, _NoLibrary(), ctypes.c_void_p(0x1000)
    return d


def _fake_filter(n, known, init_flag=False, cap=None, **flags):
    f = capi.DenseEKFSLAM.__new__(capi.DenseEKFSLAM)
    f.n, f.handle, f._known, f._init_flag, f.params, f._device = n, _fake_handle(3 + 2 * (cap or n)), known, init_flag, None, -1
    f.deferred, f.grow_live, f.joseph = (flags.get(k, False) for k in ("deferred", "grow_live", "joseph"))
    return f


def test_wrapper_checks_come_before_the_library():
    d, s = _fake_handle(9), _fake_handle(9)
    closed = _fake_handle(9)
    closed._h = None
    bad = [lambda: d.extract_map(object()), lambda: d.extract_map(d), lambda: d.extract_map(closed), lambda: closed.extract_map(s),
           lambda: d.extract_map(s, [[0, 1]]), lambda: d.extract_map(s, [0.5]), lambda: d.extract_map(s, [0, -1]),
           lambda: d.extract_map(s, [1, 0, 1]), lambda: d.extract_map(s, [0, 1, 2, 3]), closed.extract_launch_info]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    f, g = _fake_filter(6, 4), _fake_filter(6, 4)
    placed = _fake_filter(6, 6, init_flag=True)
    bad = [lambda: f.submap([0, 4]), lambda: f.submap([-1]), lambda: f.submap([1, 1]), lambda: f.submap([[0]]),
           lambda: f.submap([0.0]), lambda: placed.submap([0]), lambda: f.submap([0], into=f), lambda: f.submap([0], into=object()),
           lambda: f.clone(into=f), lambda: f.clone(into=_fake_filter(5, 0)), lambda: f.clone(into=_fake_filter(6, 0, cap=7)),
           lambda: f.clone(into=_fake_filter(6, 0, deferred=True)), lambda: f.clone(into=_fake_filter(6, 0, grow_live=True)),
           lambda: f.clone(into=_fake_filter(6, 0, joseph=True)), lambda: f.restore(object()), lambda: f.restore(f)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert (g._known, g._init_flag) == (4, False)


def test_calls_are_declared_bound_and_documented():
    for name in ("ekf_dense64_extract_launch_info", "ekf_dense64_extract_map"):
        assert re.search(r"^ekf_status\s+" + name + r"\s*\(", HDR, re.M) and name in capi.SYMBOLS
        assert hasattr(capi.load(), name)
    text = " ".join(re.sub(r"\n \*", "\n", HDR).split())
    block = text[text.index("/* A map, or a submap, copied into a second handle"):text.index("ekf_status ekf_dense64_extract_launch_info")]
    for rule in ("iota(3 + 2 t + c) = 3 + 2 keep[t] + c", "A PURE COPY", "PENDING ROWS ARE CARRIED, NOT APPLIED",
                 "SRC IS UNCHANGED BIT FOR BIT", "DST IS THE ONE OVERWRITTEN",
                 "THE CHECKS COME IN THIS ORDER: (1) NULL dst; (2) NULL src; (3) dst == src; (4) the handles live on different "
                 "devices; (5) src's live dimension not odd or below 3; (6) k < 0, or keep == NULL with k neither b nor -1; "
                 "(7) an index of keep outside [0, b); (8) an index of keep repeated; (9) 3 + 2 k > dst's N",
                 "EKF_ERR_NOMEM", "ORIGINS SIT ON ODD INDICES", "A COLUMN TILE WHOSE LANDMARKS ARE A CONTIGUOUS ASCENDING RUN OF SRC",
                 "NO ATOMICS, NO REDUCTIONS: A RUN REPEATS BIT FOR BIT", "16 Nd^2", "k = 0 copies the pose alone"):
        assert rule in block, rule
    for doc, words in (("DESIGN.md", "4.8.23"), ("DESIGN.md", "k_ex_corner"), ("README.md", "ekf_dense64_extract.hip"),
                       ("INTEGRATION.md", "restore("), ("INTEGRATION.md", "submap(")):
        assert words in open(os.path.join(ROOT, doc)).read(), (doc, words)
    assert "ekf_dense64_extract.hip" in open(os.path.join(ROOT, "ekf_slam_ml_amd", "csrc", "Makefile")).read()
    for method in ("extract_map", "extract_launch_info"):
        assert callable(getattr(capi.DensePropagator64, method))
    for method in ("clone", "restore", "submap"):
        assert callable(getattr(capi.DenseEKFSLAM, method))
