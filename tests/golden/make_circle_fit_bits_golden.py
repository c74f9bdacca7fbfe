"""Writes tests/golden/circle_fit_bits.npz: the raw outputs of the two circle-fit kernels -- k_circles through
circle_fit_scans(..., want_all=True) at S = 1 and k_scan_circles through DensePropagator64.fit_scan(..., want_all=True) -- on
29 scans of tests/dense_scan_cases.py and test_circle_oracle.RANGES, with the scans themselves (a scan built again on another
machine could differ in its last bit).  tests/test_gpu_circle_fit_bits.py replays the scans and asks for the same bytes, so
the file is recorded on the commit whose arithmetic is to be kept, run by hand on a machine with the GPU:

    python tests/golden/make_circle_fit_bits_golden.py

Layout: ranges (all scans end to end), nb [n], names [n]; per kernel K in (lane, wave): K_count [n] circles kept, K_clusters
[n], K_centres [sum count, 2], K_radii [sum count], K_all [sum clusters, 4] -- only the rows the kernel wrote.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from ekf_slam_ml_amd import capi  # noqa: E402
import dense_scan_cases as sc  # noqa: E402
from test_circle_oracle import RANGES  # noqa: E402

MAX_OUT = 32
NONFINITE = "nan_inf"            # the one scan whose outputs are compared up to a NaN's payload


def scans():
    sim = sc.simulated_scans()[1]
    wrap = np.full(360, 3.0); wrap[:10] = 1.0; wrap[-12:] = 1.05
    nan = sim[3].copy()
    nan[50], nan[200], nan[201] = np.nan, np.inf, np.inf       # test_gpu_dense64_scan.test_nan_and_inf_ranges_against_k_circles
    out = [("kat", np.array(RANGES))]
    out += [(f"sim{s}", sim[s]) for s in range(8)]
    out += [(f"beams{nb}_{s}", sc.beam_count_scans(nb)[s]) for nb in (90, 1024) for s in range(2)]
    out += [("circles3", sc.circles_scan(3)), ("many", sc.many_clusters_scan())]
    out += [(f"long{n}", sc.long_cluster_scan(n)) for n in (65, 129, 300)]
    out += [(f"len{n}", sc.length_scan(n)) for n in (6, 7)]
    out += [(f"position{k}", r) for k, (r, _) in enumerate(sc.position_scans(360, 9))]
    out += [("flat", np.full(360, 1.0)), ("saw", sc.saw(360)), ("wrap", wrap)]
    out += [(f"ramp{n}", sc.ramp_scan(n)) for n in (8, 65)]
    out += [(NONFINITE, nan)]
    return [(name, np.ascontiguousarray(r, dtype=np.float64)) for name, r in out]


def main():
    cases = scans()
    dev = capi.DensePropagator64(23)
    rec = {"lane": [], "wave": []}
    for _, r in cases:
        cen, rad, allc = capi.circle_fit_scans(r, max_out=MAX_OUT, want_all=True)
        rec["lane"].append((cen[0], rad[0], allc[0]))
        rec["wave"].append(dev.fit_scan(r, max_out=MAX_OUT, want_all=True)[:3])
    dev.close()
    # a scan of k_circles does not depend on its neighbours in the batch: the test relies on it
    b360 = [i for i, (_, r) in enumerate(cases) if len(r) == 360]
    cen, rad, allc = capi.circle_fit_scans(np.stack([cases[i][1] for i in b360]), max_out=MAX_OUT, want_all=True)
    for j, i in enumerate(b360):
        for got, want in zip((cen[j], rad[j], allc[j]), rec["lane"][i]):
            assert got.shape == want.shape and (got.tobytes() == want.tobytes() or cases[i][0] == NONFINITE), cases[i][0]
    out = {"ranges": np.concatenate([r for _, r in cases]), "nb": np.array([len(r) for _, r in cases], dtype=np.int32),
           "names": np.array([name for name, _ in cases])}
    for k, rows in rec.items():
        out[k + "_count"] = np.array([len(c) for c, _, _ in rows], dtype=np.int32)
        out[k + "_clusters"] = np.array([len(a) for _, _, a in rows], dtype=np.int32)
        out[k + "_centres"] = np.concatenate([c.reshape(-1, 2) for c, _, _ in rows])
        out[k + "_radii"] = np.concatenate([x for _, x, _ in rows])
        out[k + "_all"] = np.concatenate([a.reshape(-1, 4) for _, _, a in rows])
    for (name, r), lane, wave in zip(cases, rec["lane"], rec["wave"]):
        print(f"{name:12s} {len(r):5d} beams  k_circles {len(lane[2]):3d} clusters {len(lane[0]):2d} circles   "
              f"k_scan_circles {len(wave[2]):3d} clusters {len(wave[0]):2d} circles   "
              f"non-finite outputs {int((~np.isfinite(lane[2])).sum())} / {int((~np.isfinite(wave[2])).sum())}")
    path = os.path.join(HERE, "circle_fit_bits.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "scans")


if __name__ == "__main__":
    main()
