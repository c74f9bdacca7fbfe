"""Extended differential check of the symmetric option of the delayed mode (row-only gain steps, mirrored flush, rows-only
prediction upkeep inside a run) against the eager run of the same pool: random pool sizes, map sizes (around the 256
threshold of the mirrored flush too), corrections per flush, reading slots per step, steps without any visible landmark,
run boundaries.  States within 1e-9, covariances within 1e-9 relative; after every run the covariance handed back must be
symmetric to the bit outside the 32 x 32 diagonal squares when the mirrored flush ran.
(scenarios and runs: tests/pool_soak_cases.py, which the seeded slice under -m gpu shares -- SYMMETRIC_SEEDS, tests/test_gpu_pool_soak.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: F401  (one HIP runtime)
from ekf_slam_ml_amd import capi as hip
import pool_soak_cases as cases

N_SCEN = int(sys.argv[1]) if len(sys.argv) > 1 else 60
bad = 0
for seed in range(N_SCEN):
    r = cases.run_symmetric(hip, cases.symmetric_scenario(seed))
    if not r.ok:
        bad += 1
        print(r.fail_line(), flush=True)
    if seed % 10 == 9:
        print("scenario", seed, "failures so far", bad, flush=True)
print("done, failures:", bad)
