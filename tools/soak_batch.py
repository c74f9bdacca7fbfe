"""Extended differential check of the batched unknown-association run against the single-filter API (bit for bit):
random pool sizes, map sizes, ragged measurement counts, split runs, LDS-resident / multi-kernel / prefix switches.
(scenarios and runs: tests/pool_soak_cases.py, which the seeded slice under -m gpu shares -- BATCH_SEEDS, tests/test_gpu_pool_soak.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: F401  (one HIP runtime)
from ekf_slam_ml_amd import capi as hip
import pool_soak_cases as cases

N_SCEN = int(sys.argv[1]) if len(sys.argv) > 1 else 200
bad = 0
for seed in range(N_SCEN):
    r = cases.run_batch(hip, cases.batch_scenario(seed))
    if not r.ok:
        bad += 1
        print(r.fail_line(), flush=True)
    if seed % 50 == 0:
        print("scenario", seed, "failures so far", bad, flush=True)
print("done, failures:", bad)
