"""Extended differential check of the column panel of delayed known-association runs (EKF_FORM_COLUMN_PANEL): random pools
(1-19 filters, n = 100 ... 1000 around the panel's minimum dimension 256, 1-64 corrections per flush, 1-6 reading slots per
step, blind steps, filters that sit steps out, random run boundaries with and without a getter in between, plain and strip
flush) with the panel on, with the one-slot plan, and with the panel off: state and covariance of every filter must be
BIT-identical between the three; with the kept current rows / columns on top (the default) within 1e-10 of them; and all
within 1e-9 of the eager run.   python tools/soak_panel.py [N=60] [first_seed=0]
(scenarios and runs: tests/pool_soak_cases.py, which the seeded slice under -m gpu shares -- PANEL_SEEDS, tests/test_gpu_pool_soak.py)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from ekf_slam_ml_amd import capi as hip
import pool_soak_cases as cases

N_SCEN = int(sys.argv[1]) if len(sys.argv) > 1 else 60
FIRST = int(sys.argv[2]) if len(sys.argv) > 2 else 0
bad = 0
for seed in range(FIRST, FIRST + N_SCEN):
    r = cases.run_panel(hip, cases.panel_scenario(seed))
    if not r.ok:
        bad += 1
        print(r.fail_line(), flush=True)
    if (seed - FIRST) % 10 == 9:
        print("scenario", seed, "failures so far", bad, "| last: panel launches", r.counts["panel"]["gain_from_panel"], flush=True)
print("done, failures:", bad)
