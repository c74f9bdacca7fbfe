"""CPU: the ledger behind every device allocation (ekf_device_mem.hpp: DeviceLedger, ScopedLedger, DeviceBuf), driven by
tests/cpp/device_mem_check.cpp over a fake memory policy that fails the k-th allocation or the k-th fill, for every k and
with no failure: a group is complete and initialised or absent, a refused growth leaves the old buffer in force, a scope
frees what it allocated however it ends, nothing is freed twice or filled after it was freed.  Built plain and with
AddressSanitizer + UBSan (a stand-alone program: nothing is preloaded)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WANT = ["ok replace_group 1", "ok replace_group 3", "ok replace_group 9", "ok grow", "ok scoped", "ok other"]


@pytest.mark.parametrize("sanitize", [False, True])
def test_device_ledger_on_a_fake_policy(tmp_path, sanitize):
    exe = str(tmp_path / "device_mem_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "ekf_slam_ml_amd", "csrc"),
                    "-o", exe, os.path.join(HERE, "cpp", "device_mem_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.split("\n")[:-1] == WANT, run.stdout
