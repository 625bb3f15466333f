"""The grouped weight-gradient planner (csrc/conv_wgrad_plan.hip) is host-only code: tools/wgrad_plan_check.hip links it into a stand-alone
program -- no kernel file, no Python -- built with AddressSanitizer and UBSan, which plans the lists of tests/golden/gen_wgrad_layout_parent.py
at every dealing mode, checks each layout's structure and asks for every refusal. This test builds and runs that program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_planner_runs_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wgrad_plan_check")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           os.path.join(ROOT, "tools", "wgrad_plan_check.hip"), os.path.join(ROOT, "unit_amd", "csrc", "conv_wgrad_plan.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("UNIT_WGRAD_GANG", "UNIT_WGRAD_DEAL")}
    ran = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stderr
    assert ran.stderr == ""
