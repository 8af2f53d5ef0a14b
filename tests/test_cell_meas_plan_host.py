"""Host check of the neighbour-cell measurement's host-only rules (srsran_amd/csrc/cell_meas_plan.h: the input contract
of a job, the block count, the grouping by capture): builds tools/cell_meas_plan_check under the address and
undefined-behaviour sanitizers and runs it as a child process.  No GPU, no HIP headers, nothing preloaded; what it
checks is listed at the top of tools/cell_meas_plan_check/main.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_meas_plan_check(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tools/cell_meas_plan_check"
    exe = str(tmp_path / "cell_meas_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + os.path.join(ROOT, "srsran_amd", "csrc"),
                            os.path.join(ROOT, "tools", "cell_meas_plan_check", "main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "cell_meas_plan_check: OK" in run.stdout
