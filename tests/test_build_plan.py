"""plan_build / plan_build_step (csrc/idist_build_plan.hpp): set, tiles, kernels and streams of a build, and what every step of its
schedule launches on which stream, as pure functions of plain values.  Every build variant gives the same graph, so no parity test can
see a wrong rule — this one holds the DECISIONS: alone on the CPU (tests/host/build_plan.cpp) against tests/golden/build_plan.txt, a
table recorded from run_build as it stood before the policy became these functions (one line per case: facts and knobs -> the plan,
the number of steps and a digest of the steps; what it must hold is listed in its header and checked), and against the properties
every plan and every step has over the full cross product of the table's lists.  An intended change of policy is made by regenerating
the table (`build_plan print`) and reviewing its diff."""
import os
import subprocess

import engines


def test_plan_against_recorded_table(tmp_path):
    exe = str(tmp_path / "build_plan")
    simt = os.path.join(engines.ROOT, "tests", "simt")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                           "-Wno-unused-value", "-Wno-unused-result", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-DIDIST_EMU",
                           "-I" + simt, os.path.join(engines.ROOT, "tests", "host", "build_plan.cpp"), os.path.join(simt, "hip_emu.cpp"),
                           "-o", exe])
    table = os.path.join(engines.ROOT, "tests", "golden", "build_plan.txt")
    out = subprocess.run([exe, "check", table], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "build_plan ok" in out.stdout, out.stdout + out.stderr
    # `print` regenerates the committed file, line for line
    out = subprocess.run([exe, "print"], capture_output=True, text=True, timeout=300)
    with open(table) as f:
        assert out.returncode == 0 and out.stdout == f.read()
