"""plan_search (csrc/idist_search_plan.hpp): which kernel, visited set, LDS and residency a search launch gets, as a pure function of
plain values.  Results are the same on every walk, so no parity test can see a wrong rule — this one holds the DECISIONS: alone on the
CPU (tests/host/search_plan.cpp) against tests/golden/search_plan.txt, a table recorded from launch_search as it stood before the
policy became that function (one line per case: facts and knobs -> the plan; it must hold every SearchWalk and an lds_short line), and
against the properties every plan has over the full cross product of the table's lists.  An intended change of policy is made by
regenerating the table (`search_plan print`) and reviewing its diff."""
import os
import subprocess

import engines


def test_plan_against_recorded_table(tmp_path):
    exe = str(tmp_path / "search_plan")
    simt = os.path.join(engines.ROOT, "tests", "simt")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-unused-variable",
                           "-Wno-unused-value", "-Wno-unused-result", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-DIDIST_EMU",
                           "-I" + simt, os.path.join(engines.ROOT, "tests", "host", "search_plan.cpp"), os.path.join(simt, "hip_emu.cpp"),
                           "-o", exe])
    table = os.path.join(engines.ROOT, "tests", "golden", "search_plan.txt")
    out = subprocess.run([exe, "check", table], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "search_plan ok" in out.stdout, out.stdout + out.stderr
    # `print` regenerates the committed file, line for line
    out = subprocess.run([exe, "print"], capture_output=True, text=True, timeout=300)
    with open(table) as f:
        assert out.returncode == 0 and out.stdout == f.read()
