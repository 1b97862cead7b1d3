"""Which engine a test module runs on.

  * "emu": the product's csrc compiled for the CPU lockstep emulator (tests/simt) — test
    infrastructure that lets the real kernel source + C-ABI host code run without a GPU.
    Selected only here, by swapping the ctypes handle inside the test process; the product
    has no switch for it.
  * "gpu": instant-distance_amd/csrc/libidist.so on a real MI355X (pytest -m gpu).
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "simt", "_build", "libidist_emu.so")


def engine_params():
    return [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


_CUS = {}


def cu_count(kind):
    """The CU count the engine sizes its grids by: 1 under the emulator (its multiProcessorCount); on the GPU device 0's, asked of
    torch in a child process, once — torch brings a HIP runtime of its own, which must not be initialised next to the library's."""
    if kind != "gpu":
        return 1
    if "gpu" not in _CUS:
        out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                             capture_output=True, text=True, timeout=300, check=True).stdout
        _CUS["gpu"] = int(out.split()[-1])
        assert 1 <= _CUS["gpu"] <= 1024
    return _CUS["gpu"]


def build_emu():
    # everything the emulator library is compiled from: every source of csrc, the C ABI, the emulator itself
    csrc = os.path.join(ROOT, "instant-distance_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp"))]
    srcs += [os.path.join(ROOT, "include", "idist.h")]
    srcs += [os.path.join(ROOT, "tests", "simt", f) for f in ("hip_emu.hpp", "hip_emu.cpp")]
    def stale():
        return not os.path.exists(EMU_SO) or os.path.getmtime(EMU_SO) < max(os.path.getmtime(s) for s in srcs)

    if stale():
        # pytest-xdist workers race for the rebuild: one builds (into a temporary name, renamed when complete), the others wait
        import fcntl

        os.makedirs(os.path.dirname(EMU_SO), exist_ok=True)
        with open(EMU_SO + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if stale():
                subprocess.check_call([os.path.join(ROOT, "tests", "simt", "build_emu.sh")], stdout=subprocess.DEVNULL)
    return EMU_SO
