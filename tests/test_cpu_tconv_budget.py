"""Register / scratch budget of the transposed-convolution kernel (kernels_tconv.hip), from the compiler's kernel-resource-usage remarks
(the method of test_cpu_kernel_budget.py; hipcc cross-compiles for gfx950 without a GPU): its eight accumulator tiles and the fragments
of one tap stay in registers -- no scratch -- inside the 256 registers of two waves per SIMD."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-artistic-videos_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize",
         "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include")]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_every_instantiation_of_the_transposed_kernel_fits(tmp_path):
    p = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "kernels_tconv.hip"), "-o", str(tmp_path / "tconv.o")],
                       stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "conv_tconv_kernel" in k}
    assert kernels, usage.keys()
    for name, u in kernels.items():
        assert u["ScratchSize"] == 0 and u["VGPRs"] <= 256, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 256 and u["Occupancy"] >= 2, (name, u)      # two blocks of four waves per CU
