"""What the tests of the optical-flow estimator share (tests/test_gpu_flow*.py, and the resource gates of tests/test_cpu_flow_*.py): moving
arrays to the device, the three gates against the numpy models, the compiler's resource report of the kernels, and the two helpers of the
executables' tests.  With e32 = max|M32 - M64| of the two CPU models on the same input, every gate bounds max|GPU - M64|; the gates
differ and each test keeps its own.  Nothing is measured against the code under test."""
import os
import re
import subprocess

import numpy as np


def dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def gate_floor(gpu, m32, m64, what):
    """tests/test_gpu_flow.py: max(4 e32, 2^-20 max(1, max|M64|)), and 4 e32 itself within the 0.02 px the estimator was specified to"""
    e32 = float(np.abs(m32.astype(np.float64) - m64).max())
    bound = max(4 * e32, 2.0 ** -20 * max(1.0, float(np.abs(m64).max())))
    err = float(np.abs(gpu.astype(np.float64) - m64).max())
    print(f"{what}: e32 {e32:.3e}  max|GPU - M64| {err:.3e}  bound {bound:.3e}")
    assert 4 * e32 <= 0.02, (what, e32)
    assert err <= bound, (what, err, bound)


def gate_stage_robust(gpu, m32, m64, what):
    """tests/test_gpu_flow_robust.py, the stage entries: max(4 e32, 2^-20 max(1, max|M64|))"""
    e32 = float(np.abs(m32.astype(np.float64) - m64).max())
    bound = max(4 * e32, 2.0 ** -20 * max(1.0, float(np.abs(m64).max())))
    err = float(np.abs(gpu.astype(np.float64) - m64).max())
    print(f"{what}: e32 {e32:.3e}  max|GPU - M64| {err:.3e}  bound {bound:.3e}  bit-equal to M32: {np.array_equal(gpu, m32)}")
    assert err <= bound, (what, err, bound)


def gate_4e32(gpu, m32, m64, what):
    """tests/test_gpu_flow_grad.py: 4 e32, no floor, and every value finite"""
    e32 = float(np.abs(m32.astype(np.float64) - m64).max())
    err = float(np.abs(gpu.astype(np.float64) - m64).max())
    print(f"{what}: e32 {e32:.3e}  max|GPU - M64| {err:.3e}  bound {4 * e32:.3e}  max|M64| {np.abs(m64).max():.3g}  bit-equal to M32: {np.array_equal(gpu, m32)}")
    assert np.isfinite(gpu).all() and err <= 4 * e32, (what, err, e32)


_usage = {}


def kernel_resource_usage(hipcc, tmp_path):
    """{mangled kernel name: {VGPRs, AGPRs, ScratchSize, Occupancy, LDS}} of csrc/kernels_flow.hip: the compiler's kernel-resource-usage
    remarks with the Makefile's flags (as tests/test_cpu_kernel_budget.py reads them), compiled once per run"""
    if not _usage:
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fhip-fp32-correctly-rounded-divide-sqrt", "-ffp-contract=off",
                            "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(root, "include"),
                            os.path.join(root, "fast-artistic-videos_amd", "csrc", "kernels_flow.hip"), "-o", str(tmp_path / "flow.o")],
                           capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        cur = None
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = _usage.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return _usage


def write_ppm(path, a):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0])); f.write(np.ascontiguousarray(a).tobytes())


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (cmd, r.stdout[-2000:], r.stderr[-2000:])
    return r
