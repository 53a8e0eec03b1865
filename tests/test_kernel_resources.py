"""Register and scratch budget of the checksum kernel, from the compiler's own
resource remarks (no GPU): validate_kernel runs at eight waves per SIMD only
while it stays within 64 VGPRs, and the default grid (8 workgroups per CU)
is clamped to the occupancy fit, so one register too many silently costs a
quarter of the waves."""
import re
import shutil
import subprocess

import pytest

from redpanda_amd import _build

HIPCC = shutil.which("hipcc")
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

REMARK = re.compile(r"remark: \s*([A-Za-z][A-Za-z /\[\]]*?):\s*(\S+)")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel name fragment -> {remark label -> value}} of rpgpu_kernels.hip."""
    out = tmp_path_factory.mktemp("resources") / "rpgpu_kernels.o"
    r = subprocess.run([HIPCC, *_build.rpgpu_flags(), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", str(_build.CSRC / "rpgpu_kernels.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        label, value = m.group(1).strip(), m.group(2)
        if label == "Function Name":
            cur = kernels.setdefault(value, {})
        elif cur is not None and value.isdigit():
            cur[label] = int(value)
    return kernels


def kernel(usage, name):
    hits = [v for k, v in usage.items() if f"{len(name)}{name}E" in k]  # Itanium mangling: <len><name>
    assert len(hits) == 1, (name, sorted(usage))
    return hits[0]


def test_validate_kernel_fits_eight_waves(usage):
    u = kernel(usage, "validate_kernel")
    print(u)
    assert u["VGPRs"] <= 64
    assert u["AGPRs"] == 0
    assert u["ScratchSize [bytes/lane]"] == 0
    assert u["VGPRs Spill"] == 0
    assert u["SGPRs Spill"] == 0
    assert u["Occupancy [waves/SIMD]"] == 8
    assert u["LDS Size [bytes/block]"] <= 20480
