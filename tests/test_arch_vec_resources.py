"""The one-launch tower rollout (tower_rollout_kernel, ph_arch.hip) checked where it is compiled (no GPU), by the method of
tests/test_kernel_resources.py: hipcc's resource-usage remarks for gfx950.  The kernel loops the body of tower_fwd_kernel and
advances the step's argument record in registers: the loop may cost registers, it may not add scratch -- a by-value argument record
that reaches scratch is a round trip per field per step."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def arch(tmp_path_factory):
    out = tmp_path_factory.mktemp("res") / "x.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "ph_arch.hip"), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|LDS Size \[bytes/block\]):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def _one(kernels, stem, valu):
    hit = {n: k for n, k in kernels.items() if stem + "ILb%dEE" % valu in n}
    assert len(hit) == 1, (stem, valu, sorted(kernels))
    return next(iter(hit.values()))


@pytest.mark.parametrize("valu", [0, 1])
def test_tower_rollout_kernel_adds_no_scratch_to_the_forward_it_loops(arch, valu):
    fwd, roll = _one(arch, "tower_fwd_kernel", valu), _one(arch, "tower_rollout_kernel", valu)
    print("VALU", valu, "forward", fwd, "rollout", roll)
    assert roll["ScratchSize"] <= fwd["ScratchSize"], (roll, fwd)
    assert roll["VGPRs Spill"] <= fwd["VGPRs Spill"], (roll, fwd)
