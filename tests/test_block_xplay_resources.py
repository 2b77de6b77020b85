"""The kernels of the block worlds' cross-play checked where they are compiled (no GPU), by the method of
tests/test_adap_members_resources.py: hipcc's resource-usage remarks for gfx950.

group_fwd16h_kernel and group_fwd32_kernel (ph_policy.hip) patch a by-value launch record with a member's fields from the
device-side table and hand it to a forward body; the scripted rule and the step's two book-keeping kernels (ph_block.hip) unpack a
table into registers: none of them may reach scratch.  pool_fwd16h_kernel -- the grouped forward of every Liar's Dice population --
must be what it was: its figures are those tests/test_adap_members_resources.py records."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

PARENT_FWD16H = {"VGPRs": 179, "AGPRs": 8, "TotalSGPRs": 106, "ScratchSize": 0, "VGPRs Spill": 0, "LDS Size": 0}
NEW_KERNELS = {"ph_policy.hip": ["group_fwd16h_kernel", "group_fwd32_kernel"],
               "ph_block.hip": ["block_scripted_actions_kernel", "block_group_scripted_kernel", "block_xp_after_ego_kernel",
                                "block_xp_after_alt_kernel"]}


def _remarks(unit, out):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, unit), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]):\s+(\d+)",
                      line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("res")
    return {unit: _remarks(unit, tmp / (unit + ".o")) for unit in NEW_KERNELS}


def _one(kernels, stem):
    hit = {n: k for n, k in kernels.items() if stem in n}
    assert len(hit) == 1, (stem, sorted(kernels))
    return next(iter(hit.values()))


@pytest.mark.parametrize("unit,stem", [(u, s) for u, stems in NEW_KERNELS.items() for s in stems])
def test_new_kernel_has_no_scratch_and_no_spills(units, unit, stem):
    k = _one(units[unit], stem)
    print(stem, k)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["VGPRs"] + k["AGPRs"] <= 256, k


def test_pool_fwd16h_kernel_is_what_it_was(units):
    k = _one(units["ph_policy.hip"], "pool_fwd16h_kernelILb0EE")
    print("pool_fwd16h_kernel", k, "recorded", PARENT_FWD16H)
    assert {key: k[key] for key in PARENT_FWD16H} == PARENT_FWD16H, k
