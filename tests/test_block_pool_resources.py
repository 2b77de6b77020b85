"""The kernels of the block worlds' partner pool checked where they are compiled (no GPU), by the method of
tests/test_block_xplay_resources.py: hipcc's resource-usage remarks for gfx950.

group_learn16h_kernel (ph_policy.hip) patches a by-value launch record with a learner's parameters, caches and ragged-buffer bases
from the device-side member table and hands it to the 16-row one-hot body; the step's two book-keeping kernels (ph_block.hip) unpack
a table and a PoolBook lane into registers: none of them may reach scratch or spill a register.  The kernels beside them must be
what they were: pool_fwd16h_kernel its recorded figures, group_fwd16h_kernel and group_fwd32_kernel the figures of the parent
commit's ph_policy.hip."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# pool_fwd16h_kernel<false>: what tests/test_adap_members_resources.py and tests/test_block_xplay_resources.py record
POOL_FWD16H = {"VGPRs": 179, "AGPRs": 8, "TotalSGPRs": 106, "ScratchSize": 0, "VGPRs Spill": 0, "LDS Size": 0}
# the parent commit's ph_policy.hip ("Cross-play evaluation of the block worlds on the device"), compiled once with this file's
# command line (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage) when the learner tiles were added
PARENT_GROUP = {
    "group_fwd16h_kernel": {"VGPRs": 178, "AGPRs": 8, "TotalSGPRs": 106, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0, "LDS Size": 0},
    "group_fwd32_kernel": {"VGPRs": 132, "AGPRs": 16, "TotalSGPRs": 106, "ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0, "LDS Size": 0},
}
NEW_KERNELS = {"ph_policy.hip": ["group_learn16h_kernel"],
               "ph_block.hip": ["block_pool_after_ego_kernel", "block_pool_after_alt_kernel"]}


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
    print("pool_fwd16h_kernel", k, "recorded", POOL_FWD16H)
    assert {key: k[key] for key in POOL_FWD16H} == POOL_FWD16H, k


@pytest.mark.parametrize("stem", sorted(PARENT_GROUP))
def test_group_forward_kernels_are_what_the_parent_commit_built(units, stem):
    k = _one(units["ph_policy.hip"], stem)
    print(stem, k, "parent", PARENT_GROUP[stem])
    assert {key: k[key] for key in PARENT_GROUP[stem]} == PARENT_GROUP[stem], k


def test_no_new_kernel_name_holds_a_stem_another_resource_test_looks_up():
    """tests/test_*_resources.py find a kernel by a substring of its mangled name and assert exactly one match"""
    stems = ["group_fwd16h_kernel", "group_fwd32_kernel", "pool_fwd16h_kernel", "pool_adap_kernel", "block_xp_after_ego_kernel",
             "block_xp_after_alt_kernel", "block_scripted_actions_kernel", "block_group_scripted_kernel", "policy_fwd16_kernel",
             "policy_fwd16h_kernel", "liar_rollout_kernel"]
    for names in NEW_KERNELS.values():
        for name in names:
            assert not any(stem in name for stem in stems), name
