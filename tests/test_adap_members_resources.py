"""The ADAP tiles of the pool's grouped forward (pool_adap_kernel, ph_policy.hip) checked where they are compiled (no GPU), by the
method of tests/test_arch_vec_resources.py: hipcc's resource-usage remarks for gfx950.

pool_adap_kernel patches a by-value launch record with a member's fields from the device-side table and hands it to the general
32-row forward: it may not reach scratch.  pool_fwd16h_kernel -- the kernel of every population WITHOUT an ADAP member -- must be
what it was: its figures are held to those of a build of the commit before ADAP members, recorded here from that build (not from
this tree)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# pool_fwd16h_kernel<false> of the parent commit (ph_policy.hip, -O3, gfx950): LDS is dynamic, hence 0 static bytes
PARENT_FWD16H = {"VGPRs": 179, "AGPRs": 8, "TotalSGPRs": 106, "ScratchSize": 0, "VGPRs Spill": 0, "LDS Size": 0}


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    out = tmp_path_factory.mktemp("res") / "x.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "ph_policy.hip"), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
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


def _one(kernels, stem):
    hit = {n: k for n, k in kernels.items() if stem in n}
    assert len(hit) == 1, (stem, sorted(kernels))
    return next(iter(hit.values()))


def test_pool_adap_kernel_has_no_scratch_and_no_spills(policy):
    k = _one(policy, "pool_adap_kernel")
    print("pool_adap_kernel", k)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["VGPRs"] + k["AGPRs"] <= 256, k


def test_pool_fwd16h_kernel_is_what_the_parent_commit_built(policy):
    k = _one(policy, "pool_fwd16h_kernelILb0EE")
    print("pool_fwd16h_kernel", k, "parent", PARENT_FWD16H)
    assert {key: k[key] for key in PARENT_FWD16H} == PARENT_FWD16H, k
