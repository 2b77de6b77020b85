"""What the tail wave of the one-launch rollout (csrc/ph_policy.hip: policy_fwd16_body, TW = 4) may cost, checked where the kernels
are compiled (no GPU).  ph_policy.hip is compiled for gfx950 twice in one session -- this tree's and the tree of the commit in front
of the one that brought the tail wave (the one that added this file) -- and hipcc's resource remarks and the code objects' metadata are
compared.  The parent is fixed: these forms of the body are pinned to what they cost before the tail wave, as
tests/test_kernel_resources.py pins other kernels to numbers.  A later change that moves one of their figures on purpose rewrites the
comparison and says so.  Only the kernels that instantiate policy_fwd16_body are compared, so work on the unit's other kernels does
not touch it.  Without the history to build the parent from (no .git, a shallow clone) the comparison is skipped with that reason;
the first test below needs no history.

  * the MFMA instantiations of policy_fwd16_rollout_kernel are the ONLY kernels of the unit whose workgroup size changed (256 ->
    320), and no rollout instantiation has scratch or a spilled vector register;
  * the per-step, the multi-agent and the exchange-rollout forms of the same body and the rollout's VALU cross-check, which keep
    wave 0 as their tail wave, report the parent's registers, LDS and scratch, figure for figure."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
THIS = os.path.relpath(os.path.abspath(__file__), ROOT)
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "LDS Size")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def _compile(root, out_dir):
    """{kernel: figures + 'threads'} of ph_policy.hip in the tree under `root`"""
    csrc = os.path.join(root, "pantheonrl_amd", "csrc")
    asm = os.path.join(out_dir, "ph_policy.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(root, "include"), "-I", csrc,
                        "--cuda-device-only", "-S", os.path.join(csrc, "ph_policy.hip"), "-o", asm,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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
    threads = None     # the code-object metadata lists, per kernel, .max_flat_workgroup_size in front of .name
    for line in open(asm):
        m = re.match(r"\s+\.max_flat_workgroup_size:\s+(\d+)", line)
        if m:
            threads = int(m.group(1))
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m and m.group(1) in kernels and threads is not None:
            kernels[m.group(1)]["threads"] = threads
            threads = None
    assert kernels and all("threads" in k and all(f in k for f in FIGURES) for k in kernels.values()), kernels
    return kernels


SOURCES = ("pantheonrl_amd/csrc", "include")


def _parent_tree(dst):
    """(tree, None) of the commit in front of the one that added this file -- in front of the work tree while the file is
    uncommitted -- or (None, why not)"""
    def git(*args, **kw):
        return subprocess.run(["git", "-C", ROOT, *args], capture_output=True, timeout=120, **kw)
    if shutil.which("git") is None or git("rev-parse", "--git-dir").returncode != 0:
        return None, "no git history here to build the parent's ph_policy.hip from"
    added = git("log", "--diff-filter=A", "--format=%H", "--", THIS).stdout.decode().split()
    rev = added[-1] + "^" if added else "HEAD"
    if git("rev-parse", "--verify", rev + "^{commit}").returncode != 0:
        return None, "the commit in front of the tail wave's is not in this history (shallow clone)"
    tar = git("archive", rev, *SOURCES)
    if tar.returncode != 0:
        return None, "git archive of the parent failed: " + tar.stderr.decode()[-200:]
    subprocess.run(["tar", "-x", "-C", dst], input=tar.stdout, check=True, timeout=120)
    return dst, None


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    parent_root, why_not = _parent_tree(str(tmp_path_factory.mktemp("parent_tree")))
    with ThreadPoolExecutor(max_workers=2) as pool:
        change = pool.submit(_compile, ROOT, str(tmp_path_factory.mktemp("change")))
        parent = pool.submit(_compile, parent_root, str(tmp_path_factory.mktemp("parent"))) if parent_root else None
        return change.result(), (parent.result() if parent else why_not)


def _is_tail_wave_rollout(name):     # policy_fwd16_rollout_kernel<VALU = false, LEAN = *>
    return "policy_fwd16_rollout_kernelILb0E" in name


def test_rollout_instantiations_have_five_waves_and_no_scratch(builds):
    change, _ = builds
    rollout = {n: k for n, k in change.items() if "policy_fwd16_rollout_kernel" in n}
    assert any(_is_tail_wave_rollout(n) for n in rollout) and not all(_is_tail_wave_rollout(n) for n in rollout), sorted(rollout)
    for n, k in rollout.items():
        assert k["threads"] == (320 if _is_tail_wave_rollout(n) else 256), (n, k)      # (the VALU cross-check keeps wave 0's tail)
        assert k["ScratchSize"] == 0, (n, k)
        if _is_tail_wave_rollout(n):     # two waves share SIMD 0: both have to fit its 512 registers, without a spill
            assert k["VGPRs Spill"] == 0 and k["VGPRs"] + k["AGPRs"] <= 256, (n, k)


def test_only_the_rollout_changed_its_workgroup_and_the_other_forms_keep_the_parents_figures(builds):
    change, parent = builds
    if isinstance(parent, str):
        pytest.skip(parent)
    resized = {n for n in change if n in parent and change[n]["threads"] != parent[n]["threads"]}
    assert resized == {n for n in change if _is_tail_wave_rollout(n)}, sorted(resized)
    for n in resized:
        assert (parent[n]["threads"], change[n]["threads"]) == (256, 320), (n, parent[n], change[n])
    body_forms = [n for n in change if re.search(r"policy_fwd16_(kernel|multi_kernel|exchange_rollout_kernel|rollout_kernel)", n) and n not in resized]
    assert set(body_forms) <= set(parent), sorted(set(body_forms) - set(parent))
    assert {"policy_fwd16_kernel", "policy_fwd16_multi_kernel", "policy_fwd16_exchange_rollout_kernel", "policy_fwd16_rollout_kernel"} <= \
        {re.search(r"policy_fwd16_\w*?kernel", n).group(0) for n in body_forms}, sorted(body_forms)
    for n in body_forms:
        assert {f: change[n][f] for f in FIGURES} == {f: parent[n][f] for f in FIGURES}, (n, parent[n], change[n])
