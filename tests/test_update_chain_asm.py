"""The serial sections the two-launch minibatch step must not grow back, read off hipcc's gfx950 assembly of ph_ppo.hip (no GPU):

* ppo_reduce_kernel issues its early loads (the KL stop flag, the slab position's parameter index) and starts the slab walk without
  waiting for either -- a wait for a vector load in front of the first slab load is a cold memory round trip every wave of every
  block sits through (the compiler put one there when the table lookup stood in a divergent block);
* ppo_adam_kernel has ONE barrier: the bias corrections come from the train() call's table or are computed in front of it, and every
  lane folds the four wave sums itself, so there is no single-lane section whose result a second barrier would broadcast."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

REDUCE = ["_ZN2ph17ppo_reduce_kernelILi%dEEEvNS_10ReduceArgsE" % v for v in (1, 2, 4)]
ADAM = "_ZN2ph15ppo_adam_kernelENS_8AdamArgsE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel symbol -> its instructions in text order (mnemonic and operands, no labels, directives or comments)"""
    out = tmp_path_factory.mktemp("asm") / "ppo.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
                        "--cuda-device-only", os.path.join(CSRC, "ph_ppo.hip"), "-o", str(out)], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    found = {}
    for name in REDUCE + [ADAM]:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.M | re.S)
        assert m, name
        found[name] = [l.strip() for l in m.group(1).splitlines()
                       if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    return found


@pytest.mark.parametrize("name", REDUCE)
def test_reduce_kernel_waits_for_no_vector_load_before_its_first_slab_load(kernels, name):
    ins = kernels[name]
    first = next(i for i, l in enumerate(ins) if l.startswith("buffer_load"))
    early = [l for l in ins[:first] if l.startswith(("global_load", "flat_load"))]
    assert early, (name, "the stop flag and the table lookup go out in front of the slab walk")
    waits = [l for l in ins[:first] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert not waits, (name, first, waits)


def test_adam_kernel_has_one_barrier(kernels):
    ins = kernels[ADAM]
    assert sum(l.startswith("s_barrier") for l in ins) == 1
