"""One minibatch step of behavioural cloning -- the row loss with dL/dlogits, the minibatch schedule, the statistics row, Adam's bias
corrections, moments and the two parameter updates -- is defined in pantheonrl_amd/csrc/ph_bc_loss.h (on top of ph_bc_row.h), and both
training kernels of ph_bc.hip, bc_train_kernel and bc_train_mfma_kernel, call it.  A kernel that writes one of these out again is a
second copy to keep in step: the GPU tests compare each kernel with the checker, not the copies with each other.

TWO written-out copies stay, each because the helper called at the site changed its kernel's compiled resources and the conversion's
rule was that no kernel's registers move (the policy tail of ppo_grad_split_oh_kernel is the precedent, tests/
test_loss_single_definition.py; comments at both sites name the header):

* STATS_EXCEPTION: bc_train_kernel's statistics row.  That kernel scales its four block sums in every thread, in front of its
  `tid == 0` branch; with bc_write_stats called there -- in any of four placements, or in a form that takes the scaled sums -- the
  scaling is emitted behind the branch and the kernel spills 50 SGPRs, not 49.  bc_train_mfma_kernel calls the helper.
* SCATTER_EXCEPTION: bc_train_mfma_kernel's one-hot scatter.  With bc_hot_feature called there the compiler merges the site's two
  bounds loads and drops its branch, and bc_train_mfma_kernel<false> goes from 104 to 102 AGPRs.  bc_train_kernel's scatter, the
  forward and the clone tile call the helper.

The check is textual, over csrc/*.hip and *.h without their // comments: it finds a pasted copy, which keeps the names c / act,
x / n and neglogp / ent_loss / l2_loss; it does not find a copy rewritten under other names."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pantheonrl_amd", "csrc")
HEADER, ROW_HEADER, KERNELS = "ph_bc_loss.h", "ph_bc_row.h", "ph_bc.hip"
DLOGITS = re.compile(r"\(\s*c\s*==\s*act\s*\)\s*\?\s*1\.f\s*:\s*0\.f")                  # the [c = a] of dL/dlogits
HOT_CLAMP = re.compile(r"x\s*>=\s*n\s*\?\s*n\s*-\s*1\s*:\s*x")                            # the one-hot clamp of an observation value
STATS_ROW = re.compile(r"neglogp\s*\+\s*ent_loss\s*\+\s*l2_loss")                         # st[6], the loss of the statistics row
STATS_EXCEPTION = {KERNELS: 1}      # bc_train_kernel's statistics row (docstring)
SCATTER_EXCEPTION = {KERNELS: 1}    # bc_train_mfma_kernel's one-hot scatter (docstring)


def _code(path):
    """the file without its // comments"""
    return "\n".join(line.split("//")[0] for line in open(path).read().splitlines())


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert os.path.join(CSRC, HEADER) in files and len(files) > 20
    return files


def _counts(pattern, files):
    found = {os.path.basename(p): len(pattern.findall(_code(p))) for p in files}
    return {name: n for name, n in found.items() if n}


def test_dlogits_and_the_statistics_row_stand_in_the_loss_header():
    assert _counts(DLOGITS, _sources()) == {HEADER: 1}
    assert _counts(STATS_ROW, _sources()) == {HEADER: 1, **STATS_EXCEPTION}


def test_one_hot_clamp_of_the_bc_kernels_stands_in_the_row_header():
    """among the BC files: the PPO kernels' one-hot staging (ph_device.h, ph_ppo.hip) has its own and is not behavioural cloning's"""
    bc = [p for p in _sources() if os.path.basename(p).startswith("ph_bc")]
    assert len(bc) == 3, bc
    assert _counts(HOT_CLAMP, bc) == {ROW_HEADER: 1, **SCATTER_EXCEPTION}


def test_training_kernels_call_the_header():
    code = _code(os.path.join(CSRC, KERNELS))
    assert '#include "%s"' % HEADER in code
    assert "__logf(" not in code                      # no log-sum-exp of its own: bc_lse, through bc_loss_row and in the forward
    assert "h -= __expf(lq) * lq" not in code         # nor an entropy sum: bc_entropy
    calls = {name: len(re.findall(r"\b%s\(" % name, code)) for name in
             ("bc_loss_row", "bc_adam_moments", "bc_bias_corrections", "bc_schedule", "bc_write_stats", "bc_hot_feature",
              "bc_adam_param_ieee", "bc_adam_param_fast", "bc_entropy")}
    for name in ("bc_loss_row", "bc_adam_moments", "bc_bias_corrections", "bc_schedule"):
        assert calls[name] == 2, calls               # once per training kernel
    assert calls["bc_write_stats"] == 2 - STATS_EXCEPTION[KERNELS], calls
    assert calls["bc_hot_feature"] == 3 - SCATTER_EXCEPTION[KERNELS], calls     # bc_train_kernel's scatter and the forward
    assert calls["bc_adam_param_ieee"] == 1 and calls["bc_adam_param_fast"] == 1 and calls["bc_entropy"] == 1, calls
    # the schedule's arithmetic and the bias corrections are not written out beside the calls
    assert "per_epoch" not in code and "1.0 - b1t" not in code and "1.0f - a.beta1" not in code
