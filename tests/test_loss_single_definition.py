"""The PPO row loss is defined in pantheonrl_amd/csrc/ph_ppo_loss.h: the torch.min / clamp backward gate of the clipped surrogate (the
comparison of pl1 with pl2) and the clip_range_vf clamp (fminf(fmaxf(dlt, ...) stand there once each and in no other .hip or .h file
under csrc -- with ONE exception, below.  A kernel that writes either out again is a second copy to keep in step
(tests/offpolicy_cases.py has one case per caller, tests/test_offpolicy_checks.py the ways a copy goes wrong).

The check is textual: it finds a pasted copy, which keeps the names pl1 / pl2 / dlt; it does not find a copy rewritten under other
names."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pantheonrl_amd", "csrc")
HEADER = "ph_ppo_loss.h"
# The one written-out copy of the gate that stays: the policy tail of ppo_grad_split_oh_kernel.  Calling ppo_policy_row there changed
# the VGPR count of five of that kernel's instantiations (by 1-2 out of 384-432) and no statement order restored it, so the site
# keeps its own body (comment at the site).  Its value tail calls the header, so the clamp has no exception.
GATE_EXCEPTION = "ph_ppo_split_oh.hip"
GATE = re.compile(r"pl1\s*(<=|>=|<|>|==|!=)\s*(\w+\.)?pl2|pl2\s*(<=|>=|<|>|==|!=)\s*(\w+\.)?pl1")     # pl1 < pl2, o.pl1 > o.pl2, ...
CLAMP = re.compile(r"fminf\s*\(\s*fmaxf\s*\(\s*dlt")


def _code(path):
    """the file without its // comments"""
    return "\n".join(line.split("//")[0] for line in open(path).read().splitlines())


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert os.path.join(CSRC, HEADER) in files and len(files) > 20
    return files


def test_policy_gate_and_value_clamp_stand_in_the_loss_header_alone():
    gate, clamp = {}, {}
    for path in _sources():
        code = _code(path)
        name = os.path.basename(path)
        if GATE.search(code):
            gate[name] = [m.group(0) for m in GATE.finditer(code)]
        if CLAMP.search(code):
            clamp[name] = len(CLAMP.findall(code))
    assert sorted(gate) == sorted([HEADER, GATE_EXCEPTION]), gate
    # one gate expression each: the two comparisons of `(pl1 < pl2) ? 1 : ((pl1 > pl2) ? inr : tie)`
    assert len(gate[HEADER]) == 2 and len(gate[GATE_EXCEPTION]) == 2, gate
    assert clamp == {HEADER: 1}, clamp


def test_every_gradient_kernel_file_calls_the_header():
    for name in ("ph_ppo.hip", "ph_ppo_fast.hip", "ph_ppo_split.hip", "ph_ppo_split_oh.hip", "ph_arch.hip", "ph_modular.hip",
                 "ph_adapmult.hip"):
        code = _code(os.path.join(CSRC, name))
        assert '#include "%s"' % HEADER in code, name
        if name != GATE_EXCEPTION:
            assert re.search(r"\bppo_policy_row\(|\bppo_two_pass_row\(", code), name
        assert re.search(r"\bppo_value_row\(", code), name
