"""The vectorised Liar's Dice step -- after_ego / after_reply / after_opening -- is written once, in pantheonrl_amd/csrc/ph_liar_step.h,
and instantiated for self-play, the partner pool and cross-play (ph_envs.hip).  A file that deals or plays a move itself is a second
copy of the step to keep bitwise in step by hand: `liar_deal(` is called in the shared step header, in ph_envs.hip (liar_reset_kernel)
and in ph_liar.h (its definition) only; ph_pool.hip and ph_xplay.hip call neither `liar_move(` nor `liar_deal(`; and the C ABI
validates the game block of all three step descriptions in one place, so its alignment message stands once in ph_abi.hip.

The check is textual (comments stripped): it finds a pasted copy of the step, which keeps these names; it does not find a copy
rewritten under other names."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pantheonrl_amd", "csrc")
STEP_HEADER = "ph_liar_step.h"
DEAL = re.compile(r"\bliar_deal\s*\(")
MOVE = re.compile(r"\bliar_move\s*\(")
ALIGNMENT = "hands/history must be 16-byte aligned"


def _code(path):
    """the file without its // comments"""
    return "\n".join(line.split("//")[0] for line in open(path).read().splitlines())


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert os.path.join(CSRC, STEP_HEADER) in files and len(files) > 20
    return files


def test_tables_are_dealt_by_the_shared_step_the_reset_kernel_and_nothing_else():
    deals = {}
    for path in _sources():
        n = len(DEAL.findall(_code(path)))
        if n:
            deals[os.path.basename(path)] = n
    # the step's one re-deal; liar_reset_kernel's; the definition
    assert deals == {STEP_HEADER: 1, "ph_envs.hip": 1, "ph_liar.h": 1}, deals


def test_pool_and_crossplay_files_hold_no_step_of_their_own():
    for name in ("ph_pool.hip", "ph_xplay.hip", "ph_pool.h", "ph_xplay.h"):
        code = _code(os.path.join(CSRC, name))
        assert not MOVE.search(code) and not DEAL.search(code), name
    step = _code(os.path.join(CSRC, STEP_HEADER))
    assert len(MOVE.findall(step)) == 3      # the ego's move, the reply, the opening


def test_the_game_block_of_every_step_description_is_validated_in_one_place():
    code = _code(os.path.join(CSRC, "ph_abi.hip"))
    assert code.count(ALIGNMENT) == 1
    assert len(re.findall(r"\bint check_liar_game\s*\(", code)) == 1
    # self-play (step, step_arch and rollout through check_liar_selfplay), the pool and cross-play
    assert len(re.findall(r"\bcheck_liar_game\s*\(", code)) == 4
    for entry in ("ph_liar_pool_step", "ph_liar_xplay_step", "liar_selfplay_step_run"):
        body = code[code.index("int " + entry + "("):]
        body = body[:body.index("\n}\n")]
        assert "liar_step_run(" in body and "launch_liar_pass" not in body, entry
    assert code.count("launch_liar_pass(") == 3     # the one runner's three passes
