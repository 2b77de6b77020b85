"""A member kind of the device-resident Liar's Dice drivers is an entry in a table, not a fifth copy of a call: in
pantheonrl_amd/envs/vec.py and envs/crossplay.py together the `ph_liar_pool_step` family is called from one place and the
`ph_liar_xplay_step` family from one place (the widest entry point, handed None for the arrays nobody needs); the members' code
names `ph_policy_forward(` at most once and the tower forwards not at all -- the policy answers which entry point serves its network
(ppo.py: `_native_forward`, `_native_forward_ragged`, `_native_scripted`); and the helpers tests share live in `tests/*_cases.py`
and the like, never in another test module.

The checks are textual: they find a pasted call, which keeps these names; they do not find one reached under another name."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = [os.path.join(ROOT, "pantheonrl_amd", "envs", name) for name in ("vec.py", "crossplay.py")]
TEST_IMPORT = re.compile(r"^\s*(?:from\s+tests\.test_\w+\s+import|from\s+tests\s+import\s+.*\btest_\w+|import\s+tests\.test_\w+)", re.M)


def _members_code():
    return "\n".join(open(path).read() for path in MEMBERS)


def test_each_step_family_is_called_from_one_place():
    code = _members_code()
    for family in ("ph_liar_pool_step", "ph_liar_xplay_step"):
        calls = re.findall(r"\." + family + r"\w*\(", code)
        assert len(calls) == 1, (family, calls)


def test_members_reach_the_forwards_through_the_policy():
    code = _members_code()
    assert "ph_arch_forward" not in code                    # (ph_arch_forward_ragged included)
    assert code.count("ph_policy_forward(") <= 1


def test_no_test_file_imports_from_another_test_module():
    offenders = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)):
        found = TEST_IMPORT.findall(open(path).read())
        if found:
            offenders[os.path.relpath(path, ROOT)] = len(found)
    assert not offenders, offenders
