"""`policy_kwargs net_arch` towers as members of the device-resident pool and cross-play, checked without a GPU: the three `_arch`
entry points in the header, the library and the ctypes mirror; the member struct's size; the command lines' plans (no device, no
file touched); the README's table of environment switches against the switches the package reads; and hipcc's resource remarks
for pool_tower_kernel (the method of tests/test_arch_vec_resources.py)."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

from pantheonrl_amd import _native as nat
from pantheonrl_amd import crossplay as xcli
from pantheonrl_amd import trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRY_POINTS = ("ph_pool_forward_arch", "ph_liar_pool_step_arch", "ph_liar_xplay_step_arch")

# tower_fwd_kernel<false> (the MFMA instantiation) on the commit before pool_tower_kernel (3f6dbe1), from the command of the
# `remarks` fixture below (hipcc --offload-arch=gfx950 -O3 -std=c++17, -Rpass-analysis=kernel-resource-usage): VGPRs 165, AGPRs 16,
# scratch 0, no spill; this tree's tower_fwd_kernel<false> is the same.  pool_tower_kernel<false> as built: VGPRs 165, AGPRs 16,
# scratch 0, no spill, 2 waves per SIMD.  So the patching costs no vector register as measured -- the member's record and the map
# are wave-uniform and live in scalar registers -- and that is the bound: the forward's own count.
PARENT_TOWER_FWD_VGPRS = 165


def test_the_three_entry_points_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "pantheon_hip.h")).read()
    declared = set(re.findall(r"^int\s*(ph_[a-z_0-9]+)\s*\(", header, flags=re.M))
    lib = nat.load()
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert getattr(lib, name).argtypes == nat.SIGNATURES[name], name
    assert nat.SIGNATURES["ph_pool_forward_arch"][:-1] == nat.SIGNATURES["ph_pool_forward"]
    assert nat.SIGNATURES["ph_pool_forward_arch"][-1] is C.POINTER(C.POINTER(nat.PhArch))
    assert nat.SIGNATURES["ph_liar_xplay_step_arch"] == [C.c_void_p, C.POINTER(nat.PhLiarXplay), C.POINTER(C.POINTER(nat.PhArch)),
                                                         C.c_ulonglong, C.c_int]
    assert re.search(r"#define PH_ABI_VERSION 7\b", header)
    flat = " ".join(header.split())
    assert "adds one launch per grouped forward" in flat        # the launch counts stand beside the entry points


def test_the_member_struct_keeps_its_layout():
    assert C.sizeof(nat.PhPoolMember) == 80
    assert [f[0] for f in nat.PhPoolMember._fields_] == ["kind", "params", "rb", "pos", "boundary", "term", "open", "values", "log_probs",
                                                         "seed"]


TOWER = '{"policy_kwargs": {"net_arch": [{"pi": [128, 128], "vf": [128, 128]}]}}'


def test_pool_plan_takes_tower_configs_and_a_fixed_tower_checkpoint_without_a_device(monkeypatch):
    monkeypatch.setattr(nat, "Context", None)
    monkeypatch.setattr(trainer, "gen_load", None)
    fixed = '{"type": "PPO", "location": "m/tower"}'
    args = trainer.parse_cli(["LiarsDice-v0", "PPO", "PPO", "FIXED", "DEFAULT", "--n-envs", "8", "--ego-config", TOWER, "--alt-config",
                              TOWER, fixed, "{}"])
    plan = trainer.pool_plan(args)
    assert [kind for kind, _ in plan["members"]] == ["PPO", "FIXED", "DEFAULT"] and plan["resample"] == "robin"
    assert plan["members"][0][1]["policy_kwargs"]["net_arch"] == [dict(pi=[128, 128], vf=[128, 128])]
    assert plan["members"][1][1] == {"type": "PPO", "location": "m/tower"}
    assert args.ego_config["policy_kwargs"]["net_arch"] == [dict(pi=[128, 128], vf=[128, 128])]


def test_crossplay_plan_sizes_a_population_with_a_tower_checkpoint_without_a_device_or_a_file(monkeypatch):
    monkeypatch.setattr(nat, "Context", None)
    parse = xcli.build_parser().parse_args
    size = xcli.plan(parse(["LiarsDice-v0", "--agents", "m/tower", "m/plain", "DEFAULT", "--n-envs", "32", "-t", "6"]))
    assert size["n_members"] == 3 and size["n_pairs"] == 9 and size["episodes_per_table"] >= 1
    assert xcli.parse_agent("m/tower") == ("PPO", "m/tower")


def _stub_policies():
    """a net_arch tower policy and a 64-64 one as far as the member classes look at them without a device: class, spec, arch"""
    from pantheonrl_amd.envs.vec import VecLiarsDice
    from pantheonrl_amd.ppo import ActorCriticPolicy, ArchActorCriticPolicy
    from pantheonrl_amd.spaces import make_spec
    spec = make_spec(VecLiarsDice.observation_space, VecLiarsDice.action_space)
    tower = ArchActorCriticPolicy.__new__(ArchActorCriticPolicy)
    tower.spec, tower.arch, tower.net_arch = spec, nat.make_arch([128, 128]), (128, 128)
    plain = ActorCriticPolicy.__new__(ActorCriticPolicy)
    plain.spec = spec
    return tower, plain


def test_load_member_seats_a_tower_only_where_it_is_told_to(monkeypatch):
    from pantheonrl_amd import tester
    from pantheonrl_amd.envs.vec import FrozenVecPartner, TowerFrozenVecPartner
    tower, plain = _stub_policies()
    loaded = {"m/tower": tower, "m/plain": plain}
    monkeypatch.setattr(tester, "gen_load", lambda cfg, kind, location: type("Model", (), dict(policy=loaded[location]))())
    member = tester.load_member("PPO", {}, "m/tower", "cuda", towers=True)
    assert type(member) is TowerFrozenVecPartner and member.policy is tower
    assert type(tester.load_member("PPO", {}, "m/plain", "cuda", towers=True)) is FrozenVecPartner
    assert type(tester.load_member("PPO", {}, "m/plain", "cuda")) is FrozenVecPartner
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):          # the default, and so `tester ... --n-envs`, keeps refusing
        tester.load_member("PPO", {}, "m/tower", "cuda")


def test_the_command_lines_pass_towers_where_the_issue_puts_it(monkeypatch):
    """crossplay seats tower checkpoints, `tester ... --n-envs` does not: what each hands to load_member"""
    import argparse
    from pantheonrl_amd import tester
    calls = []

    class Stop(Exception):
        pass

    def spy(policy_type, config, location, device, towers=False):
        calls.append((location, towers))
        raise Stop
    monkeypatch.setattr(tester, "load_member", spy)
    with pytest.raises(Stop):
        xcli.run(["LiarsDice-v0", "--agents", "m/tower", "DEFAULT", "--n-envs", "8", "-t", "2"])
    with pytest.raises(Stop):
        tester.run_vectorised(argparse.Namespace(n_envs=8, total_episodes=8, ego="PPO", ego_config={}, ego_load="m/tower", alt="DEFAULT",
                                                 alt_config={}, alt_load=None, device="cuda", record=None, seed=0, env_config={}))
    assert calls == [("m/tower", True), ("m/tower", False)]


def test_the_readme_switch_table_names_the_switches_the_package_reads():
    """no new environment switch: every variable the native layer reads, and every variable the Python files of the pool, cross-play
    and their command lines read, has a row in README.md's switch table (the method of tests/test_native_abi.py, any prefix)"""
    section = open(os.path.join(ROOT, "README.md")).read().split("## Switches", 1)[1].split("\n## ", 1)[0]
    listed = set(re.findall(r"[A-Z][A-Z0-9]*_[A-Z0-9_]+", "\n".join(re.findall(r"^\|([^|]*)\|", section, flags=re.M))))
    read = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        read |= set(re.findall(r"getenv\(\s*\"([A-Z][A-Z0-9_]+)\"", open(path).read()))
    assert "PH_FWD16H" in read, "no switch found: the pattern above no longer matches the sources"
    for name in ("envs/vec.py", "envs/crossplay.py", "trainer.py", "tester.py", "crossplay.py"):
        src = open(os.path.join(ROOT, "pantheonrl_amd", name)).read()
        read |= set(re.findall(r"environ(?:\.get\(|\[)\s*\"([A-Z][A-Z0-9_]+)\"", src))
    assert "LIAR_PERSISTENT" in read
    assert read <= listed, sorted(read - listed)


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("res") / "x.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "ph_arch.hip"), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=1800)
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


def test_pool_tower_kernel_costs_no_scratch_and_the_forward_body_plus_the_patching(remarks):
    """the member's ArchDims come from the device-side member table, never from a by-value argument indexed by the member: nothing
    of the kernel's argument block reaches scratch"""
    hit = {n: k for n, k in remarks.items() if "pool_tower_kernelILb0EE" in n}
    assert len(hit) == 1 and not any("pool_tower_kernelILb1EE" in n for n in remarks), sorted(remarks)   # only mode 0 is built
    pool = next(iter(hit.values()))
    fwd = next(k for n, k in remarks.items() if "tower_fwd_kernelILb0EE" in n)
    print("tower_fwd_kernel<false>", fwd, "pool_tower_kernel<false>", pool)
    assert pool["ScratchSize"] == 0 and pool["VGPRs Spill"] == 0 and pool["LDS Size"] == 0, pool
    assert fwd["VGPRs"] <= PARENT_TOWER_FWD_VGPRS, fwd                  # the mapped body left the plain instantiation alone
    assert pool["VGPRs"] <= fwd["VGPRs"], (pool, fwd)
    assert pool["AGPRs"] <= fwd["AGPRs"], (pool, fwd)
