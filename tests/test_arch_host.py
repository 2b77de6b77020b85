"""not-gpu: `policy_kwargs net_arch` -- what is accepted and refused, the parameter layout of towers of a run-time shape
(ph_arch_layout_of), the checker of the GPU tests anchored to the 64-wide one, and the tower kernels' registers and LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch as th

from oracle import sb3_oracle as orc
from pantheonrl_amd import _native as nat
from pantheonrl_amd import spaces as sp
from tests import helpers as H
from tests.arch_oracle import ARCHES, SPECS, ArchPolicyOracle, arch_id, param_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pantheonrl_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _spec(name):
    obs_s, act_s = H.CONFIGS[name]
    return sp.make_spec(H.to_space(obs_s), H.to_space(act_s, "act"))


def test_check_policy_kwargs_accepts_the_arch_matrix_and_refuses_the_rest():
    from pantheonrl_amd.ppo import PPO, UnsupportedPolicyConfig, check_policy_kwargs
    for a in ARCHES:
        want = {} if a == (64, 64) else {"net_arch": a}
        assert check_policy_kwargs({"net_arch": [dict(pi=list(a), vf=list(a))]}) == want
        assert check_policy_kwargs({"net_arch": dict(vf=list(a), pi=list(a))}) == want
        assert check_policy_kwargs({"net_arch": [dict(pi=tuple(a), vf=list(a))], "ortho_init": False}) == dict(want, ortho_init=False)
    bad = [[32, 32], [64, dict(pi=[64], vf=[64])], [dict(pi=[128, 128], vf=[128])], [dict(pi=[128], vf=[64])],
           [dict(pi=[], vf=[])], dict(pi=[], vf=[64]), [dict(pi=[64] * 4, vf=[64] * 4)], [dict(pi=[48], vf=[48])],
           [dict(pi=[16], vf=[16])], [dict(pi=[288], vf=[288])], [dict(pi=[0], vf=[0])], [dict(pi=[64.0, 64.0], vf=[64.0, 64.0])],
           [dict(pi=["64"], vf=["64"])], [dict(pi=[128, 128])], [dict(pi=[128], vf=[128], qf=[128])], [], None, "auto", 64,
           [dict(pi=128, vf=128)], [dict(pi=[True], vf=[True])]]
    env = type("E", (), dict(observation_space=sp.Discrete(1), action_space=sp.Discrete(3)))()
    for arch in bad:
        with pytest.raises(UnsupportedPolicyConfig, match="net_arch"):
            check_policy_kwargs({"net_arch": arch})
        with pytest.raises(UnsupportedPolicyConfig, match="net_arch"):       # before any device is touched
            PPO("MlpPolicy", env, policy_kwargs={"net_arch": arch}, device="cpu")
    with pytest.raises(UnsupportedPolicyConfig, match="activation_fn"):
        check_policy_kwargs({"net_arch": [dict(pi=[128], vf=[128])], "activation_fn": th.nn.ReLU})
    # a non-default arch with a Box action space, and on the algorithms with networks of their own: refused by name
    box_env = type("E", (), dict(observation_space=sp.Box(-1, 1, (4,)), action_space=sp.Box(-1, 1, (2,))))()
    with pytest.raises(UnsupportedPolicyConfig, match="net_arch"):
        PPO("MlpPolicy", box_env, policy_kwargs={"net_arch": [dict(pi=[128], vf=[128])]}, device="cpu")
    from pantheonrl_amd import ADAP
    with pytest.raises(UnsupportedPolicyConfig, match="net_arch"):
        ADAP("AdapPolicy", env, policy_kwargs={"net_arch": [dict(pi=[128], vf=[128])]}, device="cpu")


@pytest.mark.parametrize("obs,act,arch,P", [
    (sp.Discrete(1), sp.Discrete(3), (32,), 260),                                                          # RPS
    (sp.Box(-np.inf, np.inf, (62,)), sp.Discrete(6), (128, 128), 50055),                                   # Overcooked
    (sp.Box(-np.inf, np.inf, (48,)), sp.Discrete(5), (64, 64, 64), 23302),                                 # MPE N=8
    (sp.MultiDiscrete([7] * 6 + [7, 12] * 12), sp.MultiDiscrete([7, 12]), (256, 128), 207124),             # Liar's Dice
])
def test_arch_layout_parameter_counts(obs, act, arch, P):
    lay = nat.arch_layout_of(sp.make_spec(obs, act), nat.make_arch(arch))
    assert lay.P == P == param_count(lay.F, lay.L, arch)


@pytest.mark.parametrize("name", SPECS)
def test_arch_layout_is_contiguous_in_the_stated_order_and_equals_ph_layout_at_64_64(name):
    spec = _spec(name)
    base = nat.layout_of(spec)
    for a in ARCHES:
        lay = nat.arch_layout_of(spec, nat.make_arch(a))
        assert (lay.D, lay.F, lay.A, lay.L) == (base.D, base.F, base.A, base.L)
        assert lay.P == param_count(base.F, base.L, a)
        off = 0
        for oW, ob in ((lay.pi_W, lay.pi_b), (lay.vf_W, lay.vf_b)):
            fin = base.F
            for l, w in enumerate(a):
                assert oW[l] == off
                off += fin * w
                assert ob[l] == off
                off += w
                fin = w
        assert lay.act_W == off and lay.act_b == off + a[-1] * base.L and lay.val_W == lay.act_b + base.L
        assert lay.val_b == lay.val_W + a[-1] == lay.P - 1
    lay = nat.arch_layout_of(spec, nat.make_arch((64, 64)))
    got = dict(D=lay.D, F=lay.F, A=lay.A, L=lay.L, P=lay.P, pi_W1=lay.pi_W[0], pi_b1=lay.pi_b[0], pi_W2=lay.pi_W[1],
               pi_b2=lay.pi_b[1], vf_W1=lay.vf_W[0], vf_b1=lay.vf_b[0], vf_W2=lay.vf_W[1], vf_b2=lay.vf_b[1], act_W=lay.act_W,
               act_b=lay.act_b, val_W=lay.val_W, val_b=lay.val_b)
    for k, _ in nat.PhLayout._fields_:
        assert got[k] == getattr(base, k), k


def test_a_spec_too_large_for_the_lds_tile_is_refused_by_name():
    """one-hot observations keep R x D hot positions in LDS: 256 components beside three 256-wide layers do not fit even at 32 rows;
    ph_arch_lds_bytes reports the figure, the device entry points refuse it with a message (GPU test)"""
    spec = sp.make_spec(sp.MultiDiscrete([2] * 256), sp.Discrete(3))
    g, rows, f = nat.arch_lds_bytes(spec, nat.make_arch((256, 256, 256)))
    assert rows == 32 and g == f > 160 * 1024


def test_bad_arches_give_an_error_string():
    spec = _spec("overcooked")
    for widths, word in (((), "n_layers"), ((64, 64, 64, 64), "n_layers"), ((48,), "width 48"), ((288,), "width 288"),
                         ((64, 0), "width 0"), ((16,), "width 16"), ((-32,), "width -32")):
        arch = nat.make_arch(widths)
        arch.n_layers = len(widths)
        with pytest.raises(nat.NativeError, match=word):
            nat.arch_layout_of(spec, arch)
    box = sp.make_spec(sp.Box(-1, 1, (3,)), sp.Box(-1, 1, (2,)))
    with pytest.raises(nat.NativeError, match="categorical"):
        nat.arch_layout_of(box, nat.make_arch((128,)))
    assert nat.load().ph_arch_layout_of(C.byref(spec), None, None) != 0


@pytest.mark.parametrize("name", ["overcooked", "liar", "wide", "rps"])
def test_the_checker_at_64_64_is_the_64_wide_checker_bit_for_bit(name):
    base = H.oracle_policy(name, seed=2)
    obs_s, act_s = H.CONFIGS[name]
    th.manual_seed(9)
    mine = ArchPolicyOracle(obs_s, act_s, (64, 64))
    mine.load_flat_params(base.flat_params())
    assert np.array_equal(mine.flat_params(), base.flat_params())
    ob = H.filled_oracle_buffer(name, base, 8, 6, seed=2)
    obs = th.as_tensor(H.sample_obs(obs_s, 77, np.random.default_rng(0)))
    with th.no_grad():
        assert th.equal(mine.logits(obs), base.logits(obs)) and th.equal(mine.predict_values(obs), base.predict_values(obs))
    idx = np.random.default_rng(1).permutation(48)[:40]
    grads = []
    for pol in (base, mine):
        mb = {k: th.as_tensor(v[idx]) for k, v in ob.flat().items()}
        pol.optimizer.zero_grad()
        orc.ppo_minibatch_loss(pol, mb, orc.PPOHyper(ent_coef=0.01))[0].backward()
        grads.append(pol.flat_grads())
    assert np.array_equal(grads[0], grads[1])
    for a in ARCHES:
        assert ArchPolicyOracle(obs_s, act_s, a).flat_params().size == param_count(obs_s.flat_len, act_s.flat_len, a)


def test_policy_class_tensor_table_follows_sb3_names_and_the_layout():
    """ArchActorCriticPolicy._tensors without a device: names, offsets and shapes (what state_dict / load_state_dict walk)."""
    from pantheonrl_amd.ppo import ArchActorCriticPolicy
    pol = ArchActorCriticPolicy.__new__(ArchActorCriticPolicy)
    pol.net_arch = (256, 128, 32)
    pol.layout = nat.arch_layout_of(_spec("liar"), nat.make_arch(pol.net_arch))
    t = pol._tensors()
    assert [x[0] for x in t] == ["mlp_extractor.policy_net.0", "mlp_extractor.policy_net.2", "mlp_extractor.policy_net.4",
                                 "mlp_extractor.value_net.0", "mlp_extractor.value_net.2", "mlp_extractor.value_net.4",
                                 "action_net", "value_net"]
    assert [(x[3], x[4]) for x in t] == [(270, 256), (256, 128), (128, 32)] * 2 + [(32, 19), (32, 1)]
    end = 0
    for _, woff, boff, fin, fout, _ in t:
        assert woff == end and boff == woff + fin * fout
        end = boff + fout
    assert end == pol.layout.P
    assert [x[5] for x in t] == [np.sqrt(2)] * 6 + [0.01, 1.0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tower_kernels_have_no_scratch_and_fit_the_lds(tmp_path):
    out = tmp_path / "x.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "ph_arch.hip"), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|LDS Size \[bytes/block\]):\s+(\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    grad = {n: k for n, k in kernels.items() if "tower_grad_kernel" in n}
    fwd = {n: k for n, k in kernels.items() if "tower_fwd_kernel" in n}
    assert len(grad) == 4 and len(fwd) == 2, sorted(kernels)     # R = 64, 32 x MFMA, VALU; forward MFMA, VALU
    static = 0
    for n, k in list(grad.items()) + list(fwd.items()):
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (n, k)
        assert k["VGPRs"] + k.get("AGPRs", 0) <= 512, (n, k)
        if "tower_grad_kernelILi64E" in n:     # 64-row tiles below 80 KiB are planned two workgroups (eight waves) per CU: 256 a wave
            assert k["VGPRs"] + k.get("AGPRs", 0) <= 256, (n, k)
        static = max(static, k["LDS Size"])
    # static + requested dynamic LDS of every arch x spec of the matrix: at most the CU's 160 KiB, 64-row tiles where they fit
    for name in SPECS:
        for a in ARCHES:
            g, rows, f = nat.arch_lds_bytes(_spec(name), nat.make_arch(a))
            assert static + g <= 160 * 1024 and static + f <= 160 * 1024, (name, a, g, f)
            assert rows in (32, 64), (name, a, rows)
    g, rows, _ = nat.arch_lds_bytes(_spec("overcooked"), nat.make_arch((64, 64)))
    assert rows == 64 and 2 * (static + g) <= 160 * 1024, g     # two workgroups per CU at the default shape, as ppo_grad_kernel
    assert nat.arch_lds_bytes(_spec("liar"), nat.make_arch((256, 256, 256)))[1] == 32
    for n in list(grad) + list(fwd):                              # names of their own: the 64-wide units' instantiation counts stay
        assert not any(w in n for w in ("ppo_grad_kernel", "ppo_grad_split", "policy_fwd16")), n
    assert [arch_id(a) for a in ARCHES][-1] == "64x64"
