"""The gradient pair and the train pair of the net_arch tower kernels against the checker (tests/test_gpu_arch.py), shared with
the off-policy and sharp-policy tests."""
import ctypes as C

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import arch_oracle as A
from tests import helpers as H


def _grad_pair(name, arch, T, E, idx, hp, seed=11, gemm_mode=0, fill=None, prepare=None):
    """fill: another buffer builder than helpers.filled_oracle_buffer (a stale buffer: tests/offpolicy_cases.py); idx may be a
    function (checker, buffer) -> rows.  prepare(checker): called on the checker right after it is built, before the buffer and the
    device policy are made (tests/sharp_cases.py sharpens its action head there)"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.ppo import PPO
    orac = A.oracle_policy(name, arch, seed=seed)
    if prepare is not None:
        prepare(orac)
    ob = (fill or H.filled_oracle_buffer)(name, orac, T, E, seed=seed)
    if callable(idx):
        idx = idx(orac, ob)
    pol = A.device_policy(name, orac)
    buf = H.make_device_buffer(name, pol, T, E)
    H.upload_buffer(buf, ob)
    mb = {k: th.as_tensor(v[idx]) for k, v in ob.flat().items()}
    orac.optimizer.zero_grad()
    loss, stats_ref = orc.ppo_minibatch_loss(orac, mb, hp)
    loss.backward()
    g_ref = orac.flat_grads()
    model = PPO.__new__(PPO)
    for k in ("learning_rate", "clip_range", "clip_range_vf", "ent_coef", "vf_coef", "max_grad_norm", "target_kl", "normalize_advantage"):
        setattr(model, k, getattr(hp, k))
    h = PPO.hyper(model)
    idx_t = th.as_tensor(np.asarray(idx, np.int32)).cuda()
    modes = (gemm_mode,) if isinstance(gemm_mode, int) else gemm_mode
    out = []
    for mode in modes:
        g = th.zeros(pol.layout.P, device="cuda")
        st = th.zeros(nat.PH_NSTAT, device="cuda")
        pol._bind()
        nat.check(pol.ctx.lib.ph_arch_minibatch_grad(pol.ctx.handle, C.byref(pol.spec), C.byref(pol.arch), pol.params.data_ptr(),
                                                     C.byref(buf.c_struct()), C.byref(h), idx_t.data_ptr(), len(idx), g.data_ptr(),
                                                     st.data_ptr(), mode))
        th.cuda.synchronize()
        out.append((g.cpu().numpy(), st.cpu().numpy()))
    return out, g_ref, stats_ref


def _model(name, arch, T, E, hp, cls_kwargs=True):
    from pantheonrl_amd.ppo import PPO
    return PPO("MlpPolicy", A.space_env(name), n_steps=T, n_envs=E, batch_size=hp.batch_size, n_epochs=hp.n_epochs,
               learning_rate=hp.learning_rate, clip_range=hp.clip_range, clip_range_vf=hp.clip_range_vf,
               normalize_advantage=hp.normalize_advantage, ent_coef=hp.ent_coef, vf_coef=hp.vf_coef, max_grad_norm=hp.max_grad_norm,
               target_kl=hp.target_kl, seed=0, policy_kwargs=A.kwargs_of(arch) if cls_kwargs else None)


def _train_pair(name, arch, T, E, hp, seed=21, f64=False, fill=None):
    """f64: also the chain on a float64 copy of the checker, its Adam state left in model.checker64_state.  fill: another buffer
    builder than helpers.filled_oracle_buffer (a stale buffer: tests/offpolicy_cases.py)"""
    from pantheonrl_amd.ppo import ArchActorCriticPolicy
    orac = A.oracle_policy(name, arch, seed=seed)
    o64 = H.double_copy(orac)[0] if f64 else None
    ob = (fill or H.filled_oracle_buffer)(name, orac, T, E, seed=seed)
    model = _model(name, arch, T, E, hp)
    assert type(model.policy) is ArchActorCriticPolicy and model.policy.net_arch == tuple(arch)
    model.policy.set_flat_params(orac.flat_params())
    H.upload_buffer(model.rollout_buffer, ob)
    perms = np.stack([np.random.default_rng(seed + ep).permutation(T * E) for ep in range(hp.n_epochs)])
    model.train(perms=perms)
    stats_ref = orc.ppo_train(orac, ob, hp, perms)
    if f64:
        model.checker64_state = H.chain64_state(o64, lambda o: orc.ppo_train(o, ob, hp, perms))
    return model, orac, stats_ref
