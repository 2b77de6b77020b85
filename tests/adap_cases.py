"""The ADAP model, its loss description, context samples and gradient pair against the checker (tests/test_gpu_adap.py), shared
with the other ADAP tests."""
import ctypes as C

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import helpers as H


CTX = {"adap_oc": 3, "adap_small": 3, "adap_multi": 4}


def _adap_struct(nat, cs, n_ctx, n_states, coef, keep, state_idx=None, contexts=None, n_mb=1, sampler="l2", seed=0,
                 want_used=False):
    ad = nat.PhAdapLoss()
    ad.context_size, ad.num_context_samples, ad.num_state_samples = cs, n_ctx, n_states
    ad.sampler, ad.context_loss_coeff, ad.seed = nat.CONTEXT_SAMPLERS[sampler], coef, seed
    if state_idx is not None:
        t = th.as_tensor(np.ascontiguousarray(state_idx, dtype=np.int32)).cuda()
        keep.append(t)
        ad.state_idx = t.data_ptr()
    if contexts is not None:
        t = th.as_tensor(np.ascontiguousarray(contexts, dtype=np.float32)).cuda()
        keep.append(t)
        ad.contexts = t.data_ptr()
    loss = th.zeros(n_mb, device="cuda")
    keep.append(loss)
    ad.context_loss = loss.data_ptr()
    used = None
    if want_used:
        used = (th.full((n_mb, n_states), -1, dtype=th.int32, device="cuda"), th.zeros((n_mb, n_ctx, cs), device="cuda"))
        keep.extend(used)
        ad.used_state_idx, ad.used_contexts = used[0].data_ptr(), used[1].data_ptr()
    return ad, loss, used


def _context_samples(cs, nb, n_ctx, n_states, seed):
    """teacher-forced samples of one minibatch of nb rows: (state positions, -1 past min(n_states, nb); contexts)"""
    rng = np.random.default_rng(seed + nb)
    ns = min(n_states, nb)
    sidx = np.full(n_states, -1, np.int32)
    sidx[:ns] = rng.permutation(nb)[:ns]
    return sidx, orc.adap_sample_contexts("l2", cs, n_ctx, rng.random((n_ctx, cs)))


def _grad_pair(name, T, E, idx, hp, n_ctx, n_states, coef, seed=5, sampler=None, gemm_mode=0, fill=None, prepare=None):
    """device and oracle gradient of one minibatch with the context term; samples teacher-forced unless `sampler`.  fill: another
    buffer builder than helpers.filled_oracle_buffer (a stale buffer: tests/offpolicy_cases.py); idx may be a function (checker,
    buffer) -> rows.  prepare(checker): called on the checker right after it is built, before the buffer and the
    device policy are made (tests/sharp_cases.py sharpens its action head there)"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.ppo import PPO
    cs = CTX[name]
    orac = H.oracle_policy(name, seed=seed)
    if prepare is not None:
        prepare(orac)
    ob = (fill or H.filled_oracle_buffer)(name, orac, T, E, seed=seed)
    if callable(idx):
        idx = idx(orac, ob)
    pol = H.device_policy(name, orac)
    pol.gemm_mode = gemm_mode
    buf = H.make_device_buffer(name, pol, T, E)
    H.upload_buffer(buf, ob)
    nb = len(idx)
    ns = min(n_states, nb)
    keep = []
    if sampler is None:
        sidx, ctxs = _context_samples(cs, nb, n_ctx, n_states, seed)
        ad, loss_t, used = _adap_struct(nat, cs, n_ctx, n_states, coef, keep, sidx[None], ctxs[None])
    else:
        ad, loss_t, used = _adap_struct(nat, cs, n_ctx, n_states, coef, keep, sampler=sampler, seed=seed, want_used=True)
    model = PPO.__new__(PPO)
    for k in ("learning_rate", "clip_range", "clip_range_vf", "ent_coef", "vf_coef", "max_grad_norm", "target_kl",
              "normalize_advantage"):
        setattr(model, k, getattr(hp, k))
    h = PPO.hyper(model)
    idx_t = th.as_tensor(np.asarray(idx, np.int32)).cuda()
    g = th.zeros(pol.layout.P, device="cuda")
    st = th.zeros(nat.PH_NSTAT, device="cuda")
    pol._bind()
    nat.check(pol.ctx.lib.ph_adap_minibatch_grad(pol.ctx.handle, C.byref(pol.spec), pol.params.data_ptr(),
                                                 C.byref(buf.c_struct()), C.byref(h), idx_t.data_ptr(), nb, g.data_ptr(),
                                                 st.data_ptr(), gemm_mode, C.byref(ad)))
    th.cuda.synchronize()
    if sampler is not None:
        sidx, ctxs = used[0][0].cpu().numpy(), used[1][0].cpu().numpy()
    flat = ob.flat()
    mb = {k: th.as_tensor(v[idx]) for k, v in flat.items()}
    orac.optimizer.zero_grad()
    loss, stats_ref = orc.ppo_minibatch_loss(orac, mb, hp)
    cl = orc.adap_context_loss(orac, mb["observations"], cs, sidx[:ns], ctxs)
    (loss + coef * cl).backward()
    stats_ref["context_loss"], stats_ref["loss"] = cl.item(), (loss + coef * cl).item()
    return g.cpu().numpy(), orac.flat_grads(), st.cpu().numpy(), stats_ref, float(loss_t.item()), sidx[:ns], ctxs, pol.layout


def _assert_grads(g, g_ref):
    scale = np.abs(g_ref).max()
    err = np.abs(g - g_ref)
    assert err.max() <= 1e-6 + 2e-4 * scale, (err.max(), scale, int(err.argmax()))


def _adap_model(name, T, E, hp, coef=0.1, n_ctx=5, n_states=32, sampler="l2", seed=0):
    from pantheonrl_amd.adap import ADAP
    from pantheonrl_amd import spaces as sp
    obs_s, act_s = H.CONFIGS[name]
    cs = CTX[name]
    env = type("E", (), dict(observation_space=sp.Box(-np.inf, np.inf, (obs_s.dim - cs,)), action_space=H.to_space(act_s),
                             _is_dummy_space_env=True))()
    return ADAP("AdapPolicy", env, n_steps=T, n_envs=E, batch_size=hp.batch_size, n_epochs=hp.n_epochs,
                learning_rate=hp.learning_rate, clip_range=hp.clip_range, clip_range_vf=hp.clip_range_vf,
                normalize_advantage=hp.normalize_advantage, ent_coef=hp.ent_coef, vf_coef=hp.vf_coef,
                max_grad_norm=hp.max_grad_norm, target_kl=hp.target_kl, seed=seed, context_loss_coeff=coef,
                context_size=cs, num_context_samples=n_ctx, num_state_samples=n_states, context_sampler=sampler)
