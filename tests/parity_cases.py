"""The gradient pair, the train pair and their comparisons of the 64-wide PPO kernels against the checker
(tests/test_gpu_parity.py), shared with the other policy families' tests."""
import copy

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import helpers as H


def _grad_pair(name, T, E, idx, hp: orc.PPOHyper, seed=11, gemm_mode=0, f64=False, obs_fn=None, w1_scale=1.0, fill=None,
               prepare=None):
    """device minibatch gradient, the oracle's autograd gradient (float32 as the reference computes it; f64: the same graph in
    float64 -- the yardstick for "which float32 path is closer to the true gradient").  obs_fn: other observation
    distributions than N(0, 1); w1_scale multiplies both first-layer weight matrices (keeps pre-activations in tanh's live range
    when the observations are rescaled).  fill: another buffer builder than helpers.filled_oracle_buffer (a stale buffer:
    tests/offpolicy_cases.py); idx may be a function (checker, buffer) -> rows.  prepare(checker): called on the checker right after it is built, before the buffer and the
    device policy are made (tests/sharp_cases.py sharpens its action head there)"""
    import ctypes as C
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.ppo import PPO
    orac = H.oracle_policy(name, seed=seed)
    if prepare is not None:
        prepare(orac)
    if w1_scale != 1.0:
        with th.no_grad():
            orac.policy_net[0].weight.mul_(w1_scale)
            orac.value_net_mlp[0].weight.mul_(w1_scale)
    ob = (fill or H.filled_oracle_buffer)(name, orac, T, E, seed=seed, obs_fn=obs_fn)
    if callable(idx):
        idx = idx(orac, ob)
    pol = H.device_policy(name, orac)
    pol.gemm_mode = gemm_mode
    buf = H.make_device_buffer(name, pol, T, E)
    H.upload_buffer(buf, ob)
    # oracle gradient
    flat = ob.flat()
    mb = {k: th.as_tensor(v[idx]) for k, v in flat.items()}
    orac.optimizer.zero_grad()
    loss, stats_ref = orc.ppo_minibatch_loss(orac, mb, hp)
    loss.backward()
    g_ref = orac.flat_grads()
    if f64:
        o64 = copy.deepcopy(orac).double()
        mb64 = {k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
        o64.optimizer = None
        for q in o64.parameters():
            q.grad = None
        # the loss of orc.ppo_minibatch_loss written out on the float64 modules (Box observations, one Discrete head; the
        # oracle's own entry point casts observations to float32)
        lat_pi, lat_vf = o64.policy_net(mb64["observations"]), o64.value_net_mlp(mb64["observations"])
        logp_all = th.log_softmax(o64.action_net(lat_pi), dim=-1)
        act64 = mb64["actions"].long().flatten()
        log_prob = logp_all.gather(1, act64[:, None])[:, 0]
        entropy = -(logp_all.exp() * logp_all).sum(-1)
        values = o64.value_net(lat_vf).flatten()
        adv = mb64["advantages"]
        if hp.normalize_advantage and len(adv) > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = th.exp(log_prob - mb64["old_log_prob"])
        pl = -th.min(adv * ratio, adv * th.clamp(ratio, 1 - hp.clip_range, 1 + hp.clip_range)).mean()
        vp = values if hp.clip_range_vf is None else mb64["old_values"] + th.clamp(values - mb64["old_values"], -hp.clip_range_vf,
                                                                                  hp.clip_range_vf)
        loss64 = pl + hp.ent_coef * (-entropy.mean()) + hp.vf_coef * ((mb64["returns"] - vp) ** 2).mean()
        loss64.backward()
        parts = []
        for seq in (o64.policy_net, o64.value_net_mlp):       # the flat parameter order of MlpPolicyOracle.flat_grads, kept in float64
            for li in (0, 2):
                parts += [seq[li].weight.grad.t().contiguous().reshape(-1), seq[li].bias.grad]
        parts += [o64.action_net.weight.grad.t().contiguous().reshape(-1), o64.action_net.bias.grad,
                  o64.value_net.weight.grad.reshape(-1), o64.value_net.bias.grad]
        g_ref = th.cat(parts).numpy().copy()
    # device gradient
    model = PPO.__new__(PPO)
    for k in ("learning_rate", "clip_range", "clip_range_vf", "ent_coef", "vf_coef", "max_grad_norm", "target_kl",
              "normalize_advantage"):
        setattr(model, k, getattr(hp, k))
    h = PPO.hyper(model)
    idx_t = th.as_tensor(np.asarray(idx, np.int32)).cuda()
    g = th.zeros(pol.layout.P, device="cuda")
    st = th.zeros(nat.PH_NSTAT, device="cuda")
    pol._bind()
    nat.check(pol.ctx.lib.ph_ppo_minibatch_grad(pol.ctx.handle, C.byref(pol.spec), pol.params.data_ptr(),
                                                C.byref(buf.c_struct()), C.byref(h), idx_t.data_ptr(), len(idx),
                                                g.data_ptr(), st.data_ptr(), gemm_mode))
    th.cuda.synchronize()
    return g.cpu().numpy(), g_ref, st.cpu().numpy(), stats_ref, pol.layout


def _assert_grads(g, g_ref, lay):
    scale = np.abs(g_ref).max()
    err = np.abs(g - g_ref)
    assert err.max() <= 1e-6 + 2e-4 * scale, (err.max(), scale, int(err.argmax()), lay.P)


def _train_pair(name, T, E, hp: orc.PPOHyper, seed=21, device_perms=False, f64=False, fill=None, exclusive=None):
    """f64: also run the chain on a float64 copy of the checker (same buffer, same permutations) and leave its Adam state in
    model.checker64_state -- the yardstick of helpers.assert_chain_moments.  fill: another buffer builder than
    helpers.filled_oracle_buffer (a stale buffer: tests/offpolicy_cases.py); exclusive: set_exclusive_device before training"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.ppo import PPO
    orac = H.oracle_policy(name, seed=seed)
    o64 = H.double_copy(orac)[0] if f64 else None
    ob = (fill or H.filled_oracle_buffer)(name, orac, T, E, seed=seed)
    obs_s, act_s = H.CONFIGS[name]
    env = type("E", (), dict(observation_space=H.to_space(obs_s), action_space=H.to_space(act_s),
                             _is_dummy_space_env=True))()
    model = PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=hp.batch_size, n_epochs=hp.n_epochs,
                learning_rate=hp.learning_rate, clip_range=hp.clip_range, clip_range_vf=hp.clip_range_vf,
                normalize_advantage=hp.normalize_advantage, ent_coef=hp.ent_coef, vf_coef=hp.vf_coef,
                max_grad_norm=hp.max_grad_norm, target_kl=hp.target_kl, seed=0)
    if exclusive is not None:
        model.policy.ctx.set_exclusive_device(exclusive)
    model.policy.set_flat_params(orac.flat_params())
    H.upload_buffer(model.rollout_buffer, ob)
    N = T * E
    if device_perms:
        model.device_permutations = True
        perms = np.stack([nat.feistel_indices(N, model.permutation_seed + 1, ep) for ep in range(hp.n_epochs)])
        model.train()
    else:
        perms = np.stack([np.random.default_rng(seed + ep).permutation(N) for ep in range(hp.n_epochs)])
        model.train(perms=perms)
    stats_ref = orc.ppo_train(orac, ob, hp, perms)
    if f64:
        model.checker64_state = H.chain64_state(o64, lambda o: orc.ppo_train(o, ob, hp, perms))
    return model, orac, stats_ref


# Per-statistic tolerances of the train() comparisons (device statistics vs the oracle's, minibatch by minibatch).  The loss
# terms are means of f32 row terms summed in another order (relative 2e-4, absolute floor 2e-5); approx_kl = mean((ratio - 1) -
# log ratio) cancels to ~1e-7 per row, so it gets an absolute 3e-6; clip_fraction is a COUNT / nb -- a row whose ratio sits on
# the clip boundary may fall either way, so one row of slack; grad_norm relative 2e-4.
def _assert_train_stats(row, ref, nb, where=()):
    tol = {"policy_loss": lambda x: 2e-5 + 2e-4 * abs(x), "value_loss": lambda x: 2e-5 + 2e-4 * abs(x),
           "entropy_loss": lambda x: 2e-5 + 2e-4 * abs(x), "loss": lambda x: 3e-5 + 2e-4 * abs(x),
           "approx_kl": lambda x: 3e-6 + 2e-4 * abs(x), "clip_fraction": lambda x: 1.0 / nb + 1e-7,
           "grad_norm": lambda x: 1e-5 + 2e-4 * abs(x)}
    for j, k in enumerate(("policy_loss", "value_loss", "entropy_loss", "clip_fraction", "approx_kl", "loss", "grad_norm")):
        assert abs(row[j] - ref[k]) <= tol[k](ref[k]), (where, k, row[j], ref[k])
