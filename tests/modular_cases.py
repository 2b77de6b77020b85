"""The ModularAlgorithm shapes, checker, device model, filled buffers and gradient pair (tests/test_gpu_modular.py), shared with
the sampler, optimizer, off-policy and sharp-policy tests."""
import ctypes as C

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import helpers as H


SHAPES = {"mod_oc": (orc.SpaceSpec("box", dim=62), orc.SpaceSpec("discrete", nvec=(6,))),
          "mod_small": (orc.SpaceSpec("box", dim=6), orc.SpaceSpec("discrete", nvec=(5,))),
          "mod_rps": (orc.SpaceSpec("discrete", nvec=(1,)), orc.SpaceSpec("discrete", nvec=(3,))),
          "mod_md": (orc.SpaceSpec("multidiscrete", nvec=(3, 4, 5)), orc.SpaceSpec("discrete", nvec=(8,)))}


def _oracle(name, K, seed=3, perturb=0.3, **kw):
    th.manual_seed(seed)
    obs_s, act_s = SHAPES[name]
    pol = orc.ModularPolicyOracle(obs_s, act_s, num_partners=K, **kw)
    g = th.Generator().manual_seed(seed + 1)
    with th.no_grad():       # biases and the 0.01-gain heads perturbed so that logits and values are not ~0
        seen = set()
        for p in pol.parameters():
            if id(p) in seen:
                continue
            seen.add(id(p))
            if p.ndim == 1:
                p.add_(perturb * th.randn(p.shape, generator=g))
        for head in [pol.action_net] + [pm["act"] for pm in _unique(pol)]:
            head.weight.add_(perturb * th.randn(head.weight.shape, generator=g))
    return pol


def _unique(pol):
    out, seen = [], set()
    for pm in pol.partners:
        if id(pm) not in seen:
            seen.add(id(pm))
            out.append(pm)
    return out


def _flat(pol, grads=False):
    """the device's parameter order: main network, then every DISTINCT module (baseline shares one)"""
    def vec(t, transpose):
        x = (t.grad if grads else t.detach())
        if x is None:
            x = th.zeros_like(t)
        return (x.t() if transpose else x).contiguous().reshape(-1)
    out = []
    for seq in (pol.policy_net, pol.value_net_mlp):
        for i in (0, 2):
            out += [vec(seq[i].weight, True), vec(seq[i].bias, False)]
    out += [vec(pol.action_net.weight, True), vec(pol.action_net.bias, False), vec(pol.value_net.weight, False),
            vec(pol.value_net.bias, False)]
    for pm in _unique(pol):
        for seq in (pm["pi"], pm["vf"]):
            for i in (0, 2):
                out += [vec(seq[i].weight, True), vec(seq[i].bias, False)]
        out += [vec(pm["act"].weight, True), vec(pm["act"].bias, False), vec(pm["val"].weight, False), vec(pm["val"].bias, False)]
    return th.cat(out).numpy().astype(np.float32).copy()


def _flat_adam_state(pol):
    """(m, v, steps) of the checker's Adam in _flat's order (helpers.flat_adam_state)"""
    return H.flat_adam_state(pol, flat_fn=_flat)


def _load_flat_adam_state(pol, m, v, steps):
    H.load_flat_adam_state(pol, m, v, steps, flat_fn=_flat)


def _value_side(pol):
    """per entry of _flat's order: j for the value side (value tower + value head) of distinct module j -- the parameters that
    join the optimizer when that module's partner is first trained and count their own steps -- and -1 for everything else"""
    params, idx = H._flat_layout(pol, _flat)
    owner = {}
    for j, pm in enumerate(_unique(pol)):
        for p in list(pm["vf"].parameters()) + list(pm["val"].parameters()):
            owner[id(p)] = j
    label = np.concatenate([np.full(p.numel(), owner.get(id(p), -1), np.int64) for p in params])
    return label[idx]


def _device(name, orac, K, **kw):
    from pantheonrl_amd.modular import ModularPolicy
    obs_s, act_s = SHAPES[name]
    pol = ModularPolicy(H.to_space(obs_s), H.to_space(act_s), device="cuda", seed=0, num_partners=K, **kw)
    flat = _flat(orac)
    assert flat.size == pol.P_total, (flat.size, pol.P_total)
    pol.set_flat_params(flat)
    return pol


def _filled(orac, name, partner, T, E, seed=0):
    rng = np.random.default_rng(seed)
    obs_s, act_s = SHAPES[name]
    buf = orc.RolloutBufferOracle(T, E, obs_s.stored_len, 1)
    es = np.ones(E, np.float32)
    for _ in range(T):
        obs = H.sample_obs(obs_s, E, rng)
        with th.no_grad():
            a, v, lp = orac.forward(th.as_tensor(obs), partner_idx=partner, uniforms=th.as_tensor(rng.random((E, 1)).astype(np.float32)))
        buf.add(obs, a.numpy().astype(np.float32), rng.standard_normal(E).astype(np.float32), es, v.flatten(), lp)
        es = (rng.random(E) < 0.1).astype(np.float32)
    buf.compute_returns_and_advantage(rng.standard_normal(E).astype(np.float32), es)
    return buf


def _device_buffer(pol, name, ob):
    from pantheonrl_amd.ppo import RolloutBuffer
    obs_s, act_s = SHAPES[name]
    buf = RolloutBuffer(ob.T, H.to_space(obs_s), H.to_space(act_s), pol.device, pol.ctx, pol.spec, n_envs=ob.E)
    H.upload_buffer(buf, ob)
    return buf


def _grad_pair(name, K, partner, T, E, nb, coef, hp, kw=None, seed=5, gemm_mode=0, fill=None, idx=None, prepare=None):
    """fill: another buffer builder (name, checker, T, E, seed=) than _filled (a stale buffer: tests/offpolicy_cases.py); idx: the
    minibatch rows, or a function (checker, buffer) -> rows, instead of the first nb of a seeded permutation.  prepare(checker): called on the checker right after it is built, before the buffer and the
    device policy are made (tests/sharp_cases.py sharpens its action head there)"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.modular import ModularAlgorithm  # noqa: F401  (import check)
    kw = kw or {}
    orac = _oracle(name, K, seed=seed, **kw)
    if prepare is not None:
        prepare(orac)
    ob = fill(name, orac, T, E, seed=seed) if fill is not None else _filled(orac, name, partner, T, E, seed=seed)
    pol = _device(name, orac, K, **kw)
    pol.gemm_mode = gemm_mode
    buf = _device_buffer(pol, name, ob)
    if idx is None:
        idx = np.random.default_rng(nb).permutation(T * E)[:nb]
    elif callable(idx):
        idx = idx(orac, ob)
    idx = np.asarray(idx)
    nb = len(idx)
    mb = ob.minibatch(idx) if hasattr(ob, "minibatch") else next(iter(ob.get(nb, idx)))
    for p in orac.parameters():
        p.grad = None
    loss, st_ref = orc.modular_minibatch_loss(orac, mb, hp, partner, coef)
    loss.backward()
    g_ref = _flat(orac, grads=True)
    hpc = nat.PhPpoHyper()
    hpc.learning_rate, hpc.clip_range = hp.learning_rate, hp.clip_range
    hpc.clip_range_vf = -1.0 if hp.clip_range_vf is None else hp.clip_range_vf
    hpc.ent_coef, hpc.vf_coef, hpc.max_grad_norm, hpc.target_kl = hp.ent_coef, hp.vf_coef, hp.max_grad_norm, -1.0
    hpc.normalize_advantage, hpc.adam_beta1, hpc.adam_beta2, hpc.adam_eps = 1, 0.9, 0.999, 1e-5
    grad = th.zeros(pol.P_total, device="cuda")
    stats = th.zeros(nat.PH_NSTAT, device="cuda")
    idx_t = th.as_tensor(idx.astype(np.int32)).cuda()
    pol._bind()
    nat.check(pol.ctx.lib.ph_modular_minibatch_grad(pol.ctx.handle, C.byref(pol.spec), C.byref(pol.mod), pol.params.data_ptr(),
                                                    partner, C.byref(buf.c_struct()), C.byref(hpc), idx_t.data_ptr(), nb,
                                                    float(coef), grad.data_ptr(), stats.data_ptr(), gemm_mode))
    th.cuda.synchronize()
    return grad.cpu().numpy(), g_ref, stats.cpu().numpy(), st_ref, pol


def _algo(name, K, T, E, hp, coef, kw=None, seed=0):
    from pantheonrl_amd.modular import ModularAlgorithm
    obs_s, act_s = SHAPES[name]
    env = type("E", (), dict(observation_space=H.to_space(obs_s), action_space=H.to_space(act_s), _is_dummy_space_env=True))()
    return ModularAlgorithm("ModularPolicy", env, n_steps=T, n_envs=E, batch_size=hp.batch_size, n_epochs=hp.n_epochs,
                            learning_rate=hp.learning_rate, clip_range=hp.clip_range, clip_range_vf=hp.clip_range_vf,
                            ent_coef=hp.ent_coef, vf_coef=hp.vf_coef, max_grad_norm=hp.max_grad_norm, target_kl=hp.target_kl,
                            seed=seed, marginal_reg_coef=coef, policy_kwargs=dict(num_partners=K, **(kw or {})))
