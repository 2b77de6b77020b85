"""Shared test plumbing: matched (oracle, device) policy pairs and synthetic rollouts.  The oracle is the checker."""
from __future__ import annotations

import numpy as np
import torch as th

from oracle.sb3_oracle import GaussianMlpPolicyOracle, MlpPolicyOracle, PPOHyper, RolloutBufferOracle, SpaceSpec

# BASELINE.json configs: name -> (obs SpaceSpec, act SpaceSpec)
CONFIGS = {
    "rps": (SpaceSpec("discrete", nvec=(1,)), SpaceSpec("discrete", nvec=(3,))),
    "liar": (SpaceSpec("multidiscrete", nvec=tuple([7] * 6 + [7, 12] * 12)), SpaceSpec("multidiscrete", nvec=(7, 12))),
    "overcooked": (SpaceSpec("box", dim=62), SpaceSpec("discrete", nvec=(6,))),
    "mpe8": (SpaceSpec("box", dim=48), SpaceSpec("discrete", nvec=(5,))),
    "wide": (SpaceSpec("box", dim=130), SpaceSpec("multidiscrete", nvec=(3, 30, 7))),  # 3 feature chunks, Lp=64
    # one-hot observations with heads the 8-logit fast path does not take (policy_fwd16h_kernel): three action components
    # filling all 32 logit lanes (the middle one straddles the 16-lane DPP row boundary); one 20-way Discrete head
    "onehot32": (SpaceSpec("multidiscrete", nvec=(3, 4, 5, 2, 6)), SpaceSpec("multidiscrete", nvec=(5, 16, 11))),
    "discrete20": (SpaceSpec("discrete", nvec=(5,)), SpaceSpec("discrete", nvec=(20,))),
    # every instantiation of the general gradient kernel (observation kind x head class x logit padding): four 16-way action
    # components = 64 logits through the per-component head phase; one-hot observations of exactly two 64-feature chunks with
    # a 20-way head (one lane per row); a 17-way component (too wide for the per-component phase) beside a small one
    "quad16": (SpaceSpec("box", dim=20), SpaceSpec("multidiscrete", nvec=(16, 16, 16, 16))),
    "onehot128": (SpaceSpec("multidiscrete", nvec=(32, 32, 32, 32)), SpaceSpec("discrete", nvec=(20,))),
    "onehot17": (SpaceSpec("multidiscrete", nvec=(9, 40, 30)), SpaceSpec("multidiscrete", nvec=(17, 3))),
    # ADAP: the stored observation is (environment observation ++ context) -- adap_learn.py:448-452
    "adap_oc": (SpaceSpec("box", dim=62 + 3), SpaceSpec("discrete", nvec=(6,))),            # two feature chunks
    "adap_small": (SpaceSpec("box", dim=35 + 3), SpaceSpec("discrete", nvec=(5,))),         # the 64-row fast gradient kernel
    "adap_multi": (SpaceSpec("box", dim=20 + 4), SpaceSpec("multidiscrete", nvec=(3, 9, 4))),
    # corners of the split gradient kernel's shape class: one feature; all 64 features (no free column for the folded bias) with
    # all 8 logits; 63 features (the bias column is the last free one) with a 2-logit head
    "box1": (SpaceSpec("box", dim=1), SpaceSpec("discrete", nvec=(2,))),
    "box64": (SpaceSpec("box", dim=64), SpaceSpec("discrete", nvec=(8,))),
    "box63": (SpaceSpec("box", dim=63), SpaceSpec("discrete", nvec=(2,))),
    # Box observations of three and four feature chunks with heads inside the wide split kernel's class (<= 32 logits)
    "box130": (SpaceSpec("box", dim=130), SpaceSpec("multidiscrete", nvec=(5, 16, 11))),
    "box200": (SpaceSpec("box", dim=200), SpaceSpec("discrete", nvec=(20,))),
    # Box (continuous) action spaces: SB3's DiagGaussian head on the general kernels -- one dimension on the shape the categorical
    # fast kernels would take, MPE's continuous 5-vector, two feature chunks, one-hot observations, the widest head (16)
    "gauss1": (SpaceSpec("box", dim=62), SpaceSpec("box", dim=1)),
    "gauss5": (SpaceSpec("box", dim=48), SpaceSpec("box", dim=5)),
    "gauss_wide": (SpaceSpec("box", dim=70), SpaceSpec("box", dim=3)),
    "gauss_onehot": (SpaceSpec("multidiscrete", nvec=(3, 4, 5, 2, 6)), SpaceSpec("box", dim=2)),
    "gauss16": (SpaceSpec("box", dim=8), SpaceSpec("box", dim=16)),
}


def to_space(spec: SpaceSpec, role: str = "obs"):
    from pantheonrl_amd import spaces as sp
    if spec.kind == "box":
        return sp.Box(-np.inf, np.inf, (spec.dim,)) if role == "obs" else sp.Box(-1.0, 1.0, (spec.dim,))
    if spec.kind == "discrete":
        return sp.Discrete(spec.nvec[0])
    return sp.MultiDiscrete(list(spec.nvec))


def sample_obs(spec: SpaceSpec, n: int, rng: np.random.Generator) -> np.ndarray:
    if spec.kind == "box":
        return rng.standard_normal((n, spec.dim)).astype(np.float32)
    return np.stack([rng.integers(0, k, size=n) for k in spec.nvec], axis=1).astype(np.float32)


def oracle_policy(name: str, seed: int = 0, perturb: float = 0.3) -> MlpPolicyOracle:
    """seeded oracle policy; biases and the 0.01-gain action head are perturbed so logits are not ~uniform."""
    th.manual_seed(seed)
    obs_s, act_s = CONFIGS[name]
    pol = (GaussianMlpPolicyOracle if act_s.kind == "box" else MlpPolicyOracle)(obs_s, act_s)
    g = th.Generator().manual_seed(seed + 1)
    with th.no_grad():
        for p in pol.parameters():
            if p.ndim == 1:
                p.add_(perturb * th.randn(p.shape, generator=g))
        pol.action_net.weight.add_(perturb * th.randn(pol.action_net.weight.shape, generator=g))
    return pol


def device_policy(name: str, oracle: MlpPolicyOracle):
    from pantheonrl_amd.ppo import ActorCriticPolicy, GaussianActorCriticPolicy
    obs_s, act_s = CONFIGS[name]
    cls = GaussianActorCriticPolicy if act_s.kind == "box" else ActorCriticPolicy
    pol = cls(to_space(obs_s), to_space(act_s, "act"), device="cuda", seed=0)
    pol.set_flat_params(oracle.flat_params())
    return pol


def filled_oracle_buffer(name: str, oracle: MlpPolicyOracle, T: int, E: int, seed: int = 0,
                         p_done: float = 0.05, obs_fn=None) -> RolloutBufferOracle:
    """a full rollout buffer produced by the oracle policy on synthetic inputs (SURVEY.md 8d generators).
    obs_fn(obs, rng) -> obs replaces the N(0, 1) Box observations (integer-valued / rescaled features)."""
    rng = np.random.default_rng(seed)
    obs_s, act_s = CONFIGS[name]
    buf = RolloutBufferOracle(T, E, obs_s.stored_len, act_s.stored_len)
    starts = np.ones(E, np.float32)
    values = None
    for _ in range(T):
        obs = sample_obs(obs_s, E, rng)
        if obs_fn is not None:
            obs = np.ascontiguousarray(obs_fn(obs, rng), dtype=np.float32)
        with th.no_grad():
            actions, values, logp = oracle.forward(th.as_tensor(obs))
        buf.add(obs, actions.numpy(), rng.standard_normal(E).astype(np.float32), starts, values, logp)
        starts = (rng.random(E) < p_done).astype(np.float32)
    buf.compute_returns_and_advantage(values, starts)
    return buf


def stale_oracle_buffer(name: str, oracle, T: int, E: int, seed: int = 0, drift: float = 0.03, fill=None):
    """a rollout buffer the policy under test did NOT fill: a deep copy of the checker with drift * N(0, 1) (seeded) added to every
    parameter is the behaviour policy and fills the buffer through `fill(name, behaviour, T, E, seed=seed)` (filled_oracle_buffer
    unless given); `oracle` itself is left as it was.  Against this buffer the checker's ratios leave 1 and its values leave the
    stored ones, so both clips of the PPO loss are live (tests/offpolicy_cases.py)."""
    import copy
    beh = copy.deepcopy(oracle)
    g = th.Generator().manual_seed(seed + 7919)
    with th.no_grad():
        for p in beh.parameters():
            p.add_(drift * th.randn(p.shape, generator=g))
    with th.random.fork_rng(devices=[]):       # the checker samples from torch's global stream: the same buffer on every call
        th.manual_seed(seed)
        return (fill or filled_oracle_buffer)(name, beh, T, E, seed=seed)


OFFPOLICY_CLASSES = ("P1", "P2", "P3", "P4", "P5", "V1", "V2", "V3")
EDGE_MARGIN = 1e-4      # five times the forward tolerance (2e-5 * s on log-probs and values)


def offpolicy_rows(oracle64, mb, hp: PPOHyper, s: float = 1.0, always_normalize: bool = False, **eval_kw):
    """per row of minibatch `mb`, on a float64 copy of the checker (double_copy): ratio = exp(logp - old_logp), the advantage as
    the loss sees it (normalised where hp says so; always_normalize: Modular's loss has no switch) and dlt = v - old_v, with the
    classes of the two clips as boolean masks:
        P1 ratio > 1+c, adv > 0 (clipped: no policy gradient)     P2 ratio > 1+c, adv < 0 (outside, but live: pl1 < pl2)
        P3 ratio < 1-c, adv > 0 (live)                            P4 ratio < 1-c, adv < 0 (clipped)       P5 inside [1-c, 1+c]
        V1 dlt > c_vf       V2 dlt < -c_vf       V3 inside          (None where hp.clip_range_vf is None)
    and `edge`: |ratio - (1 +- c)| < 1e-4 s ratio or ||dlt| - c_vf| < 1e-4 s, s = max(1, w_last / 64) -- rows a device within its
    forward tolerance may put on the other side of a clip.  eval_kw goes to evaluate_actions (Modular: partner_idx)."""
    mb64 = {k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
    actions = mb64["actions"]
    if oracle64.act_space.kind == "discrete":
        actions = actions.long().flatten()
    with float64_checker(), th.no_grad():
        values, logp, _ = oracle64.evaluate_actions(mb64["observations"], actions, **eval_kw)
    assert logp.dtype == th.float64 and values.dtype == th.float64
    adv = mb64["advantages"]
    if (hp.normalize_advantage or always_normalize) and (len(adv) > 1 or always_normalize):
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = th.exp(logp - mb64["old_log_prob"]).numpy()
    adv = adv.numpy()
    dlt = (values.flatten() - mb64["old_values"]).numpy()
    c, cv = hp.clip_range, hp.clip_range_vf
    hi, lo = ratio > 1 + c, ratio < 1 - c
    out = dict(ratio=ratio, adv=adv, dlt=dlt, P1=hi & (adv > 0), P2=hi & (adv < 0), P3=lo & (adv > 0), P4=lo & (adv < 0),
               P5=~hi & ~lo, V1=None, V2=None, V3=None)
    edge = np.minimum(np.abs(ratio - (1 + c)), np.abs(ratio - (1 - c))) < EDGE_MARGIN * s * ratio
    if cv is not None:
        out.update(V1=dlt > cv, V2=dlt < -cv, V3=np.abs(dlt) <= cv)
        edge |= np.abs(np.abs(dlt) - cv) < EDGE_MARGIN * s
    out["edge"] = edge
    return out


def flat_blocks(oracle, flat_fn=None):
    """(block, names): block[i] = which parameter tensor (a weight matrix, a bias, the Gaussian log_std) flat entry i belongs to,
    names[b] its module path -- read off the checker's own flat order like _flat_layout"""
    params, idx = _flat_layout(oracle, flat_fn)
    owner = np.concatenate([np.full(p.numel(), b, np.int64) for b, p in enumerate(params)])
    by_id = {id(p): n for n, p in oracle.named_parameters()}
    return owner[idx], [by_id.get(id(p), "param%d" % b) for b, p in enumerate(params)]


def flat_grads_exact(oracle, flat_fn=None):
    """the checker's gradients in flat order WITHOUT the float32 cast of flat_grads() (a float64 copy keeps float64); a parameter the
    loss does not reach counts as zero"""
    params, idx = _flat_layout(oracle, flat_fn)
    g = np.concatenate([(th.zeros_like(p) if p.grad is None else p.grad).detach().reshape(-1).numpy().astype(np.float64)
                        for p in params])
    return g[idx]


def assert_block_gradients(g, g32, g64, block, names, where=()):
    """the device gradient against the float32 checker's: the project's rule over the whole vector (1e-6 + 2e-4 of the largest
    entry), and per parameter block b  max|g_b - g32_b| <= 1e-6 + max(2e-4 M_b, 4 d_b), M_b the block's largest float64 entry and
    d_b the checker's own float32-vs-float64 difference in the block (CHAIN_FACTOR, for assert_chain_moments' reason: the device
    differs from torch's float32 by another summation order and fast_tanh, not only by rounding).  Prints every block."""
    g, g32, g64 = np.asarray(g, np.float64), np.asarray(g32, np.float64), np.asarray(g64, np.float64)
    assert g.shape == g32.shape == g64.shape == block.shape, (g.shape, g32.shape, g64.shape, block.shape)
    bad = []
    for b, name in enumerate(names):
        sel = block == b
        M = np.abs(g64[sel]).max()
        d = np.abs(g32[sel] - g64[sel]).max()
        err = np.abs(g[sel] - g32[sel]).max()
        allowed = 1e-6 + max(2e-4 * M, CHAIN_FACTOR * d)
        print(where, "block %-28s n=%-6d max %.3g  checker f32 vs f64 d = %.3g  device vs checker %.3g  allowed %.3g"
              % (name, int(sel.sum()), M, d, err, allowed))
        if not err <= allowed:
            bad.append((name, err, allowed))
    scale = np.abs(g32).max()
    err = np.abs(g - g32).max()
    print(where, "whole gradient: device vs checker %.3g allowed %.3g (of max entry %.3g)" % (err, 1e-6 + 2e-4 * scale, scale))
    assert err <= 1e-6 + 2e-4 * scale, (where, err, scale, int(np.abs(g - g32).argmax()))
    assert not bad, (where, bad)


def upload_buffer(dev_buf, ob: RolloutBufferOracle) -> None:
    """copy every array of an oracle buffer into a device RolloutBuffer (marks it full)."""
    for k in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
        getattr(dev_buf, k).copy_(th.as_tensor(getattr(ob, k)))
    dev_buf.pos, dev_buf.full = dev_buf.buffer_size, True


def make_device_buffer(name: str, pol, T: int, E: int):
    from pantheonrl_amd.ppo import RolloutBuffer
    obs_s, act_s = CONFIGS[name]
    return RolloutBuffer(T, to_space(obs_s), to_space(act_s, "act"), pol.device, pol.ctx, pol.spec, n_envs=E)


# --------------------------------------------------------------------------------------
# Adam state of a checker in the flat layout of its parameters (tests/test_optimizer_checks.py, tests/test_gpu_optimizer.py)
# --------------------------------------------------------------------------------------
def _flat_layout(oracle, flat_fn=None):
    """(parameters in optimizer order, idx): flat vector entry i is entry idx[i] of the concatenated parameters.  Read off the
    class's own flat_params() (or `flat_fn(oracle)`, e.g. modular_cases._flat) by filling every parameter with its running
    index -- float32 holds integers below 2**24 exactly -- so the order and the transpositions can never differ from it."""
    params = list(oracle.parameters())
    total = sum(p.numel() for p in params)
    assert total < 2 ** 24
    saved = [p.detach().clone() for p in params]
    try:
        with th.no_grad():
            o = 0
            for p in params:
                p.copy_(th.arange(o, o + p.numel(), dtype=th.float32).reshape(p.shape))
                o += p.numel()
        flat = flat_fn(oracle) if flat_fn is not None else oracle.flat_params()
    finally:
        with th.no_grad():
            for p, s in zip(params, saved):
                p.copy_(s)
    idx = np.asarray(flat, np.float64).astype(np.int64)
    assert np.array_equal(idx.astype(np.float32), np.asarray(flat, np.float32))
    return params, idx


def flat_adam_state(oracle, optimizer=None, flat_fn=None):
    """-> (m, v, steps): exp_avg, exp_avg_sq (float32) and the per-parameter step (int64, one per flat entry) of the checker's
    Adam in the order and transposition of flat_params() / flat_grads().  A parameter without state gives zeros and step 0."""
    opt = optimizer if optimizer is not None else oracle.optimizer
    params, idx = _flat_layout(oracle, flat_fn)
    ms, vs, ts = [], [], []
    for p in params:
        st = opt.state.get(p, {})
        n = p.numel()
        if len(st) == 0:
            ms.append(np.zeros(n, np.float32)), vs.append(np.zeros(n, np.float32)), ts.append(np.zeros(n, np.int64))
        else:
            ms.append(st["exp_avg"].detach().reshape(-1).numpy().copy())      # (float64 for a .double() checker)
            vs.append(st["exp_avg_sq"].detach().reshape(-1).numpy().copy())
            ts.append(np.full(n, int(round(float(st["step"]))), np.int64))
    return np.concatenate(ms)[idx], np.concatenate(vs)[idx], np.concatenate(ts)[idx]


def load_flat_adam_state(oracle, m, v, steps, optimizer=None, flat_fn=None) -> None:
    """the inverse of flat_adam_state: afterwards optimizer.step() continues from (m, v, steps).  `steps`: one integer, or one
    per flat entry (equal within a parameter).  A parameter whose step is 0 is left without state (torch creates it at the
    parameter's first gradient); one with state gets a zero gradient tensor where it has none, which is what a parameter that
    has taken part in a step carries under torch 1.13's zero_grad (oracle.modular_train)."""
    opt = optimizer if optimizer is not None else oracle.optimizer
    params, idx = _flat_layout(oracle, flat_fn)
    total = sum(p.numel() for p in params)
    m, v = np.asarray(m, np.float32), np.asarray(v, np.float32)
    steps = np.broadcast_to(np.asarray(steps, np.int64), (len(idx),))
    assert m.shape == v.shape == (len(idx),)
    cm, cv, ct = np.zeros(total, np.float32), np.zeros(total, np.float32), np.zeros(total, np.int64)
    cm[idx], cv[idx], ct[idx] = m, v, steps
    o = 0
    for p in params:
        n = p.numel()
        t = ct[o:o + n]
        assert (t == t[0]).all(), "one step count per parameter tensor"
        opt.state.pop(p, None)
        if t[0] > 0:
            opt.state[p] = {"step": th.tensor(float(t[0]), dtype=th.float32),
                            "exp_avg": th.as_tensor(cm[o:o + n].copy()).reshape(p.shape).to(p.dtype),
                            "exp_avg_sq": th.as_tensor(cv[o:o + n].copy()).reshape(p.shape).to(p.dtype)}
            if p.grad is None:
                p.grad = th.zeros_like(p)
        else:
            assert not cm[o:o + n].any() and not cv[o:o + n].any(), "moments without a step count"
        o += n


def load_device_adam_state(obj, m, v, step, mod_first=None) -> None:
    """the device side: obj.adam_m / adam_v / opt_step (a policy, or a BC object) <- (m, v, step); mod_first for ModularPolicy"""
    obj.adam_m.copy_(th.as_tensor(np.asarray(m, np.float32)))
    obj.adam_v.copy_(th.as_tensor(np.asarray(v, np.float32)))
    obj.opt_step.fill_(int(step))
    if mod_first is not None:
        obj.mod_first.copy_(th.as_tensor(np.asarray(mod_first, np.int32)))


def read_device_adam_state(obj):
    return obj.adam_m.cpu().numpy().copy(), obj.adam_v.cpu().numpy().copy(), int(obj.opt_step.item())


# --------------------------------------------------------------------------------------
# Adam moments after a CHAIN of steps: the allowance is measured on the checker (float32 run against a float64 run)
# --------------------------------------------------------------------------------------
class float64_checker:
    """context: the checker computes in float64 on a `.double()` copy of a checker class -- preprocess_obs hands out float64
    features and the rollout buffer float64 minibatches (the stored numbers are the same float32 values)"""

    def __enter__(self):
        from oracle import sb3_oracle as orc
        self._orc, self._pre, self._get = orc, orc.preprocess_obs, orc.RolloutBufferOracle.get
        pre, get = self._pre, self._get

        def get64(buf, batch_size, indices=None):
            for mb in get(buf, batch_size, indices):
                yield {k: t.double() for k, t in mb.items()}
        orc.preprocess_obs = lambda obs, space: pre(obs, space).double()
        orc.RolloutBufferOracle.get = get64
        return self

    def __exit__(self, *exc):
        self._orc.preprocess_obs, self._orc.RolloutBufferOracle.get = self._pre, self._get
        return False


def double_copy(oracle, optimizer=None):
    """(float64 deep copy of a checker BEFORE a chain, its fresh Adam with the same lr / eps / betas)"""
    import copy
    src = optimizer if optimizer is not None else oracle.optimizer
    assert all(len(s) == 0 for s in src.state.values()) or len(src.state) == 0, "copy before the first step"
    o64 = copy.deepcopy(oracle).double()
    g = src.param_groups[0]
    opt = th.optim.Adam(o64.parameters(), lr=g["lr"], betas=g["betas"], eps=g["eps"])
    if optimizer is None:
        o64.optimizer = opt
    return o64, opt


def unit_hyper(hp: PPOHyper, n_rows: int, max_grad_norm: float, learning_rate: float = 3e-4) -> PPOHyper:
    """the hyper-parameters of ONE optimizer step: one epoch, the whole buffer as one minibatch"""
    import dataclasses
    return dataclasses.replace(hp, n_epochs=1, batch_size=n_rows, max_grad_norm=max_grad_norm, learning_rate=learning_rate)


def unit_gradient(oracle, run):
    """(gradient of the unit's loss in flat_grads() order as float64, its norm as the checker computed it): `run(checker,
    max_grad_norm)` takes one step on a deep copy with max_grad_norm = 1e9, which multiplies the gradient by exactly 1"""
    import copy
    c = copy.deepcopy(oracle)
    stats = run(c, 1e9)
    return c.flat_grads().astype(np.float64), float(stats[0]["grad_norm"])


CHAIN_FLOOR, CHAIN_FACTOR = 4e-4, 4.0


def chain64_state(o64, run, optimizer=None, flat_fn=None):
    """run(o64): the chain on the float64 copy (same buffer, same permutations) -> its (m, v, steps)"""
    with float64_checker():
        run(o64)
    return flat_adam_state(o64, optimizer, flat_fn)


def assert_chain_moments(dev_m, dev_v, ref32, ref64, where=()):
    """Adam moments of the device after a chain of steps against the float32 checker's (`ref32`, `ref64`: (m, v, steps) from
    flat_adam_state of the float32 run and of the float64 run of the same chain).  d = largest entrywise |float32 - float64|
    relative to the largest float64 entry; the device is allowed max(4 d, 4e-4) of the largest entry: 4e-4 is the one-step
    figure (the 2e-4 gradient tolerance plus the 2e-4 of the clip coefficient), the factor 4 is for what separates the device
    from torch's float32 rather than from float64 (another summation order in every reduction, fast_tanh's 2e-7 per activation).
    Prints d and the observed error beside the allowance; returns (d_m, d_v)."""
    out = []
    for name, dev, a32, a64 in (("adam_m", dev_m, ref32[0], ref64[0]), ("adam_v", dev_v, ref32[1], ref64[1])):
        a64 = np.asarray(a64, np.float64)
        scale = np.abs(a64).max()
        d = np.abs(np.asarray(a32, np.float64) - a64).max() / scale
        allowed = max(CHAIN_FACTOR * d, CHAIN_FLOOR)
        err = np.abs(np.asarray(dev, np.float64) - np.asarray(a32, np.float64)).max() / scale
        print(where, name, "chain: checker f32 vs f64 d = %.3g, device vs checker %.3g, allowed %.3g (of max entry %.3g)"
              % (d, err, allowed, scale))
        assert err <= allowed, (where, name, err, allowed, d)
        out.append(d)
    return tuple(out)


__all__ = ["CONFIGS", "PPOHyper", "to_space", "sample_obs", "oracle_policy", "device_policy",
           "filled_oracle_buffer", "upload_buffer", "make_device_buffer", "flat_adam_state", "load_flat_adam_state",
           "load_device_adam_state", "read_device_adam_state", "unit_hyper", "unit_gradient", "float64_checker", "double_copy", "chain64_state", "assert_chain_moments",
           "stale_oracle_buffer", "offpolicy_rows", "OFFPOLICY_CLASSES", "flat_blocks", "flat_grads_exact", "assert_block_gradients"]
