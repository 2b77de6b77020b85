"""The unit scenarios of the clip + Adam checks (tests/test_optimizer_checks.py), shared with the GPU optimizer tests and the BC
checks."""
import copy

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import helpers as H
from tests import modular_cases as M


SEED = 21
SPECS = [("overcooked", 32, 8), ("liar", 16, 6), ("rps", 128, 1)]


def ppo_unit(name, T, E, seed=SEED, make_oracle=None, hp=None, adap=None):
    """-> (checker, buffer, run, g_ref, n_ref).  run(checker, max_grad_norm, lr=3e-4) takes ONE optimizer step on the whole buffer
    as one minibatch and returns the checker's statistics; g_ref / n_ref: that step's unclipped gradient and its norm."""
    orac = (make_oracle or H.oracle_policy)(name, seed=seed)
    ob = H.filled_oracle_buffer(name, orac, T, E, seed=seed)
    N = T * E

    def run(c, max_grad_norm, lr=3e-4):
        return orc.ppo_train(c, ob, H.unit_hyper(hp or orc.PPOHyper(), N, max_grad_norm, lr), [np.arange(N)], adap=adap)
    g_ref, n_ref = H.unit_gradient(orac, run)
    return orac, ob, run, g_ref, n_ref


def bc_checker(name, N, seed=3):
    """FeedForward32Oracle, perturbed as tests/test_gpu_bc.py does, and N rows of (obs, acts)"""
    obs_s, act_s = H.CONFIGS[name]
    rng = np.random.default_rng(seed)
    obs = H.sample_obs(obs_s, N, rng)
    acts = np.stack([rng.integers(0, k, size=N) for k in act_s.nvec], axis=1).astype(np.float32)
    th.manual_seed(seed)
    orac = orc.FeedForward32Oracle(obs_s, act_s)
    with th.no_grad():
        g = th.Generator().manual_seed(seed + 1)
        for p in orac.parameters():
            p.add_(0.2 * th.randn(p.shape, generator=g) * (1.0 if p.ndim == 1 else 0.3))
    return orac, obs, acts


def bc_flat_grads(orac):
    out = []
    for lin in orac._linears():
        out += [lin.weight.grad.t().contiguous().reshape(-1), lin.bias.grad]
    out += [orac.value_net.weight.grad.reshape(-1), orac.value_net.bias.grad]
    return th.cat(out).numpy().astype(np.float64)


def bc_data_gradient(orac, obs, acts):
    """gradient of BC's loss WITHOUT the L2 term on the whole data set as one batch (optimizer_bound adds l2 * p0 itself)"""
    c = copy.deepcopy(orac)
    loss, _ = orc.bc_loss(c, th.as_tensor(obs), th.as_tensor(acts), 1e-3, 0.0)
    loss.backward()
    return bc_flat_grads(c)


BC_SCENARIOS = ("fresh", "resumed", "late", "eps")
BC_ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip=False)


def bc_scenario_state(scenario, P, seed=0):
    """-> (m0, v0, t0): BC's states -- random as for PPO; "eps" at BC's scale (Adam's eps is 1e-8 there)"""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(P), rng.standard_normal(P)
    if scenario == "fresh":
        return np.zeros(P, np.float32), np.zeros(P, np.float32), 0
    s, t0 = {"resumed": (1e-3, 7), "late": (1e-3, 100000), "eps": (1e-8, 100000)}[scenario]
    return (s * a).astype(np.float32), ((s * b) ** 2).astype(np.float32), t0


# Modular: the three-step unit (one train() call: partner 0, 1, 2 in turn, n_epochs = 1, the whole buffer as one minibatch)
MOD = dict(name="mod_small", K=3, T=8, E=8, coef=0.3, t0=7, first=(0, 3, -1), seed=7)


def modular_unit(max_norm_factor=None):
    """-> dict: a fresh checker, its K buffers, the loaded state (p0, m0, v0, per-entry steps, value-side labels) of MOD.
    Module 0's value side joined at step 0, module 1's at step 3 (it has counted 4 steps), module 2's has not joined."""
    c = MOD
    orac = M._oracle(c["name"], c["K"], seed=c["seed"])
    bufs = [M._filled(orac, c["name"], k, c["T"], c["E"], seed=20 + k) for k in range(c["K"])]
    label = M._value_side(orac)
    P = label.size
    rng = np.random.default_rng(5)
    m0 = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    v0 = ((1e-3 * rng.standard_normal(P)) ** 2).astype(np.float32)
    steps = np.full(P, c["t0"], np.int64)
    for j, first in enumerate(c["first"]):
        steps[label == j] = c["t0"] - first if first >= 0 else 0
    m0[steps == 0] = 0
    v0[steps == 0] = 0
    return dict(orac=orac, bufs=bufs, label=label, p0=M._flat(orac), m0=m0, v0=v0, steps=steps)


def modular_hp(max_grad_norm):
    c = MOD
    return orc.PPOHyper(batch_size=c["T"] * c["E"], n_epochs=1, ent_coef=0.01, max_grad_norm=max_grad_norm)


def modular_unit_run(orac, bufs, max_grad_norm):
    N = MOD["T"] * MOD["E"]
    return orc.modular_train(orac, bufs, modular_hp(max_grad_norm), MOD["coef"], perms=[[np.arange(N)]] * MOD["K"])


def modular_recorded_steps(u, max_grad_norm, n=None):
    """the unit on the checker, written out as modular_train does it, recording per step the unclipped gradient in _flat's order
    and which entries torch steps (their parameter has a gradient tensor) -> (grads, lives, norms); the checker in u is stepped
    (n: only the first n partners)"""
    orac, bufs = u["orac"], u["bufs"]
    M._load_flat_adam_state(orac, u["m0"], u["v0"], u["steps"])
    hp = modular_hp(max_grad_norm)
    N = MOD["T"] * MOD["E"]
    grads, lives, norms = [], [], []
    params, idx = H._flat_layout(orac, M._flat)
    for k, buf in enumerate(bufs[:n]):
        mb = next(iter(buf.get(N, np.arange(N))))
        loss, _ = orc.modular_minibatch_loss(orac, mb, hp, k, MOD["coef"])
        orac.optimizer.zero_grad(set_to_none=False)
        loss.backward()
        grads.append(M._flat(orac, grads=True).astype(np.float64))
        lives.append(np.concatenate([np.full(p.numel(), p.grad is not None) for p in params])[idx])
        norms.append(float(th.nn.utils.clip_grad_norm_(orac.parameters(), hp.max_grad_norm)))
        orac.optimizer.step()
    return grads, lives, norms


def chain_allowance(a32, a64):
    """Numbers: d = largest |float32 - float64| relative to the largest float64 entry; allowed max(4 d, 4e-4) of that entry"""
    scale = np.abs(a64).max()
    d = np.abs(np.asarray(a32, np.float64) - a64).max() / scale
    return max(H.CHAIN_FACTOR * d, H.CHAIN_FLOOR) * scale, d
