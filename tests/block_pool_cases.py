"""The cases of the block worlds' partner-pool tests, written once: models and members built from (variant, kind, size, seed), the
pool built from them, the snapshot of a pool's state and the comparison of two snapshots.

Two runs from the same arguments are the same run: every policy is initialised from its seed and nothing here reads a clock or a
global generator.  A snapshot holds only what is defined: of a ragged buffer (a learner writes column e at its own row pos[e]) the
rows below `pos`."""
from __future__ import annotations

import numpy as np
import torch as th

from pantheonrl_amd import _native as nat

RB_KEYS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs")
KINDS = dict(learner=nat.PH_POOL_LEARNER, frozen=nat.PH_POOL_FROZEN, scripted=nat.PH_POOL_SCRIPTED)
END_BIAS = 3.0        # what the planner's end-token bias is raised by, so that games end (p(end) >= 0.40 per token)


def ppo(variant, seat, E, T, seed, gae_mode=1):
    """PPO on the variant's planner (seat 0) or constructor (seat 1) spaces, with device permutations"""
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import VecBlockWorld
    model = PPO("MlpPolicy", VecBlockWorld.seat_spaces(variant)[seat], n_steps=T, n_envs=E, batch_size=max(8, E * T // 2), n_epochs=2,
                seed=seed)
    model.device_permutations = True
    if gae_mode is not None:
        model.rollout_buffer.gae_mode = gae_mode
    return model


def bias_end_token(policy, bias=END_BIAS):
    """raise the planner's end-token logit bias (as tests/test_gpu_block_xplay.py's _biased_planner): games end within a few tokens"""
    with th.no_grad():
        policy.params[policy.layout.act_b + policy.layout.L - 1] += bias
    return policy


def member(variant, kind, E, T_alt, seed):
    from pantheonrl_amd.envs.vec import FrozenVecPartner, RaggedVecOnPolicyAgent, VecBlockScriptedPartner
    if kind == "scripted":
        return VecBlockScriptedPartner(variant, "DEFAULT")
    if kind == "easy":
        return VecBlockScriptedPartner(variant, "EASY")
    if kind == "learner":
        return RaggedVecOnPolicyAgent(ppo(variant, 1, E, T_alt, seed))
    return FrozenVecPartner(ppo(variant, 1, 4, 2, seed).policy)


def pool(variant, E, T_ego, T_alt, kinds, seed=0, native=True, resample="robin", biased=True, before=None):
    """-> (pool, ego, members): the ego from `seed` (its end-token bias raised when `biased`), member k from seed + 1 + k, the worlds
    from seed + 7.  `before(members)` runs in front of the constructor"""
    from pantheonrl_amd.envs.vec import VecBlockPartnerPool
    from pantheonrl_amd.vec import VecOnPolicyAgent
    ego = VecOnPolicyAgent(ppo(variant, 0, E, T_ego, seed))
    if biased:
        bias_end_token(ego.model.policy)
    members = [member(variant, kind, E, T_alt, seed + 1 + k) for k, kind in enumerate(kinds)]
    if before is not None:
        before(members)
    return VecBlockPartnerPool(variant, E, ego, members, seed=seed + 7, resample=resample, native=native), ego, members


def recorded_rows(x, pos):
    """the defined part of a learner's (T, E, ...) array: rows below pos[e] of every column e"""
    return x[np.arange(x.shape[0])[:, None] < pos[None, :]]


def snapshot(sp, ego, members):
    """the pool's state: the game, both observations, who sits where, the ego's buffer, each learner's recorded rows, book and
    parameters, the episode count"""
    th.cuda.synchronize()
    out = dict(state=sp.env.state.cpu().numpy().copy(), obs_ego=sp.obs_ego.cpu().numpy().copy(), obs_alt=sp.obs_alt.cpu().numpy().copy(),
               pid=sp.partnerid.cpu().numpy().copy(), acted=sp.alt_acted.cpu().numpy().copy(), episodes=sp.episodes,
               ego_it=ego.iteration, pe=ego.model.policy.get_flat_params().copy(),
               e_last=ego._last_episode_starts.cpu().numpy().copy())
    out.update({"e_" + k: v.copy() for k, v in ego.model.rollout_buffer.host().items() if k in RB_KEYS[:4]})
    for i, m in enumerate(members):
        if not hasattr(m, "pos"):
            continue
        pos = m.pos.cpu().numpy().copy()
        out[f"m{i}_pos"] = pos
        out[f"m{i}_flags"] = np.stack([t.cpu().numpy() for t in (m.boundary, m.term, m.open)])
        out[f"m{i}_it"] = m.iteration
        out[f"m{i}_params"] = m.model.policy.get_flat_params().copy()
        for k, v in m.model.rollout_buffer.host().items():
            if k in RB_KEYS:
                out[f"m{i}_{k}"] = recorded_rows(v, pos).copy()
    return out


def same_state(a, b, where=""):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), (where, key)
