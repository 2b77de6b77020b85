"""The cases of the device-resident Liar's Dice tests -- the partner pool, cross-play, self-play, the move log -- written once: the
member kinds, the models and members built from (kind, size, seed), the drivers built from them, the snapshots of a driver's state
and the comparison of two snapshots.  A new member kind is an entry in KINDS (or ADAPS) and, if it is built another way, a branch
in `member`.

Two runs from the same arguments are the same run: every policy is initialised from its seed, `sharpen` draws from the seed, and
nothing here reads a clock or a global generator.  A snapshot holds only what is defined: of a ragged buffer (a learner at seat 1
writes column e at its own row pos[e]) the rows below `pos`, selected by `recorded_rows` -- so two snapshots are compared key by
key with nothing masked at the comparison."""
from __future__ import annotations

import ctypes as C
from collections import deque

import numpy as np
import torch as th

from pantheonrl_amd import _native as nat

RB_KEYS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs")
XSTATE = ("hands", "history", "nmoves", "obs_ego", "obs_alt", "games", "playing", "tables_left", "returns", "lengths", "ep_return",
          "ep_length")
# member kinds: name -> (PH_POOL_* kind, tower widths or None)
KINDS = dict(learner=(nat.PH_POOL_LEARNER, None), frozen=(nat.PH_POOL_FROZEN, None), scripted=(nat.PH_POOL_SCRIPTED, None),
             clone=(nat.PH_POOL_CLONE, None), ltower32=(nat.PH_POOL_LEARNER, (32,)), ftower32=(nat.PH_POOL_FROZEN, (32,)),
             ftower128=(nat.PH_POOL_FROZEN, (128, 128)), ftower256=(nat.PH_POOL_FROZEN, (256, 128)),
             ftower64x3=(nat.PH_POOL_FROZEN, (64, 64, 64)))
# frozen ADAP checkpoints (AdapFrozenVecPartner): name -> (context_size, latent form, sampler)
ADAPS = dict(adapS3=(3, "stated", "l2"), adapR3=(3, "sample", "l2"), adapS1=(1, "stated", "l2"), adapR52=(52, "sample", "l2"),
             adapC4=(4, "sample", "categorical"))


# ---- models and members ----------------------------------------------------------------------------------------------------------
def spaces():
    from pantheonrl_amd.envs.vec import VecLiarsDice
    return type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                              _is_dummy_space_env=True))()


def ppo(E, T, seed, arch=None, gae_mode=1):
    """PPO on the game's spaces with device permutations: a tower of `arch`, or the 64-wide policy; gae_mode None keeps the
    buffer's default"""
    from pantheonrl_amd import PPO
    kwargs = dict(policy_kwargs=dict(net_arch=[dict(pi=list(arch), vf=list(arch))])) if arch else {}
    model = PPO("MlpPolicy", spaces(), n_steps=T, n_envs=E, batch_size=max(8, E * T // 2), n_epochs=2, seed=seed, **kwargs)
    model.device_permutations = True
    if gae_mode is not None:
        model.rollout_buffer.gae_mode = gae_mode
    return model


def sharpen(policy, seed):
    """parameters of order one, so that the moves spread and a wrong bit moves a sample; the same seed gives the same parameters"""
    policy.set_flat_params(0.4 * np.random.default_rng(seed).standard_normal(policy.layout.P).astype(np.float32))
    return policy


def clone_policy(seed):
    """a sharpened FeedForward32Policy on the game's spaces; the same seed gives the same parameters and the same Philox key"""
    from pantheonrl_amd.bc import FeedForward32Policy
    s = spaces()
    return sharpen(FeedForward32Policy(s.observation_space, s.action_space, seed=1000 + seed), seed)


def adap_model(cs, seed, sampler="l2"):
    from pantheonrl_amd.adap import ADAP, AdapPolicy
    m = ADAP(AdapPolicy, spaces(), context_sampler=sampler, context_size=cs, n_steps=2, n_envs=4, batch_size=4, n_epochs=1, seed=seed)
    sharpen(m.policy, seed)
    return m


def latent(cs, seed):
    """the stated latent of an ADAP member built from `seed`"""
    return np.random.default_rng(900 + seed).standard_normal(cs).astype(np.float32)


def member(kind, E, T_alt, seed, sharp=False):
    """a pool / population member of `kind` (a key of KINDS or ADAPS).  `sharp`: whether a learner's or a frozen member's policy
    is sharpened -- a bool, or a predicate of the kind's name; a clone and an ADAP checkpoint always are"""
    from pantheonrl_amd.envs.vec import (AdapFrozenVecPartner, ClonedVecPartner, VecLiarDefaultPartner, frozen_partner_for,
                                         ragged_agent_for)
    if kind in ADAPS:
        cs, form, sampler = ADAPS[kind]
        return AdapFrozenVecPartner(adap_model(cs, seed, sampler).policy, "sample" if form == "sample" else latent(cs, seed), sampler)
    pool_kind, arch = KINDS[kind]
    if pool_kind == nat.PH_POOL_SCRIPTED:
        return VecLiarDefaultPartner()
    if pool_kind == nat.PH_POOL_CLONE:
        return ClonedVecPartner(clone_policy(seed))
    learner = pool_kind == nat.PH_POOL_LEARNER
    m = ragged_agent_for(ppo(E, T_alt, seed, arch)) if learner else frozen_partner_for(ppo(E, 2, seed, arch).policy)
    if sharp(kind) if callable(sharp) else sharp:
        sharpen(m.model.policy if learner else m.policy, seed)
    return m


# ---- drivers ---------------------------------------------------------------------------------------------------------------------
def pool(E, T_ego, T_alt, kinds, ego_arch=None, seed=0, native=True, resample="robin", record=0, before=None, sharp=False):
    """-> (pool, ego, members): the ego from `seed`, member k from seed + 1 + k, the dice from seed + 7.  `before(members)` runs in
    front of the constructor (e.g. loggers that must see its deal)"""
    from pantheonrl_amd.envs.vec import liar_pool_for
    from pantheonrl_amd.vec import vec_agent_for
    ego = vec_agent_for(ppo(E, T_ego, seed, ego_arch))
    members = [member(kind, E, T_alt, seed + 1 + k, sharp) for k, kind in enumerate(kinds)]
    if before is not None:
        before(members)
    return liar_pool_for(E, ego, members, seed=seed + 7, resample=resample, native=native, record=record), ego, members


def xplay(E, kinds, G, pairs=None, seed=5, native=True, record=0, cls=None, member_seed=20):
    """a cross-play of the population `kinds` (member k from member_seed + k), G games per table"""
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    members = [member(kind, 4, 2, member_seed + k) for k, kind in enumerate(kinds)]
    return (cls or VecLiarCrossPlay)(E, members, pairs=pairs, episodes_per_table=G, seed=seed, native=native, record=record)


def selfplay(E, ego_model, alt_model, seed=0, native=True, record=0, calls=None, latent_syncer=False):
    """-> (self-play, ego, alt) of two models, the dice from seed + 7.  `calls`: a list that collects the partner's forwards of the
    walk, the first deal's too -- (moves, mask), and the contexts it read where the partner is an ADAP seat"""
    from pantheonrl_amd.envs.vec import VecLiarSelfPlay, ragged_agent_for
    from pantheonrl_amd.vec import vec_agent_for
    ego = vec_agent_for(ego_model)
    alt = ragged_agent_for(alt_model, latent_syncer=ego if latent_syncer else None)
    if calls is not None:
        inner = alt.get_action

        def logged(obs, rec_mask):
            acts = inner(obs, rec_mask)
            row = (acts.cpu().numpy().copy(), rec_mask.cpu().numpy().astype(bool))
            calls.append(row + (alt.current_contexts().cpu().numpy().copy(),) if hasattr(alt, "current_contexts") else row)
            return acts
        alt.get_action = logged
    return VecLiarSelfPlay(E, ego, alt, seed=seed + 7, native=native, record=record), ego, alt


def step_through_the_plain_entry_point(sp):
    """from its next step on, the self-play `sp` (64-wide policies in both seats) steps through `ph_liar_selfplay_step` itself:
    the narrow entry point the driver's own `_arch(None, None)` call stands for -- the reference of the tests that hold the two
    bitwise equal"""
    def plain(counter, deal_only=False, ego_pos=-1):
        sp._bind()
        ctx, rb = sp.env.ctx, sp.ego.model.rollout_buffer
        nat.check(ctx.lib.ph_liar_selfplay_step(ctx.handle, C.byref(sp._desc), int(rb.pos if ego_pos < 0 else ego_pos), int(counter),
                                                int(deal_only)))
    assert sp.native and not sp.towers and not sp.adap
    sp._native_call = plain


def ctx_of(agent):
    """the engine context of an agent's policy, on the current stream"""
    ctx = agent.model.policy.ctx
    ctx.set_stream(th.cuda.current_stream(agent.model.policy.device).cuda_stream)
    return ctx


def interleave(counts):
    """member ids with the given counts, interleaved by table index (round robin over the members that still have rows left)"""
    left, out = list(counts), []
    while any(left):
        for k in range(len(left)):
            if left[k]:
                out.append(k)
                left[k] -= 1
    return np.asarray(out, np.int32)


def train_steps(sp, steps, learners=None):
    """`steps` vectorised steps of a driver; a partner-side learner (sp.learners, unless given) trains whenever it is full (the ego
    trains inside the step) -> how often each learner trained"""
    learners = sp.learners if learners is None else learners
    trained = [0] * len(learners)
    for _ in range(steps):
        sp.step()
        for i, m in enumerate(learners):
            if m.full():
                m.learn_from_buffer()
                trained[i] += 1
    th.cuda.synchronize()
    return trained


# ---- snapshots and their comparison ----------------------------------------------------------------------------------------------
def recorded_rows(v, pos):
    """the defined part of a ragged buffer's plane v (T, E, ...): column e's rows below pos[e], in row-major order"""
    return v[np.arange(v.shape[0])[:, None] < pos[None, :]] if getattr(v, "ndim", 0) >= 2 else v


def train_state(sp, ego, learners=None):
    """a training driver's state (self-play, the pool): the game and what VecLiarStep owns beside it, seat 0's six buffer
    planes and parameters, and per learner i at seat 1 its cursor, flags, value cache, iteration count, parameters and the
    recorded rows of every plane of its buffer; the pool's `pid_now` / `alt_actions` where the driver has them"""
    th.cuda.synchronize()
    learners = sp.learners if learners is None else learners
    out = dict(hands=sp.env.hands.cpu().numpy(), hist=sp.env.history.cpu().numpy(), nmoves=sp.env.nmoves.cpu().numpy(),
               ego_first=sp.ego_first.cpu().numpy().copy(), obs=sp.obs_ego.cpu().numpy().copy(), obs_alt=sp.obs_alt.cpu().numpy().copy(),
               acted=sp.alt_acted.cpu().numpy().copy(), episodes=sp.episodes, ego_it=ego.iteration,
               es=ego._last_episode_starts.cpu().numpy().copy(), pe=ego.model.policy.get_flat_params())
    if hasattr(sp, "partnerid"):
        out.update(pid_now=sp.partnerid.cpu().numpy().copy(), alt_actions=sp.alt_actions.cpu().numpy().copy())
    out.update({"e_" + k: v for k, v in ego.model.rollout_buffer.host().items() if k in RB_KEYS})
    for i, m in enumerate(learners):
        pos = m.pos.cpu().numpy()
        out[f"pos{i}"], out[f"it{i}"], out[f"p{i}"] = pos, m.iteration, m.model.policy.get_flat_params()
        out[f"flags{i}"] = np.stack([t.cpu().numpy() for t in (m.boundary, m.term, m.open)])
        out[f"values{i}"] = m.values.cpu().numpy()
        out.update({f"a{i}_" + k: recorded_rows(v, pos) for k, v in m.model.rollout_buffer.host().items()})
    return out


def xstate(xp):
    """a cross-play's state: the game, the budget, the logs"""
    th.cuda.synchronize()
    out = {k: getattr(xp.env if k in ("hands", "history", "nmoves") else xp, k).cpu().numpy().copy() for k in XSTATE}
    out["ego_first"] = xp.ego_first.cpu().numpy().copy()
    return out


def same_state(a, b, what="", ego_rows=None):
    """two snapshots hold the same keys and, key by key, the same bits; ego_rows: of seat 0's buffer planes the first rows only
    (the rest of the buffer was not written by both runs)"""
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    for key in a:
        x, y = a[key], b[key]
        if key.startswith("e_") and ego_rows is not None:
            x, y = x[:ego_rows], y[:ego_rows]
        assert np.array_equal(x, y), (what, key)


def run_pool(native, resample, kinds, E, T_ego, T_alt, steps, seed=11, **kw):
    """a pool stepped `steps` times -> train_state, with `pid` (steps, E): who sat where after every step, and `trained`"""
    sp, ego, members = pool(E, T_ego, T_alt, kinds, seed=seed, native=native, resample=resample, **kw)
    trained = [0] * len(sp.learners)
    pids = []
    for _ in range(steps):
        sp.step()
        pids.append(sp.partnerid.cpu().numpy().copy())
        for i, m in enumerate(sp.learners):
            if m.full():
                m.learn_from_buffer()
                trained[i] += 1
    out = train_state(sp, ego)
    out.update(pid=np.stack(pids), trained=trained)
    return out


# ---- the reference recorder --------------------------------------------------------------------------------------------------------
def replay_through_the_reference_recorder(events, e):
    """table e's deals and moves played through TurnBasedRecorder(LiarEnv) -> (its get_transitions(), games played).  events:
    ("deal", reset mask, hands, ego_first) and ("move", actions, is_ego, active), each over all tables, in the order they happened"""
    from pantheonrl_amd.common import Agent, Observation
    from pantheonrl_amd.common.wrappers import TurnBasedRecorder
    from pantheonrl_amd.envs.liar import LiarEnv

    class Shadow(LiarEnv):
        def __init__(self):
            super().__init__()
            self.deals = deque()

        def multi_reset(self, egofirst):
            first, hands = self.deals.popleft()
            assert bool(first) == bool(egofirst)
            self.history, self.egohand, self.althand = [], [int(x) for x in hands[:6]], [int(x) for x in hands[6:]]
            return self.getObs(egofirst)

    class Recorder(TurnBasedRecorder):
        def n_reset(self):                   # who opens is the device's draw
            self.ego_next = bool(self.env.deals[0][0])
            first = self.multi_reset(self.ego_next)
            return (0 if self.ego_next else 1,), (Observation(first),)

    class Replay(Agent):
        def __init__(self):
            self.moves = deque()

        def get_action(self, obs, record=True):
            return self.moves.popleft()

        def update(self, reward, done):
            return None

    shadow, partner, ego_moves = Shadow(), Replay(), []
    for ev in events:
        if ev[0] == "deal":
            if ev[1][e]:
                shadow.deals.append((ev[3][e], ev[2][e].copy()))
        elif ev[3][e]:
            (ego_moves if ev[2][e] else partner.moves).append(ev[1][e].copy())
    rec = Recorder(shadow)
    rec.add_partner_agent(partner)
    rec.reset()
    games = 0
    for a in ego_moves:
        _, _, done, _ = rec.step(a)
        if done:
            games += 1
            if shadow.deals:
                rec.reset()
    assert not shadow.deals and not partner.moves
    return rec.get_transitions(), games
