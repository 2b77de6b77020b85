"""The object graph of the reference's training CLI (trainer.py:92-137,182-256,394-432) on the MI355X engine.

    python -m pantheonrl_amd.trainer RPS-v0 PPO PPO --preset 1 --seed 0 -t 10000        (BASELINE config 1)

Same positional arguments and flags as the reference for the part of the surface that sits on the PPO path:
env in {RPS-v0, LiarsDice-v0, BlockEnv-v0, BlockEnv-v1}; ego in {PPO, ADAP, ADAP_MULT, ModularAlgorithm, LOAD}; each partner in {PPO, ADAP, ADAP_MULT, FIXED, DEFAULT}; JSON configs splatted
into the constructors; `--framestack`, `--preset 1`, `--ego-save/--alt-save`, `--tensorboard-log/-name`, `--seed`, `--device`,
`--total-timesteps`, `--share-latent` (ADAP ego + ADAP partners act under the ego's context).  `--record FILE` writes the episode
transitions in the reference's `.npy` format.  A ModularAlgorithm ego gets one partner module per partner agent
(`policy_kwargs = dict(num_partners=len(args.alt))`, trainer.py:131-135).  ADAP_MULT = ADAP with AdapPolicyMult (trainer.py:129-130,207-208).
"""
from __future__ import annotations

import argparse
import json
from typing import List, Tuple

import numpy as np

from . import envs as _envs
from .common import OnPolicyAgent, StaticPolicyAgent
from .common.wrappers import frame_wrap, recorder_wrap
from .envs.blockworld import BlockEnv, DefaultConstructorAgent, SBWDefaultAgent, SimpleBlockEnv
from .envs.liar import LiarDefaultAgent, LiarEnv
from .envs.rps import RPSEnv, RPSWeightedAgent
from .adap import ADAP, AdapAgent, AdapPolicy, AdapPolicyMult
from .modular import ModularAlgorithm, ModularPolicy
from .ppo import PPO

ADAP_TYPES = ["ADAP", "ADAP_MULT"]            # trainer.py:32
EGO_LIST = ["PPO", "ModularAlgorithm", "LOAD"] + ADAP_TYPES
PARTNER_LIST = ["PPO", "DEFAULT", "FIXED"] + ADAP_TYPES
OUT_OF_SCOPE = {"BC"}


class EnvException(Exception):
    """Raise when parameters do not align with the environment (reference trainer.py:37)."""


def input_check(args) -> None:
    """reject combinations the engine cannot honour, with the reference's error class, and complete the configs the way the
    reference's does (trainer.py:41-63: one `{}` per partner when no --alt-config was given, `verbose = 1` for the ego unless its
    config says otherwise, --tensorboard-log and --tensorboard-name together or not at all).  --share-latent's check is the caller's
    next step, as in the reference's main (trainer.py:399-403); pinned to the reference's text by tests/golden/ref_trainer_cli.json"""
    if args.env not in _envs.REGISTRY:
        raise EnvException(f"unknown or out-of-scope environment {args.env!r}; available: {sorted(_envs.REGISTRY)}")
    for name in [args.ego] + list(args.alt):
        if name in OUT_OF_SCOPE:
            raise EnvException(f"{name} agents are outside the PPO rollout+update path this engine implements")
    if args.ego not in EGO_LIST:
        raise EnvException(f"ego must be one of {EGO_LIST}")
    for name in args.alt:
        if name not in PARTNER_LIST:
            raise EnvException(f"partners must be among {PARTNER_LIST}")
    if args.alt_config is None:                         # trainer.py:50-52
        args.alt_config = [{} for _ in args.alt]
    elif len(args.alt_config) != len(args.alt):
        raise EnvException("Number of partners is different from number of configs")
    if "verbose" not in args.ego_config:                # trainer.py:57-59
        args.ego_config["verbose"] = 1
    if (args.tensorboard_log is not None) != (args.tensorboard_name is not None):       # trainer.py:61-63
        raise EnvException("Must define log and names for tensorboard")
    if args.framestack > 1 and args.env_config.get("framestack_incompatible", False):
        raise EnvException("this environment cannot be frame-stacked")


def latent_check(args) -> None:
    """--share-latent: every agent must be ADAP with the ego's context size and sampler (trainer.py:65-89)"""
    if args.ego not in ADAP_TYPES or not all(v in ADAP_TYPES for v in args.alt):
        raise EnvException("both agents must be ADAP or ADAP_MULT to share latent spaces")
    args.ego_config.setdefault("context_size", 3)
    args.ego_config.setdefault("context_sampler", "l2")
    for conf in args.alt_config:
        for key in ("context_size", "context_sampler"):
            if conf.setdefault(key, args.ego_config[key]) != args.ego_config[key]:
                raise EnvException("both agents must have similar configs to share latent spaces")


def generate_env(args) -> Tuple[object, object]:
    """env + the partner-side dummy env, optionally frame-stacked (trainer.py:92-104)"""
    env = _envs.make(args.env, **args.env_config)
    altenv = env.getDummyEnv(1)
    if args.framestack > 1:
        env = frame_wrap(env, args.framestack)
        altenv = env.getDummyEnv(1)   # the wrapped env carries the stacked observation space for both seats
    if args.record is not None:
        env = recorder_wrap(env)      # trainer.py:101-102
    return env, altenv


def gen_load(config: dict, policy_type: str, location: str):
    if policy_type in ADAP_TYPES:   # trainer.py:140-147: a fixed ADAP policy acts under a given latent value
        if "latent_val" not in config:
            raise EnvException("latent_val needs to be specified for FIXED ADAP policy")
        agent = ADAP.load(location, device=config.get("device", "cuda"))
        agent.policy.set_context(np.asarray(config.pop("latent_val"), np.float32))
        return agent
    if policy_type == "BC":         # trainer.py:152-153: BCShell(reconstruct_policy(location)) -- an object with a .policy
        from .bc import reconstruct_policy
        return _bc_shell(reconstruct_policy(location, device=config.get("device", "cuda")))
    if policy_type == "ModularAlgorithm":     # trainer.py:150-151
        return ModularAlgorithm.load(location, device=config.get("device", "cuda"))
    if policy_type != "PPO":
        raise EnvException("Not a valid FIXED/LOAD policy")
    return PPO.load(location, device=config.get("device", "cuda"))


class _BCShell:
    """pantheonrl.algos.bc.BCShell (bc.py:29-31): just enough of a model for StaticPolicyAgent / tester.py"""

    def __init__(self, policy):
        self.policy = policy


def _bc_shell(policy) -> _BCShell:
    return _BCShell(policy)


def generate_ego(env, args):
    """the ego learner (trainer.py:107-137)"""
    kwargs = dict(args.ego_config)
    kwargs.update(env=env, device=args.device, tensorboard_log=args.tensorboard_log)
    if args.seed is not None:
        kwargs["seed"] = args.seed
    if args.ego == "LOAD":
        model = gen_load(kwargs, kwargs["type"], kwargs["location"])
        model.set_env(env)
        if kwargs["type"] == "ModularAlgorithm":     # trainer.py:121-123: fresh partner modules for the partners of THIS run
            model.set_num_partners(len(args.alt))
        return model
    if args.ego == "ADAP":          # trainer.py:127-128
        return ADAP(policy=AdapPolicy, **kwargs)
    if args.ego == "ADAP_MULT":     # trainer.py:129-130
        return ADAP(policy=AdapPolicyMult, **kwargs)
    if args.ego == "ModularAlgorithm":               # trainer.py:131-135
        return ModularAlgorithm(policy=ModularPolicy, policy_kwargs=dict(num_partners=len(args.alt)), **kwargs)
    return PPO(policy="MlpPolicy", **kwargs)


def gen_partner(kind: str, config: dict, altenv, ego, args, index: int):
    """one partner agent (trainer.py:182-213)"""
    config = dict(config)
    if kind == "FIXED":
        return StaticPolicyAgent(gen_load(config, config["type"], config["location"]).policy)
    if kind == "DEFAULT":
        base = altenv
        while hasattr(base, "env"):      # unwrap frame-stack / recorder wrappers down to the game itself
            base = base.env
        if isinstance(base, RPSEnv):
            return RPSWeightedAgent(**config)
        if config:
            raise EnvException("No config possible for this default agent")
        if isinstance(base, LiarEnv):
            return LiarDefaultAgent()
        if base is SimpleBlockEnv.partner_env or isinstance(base, SimpleBlockEnv):     # trainer.py:172-175
            return SBWDefaultAgent()
        if base is BlockEnv.partner_env or isinstance(base, BlockEnv):
            return DefaultConstructorAgent()
        raise EnvException("No default policy available")
    agentarg = {}
    if args.tensorboard_log is not None:
        agentarg = {"tensorboard_log": args.tensorboard_log,
                    "tb_log_name": f"{args.tensorboard_name}_alt_{index}"}
    config.update(env=altenv, device=args.device, verbose=args.verbose_partner)
    if args.seed is not None:
        config["seed"] = args.seed
    # same seed as the ego (same initial weights, as in the reference: set_random_seed(seed) runs before every model's
    # init), but an action-sampling stream of its own -- see ActorCriticPolicy.__init__
    config["sampling_stream"] = index + 1
    if kind in ADAP_TYPES:          # trainer.py:205-213
        shared = ego.policy if args.share_latent else None
        return AdapAgent(ADAP(policy=AdapPolicy if kind == "ADAP" else AdapPolicyMult, **config), latent_syncer=shared, **agentarg)
    return OnPolicyAgent(PPO(policy="MlpPolicy", **config), **agentarg)


def generate_partners(altenv, env, ego, args) -> List:
    partners = []
    for i, kind in enumerate(args.alt):
        agent = gen_partner(kind, args.alt_config[i], altenv, ego, args, i)
        print(f"Partner {i}: {agent}")
        env.add_partner_agent(agent)
        partners.append(agent)
    return partners


def preset(args, preset_id: int):
    """default log / save names (trainer.py:231-256)"""
    if preset_id != 1:
        raise Exception("Invalid preset id")
    env_name = args.env
    if "layout_name" in args.env_config:
        env_name = f"{args.env}-{args.env_config['layout_name']}"
    seed = 0 if args.seed is None else args.seed
    args.tensorboard_log = args.tensorboard_log or "logs"
    args.tensorboard_name = args.tensorboard_name or f"{env_name}-{args.ego}{args.alt[0]}-{seed}"
    args.ego_save = args.ego_save or f"models/{env_name}-{args.ego}-ego-{seed}"
    args.alt_save = args.alt_save or f"models/{env_name}-{args.alt[0]}-alt-{seed}"
    return args


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train an ego agent with partner agents in a multi-agent environment "
                                            "on the MI355X PPO engine (flags as in PantheonRL's trainer.py)")
    p.add_argument("env", help="environment id")
    p.add_argument("ego", help="algorithm of the ego agent")
    p.add_argument("alt", nargs="+", help="algorithm(s) of the partner agent(s)")
    p.add_argument("--total-timesteps", "-t", type=int, default=500000)
    p.add_argument("--device", "-d", default="auto")     # (the reference's default; the engine takes it as "cuda": there is no other device)
    p.add_argument("--seed", "-s", type=int)
    p.add_argument("--ego-config", type=json.loads, default={})
    # the reference's form is ONE flag with a JSON string per partner (nargs='*', trainer.py:356-359); repeating the flag works as well
    p.add_argument("--alt-config", type=json.loads, nargs="*", action="extend")
    p.add_argument("--env-config", type=json.loads, default={})
    p.add_argument("--framestack", "-f", type=int, default=1)
    p.add_argument("--record", "-r")
    p.add_argument("--ego-save")
    p.add_argument("--alt-save")
    p.add_argument("--share-latent", "-l", action="store_true")
    p.add_argument("--tensorboard-log")
    p.add_argument("--tensorboard-name")
    p.add_argument("--verbose-partner", action="store_true")
    p.add_argument("--preset", type=int)
    p.add_argument("--n-envs", type=int, default=1,
                   help="(extension) >1: E copies of the game resident on the device, PPO-vs-PPO self-play without the "
                        "host in the step loop")
    # (no attribute unless given: the completed arguments of every other command line stay the reference's, plus n_envs)
    p.add_argument("--partner-pool", action="store_true", default=argparse.SUPPRESS,
                   help="(extension) with --n-envs: BlockEnv-v0|v1 PPO <alt>+ trains the planner against a device-resident pool "
                        "of constructors, each alt one of PPO / FIXED / DEFAULT (LiarsDice-v0 has its pool without the flag)")
    return p


POOL_KINDS = ("PPO", "FIXED", "DEFAULT")
LOG_INTERVAL = 10      # iterations between two episode-statistics records of the device-resident trainers


def pop_log_interval(env_config: dict) -> int:
    """`--env-config '{"log_interval": N}'` of the device-resident trainers: taken out of (a copy of) the env-config before the rest
    reaches the game, as `resample` is.  Every N iterations, and after the last one, the episode statistics are read and logged;
    0 = never read (no host synchronisation at all)."""
    value = env_config.pop("log_interval", LOG_INTERVAL)
    if isinstance(value, bool) or not isinstance(value, int) or value < 0:
        raise EnvException(f"--env-config log_interval must be a non-negative integer, not {value!r}")
    return value


def vectorised_plan(args):
    """the self-play pairings' share of --env-config: (log_interval, what remains for the game); the arguments are left alone"""
    env_config = dict(args.env_config)
    return pop_log_interval(env_config), env_config


class EpisodeLog:
    """The device-resident trainers' log: an EpisodeStats on the ego (always attached: one launch per iteration) and a logger in
    the ego's verbosity; `after(iteration, last)` reads and records every `log_interval` iterations and after the last one --
    the only host synchronisation this adds."""

    def __init__(self, args, ego_model, ego, env, log_interval: int):
        import time

        from .episode_stats import EpisodeStats
        from .logger import configure_logger
        self.stats = EpisodeStats(ego, env)
        self.logger = configure_logger(ego_model.verbose, args.tensorboard_log, args.tensorboard_name or "OnPolicyAlgorithm")
        self.ego, self.interval, self._clock, self._t0 = ego, int(log_interval), time.time, time.time()

    def after(self, iteration: int, last: bool = False) -> None:
        if self.interval and (last or iteration % self.interval == 0):
            from .episode_stats import record_episode_stats
            record_episode_stats(self.logger, self.stats, iteration, self.ego.num_timesteps, self._clock() - self._t0)


def pool_plan(args):
    """`LiarsDice-v0 PPO <alt>+ --n-envs E` with anything but exactly one PPO partner: the members of the device-resident partner
    pool as (kind, config) pairs, the resample rule and what remains of --env-config for the game -- checked before a device is
    touched.  None when the arguments are the single-learner self-play pairing (that path stays as it is).  With --partner-pool
    the same for `BlockEnv-v0|v1 PPO <alt>+`: the members of the pool of constructors (`block_member_config`), `block_variant` set;
    without the flag the block worlds' argument lists are refused as before."""
    alts = list(args.alt)
    if alts == ["PPO"]:
        return None
    if args.ego != "PPO" or not all(kind in POOL_KINDS for kind in alts):
        raise EnvException(f"--n-envs supports a PPO ego against PPO self-play or a pool of {list(POOL_KINDS)} partners")
    block_variant = BLOCK_VARIANTS.get(args.env)
    if args.env != "LiarsDice-v0" and not (block_variant is not None and getattr(args, "partner_pool", False)):
        raise EnvException(f"the device-resident partner pool exists for LiarsDice-v0, not {args.env}: with --n-envs the other "
                           "games take exactly one PPO partner"
                           + (" (the block worlds' pool of constructors is asked for with --partner-pool)"
                              if block_variant is not None else ""))
    from . import _native as nat
    if len(alts) > nat.PH_MAX_POOL:
        raise EnvException(f"the partner pool holds at most {nat.PH_MAX_POOL} members")
    env_config = dict(args.env_config)
    resample = env_config.pop("resample", "robin")
    log_interval = pop_log_interval(env_config)
    if resample not in nat.POOL_RESAMPLE:
        raise EnvException(f"--env-config resample must be one of {sorted(nat.POOL_RESAMPLE)}")
    members = []
    if block_variant is not None:
        block_member_config(args.env, block_variant, "PPO", dict(args.ego_config))      # (the ego: a tower is refused here too)
    for kind, config in zip(alts, args.alt_config):
        config = dict(config)
        if block_variant is not None:
            members.append((kind, block_member_config(args.env, block_variant, kind, config)))
            continue
        if kind == "FIXED":
            if "type" not in config or "location" not in config:
                raise EnvException("a FIXED partner needs 'type' and 'location' in its --alt-config")
            if config["type"] == "ADAP" and "latent_val" in config:
                config["latent_val"] = check_adap_latent(config["latent_val"], "a FIXED ADAP member's latent_val")
            elif config["type"] not in ("PPO", "BC"):
                raise EnvException("a FIXED member must be a PPO checkpoint (the 64-64 MlpPolicy) or a BC policy (bctrainer's "
                                   "shared 32-32 trunk) or an ADAP checkpoint with 'latent_val' (a list of context_size numbers, or "
                                   f"\"sample\": a context per table, redrawn at every deal), not {config['type']}")
        elif kind == "DEFAULT" and config:
            raise EnvException("No config possible for this default agent")
        members.append((kind, config))
    return dict(members=members, resample=resample, env_config=env_config, log_interval=log_interval, block_variant=block_variant)


BLOCK_VARIANTS = {"BlockEnv-v0": 0, "BlockEnv-v1": 1}


def block_member_config(env_name: str, variant: int, kind: str, config: dict) -> dict:
    """one member of the block worlds' pool of constructors, checked before a device is touched: PPO (a learner; its config goes to
    the PPO constructor), FIXED (a PPO checkpoint on the variant's constructor spaces) or DEFAULT (the variant's scripted
    constructor; on BlockEnv-v0 `{"rule": "EASY"}` seats SBWEasyPartner)"""
    if kind == "PPO":
        if (config.get("policy_kwargs") or {}).get("net_arch") is not None:
            raise EnvException(f"a net_arch tower (policy_kwargs net_arch) does not sit in the {env_name} partner pool: the ego and "
                               "the learners play PPO's 64-64 MlpPolicy")
    elif kind == "FIXED":
        if "type" not in config or "location" not in config:
            raise EnvException("a FIXED partner needs 'type' and 'location' in its --alt-config")
        if config["type"] != "PPO":
            raise EnvException(f"a FIXED member of the {env_name} pool is a PPO checkpoint (the 64-64 MlpPolicy on the constructor's "
                               f"spaces), not {config['type']}: BC clones and ADAP checkpoints do not sit in the block worlds' pool")
    elif kind == "DEFAULT":
        rule = config.pop("rule", "DEFAULT")
        if config:
            raise EnvException("the block worlds' default agent takes no config but 'rule'")
        if rule not in ("DEFAULT", "EASY"):
            raise EnvException(f"--alt-config rule must be DEFAULT or EASY, not {rule!r}")
        if rule == "EASY" and variant != 0:
            raise EnvException(f"EASY (SBWEasyPartner) exists for BlockEnv-v0 only, not {env_name}")
        config = dict(rule=rule)
    return config


def partner_pool_check(args) -> None:
    """--partner-pool: an extension beside --n-envs; it asks for the block worlds' pool of constructors, changes nothing for
    LiarsDice-v0 (whose pool needs no flag) and is refused for a game without a pool"""
    if not getattr(args, "partner_pool", False):
        return
    if args.n_envs <= 1:
        raise EnvException("--partner-pool belongs to the device-resident trainers: give --n-envs E with E > 1")
    if args.env != "LiarsDice-v0" and args.env not in BLOCK_VARIANTS:
        raise EnvException(f"--partner-pool: no device-resident partner pool exists for {args.env} (LiarsDice-v0, BlockEnv-v0 and "
                           "BlockEnv-v1 have one)")


def check_adap_latent(latent, what: str):
    """the latent of a frozen ADAP member of the device-resident pool / population: the string "sample" (a context per table, drawn
    with the checkpoint's sampler at every deal) or a list of numbers (the reference's latent_val, trainer.py:140-147; its length is
    held against the checkpoint's context_size when the file is loaded) -> "sample" or a list of floats"""
    if isinstance(latent, str):
        if latent != "sample":
            raise EnvException(f"{what} is a list of context_size numbers or \"sample\", not {latent!r}")
        return latent
    ok = isinstance(latent, (list, tuple)) and 1 <= len(latent) <= 64 and all(
        isinstance(v, (int, float)) and not isinstance(v, bool) and v == v for v in latent)
    if not ok:
        raise EnvException(f"{what} is a list of context_size (1..64) numbers or \"sample\", not {latent!r}")
    return [float(v) for v in latent]


def load_adap_member(location, latent, device):
    """a frozen ADAP checkpoint as a member of the device-resident pool / population (envs/vec.py: AdapFrozenVecPartner) under
    `latent`: the reference's FIXED ADAP partner (trainer.py:140-147: ADAP.load, then set_context) for every table"""
    from .envs.vec import AdapFrozenVecPartner
    model = ADAP.load(location, device=device)
    try:
        return AdapFrozenVecPartner(model.policy, latent, model.context_sampler)
    except Exception as e:     # the member's own words (AdapPolicyMult, a latent of another length, ...)
        raise EnvException(str(e)) from e


ADAP_VEC_ENVS = ("RPS-v0", "LiarsDice-v0")


def adap_plan(args):
    """`<env> {PPO,ADAP} {PPO,ADAP} --n-envs E` with at least one ADAP seat: who learns at which seat, whether the partner reads the
    ego's contexts (--share-latent; latent_check has made sure both are ADAP), and --env-config's share -- checked before a device
    is touched.  None when no seat is ADAP, or with a partner list (the pool's plan refuses an ADAP member in its own words)."""
    kinds = [args.ego] + list(args.alt)
    if not any(kind in ADAP_TYPES for kind in kinds):
        return None
    if "ADAP_MULT" in kinds:
        raise EnvException("ADAP_MULT (AdapPolicyMult) has no device-resident form: with --n-envs an ADAP seat is ADAP")
    if len(args.alt) != 1:
        return None
    if args.ego not in ("PPO", "ADAP") or args.alt[0] not in ("PPO", "ADAP"):
        raise EnvException("--n-envs takes ego and partner each from PPO and ADAP when a seat is ADAP, not "
                           f"{args.ego} against {args.alt[0]}")
    if args.env not in ADAP_VEC_ENVS:
        raise EnvException(f"ADAP with --n-envs exists for {' and '.join(ADAP_VEC_ENVS)}, not for the block worlds or {args.env}")
    if args.record is not None:
        raise EnvException("--n-envs cannot be combined with --record when a seat is ADAP: the device-resident recorder logs PPO "
                           "seats")
    log_interval, env_config = vectorised_plan(args)
    return dict(ego=args.ego, alt=args.alt[0], share_latent=bool(args.share_latent), log_interval=log_interval,
                env_config=env_config)


def vectorised_record_check(args) -> None:
    """what `--n-envs` cannot combine with, by name, before a device is touched.  `--record` is the device-resident move log of
    the Liar's Dice step (envs/vec.py: VecLiarStep.start_recording); frame stacking changes every kernel's shape class"""
    if args.framestack > 1:
        raise EnvException("--n-envs cannot be combined with --framestack")
    if args.record is not None and args.env != "LiarsDice-v0":
        raise EnvException(f"--n-envs cannot be combined with --record for {args.env}: the device-resident recorder exists for "
                           "LiarsDice-v0")


def record_capacity(iterations: int, n_steps: int) -> int:
    """rows per table a training run can log: at most 3 moves per vectorised step, plus the first deal's opening"""
    return 3 * int(iterations) * int(n_steps) + 1


def run_pool(args, plan):
    """the pool's object graph: the ego, one member per partner argument, `VecLiarPartnerPool.rollout_and_learn` per iteration
    (`liar_pool_for`: the tower pool where the ego, a learner or a FIXED PPO checkpoint has policy_kwargs net_arch, the ADAP pool
    where a FIXED member is an ADAP checkpoint under a latent_val)"""
    import random as _random

    import torch as th

    from .envs.vec import (ClonedVecPartner, VecLiarDefaultPartner, VecLiarsDice, frozen_partner_for, liar_pool_for,
                           ragged_agent_for)
    from .vec import vec_agent_for
    E = int(args.n_envs)
    spaces = type("Spaces", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                                     _is_dummy_space_env=True))()

    def learner(config, offset):
        config = dict(config)
        config.setdefault("n_steps", 128)
        config.setdefault("batch_size", max(64, E * config["n_steps"] // 4))
        config.update(env=spaces, device=args.device, n_envs=E)
        if args.seed is not None:
            config["seed"] = args.seed + offset
        model = PPO(policy="MlpPolicy", **config)
        model.device_permutations = True
        return model

    ego_model = learner(args.ego_config, 0)
    ego = vec_agent_for(ego_model)
    members, models = [], []
    for i, (kind, config) in enumerate(plan["members"]):
        if kind == "PPO":
            models.append(learner(config, i + 1))
            members.append(ragged_agent_for(models[-1]))
        elif kind == "FIXED":
            if config["type"] == "ADAP":
                members.append(load_adap_member(config["location"], config["latent_val"], config.get("device", args.device)))
            else:
                seat = ClonedVecPartner if config["type"] == "BC" else frozen_partner_for
                members.append(seat(gen_load(config, config["type"], config["location"]).policy))
        else:
            members.append(VecLiarDefaultPartner())
        print(f"Partner {i}: {members[-1]}")
    base = args.seed if args.seed is not None else _random.SystemRandom().randrange(2 ** 31)
    dice_seed = ((base * 0x9E3779B97F4A7C15) ^ 0xD1CE0D1CE0D1CE) & 0x7FFFFFFFFFFFFFFF
    n_steps = ego_model.n_steps
    iterations = max(1, -(-args.total_timesteps // (E * n_steps)))
    record = record_capacity(iterations, n_steps) if args.record is not None else 0
    env = liar_pool_for(E, ego, members, seed=dice_seed, resample=plan["resample"], record=record, **plan["env_config"])
    log = EpisodeLog(args, ego_model, ego, env, plan["log_interval"])
    for it in range(1, iterations + 1):
        env.rollout_and_learn(n_steps)
        log.after(it, it == iterations)
    th.cuda.synchronize()
    if record:
        from .envs.vec import write_recording
        write_recording(env, args.record)
    updates = [m.iteration for m in env.learners]
    print(f"vectorised pool play: {iterations} iterations x {E} envs x {n_steps} steps against {len(members)} members; "
          f"ego updates {ego.iteration}, learner updates {updates}")
    if args.ego_save:
        ego_model.save(args.ego_save)
    if args.alt_save:
        for i, (kind, _) in enumerate(plan["members"]):
            if kind == "PPO":       # FIXED / DEFAULT members have nothing to save (trainer.py:423-432)
                members[i].model.save(f"{args.alt_save}/{i}" if len(models) > 1 else args.alt_save)
    return ego_model, members, env


def run_block_pool(args, plan):
    """`BlockEnv-v0|v1 PPO <alt>+ --partner-pool --n-envs E`: the planner, one constructor per partner argument,
    `VecBlockPartnerPool.rollout_and_learn` per iteration.  Learners are saved to `--alt-save DIR/i` whenever the pool has more
    than one member, as the host path does."""
    import random as _random

    import torch as th

    from . import _native as nat
    from .envs.vec import (FrozenVecPartner, RaggedVecOnPolicyAgent, VecBlockPartnerPool, VecBlockScriptedPartner, VecBlockWorld,
                           check_block_pool_seat)
    from .vec import VecOnPolicyAgent
    E, variant = int(args.n_envs), plan["block_variant"]
    seat_spaces = VecBlockWorld.seat_spaces(variant)

    def learner(config, seat, offset):
        config = dict(config)
        config.setdefault("n_steps", 128)
        config.setdefault("batch_size", max(64, E * config["n_steps"] // 4))
        config.update(env=seat_spaces[seat], device=args.device, n_envs=E)
        if args.seed is not None:
            config["seed"] = args.seed + offset
        model = PPO(policy="MlpPolicy", **config)
        model.device_permutations = True
        return model

    ego_model = learner(args.ego_config, 0, 0)
    ego = VecOnPolicyAgent(ego_model)
    members = []
    try:
        for i, (kind, config) in enumerate(plan["members"]):
            if kind == "PPO":
                members.append(RaggedVecOnPolicyAgent(learner(config, 1, i + 1)))
            elif kind == "FIXED":
                members.append(FrozenVecPartner(gen_load(config, config["type"], config["location"]).policy))
                check_block_pool_seat(members[-1], variant, 1, f"FIXED member {i} ({config['location']})")
            else:
                members.append(VecBlockScriptedPartner(variant, config["rule"]))
            print(f"Partner {i}: {members[-1]}")
        base = args.seed if args.seed is not None else _random.SystemRandom().randrange(2 ** 31)
        world_seed = ((base * 0x9E3779B97F4A7C15) ^ 0xB10CB10CB10C) & 0x7FFFFFFFFFFFFFFF      # a Philox key of the worlds' own
        env = VecBlockPartnerPool(variant, E, ego, members, seed=world_seed, resample=plan["resample"], **plan["env_config"])
    except nat.NativeError as e:
        raise EnvException(str(e)) from e
    n_steps = ego_model.n_steps
    iterations = max(1, -(-args.total_timesteps // (E * n_steps)))
    log = EpisodeLog(args, ego_model, ego, env, plan["log_interval"])
    for it in range(1, iterations + 1):
        env.rollout_and_learn(n_steps)
        log.after(it, it == iterations)
    th.cuda.synchronize()
    updates = [m.iteration for m in env.learners]
    print(f"vectorised pool play: {iterations} iterations x {E} envs x {n_steps} steps against {len(members)} constructors; "
          f"ego updates {ego.iteration}, learner updates {updates}")
    if args.ego_save:
        ego_model.save(args.ego_save)
    if args.alt_save:
        for i, (kind, _) in enumerate(plan["members"]):
            if kind == "PPO":       # FIXED / DEFAULT members have nothing to save (trainer.py:423-432)
                members[i].model.save(f"{args.alt_save}/{i}" if len(members) > 1 else args.alt_save)
    return ego_model, members, env


def run_vectorised(args):
    """`<env> PPO PPO --n-envs E`: the reference's object graph with every table on the device.
    total_timesteps counts ego transitions over all tables, as SB3 does for a VecEnv.  `LiarsDice-v0 PPO <alt>+` with any other
    partner list (each of PPO / FIXED / DEFAULT) plays against the partner pool (`run_pool`)."""
    import torch as th

    from .envs.vec import VecLiarsDice, VecLiarSelfPlay, VecRPS, ragged_agent_for, selfplay_iteration
    from .vec import vec_agent_for
    vectorised_record_check(args)
    partner_pool_check(args)
    aplan = adap_plan(args)                    # an ADAP learner in either seat of the single-partner pairing
    plan = pool_plan(args) if aplan is None else None
    if plan is not None:
        return run_block_pool(args, plan) if plan["block_variant"] is not None else run_pool(args, plan)
    log_interval, env_config = vectorised_plan(args)
    if args.ego != "PPO" and aplan is None:
        raise EnvException("--n-envs supports the PPO-vs-PPO self-play pairing")
    block_variant = BLOCK_VARIANTS.get(args.env)
    game = {"RPS-v0": VecRPS, "LiarsDice-v0": VecLiarsDice}.get(args.env)
    if game is None and block_variant is None:
        raise EnvException(f"no device-resident form of {args.env}")
    E = int(args.n_envs)
    if block_variant is not None:      # the planner and the constructor have spaces of their own
        from .envs.vec import VecBlockSelfPlay, VecBlockWorld
        seat_spaces = VecBlockWorld.seat_spaces(block_variant)
    else:
        spaces = type("Spaces", (), dict(observation_space=game.observation_space, action_space=game.action_space,
                                         _is_dummy_space_env=True))()
        seat_spaces = (spaces, spaces)
    models = []
    kinds = (aplan["ego"], aplan["alt"]) if aplan is not None else ("PPO", "PPO")
    for offset, config in enumerate((dict(args.ego_config), dict(args.alt_config[0]))):
        spaces = seat_spaces[offset]
        config.setdefault("n_steps", 128)
        config.setdefault("batch_size", max(64, E * config["n_steps"] // 4))
        config.update(env=spaces, device=args.device, n_envs=E)
        if args.seed is not None:
            config["seed"] = args.seed + offset
        model = ADAP(policy=AdapPolicy, **config) if kinds[offset] == "ADAP" else PPO(policy="MlpPolicy", **config)
        model.device_permutations = True
        models.append(model)
    ego = vec_agent_for(models[0])
    syncer = ego if aplan is not None and aplan["share_latent"] else None     # --share-latent: the partner reads the ego's contexts
    n_steps = models[0].n_steps
    iterations = max(1, -(-args.total_timesteps // (E * n_steps)))
    if args.env == "RPS-v0":
        alt = vec_agent_for(models[1], latent_syncer=syncer)
        env = VecRPS(E, models[0].policy.ctx, models[0].device)
        log = EpisodeLog(args, models[0], ego, env, log_interval)
        for it in range(1, iterations + 1):
            selfplay_iteration(env, ego, alt, n_steps)
            log.after(it, it == iterations)
    elif block_variant is not None:
        alt = ragged_agent_for(models[1])
        import random as _random
        base = args.seed if args.seed is not None else _random.SystemRandom().randrange(2 ** 31)
        world_seed = ((base * 0x9E3779B97F4A7C15) ^ 0xB10CB10CB10C) & 0x7FFFFFFFFFFFFFFF      # a Philox key of the worlds' own
        env = VecBlockSelfPlay(block_variant, E, ego, alt, seed=world_seed, **env_config)
        log = EpisodeLog(args, models[0], ego, env, log_interval)
        for it in range(1, iterations + 1):
            env.rollout_and_learn(n_steps)
            log.after(it, it == iterations)
    else:
        alt = ragged_agent_for(models[1], latent_syncer=syncer)
        # the dice get a Philox key of their own: keyed by the bare seed they would BE the ego's sampling uniforms (same key,
        # same step counter, same row); without --seed every run deals a fresh sequence
        import random as _random
        base = args.seed if args.seed is not None else _random.SystemRandom().randrange(2 ** 31)
        dice_seed = ((base * 0x9E3779B97F4A7C15) ^ 0xD1CE0D1CE0D1CE) & 0x7FFFFFFFFFFFFFFF
        record = record_capacity(iterations, n_steps) if args.record is not None else 0     # recording runs launch by launch
        env = VecLiarSelfPlay(E, ego, alt, seed=dice_seed, record=record, **env_config)
        log = EpisodeLog(args, models[0], ego, env, log_interval)       # in front of the graph: its scan is captured with the update
        if iterations >= 4 and env.native and not env.adap:
            # two launch-by-launch iterations size the workspaces, the rest replay one hipGraph per iteration
            from .envs.vec import LiarIterationGraph
            graph = LiarIterationGraph(env, n_steps, warmup=2)
            log.after(2)                              # the two warm-up iterations ran inside the constructor: one record for both
            for it in range(3, iterations + 1):
                graph.launch()
                log.after(it, it == iterations)       # a read lands between two replays
        else:
            for it in range(1, iterations + 1):
                env.rollout_and_learn(n_steps)
                log.after(it, it == iterations)
    th.cuda.synchronize()
    print(f"vectorised self-play: {iterations} iterations x {E} envs x {n_steps} steps; "
          f"ego updates {ego.iteration}, partner updates {alt.iteration}")
    if args.record is not None:
        from .envs.vec import write_recording
        write_recording(env, args.record)
    if args.ego_save:
        models[0].save(args.ego_save)
    if args.alt_save:
        models[1].save(args.alt_save)
    return models[0], [alt], env


def parse_cli(argv=None):
    """argv -> the checked and completed arguments, in the order of the reference's main (trainer.py:395-403): parse, preset,
    input_check, latent_check when --share-latent"""
    args = build_parser().parse_args(argv)
    args.ego_config, args.env_config = dict(args.ego_config), dict(args.env_config)     # (argparse hands out its default objects)
    if args.preset:
        args = preset(args, args.preset)
    input_check(args)
    if args.share_latent:
        latent_check(args)
    return args


def run(argv=None):
    """parse, build the graph, learn, save -- returns (ego, partners, env) for callers and tests"""
    args = parse_cli(argv)
    print(f"Arguments: {args}")
    if args.n_envs > 1:
        return run_vectorised(args)
    partner_pool_check(args)
    env, altenv = generate_env(args)
    print(f"Environment: {env}; Partner env: {altenv}")
    ego = generate_ego(env, args)
    print(f"Ego: {ego}")
    partners = generate_partners(altenv, env, ego, args)
    learn_config = {"total_timesteps": args.total_timesteps}
    if args.tensorboard_log:
        learn_config["tb_log_name"] = args.tensorboard_name
    ego.learn(**learn_config)
    if args.record is not None:
        env.get_transitions().write_transition(args.record)   # trainer.py:415-417
    if args.ego_save:
        ego.save(args.ego_save)
    if args.alt_save:
        multiple = len(partners) > 1
        for i, partner in enumerate(partners):
            model = getattr(partner, "model", None)
            if model is None:           # DEFAULT / FIXED partners have nothing to save (trainer.py:423-432)
                continue
            model.save(f"{args.alt_save}/{i}" if multiple else args.alt_save)
    return ego, partners, env


if __name__ == "__main__":
    run()
