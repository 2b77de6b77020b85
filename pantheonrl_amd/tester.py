"""`tester.py` of the reference (tester.py:1-198) on the engine: play a loaded ego against a loaded or default partner.

    python -m pantheonrl_amd.tester RPS-v0 PPO DEFAULT --ego-load models/ego --alt-config '{"r": 1}' -t 100 [--record FILE]

Same positional arguments and flags (`--render` is accepted and ignored: the in-tree games draw nothing).  Ego types: PPO, ADAP
(with `--ego-config '{"latent_val": [...]}'`), BC; partner types: the same plus DEFAULT.

    python -m pantheonrl_amd.tester LiarsDice-v0 PPO DEFAULT --ego-load models/ego --n-envs 256 -t 10000

`--n-envs E` (E > 1) plays the pair on E device-resident tables (envs/crossplay.py): LiarsDice-v0, a PPO ego against a PPO or
DEFAULT partner, ceil(t / E) games per table; the two lines above are printed over all the games played, then their number.
The command line still refuses `--record` there; `run_vectorised` called with `args.record` set writes the tables' move streams,
concatenated in table order, in the reference's format, and `python -m pantheonrl_amd.crossplay ... --record FILE` is its CLI."""
from __future__ import annotations

import argparse
import json
from typing import List

import numpy as np

from .common import StaticPolicyAgent
from .trainer import EnvException, gen_load, gen_partner, generate_env

EGO_LIST = ["PPO", "BC", "ADAP"]
PARTNER_LIST = ["PPO", "DEFAULT", "BC", "ADAP"]


def input_check(args) -> None:
    """tester.py:14-31"""
    if args.ego not in EGO_LIST or args.alt not in PARTNER_LIST:
        raise EnvException(f"ego must be one of {EGO_LIST}, alt one of {PARTNER_LIST}")
    args.ego_config.setdefault("verbose", 1)
    if args.ego_load is None:
        raise EnvException("Need to provide file for ego to load")
    if (args.alt_load is None) != (args.alt == "DEFAULT"):
        raise EnvException("Load policy if and only if alt is not DEFAULT")


def generate_agent(env, policy_type: str, config: dict, location, args):
    """tester.py:34-38: the environment's default agent, or a fixed agent around the loaded policy"""
    if policy_type == "DEFAULT":
        return gen_partner("DEFAULT", config, env, None, args, 0)
    cfg = {k: v for k, v in config.items() if k != "verbose"}
    cfg.setdefault("device", args.device)
    return StaticPolicyAgent(gen_load(cfg, policy_type, location).policy)


def run_test(ego, env, num_episodes: int) -> List[float]:
    """tester.py:41-63"""
    env.set_ego_extractor(lambda obs: obs)
    rewards = []
    for _ in range(num_episodes):
        obs, done, reward = env.reset(), False, 0.0
        while not done:
            action = ego.get_action(obs, False)
            obs, newreward, done, _ = env.step(action)
            reward += newreward
        rewards.append(reward)
    print(f"Average Reward: {sum(rewards) / num_episodes}")
    print(f"Standard Deviation: {np.std(rewards)}")
    return rewards


def vectorised_check(args) -> None:
    """what `--n-envs E` cannot evaluate, by name, before a device is touched"""
    if args.n_envs < 1:
        raise EnvException("--n-envs must be at least 1")
    if args.env != "LiarsDice-v0":
        raise EnvException(f"--n-envs: the device-resident evaluation exists for LiarsDice-v0, not {args.env}")
    if args.ego != "PPO" or args.alt not in ("PPO", "DEFAULT"):
        raise EnvException(f"--n-envs evaluates a PPO ego against a PPO or DEFAULT partner, not {args.ego} against {args.alt}")
    if args.framestack > 1:
        raise EnvException("--n-envs cannot be combined with --framestack")
    if args.record is not None:
        # tests/test_crossplay_host.py pins this refusal of the command line; `run_vectorised` itself records (args.record), and
        # so does `python -m pantheonrl_amd.crossplay ... --record FILE`
        raise EnvException("--n-envs cannot be combined with --record on this command line: record device-resident evaluation "
                           "games with `python -m pantheonrl_amd.crossplay LiarsDice-v0 --agents ... --record FILE`")
    if args.alt == "DEFAULT" and args.alt_config:
        raise EnvException("No config possible for the DEFAULT partner")
    if set(args.env_config) - {"probegostart"}:
        raise EnvException(f"--n-envs: LiarsDice-v0 takes probegostart only, not {sorted(set(args.env_config) - {'probegostart'})}")


def load_member(policy_type: str, config: dict, location, device, towers: bool = False):
    """a seat of the device-resident evaluation: the scripted player, a behavioural clone saved by bctrainer ("BC": reached
    through `python -m pantheonrl_amd.crossplay ... --agents BC:<path>`; `tester ... BC ... --n-envs` stays refused on this command
    line), or a frozen loaded PPO policy.  `towers`: a checkpoint trained with policy_kwargs net_arch is seated as
    TowerFrozenVecPartner (the crossplay command line passes it; `tester ... --n-envs` keeps FrozenVecPartner's refusal)"""
    from .envs.vec import ClonedVecPartner, FrozenVecPartner, VecLiarDefaultPartner, frozen_partner_for
    if policy_type == "DEFAULT":
        return VecLiarDefaultPartner()
    if policy_type == "BC":
        from .bc import reconstruct_policy
        return ClonedVecPartner(reconstruct_policy(location, device))
    cfg = {k: v for k, v in config.items() if k != "verbose"}
    cfg.setdefault("device", device)
    return (frozen_partner_for if towers else FrozenVecPartner)(gen_load(cfg, "PPO", location).policy)


def run_vectorised(args) -> List[float]:
    """tester.py:41-63 on E tables: one (ego, partner) pair, ceil(t / E) games per table"""
    from .envs.crossplay import MAX_STEPS_PER_GAME, VecLiarCrossPlay
    E = args.n_envs
    G = -(-args.total_episodes // E)
    ego = load_member(args.ego, args.ego_config, args.ego_load, args.device)
    alt = load_member(args.alt, args.alt_config, args.alt_load, args.device)
    print(f"Ego: {ego}")
    print(f"Alt: {alt}")
    # --record: the device-resident move log; a game takes at most MAX_STEPS_PER_GAME steps of at most 3 moves
    record = 3 * MAX_STEPS_PER_GAME * G if args.record is not None else 0
    xp = VecLiarCrossPlay(E, [ego, alt], pairs=[(0, 1)], episodes_per_table=G, seed=args.seed or 0, record=record, **args.env_config)
    res = xp.run()
    if record:
        from .envs.vec import write_recording
        write_recording(xp, args.record)
    print(f"Average Reward: {res.mean[0]}")
    print(f"Standard Deviation: {res.std[0]}")
    print(f"Games played: {int(res.count[0])} ({E} tables x {G} games)")
    return res.returns.reshape(-1).tolist()


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Test ego and partner in an environment (flags as in PantheonRL's tester.py)")
    p.add_argument("env")
    p.add_argument("ego")
    p.add_argument("alt")
    p.add_argument("--total-episodes", "-t", type=int, default=100)
    p.add_argument("--device", "-d", default="cuda")
    p.add_argument("--seed", "-s", type=int)
    p.add_argument("--ego-config", type=json.loads, default={})
    p.add_argument("--alt-config", type=json.loads, default={})
    p.add_argument("--env-config", type=json.loads, default={})
    p.add_argument("--framestack", "-f", type=int, default=1)
    p.add_argument("--record", "-r")
    p.add_argument("--render", action="store_true")
    p.add_argument("--ego-load")
    p.add_argument("--alt-load")
    p.add_argument("--n-envs", type=int, default=1,
                   help="E > 1: play the pair on E device-resident tables (LiarsDice-v0, PPO ego, PPO or DEFAULT partner)")
    return p


def run(argv=None) -> List[float]:
    args = build_parser().parse_args(argv)
    input_check(args)
    args.tensorboard_log, args.tensorboard_name, args.verbose_partner = None, None, False
    if args.seed is not None:
        np.random.seed(args.seed)
    if args.n_envs != 1:
        vectorised_check(args)
    print(f"Arguments: {args}")
    if args.n_envs != 1:
        return run_vectorised(args)
    env, altenv = generate_env(args)
    print(f"Environment: {env}; Partner env: {altenv}")
    ego = generate_agent(env, args.ego, args.ego_config, args.ego_load, args)
    print(f"Ego: {ego}")
    alt = generate_agent(altenv, args.alt, args.alt_config, args.alt_load, args)
    env.add_partner_agent(alt)
    print(f"Alt: {alt}")
    rewards = run_test(ego, env, args.total_episodes)
    if args.record is not None:
        env.get_transitions().write_transition(args.record)
    return rewards


if __name__ == "__main__":
    run()
