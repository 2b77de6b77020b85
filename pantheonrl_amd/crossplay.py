"""Cross-play of a population of saved agents, every table on the device (envs/crossplay.py): every agent as the ego against
every agent as the partner -- the M x M matrix the reference reaches only as M^2 separate runs of tester.py (tester.py:41-63).

    python -m pantheonrl_amd.crossplay LiarsDice-v0 --agents models/a BC:models/clone.pt DEFAULT --n-envs 256 -t 1000 [--out x.npz]

An agent is a PPO checkpoint (64-64 MlpPolicy), BC:<path> (a FeedForward32Policy saved by bctrainer: the cloned "human proxy"),
ADAP:<path>@<v1,v2,...> (an ADAP checkpoint under that latent: the reference's FIXED ADAP partner with latent_val,
trainer.py:140-147), ADAP:<path>@sample (the same checkpoint with a context per table, redrawn with its own sampler at every deal)
or DEFAULT (the game's scripted player).  `-t` is the number of games per pair:
table e plays pair e % P, so a pair owns at least n_envs // P tables and every table plays ceil(t / (n_envs // P)) games.  Prints
the mean and standard-deviation matrices of the ego's return (row = ego, column = partner); `--out` writes them, with the counts,
mean lengths and the raw logs, as an .npz.  `--record FILE` logs every move on the device (envs/vec.py: VecLiarStep.start_recording)
and writes the tables' streams, concatenated in table order, in the reference's recording format; `--out` then also holds
`table_offsets` (table e's rows of the recording), `member` (who made each move) and `pair_of_table`.  With an ADAP agent `--out`
also holds `latents` (M, widest context): each ADAP agent's stated latent, NaN for a sampled one, for the other agents and in the
padding.

    python -m pantheonrl_amd.crossplay BlockEnv-v0 --agents m/plan1 m/plan2 --partners m/build1 DEFAULT EASY --n-envs 256 -t 1000

The block worlds (BlockEnv-v0, BlockEnv-v1) have different spaces per seat: `--agents` are the planners (PPO checkpoints),
`--partners` the constructors -- PPO checkpoints, DEFAULT (the game's scripted constructor) or, for BlockEnv-v0, EASY
(SBWEasyPartner).  Every planner plays every constructor; the matrices are planner x constructor.  A game ends only when the planner
says its last token, so the run stops after `--max-steps` steps (default 200 per game of a table's budget), warns about the games
that did not finish and reports the statistics of those that did; `--out` holds `mean`, `std`, `count`, `length`, `unfinished`,
`pairs`, `pair_of_table`, `games` and the logs.  `--record` and `--probegostart` belong to LiarsDice-v0."""
from __future__ import annotations

import argparse

import numpy as np

from . import _native as nat
from .trainer import EnvException


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Cross-play matrix of saved agents on device-resident tables")
    p.add_argument("env")
    p.add_argument("--agents", nargs="+", required=True,
                   help="PPO checkpoints, BC:<path> for a policy saved by bctrainer, ADAP:<path>@<v1,v2,...> or ADAP:<path>@sample for an "
                        "ADAP checkpoint under a stated or a per-table sampled latent, or DEFAULT for the scripted player")
    p.add_argument("--partners", nargs="+",
                   help="BlockEnv-v0 / BlockEnv-v1 only: the constructors -- PPO checkpoints, DEFAULT for the scripted constructor, or "
                        "(BlockEnv-v0) EASY for SBWEasyPartner; --agents are then the planners")
    p.add_argument("--n-envs", type=int, default=256)
    p.add_argument("--games", "-t", type=int, default=1000, help="games per pair")
    p.add_argument("--max-steps", type=int, help="BlockEnv-v0 / BlockEnv-v1 only: stop after this many steps (default 200 per game of "
                                                 "a table's budget) and report the games that did not finish")
    p.add_argument("--device", "-d", default="cuda")
    p.add_argument("--seed", "-s", type=int, default=0)
    p.add_argument("--probegostart", type=float, help="LiarsDice-v0 only (default 0.5)")
    p.add_argument("--out", help="write the matrices and logs to this .npz")
    p.add_argument("--record", "-r", help="write every move of every table to this .npy (TurnBasedTransitions format)")
    return p


def parse_agent(agent: str):
    """one --agents entry -> (type, location): DEFAULT -> ("DEFAULT", None), BC:<path> -> ("BC", path),
    ADAP:<path>@<v1,v2,...> -> ("ADAP", (path, [v1, v2, ...])), ADAP:<path>@sample -> ("ADAP", (path, "sample")), anything else a PPO
    checkpoint -> ("PPO", path).  No file is touched."""
    if agent == "DEFAULT":
        return "DEFAULT", None
    if agent.startswith("ADAP:"):
        form = "ADAP:<path>@<v1,v2,...> (a latent of context_size numbers) or ADAP:<path>@sample"
        path, at, latent = agent[5:].rpartition("@")
        if not at or not path or not latent:
            raise EnvException(f"--agents {agent}: an ADAP checkpoint plays under a latent: {form}")
        if latent == "sample":
            return "ADAP", (path, "sample")
        try:
            values = [float(v) for v in latent.split(",")]
        except ValueError:
            raise EnvException(f"--agents {agent}: the latent is not a list of numbers: {form}") from None
        from .trainer import check_adap_latent
        return "ADAP", (path, check_adap_latent(values, f"--agents {agent}: the latent"))
    if agent.startswith("BC:"):
        if len(agent) == 3:
            raise EnvException("--agents BC: needs the path of a policy saved by bctrainer (BC:<path>)")
        return "BC", agent[3:]
    return "PPO", agent


BLOCK_ENVS = {"BlockEnv-v0": 0, "BlockEnv-v1": 1}


def parse_block_member(entry: str, seat: int, env: str):
    """one --agents (seat 0: a planner) or --partners (seat 1: a constructor) entry of a block world -> (type, location):
    ("PPO", path), or for a constructor ("DEFAULT", None) / ("EASY", None).  No file is touched."""
    flag = ("--agents", "--partners")[seat]
    for prefix, what in (("BC:", "a BC clone"), ("ADAP:", "an ADAP checkpoint")):
        if entry.startswith(prefix):
            raise EnvException(f"{flag} {entry}: {what} does not sit in the block worlds' cross-play (frozen PPO checkpoints and, as "
                               "constructors, DEFAULT / EASY do)")
    if entry in ("DEFAULT", "EASY"):
        if seat == 0:
            raise EnvException(f"--agents {entry}: the planners of {env} are PPO checkpoints; the scripted constructors go to --partners")
        if entry == "EASY" and env != "BlockEnv-v0":
            raise EnvException(f"--partners EASY: SBWEasyPartner exists for BlockEnv-v0 only, not {env}")
        return entry, None
    return "PPO", entry


def plan_block(args) -> dict:
    """`plan` for BlockEnv-v0 / BlockEnv-v1: planners x constructors"""
    if not args.partners:
        raise EnvException(f"{args.env}: --partners names the constructors (PPO checkpoints, DEFAULT"
                           f"{', EASY' if args.env == 'BlockEnv-v0' else ''}); --agents are the planners")
    if args.record:
        raise EnvException(f"--record exists for LiarsDice-v0, not {args.env}")
    if args.probegostart is not None:
        raise EnvException(f"--probegostart exists for LiarsDice-v0, not {args.env}: the planner always moves first")
    Mp, Mc = len(args.agents), len(args.partners)
    if Mp > nat.PH_MAX_POOL or Mc > nat.PH_MAX_POOL:
        raise EnvException(f"a seat holds at most {nat.PH_MAX_POOL} agents, not {max(Mp, Mc)}")
    if args.games < 1:
        raise EnvException("-t must be at least 1")
    planners = [parse_block_member(a, 0, args.env) for a in args.agents]
    constructors = [parse_block_member(a, 1, args.env) for a in args.partners]
    P = Mp * Mc
    if args.n_envs < P:
        raise EnvException(f"{Mp} planners and {Mc} constructors make {P} pairs: --n-envs must be at least {P}, not {args.n_envs}")
    G = -(-args.games // (args.n_envs // P))
    max_steps = 200 * G if args.max_steps is None else args.max_steps
    if max_steps < 1:
        raise EnvException("--max-steps must be at least 1")
    return dict(variant=BLOCK_ENVS[args.env], n_planners=Mp, n_constructors=Mc, n_pairs=P, episodes_per_table=G, max_steps=max_steps,
                planners=planners, constructors=constructors, pairs=[(i, j) for i in range(Mp) for j in range(Mc)])


def plan(args) -> dict:
    """check the arguments and size the evaluation, before a device is touched"""
    if args.env in BLOCK_ENVS:
        return plan_block(args)
    if args.env != "LiarsDice-v0":
        raise EnvException(f"the device-resident cross-play exists for BlockEnv-v0, BlockEnv-v1, LiarsDice-v0, not {args.env}")
    if args.partners:
        raise EnvException("--partners exists for BlockEnv-v0 / BlockEnv-v1, not LiarsDice-v0: every agent of --agents sits in both seats")
    if args.max_steps is not None:
        raise EnvException("--max-steps exists for BlockEnv-v0 / BlockEnv-v1, not LiarsDice-v0: a game takes at most 7 steps")
    M = len(args.agents)
    if M > nat.PH_MAX_POOL:
        raise EnvException(f"a population holds at most {nat.PH_MAX_POOL} agents, not {M}")
    if args.games < 1:
        raise EnvException("-t must be at least 1")
    for a in args.agents:
        parse_agent(a)
    P = M * M
    if args.n_envs < P:
        raise EnvException(f"{M} agents make {P} pairs: --n-envs must be at least {P}, not {args.n_envs}")
    return dict(n_members=M, n_pairs=P, episodes_per_table=-(-args.games // (args.n_envs // P)))


def run_block(args, size: dict):
    """BlockEnv-v0 / BlockEnv-v1: every planner of --agents with every constructor of --partners"""
    from .envs.crossplay import VecBlockCrossPlay
    from .envs.vec import VecBlockScriptedPartner
    from .tester import load_member
    variant = size["variant"]
    seat = lambda kind, location: (VecBlockScriptedPartner(variant, kind) if kind != "PPO" else  # noqa: E731
                                   load_member("PPO", {}, location, args.device))
    planners = [seat(*m) for m in size["planners"]]
    constructors = [seat(*m) for m in size["constructors"]]
    xp = VecBlockCrossPlay(variant, args.n_envs, planners, constructors, pairs=size["pairs"], games=size["episodes_per_table"],
                           seed=args.seed)
    res = xp.run(max_steps=size["max_steps"])
    with np.printoptions(precision=4, suppress=True, linewidth=160):
        print(f"Planners: {args.agents}")
        print(f"Constructors: {args.partners}")
        print(f"Games per pair: {int(res.count.min())}..{int(res.count.max())} ({args.n_envs} tables x {xp.G} games, {res.steps} steps)")
        print(f"Average Reward (row = planner, column = constructor):\n{res.matrix('mean')}")
        print(f"Standard Deviation:\n{res.matrix('std')}")
    if res.unfinished:
        print(f"WARNING: {res.unfinished} of {args.n_envs * xp.G} games did not finish within {size['max_steps']} steps (a game ends "
              "only when the planner says its last token); the statistics cover the finished games")
    if args.out:
        np.savez(args.out, agents=np.asarray(args.agents), partners=np.asarray(args.partners), mean=res.matrix("mean"),
                 std=res.matrix("std"), count=res.matrix("count"), length=res.matrix("mean_length"), unfinished=np.int64(res.unfinished),
                 pairs=res.pairs, pair_of_table=res.pair_of_table, returns=res.returns, lengths=res.lengths, games=res.games)
    return res


def run(argv=None):
    args = build_parser().parse_args(argv)
    size = plan(args)
    if args.env in BLOCK_ENVS:
        return run_block(args, size)
    if args.probegostart is None:
        args.probegostart = 0.5
    from .envs.crossplay import MAX_STEPS_PER_GAME, VecLiarCrossPlay
    from .tester import load_member
    from .trainer import load_adap_member
    members = [load_adap_member(location[0], location[1], args.device) if kind == "ADAP" else
               load_member(kind, {}, location, args.device, towers=True) for kind, location in map(parse_agent, args.agents)]
    # a game takes at most MAX_STEPS_PER_GAME steps of at most 3 moves
    record = 3 * MAX_STEPS_PER_GAME * size["episodes_per_table"] if args.record else 0
    xp = VecLiarCrossPlay(args.n_envs, members, episodes_per_table=size["episodes_per_table"], seed=args.seed,
                          probegostart=args.probegostart, record=record)
    res = xp.run()
    extra = {}
    if record:
        from .envs.vec import write_recording
        rec = write_recording(xp, args.record)
        extra = dict(table_offsets=rec.table_offsets, member=rec.member.cpu().numpy())
    latents = [getattr(m, "latent", None) for m in members]
    if any(hasattr(m, "context_size") for m in members):
        width = max(m.context_size for m in members if hasattr(m, "context_size"))
        extra["latents"] = np.full((len(members), width), np.nan, np.float32)
        for k, lat in enumerate(latents):
            if lat is not None:
                extra["latents"][k, :lat.size] = lat
    with np.printoptions(precision=4, suppress=True, linewidth=160):
        print(f"Agents: {args.agents}")
        print(f"Games per pair: {int(res.count.min())}..{int(res.count.max())} ({args.n_envs} tables x {xp.G} games, {res.steps} steps)")
        print(f"Average Reward (row = ego, column = partner):\n{res.matrix('mean')}")
        print(f"Standard Deviation:\n{res.matrix('std')}")
    if args.out:
        np.savez(args.out, agents=np.asarray(args.agents), mean=res.matrix("mean"), std=res.matrix("std"), count=res.matrix("count"),
                 mean_length=res.matrix("mean_length"), returns=res.returns, lengths=res.lengths, pair_of_table=res.pair_of_table,
                 pairs=res.pairs, **extra)
    return res


if __name__ == "__main__":
    run()
