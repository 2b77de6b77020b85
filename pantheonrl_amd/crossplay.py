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
padding."""
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
    p.add_argument("--n-envs", type=int, default=256)
    p.add_argument("--games", "-t", type=int, default=1000, help="games per pair")
    p.add_argument("--device", "-d", default="cuda")
    p.add_argument("--seed", "-s", type=int, default=0)
    p.add_argument("--probegostart", type=float, default=0.5)
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


def plan(args) -> dict:
    """check the arguments and size the evaluation, before a device is touched"""
    if args.env != "LiarsDice-v0":
        raise EnvException(f"the device-resident cross-play exists for LiarsDice-v0, not {args.env}")
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


def run(argv=None):
    args = build_parser().parse_args(argv)
    size = plan(args)
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
