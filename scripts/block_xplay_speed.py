"""games per second of the cross-play evaluation of the block worlds (envs/crossplay.py: VecBlockCrossPlay): E = 256 tables, every
pair of M freshly initialised planners with M constructors (frozen, DEFAULT, frozen, EASY for BlockEnv-v0 / DEFAULT for BlockEnv-v1,
the first M of them), G games per table under the default step cap:
  native  one ph_block_xplay_step per step (two grouped forwards whatever M is)
  walk    the same evaluation through per-member forwards and torch masks (native=False)
  host    tester.run_test of ONE planner with ONE frozen constructor on the host game -- one table, one policy round trip per move
Median of 5 runs per variant, the variants alternating within a round, after one warm-up round; the host clock around a device
synchronise; a run is `run()` (the steps, the reads of tables_left, the statistics kernel and the copy of the logs), not the
construction.  A fresh planner says its last token with probability 1/16 (v0) or 1/30 (v1) per turn, so games are long; games that
the cap cuts off are not counted.  `--ms 1,4`, `--games G`, `--envs 0,1`, `--no-host`, `--out FILE`."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.common import StaticPolicyAgent  # noqa: E402
from pantheonrl_amd.envs.blockworld import BlockEnv, SimpleBlockEnv  # noqa: E402
from pantheonrl_amd.envs.crossplay import VecBlockCrossPlay  # noqa: E402
from pantheonrl_amd.envs.vec import FrozenVecPartner, VecBlockScriptedPartner, VecBlockWorld  # noqa: E402
from pantheonrl_amd.tester import run_test  # noqa: E402

E, ROUNDS = 256, 5
_p = argparse.ArgumentParser()
_p.add_argument("--ms", default="1,2,4")
_p.add_argument("--envs", default="0,1")
_p.add_argument("--games", type=int, default=8)
_p.add_argument("--host-games", type=int, default=256)
_p.add_argument("--no-host", action="store_true")
_p.add_argument("--out")
_args = _p.parse_args()
MS, G = [int(m) for m in _args.ms.split(",")], _args.games
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def device_run(variant, pols, M, native, seed):
    planners = [FrozenVecPartner(p) for p in pols[0][:M]]
    last = VecBlockScriptedPartner(0, "EASY") if variant == 0 else VecBlockScriptedPartner(1, "DEFAULT")
    constructors = [FrozenVecPartner(pols[1][0]), VecBlockScriptedPartner(variant, "DEFAULT"), FrozenVecPartner(pols[1][1]), last][:M]
    xp = VecBlockCrossPlay(variant, E, planners, constructors, games=G, seed=seed, native=native)
    th.cuda.synchronize()
    t0 = time.perf_counter()
    res = xp.run()
    th.cuda.synchronize()
    dt = time.perf_counter() - t0
    return res.count.sum() / dt, res.steps, res.unfinished, 1e6 * dt / res.steps


def host_run(variant, pols, n_games):
    env = (SimpleBlockEnv, BlockEnv)[variant]()
    env.add_partner_agent(StaticPolicyAgent(pols[1][0]))
    ego = StaticPolicyAgent(pols[0][0])
    th.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        rewards = run_test(ego, env, n_games)
    th.cuda.synchronize()
    return len(rewards) / (time.perf_counter() - t0)


for variant in [int(v) for v in _args.envs.split(",")]:
    seats = VecBlockWorld.seat_spaces(variant)
    pols = [[PPO("MlpPolicy", seats[s], n_steps=2, n_envs=4, batch_size=8, n_epochs=1, seed=10 + 10 * s + k).policy for k in range(4)]
            for s in (0, 1)]
    names = [f"native M={M}" for M in MS] + [f"walk   M={M}" for M in MS]
    say(f"cross-play evaluation of BlockEnv-v{variant}, E = {E} tables, all M x M planner x constructor pairs, {G} games per table = "
        f"{E * G} games per run, step cap {200 * G} (host: {_args.host_games} games per run); median of {ROUNDS} runs, variants "
        f"alternating, after one warm-up round")
    rate, us, steps, cut = ({n: [] for n in names} for _ in range(4))
    host = []
    for rnd in range(ROUNDS + 1):
        for name in names:
            M = int(name.split("=")[1])
            r, n, unfinished, u = device_run(variant, pols, M, name.startswith("native"), 100 + rnd)
            if rnd:
                rate[name].append(r)
                us[name].append(u)
                steps[name].append(n)
                cut[name].append(unfinished)
        if not _args.no_host:
            if rnd == 0:
                host_run(variant, pols, 16)          # warm-up: a short run is enough for a per-move loop
            else:
                host.append(host_run(variant, pols, _args.host_games))
    for name in names:
        say(f"{name}: {statistics.median(rate[name]):,.0f} games/s (min {min(rate[name]):,.0f}, max {max(rate[name]):,.0f}); "
            f"{statistics.median(us[name]):.1f} us per vectorised step (min {min(us[name]):.1f}, max {max(us[name]):.1f}); steps per run "
            f"{min(steps[name])}..{max(steps[name])}; unfinished games {min(cut[name])}..{max(cut[name])}")
    for M in MS:
        say(f"M={M}: native over walk {statistics.median(us[f'walk   M={M}']) / statistics.median(us[f'native M={M}']):.2f}x per step")
    if host:
        h = statistics.median(host)
        say(f"host   tester.run_test, planner 0 with frozen constructor 0: {h:,.0f} games/s (min {min(host):,.0f}, max {max(host):,.0f})")
        for M in MS:
            say(f"M={M}: native over the host loop {statistics.median(rate[f'native M={M}']) / h:,.0f}x")
if _args.out:
    with open(_args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
