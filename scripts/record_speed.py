"""cost of the device-resident move log (csrc/ph_record.h) per vectorised Liar's Dice step, E = 256: self-play launch by launch,
the partner pool at K = 4 and cross-play at M = 4, each with the recorder attached and detached -- the two variants alternate
on ONE environment, BLOCK steps per timed block, median of REPEATS blocks each.  The engine's step alone is timed
(`_native_call`: no updates).  `--detached-only` times the detached variant alone and needs nothing of the recorder, so the same
script gives the figures of a tree without it; `--out FILE` also writes the lines to FILE."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay  # noqa: E402
from pantheonrl_amd.envs.vec import (FrozenVecPartner, RaggedVecOnPolicyAgent, VecLiarDefaultPartner, VecLiarPartnerPool,  # noqa: E402
                                     VecLiarSelfPlay, VecLiarsDice)
from pantheonrl_amd.vec import VecOnPolicyAgent  # noqa: E402

E, T, BLOCK, REPEATS = 256, 128, 64, 7
_p = argparse.ArgumentParser()
_p.add_argument("--detached-only", action="store_true")
_p.add_argument("--out")
_args = _p.parse_args()
spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def model(seed, n_envs=E):
    m = PPO("MlpPolicy", spaces, n_steps=T, n_envs=n_envs, batch_size=n_envs * T // 4, n_epochs=10, seed=seed)
    m.device_permutations = True
    return m


def selfplay():
    ego, alt = VecOnPolicyAgent(model(0)), RaggedVecOnPolicyAgent(model(1))
    sp = VecLiarSelfPlay(E, ego, alt, seed=3)
    return sp, lambda c: sp._native_call(c, ego_pos=c % T), lambda: alt.pos.zero_()


def pool():
    ego = VecOnPolicyAgent(model(0))
    members = [RaggedVecOnPolicyAgent(model(1 + k)) for k in range(4)]
    sp = VecLiarPartnerPool(E, ego, members, seed=3)

    def rewind():
        for m in members:
            m.pos.zero_()
    return sp, lambda c: sp._native_call(c, ego_pos=c % T), rewind


def crossplay():
    members = [FrozenVecPartner(model(k, 4).policy) for k in range(3)] + [VecLiarDefaultPartner()]
    xp = VecLiarCrossPlay(E, members, episodes_per_table=4096, seed=3)      # no table spends its budget inside the measurement
    return xp, lambda c: xp._native_call(c), lambda: None


def measure(name, build):
    env, step, rewind = build()
    variants = ("detached",) if _args.detached_only else ("detached", "attached")
    times = {v: [] for v in variants}
    c = 0
    for block in range(-2, REPEATS):                       # two warm-up rounds size the workspaces
        for v in variants:
            if v == "attached":
                env.start_recording(3 * BLOCK + 1)
            rewind()
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(BLOCK):
                c += 1
                step(c)
            th.cuda.synchronize()
            dt = (time.perf_counter() - t0) / BLOCK * 1e6
            if v == "attached":
                rows = len(env.recorded())
                env.stop_recording()
                assert rows >= BLOCK * E // 2, rows         # the log was filled
            if block >= 0:
                times[v].append(dt)
    for v in variants:
        t = sorted(times[v])
        say(f"{name} {v}: median {statistics.median(t):.1f} us per vector step (min {t[0]:.1f}, max {t[-1]:.1f}; {REPEATS} blocks of "
            f"{BLOCK} steps)")
    if len(variants) == 2:
        d, a = statistics.median(times["detached"]), statistics.median(times["attached"])
        say(f"{name} attached over detached: +{a - d:.1f} us per step ({a / d:.3f}x)")


say(f"move log, E = {E}: the engine's step alone, launch by launch" + (" (detached only)" if _args.detached_only else ""))
measure("self-play", selfplay)
measure("pool K=4", pool)
measure("cross-play M=4", crossplay)
if _args.out:
    with open(_args.out, "w") as f:
        f.write("\n".join(_lines) + "\n")
