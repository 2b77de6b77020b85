"""microseconds per vectorised step of the block worlds' partner pool (envs/vec.py: VecBlockPartnerPool), E = 256 tables, both
variants, populations of K = 1, 2, 4, 8 constructors:
  K=1  learner                       K=4  learner, frozen, scripted, learner
  K=2  learner, frozen               K=8  learner, frozen, scripted, learner, frozen, scripted (EASY on v0), learner, frozen
  native     one ph_block_pool_step per step (five launches, six with a scripted member, whatever K is)
  walk       the same step through K per-member forwards and torch masks (native=False)
  selfplay   VecBlockSelfPlay's native step with the K=1 pool's planner and learner shapes, in the same session
  iteration  native rollout_and_learn: T steps, the planner's update and the update of every learner whose full() holds
A block is T = 32 steps from row 0 of the planner's buffer; the updates between two step blocks are not timed.  The host clock
around a device synchronise; the median of BLOCKS blocks with their range, the variants alternating within a round, after one
warm-up round.  The planners are untrained (they end a game with probability 1/16 or 1/30 per token), so nearly every table asks
its constructor every step: the grouped forward runs close to all E rows.

Expectation, stated before measuring: the native step does not grow with K beyond the conditional scripted launch; it costs the
self-play step plus roughly one bucket launch (a few microseconds).

`--ab ROOT` is the no-regression check instead: VecBlockSelfPlay's and VecBlockCrossPlay's native steps, this tree's library against
the tree at ROOT (the parent commit, built), one process each, alternating; the difference is judged against the parent's own
block-to-block spread.  `--worker ROOT` is one such process.  `--trace` runs 64 native steps of the K=4 pool of each variant and
nothing else, for a kernel trace taken from outside (rocprofv3 --kernel-trace --stats -- python scripts/block_pool_speed.py --trace).
`--ks 1,4`, `--envs 0,1`, `--blocks N`, `--no-walk`, `--out FILE`."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

_p = argparse.ArgumentParser()
_p.add_argument("--ks", default="1,2,4,8")
_p.add_argument("--envs", default="0,1")
_p.add_argument("--blocks", type=int, default=5)
_p.add_argument("--no-walk", action="store_true")
_p.add_argument("--ab")
_p.add_argument("--worker")
_p.add_argument("--trace", action="store_true")
_p.add_argument("--out")
_args = _p.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(_args.worker) if _args.worker else HERE)

import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.envs.vec import (FrozenVecPartner, RaggedVecOnPolicyAgent, VecBlockScriptedPartner, VecBlockSelfPlay,  # noqa: E402
                                     VecBlockWorld)
from pantheonrl_amd.vec import VecOnPolicyAgent  # noqa: E402

E, T, T_ALT = 256, 32, 16
KINDS = ["learner", "frozen", "scripted", "learner", "frozen", "easy", "learner", "frozen"]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def ppo(variant, seat, n_steps, seed):
    model = PPO("MlpPolicy", VecBlockWorld.seat_spaces(variant)[seat], n_steps=n_steps, n_envs=E, batch_size=E * n_steps // 4, n_epochs=2,
                seed=seed)
    model.device_permutations = True
    return model


def timed(fn):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    th.cuda.synchronize()
    return time.perf_counter() - t0


class Case:
    """one driver and how a block of it is timed: T steps from row 0, the updates outside the clock unless `whole`"""

    def __init__(self, sp, whole=False):
        self.sp, self.whole, self.us = sp, whole, []

    def block(self, keep):
        sp = self.sp
        if self.whole:
            dt = timed(lambda: sp.rollout_and_learn(T))
        else:
            def steps():
                for _ in range(T):
                    sp.step()
            dt = timed(steps)
            sp.ego.learn_from_buffer()
            for m in getattr(sp, "learners", None) or [sp.alt]:
                if m.full():
                    m.learn_from_buffer()
        if keep:
            self.us.append(1e6 * dt / T)

    def line(self, name):
        return f"{name}: {statistics.median(self.us):.1f} us per vectorised step (min {min(self.us):.1f}, max {max(self.us):.1f})"


def pool(variant, K, native, seed=0):
    from pantheonrl_amd.envs.vec import VecBlockPartnerPool
    members = []
    for k, kind in enumerate(KINDS[:K]):
        if kind == "learner":
            members.append(RaggedVecOnPolicyAgent(ppo(variant, 1, T_ALT, seed + 1 + k)))
        elif kind == "frozen":
            members.append(FrozenVecPartner(ppo(variant, 1, 2, seed + 1 + k).policy))
        else:
            members.append(VecBlockScriptedPartner(variant, "EASY" if kind == "easy" and variant == 0 else "DEFAULT"))
    return VecBlockPartnerPool(variant, E, VecOnPolicyAgent(ppo(variant, 0, T, seed)), members, seed=seed + 7, native=native)


def selfplay(variant, seed=0):
    return VecBlockSelfPlay(variant, E, VecOnPolicyAgent(ppo(variant, 0, T, seed)), RaggedVecOnPolicyAgent(ppo(variant, 1, T_ALT, seed + 1)),
                            seed=seed + 7, native=True)


def crossplay_case(variant):
    """the cross-play step as a Case-like object: blocks of T native steps of a 2 x 2 population with a budget no block exhausts"""
    from pantheonrl_amd.envs.crossplay import VecBlockCrossPlay
    planners = [FrozenVecPartner(ppo(variant, 0, 2, 40 + k).policy) for k in range(2)]
    constructors = [FrozenVecPartner(ppo(variant, 1, 2, 50).policy), VecBlockScriptedPartner(variant, "DEFAULT")]
    xp = VecBlockCrossPlay(variant, E, planners, constructors, games=1024, seed=5, native=True)

    class X:
        us = []

        def block(self, keep):
            def steps():
                for _ in range(T):
                    xp.step()
            dt = timed(steps)
            if keep:
                self.us.append(1e6 * dt / T)
    x = X()
    x.us = []
    return x


def worker():
    """the self-play and the cross-play native steps of both variants, alternating: one JSON line of per-block figures"""
    cases = {}
    for v in (0, 1):
        cases[f"selfplay v{v}"] = Case(selfplay(v))
        cases[f"crossplay v{v}"] = crossplay_case(v)
    for rnd in range(_args.blocks + 1):
        for c in cases.values():
            c.block(rnd > 0)
    print("AB " + json.dumps({k: c.us for k, c in cases.items()}), flush=True)


def ab(parent_root):
    roots = {"parent": os.path.abspath(parent_root), "this": HERE}
    runs = {name: {} for name in roots}
    rounds = 3
    for rnd in range(rounds):
        for name, root in roots.items():
            env = dict(os.environ, PYTHONPATH=root, PANTHEON_HIP_LIB=os.path.join(root, "pantheonrl_amd", "csrc", "libpantheon_hip.so"))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, "--blocks", str(_args.blocks)], env=env, cwd=root,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                say(f"{name} worker failed ({out.returncode}): {out.stderr[-800:]}")
                return 1
            row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("AB ")][-1][3:])
            for k, us in row.items():
                runs[name].setdefault(k, []).append(statistics.median(us))
                runs[name].setdefault(k + " blocks", []).extend(us)
    say(f"no regression by construction, shown once: native steps at E = {E}, this tree's library against the parent commit's, {rounds} "
        f"processes each, alternating; a process's figure is the median of its {_args.blocks} blocks of {T} steps")
    for k in [k for k in runs["this"] if not k.endswith(" blocks")]:
        a, b = runs["parent"][k], runs["this"][k]
        spread = max(runs["parent"][k + " blocks"]) - min(runs["parent"][k + " blocks"])
        say(f"{k}: parent {statistics.median(a):.1f} us (processes {min(a):.1f}..{max(a):.1f}; blocks spread {spread:.1f}), this tree "
            f"{statistics.median(b):.1f} us (processes {min(b):.1f}..{max(b):.1f}); difference {statistics.median(b) - statistics.median(a):+.1f} us")
    return 0


def trace():
    for v in (0, 1):
        sp = pool(v, 4, True)
        for _ in range(2):
            for _ in range(T):
                sp.step()
            sp.ego.model.rollout_buffer.pos, sp.ego.n_steps = 0, 0
            for m in sp.learners:
                m.pos.zero_()
    th.cuda.synchronize()


def main():
    ks = [int(k) for k in _args.ks.split(",")]
    for variant in [int(v) for v in _args.envs.split(",")]:
        cases = {}
        for K in ks:
            cases[f"native K={K}"] = Case(pool(variant, K, True))
        if not _args.no_walk:
            for K in ks:
                cases[f"walk   K={K}"] = Case(pool(variant, K, False))
        if 1 in ks:
            cases["selfplay  "] = Case(selfplay(variant))
        for K in ks:
            cases[f"iteration K={K}"] = Case(pool(variant, K, True), whole=True)
        say(f"partner pool of BlockEnv-v{variant}, E = {E} tables, planner n_steps {T}, learners' n_steps {T_ALT}, untrained planners; "
            f"members of K: {', '.join(KINDS)} (the first K; 'easy' is DEFAULT on v1); blocks of {T} steps; median of {_args.blocks} blocks, "
            f"variants alternating, after one warm-up round")
        for rnd in range(_args.blocks + 1):
            for c in cases.values():
                c.block(rnd > 0)
        for name, c in cases.items():
            say(c.line(name) + (" -- whole iterations: steps and every update" if c.whole else ""))
        for K in ks:
            if f"walk   K={K}" in cases:
                say(f"K={K}: walk over native {statistics.median(cases[f'walk   K={K}'].us) / statistics.median(cases[f'native K={K}'].us):.2f}x")
        if 1 in ks:
            d = statistics.median(cases["native K=1"].us) - statistics.median(cases["selfplay  "].us)
            say(f"K=1: the pool step over the self-play step {d:+.1f} us")
        base = statistics.median(cases[f"native K={ks[0]}"].us)
        say("growth with K: " + ", ".join(f"K={K} {statistics.median(cases[f'native K={K}'].us) - base:+.1f} us" for K in ks[1:]))


if _args.worker:
    worker()
elif _args.trace:
    trace()
elif _args.ab:
    rc = ab(_args.ab)
else:
    main()
if _args.out and lines:
    with open(_args.out, "a" if os.path.exists(_args.out) and _args.ab else "w") as f:
        f.write("\n".join(lines) + "\n")
if _args.ab:
    sys.exit(rc)
