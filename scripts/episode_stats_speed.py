"""What the episode statistics cost on one MI355X (profiles/episode_stats_speed.txt).

(a) the scan launch (`ph_episode_stats`) against the GAE launch (`ph_gae`, mode 0) on the same buffer at (E, T) = (256, 128),
    (1024, 128), (16384, 128): HIP events around BATCH back-to-back launches, the two kernels alternating sample by sample in one
    process, median and range of SAMPLES samples, microseconds per launch (launch gaps included, for both alike);
(b) a whole Liar's Dice self-play iteration (LiarIterationGraph, E = 256, T = 128, persistent): statistics attached and read every
    10 iterations against detached; ego steps/s per block;
(c) the partner pool at K = 4 learners (rollout_and_learn), the same comparison.
In (b) and (c) every variant runs in a child process of its own with ONE environment, as a user's run has -- two environments in
one process measured the second one built 9-13 % slower whatever it was; one workload per child, too -- and the children alternate, ROUNDS times each:
attached, detached and, with `--parent-lib PATH`, detached on another build of the library (the parent commit's; a library is
loaded once per process).  `--only a,b,c` narrows the run; `--sweep-t` adds the scan and GAE launch times against T at E = 256 and
E = 32 to (a)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

p = argparse.ArgumentParser()
p.add_argument("--only", default="a,b,c")
p.add_argument("--parent-lib")
p.add_argument("--sweep-t", action="store_true")
p.add_argument("--child", choices=("attached", "detached"), help="(internal) blocks of one variant of (b) and (c), figures as one JSON line")
p.add_argument("--blocks", type=int, default=4, help="timed blocks per child")
p.add_argument("--rounds", type=int, default=2, help="children per variant")
args = p.parse_args()
ONLY = set(args.only.split(","))

from pantheonrl_amd import _native as nat  # noqa: E402

if args.child == "detached":
    nat.SIGNATURES.pop("ph_episode_stats", None)       # another build of the library may not have the entry point: detached only

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.envs.vec import (LiarIterationGraph, RaggedVecOnPolicyAgent, VecLiarPartnerPool, VecLiarSelfPlay,  # noqa: E402
                                     VecLiarsDice)
from pantheonrl_amd.vec import VecOnPolicyAgent  # noqa: E402

SAMPLES, BATCH = 9, 50
spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()


def spread(xs):
    return f"median {statistics.median(xs):,.2f} (min {min(xs):,.2f}, max {max(xs):,.2f}, n = {len(xs)})"


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def launch_pair(E, T):
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(E + T)
    planes = {k: th.zeros((T, E), dtype=th.float32, device="cuda") for k in ("rewards", "episode_starts", "values", "log_probs",
                                                                              "advantages", "returns")}
    planes["rewards"].copy_(th.as_tensor(rng.integers(-1, 2, (T, E)).astype(np.float32)))
    planes["episode_starts"].copy_(th.as_tensor((rng.random((T, E)) < 0.15).astype(np.float32)))
    planes["values"].copy_(th.as_tensor(rng.standard_normal((T, E), dtype=np.float32)))
    rb = nat.PhRollout()
    rb.T, rb.E = T, E
    rb.observations = rb.actions = planes["values"].data_ptr()       # checked for NULL only by both entry points
    for k, t in planes.items():
        setattr(rb, k, t.data_ptr())
    last = th.zeros(E, dtype=th.float32, device="cuda")
    carry = (th.zeros(E, dtype=th.float32, device="cuda"), th.zeros(E, dtype=th.int32, device="cuda"),
             th.ones(E, dtype=th.uint8, device="cuda"))
    stats = th.zeros((1, nat.EPISODE_NSTAT), dtype=th.float64, device="cuda")
    s = nat.PhEpisodeScan()
    s.rb, s.T, s.last_dones, s.n_members, s.stats = C.pointer(rb), T, last.data_ptr(), 1, stats.data_ptr()
    s.carry_return, s.carry_length, s.carry_valid = (t.data_ptr() for t in carry)
    lib, h = ctx.lib, ctx.handle
    scan = lambda: nat.check(lib.ph_episode_stats(h, C.byref(s)))                                    # noqa: E731
    gae = lambda: nat.check(lib.ph_gae(h, C.byref(rb), planes["values"][0].data_ptr(), last.data_ptr(), 0.99, 0.95, 0))   # noqa: E731
    keep = (ctx, planes, rb, last, carry, stats, s)
    return scan, gae, keep


def timed(fn):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BATCH):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / BATCH


def part_a():
    print(f"(a) us per launch, HIP events around {BATCH} back-to-back launches, scan and GAE alternating, {SAMPLES} samples each")
    for E, T in ((256, 128), (1024, 128), (16384, 128)):
        scan, gae, keep = launch_pair(E, T)
        for _ in range(3):
            timed(scan), timed(gae)
        xs, ys = [], []
        for _ in range(SAMPLES):
            xs.append(timed(scan))
            ys.append(timed(gae))
        print(f"  E = {E:5d} T = {T}: ph_episode_stats {spread(xs)} | ph_gae {spread(ys)} | scan / GAE of medians "
              f"{statistics.median(xs) / statistics.median(ys):.2f}", flush=True)
        del keep
    if args.sweep_t:
        print("    sweep over T, median of 5: does the time follow the rows walked or is it a fixed cost?")
        for E, T in ((256, 1), (256, 16), (256, 32), (256, 64), (256, 128), (256, 256), (256, 1024), (32, 128)):
            scan, gae, keep = launch_pair(E, T)
            for _ in range(3):
                timed(scan), timed(gae)
            xs, ys = [timed(scan) for _ in range(5)], [timed(gae) for _ in range(5)]
            print(f"    E = {E:3d} T = {T:4d}: ph_episode_stats {statistics.median(xs):7.2f} us | ph_gae {statistics.median(ys):6.2f} us", flush=True)
            del keep


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------------
E, T = 256, 128


def model(seed, n_steps=T):
    m = PPO("MlpPolicy", spaces, n_steps=n_steps, n_envs=E, batch_size=E * n_steps // 4, n_epochs=10, seed=seed)
    m.device_permutations = True
    return m


class SelfPlayRun:
    per_block = 30

    def __init__(self, attach):
        ego, alt = VecOnPolicyAgent(model(0)), RaggedVecOnPolicyAgent(model(1))
        self.sp = VecLiarSelfPlay(E, ego, alt, seed=3)
        self.stats = None
        if attach:
            from pantheonrl_amd.episode_stats import EpisodeStats
            self.stats = EpisodeStats(ego, self.sp)
        self.graph = LiarIterationGraph(self.sp, T, warmup=2)
        self.it = 0

    def iteration(self):
        self.graph.launch()
        self.it += 1
        if self.stats is not None and self.it % 10 == 0:
            self.stats.read()


class PoolRun(SelfPlayRun):
    per_block = 4

    def __init__(self, attach, K=4):
        ego = VecOnPolicyAgent(model(0))
        members = [RaggedVecOnPolicyAgent(model(1 + k, max(16, T // K))) for k in range(K)]
        self.sp = VecLiarPartnerPool(E, ego, members, seed=3)
        self.stats = None
        if attach:
            from pantheonrl_amd.episode_stats import EpisodeStats
            self.stats = EpisodeStats(ego, self.sp)
        self.it = 0
        self.iteration()

    def iteration(self):
        self.sp.rollout_and_learn(T)
        self.it += 1
        if self.stats is not None and self.it % 10 == 0:
            self.stats.read()


def block(run):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(run.per_block):
        run.iteration()
    th.cuda.synchronize()
    return E * T * run.per_block / (time.perf_counter() - t0)


def measure(cls, attach, blocks):
    run = cls(attach)
    block(run)                                        # warm-up block
    return [block(run) for _ in range(blocks)]


def child(variant, lib, which):
    env = dict(os.environ)
    if lib:
        env["PANTHEON_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--only", which,
                        "--blocks", str(args.blocks)], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child {variant} on {lib or 'this library'} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if args.child:
        attach = args.child == "attached"
        out = {}
        if "b" in ONLY:
            out["b"] = measure(SelfPlayRun, attach, args.blocks)
        if "c" in ONLY:
            out["c"] = measure(PoolRun, attach, args.blocks)
        print(json.dumps(out))
        return
    print(f"device: {th.cuda.get_device_name(0)}; library {os.path.relpath(nat.LIB_PATH, ROOT)}")
    if "a" in ONLY:
        part_a()
    bc = sorted(ONLY & {"b", "c"})
    if not bc:
        return
    variants = [("attached (read every 10 iterations)", "attached", None), ("detached", "detached", None)]
    if args.parent_lib:
        variants.append(("parent library, detached", "detached", args.parent_lib))
    got = {name: {k: [] for k in bc} for name, _, _ in variants}
    for _ in range(args.rounds):                      # the children alternate
        for name, variant, lib in variants:
            for k in bc:                              # one workload per process, too
                got[name][k] += child(variant, lib, k)[k]
    names = {"b": f"(b) Liar's Dice self-play, LiarIterationGraph, E = {E}, T = {T}, persistent, {SelfPlayRun.per_block} iterations per block",
             "c": f"(c) partner pool, K = 4 learners, E = {E}, T = {T}, rollout_and_learn, {PoolRun.per_block} iterations per block"}
    for k in bc:
        print(names[k] + f": ego steps/s, one process per variant, {args.rounds} processes x {args.blocks} blocks each, alternating")
        for name, _, _ in variants:
            print(f"  {name:38s} {spread(got[name][k])}")
        med = {name: statistics.median(got[name][k]) for name, _, _ in variants}
        line = f"  attached / detached of medians {med[variants[0][0]] / med['detached']:.4f}"
        if args.parent_lib:
            line += f"; attached / parent {med[variants[0][0]] / med[variants[2][0]]:.4f}; detached / parent {med['detached'] / med[variants[2][0]]:.4f}"
        print(line, flush=True)


main()
