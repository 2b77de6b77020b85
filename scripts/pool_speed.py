"""steady-state throughput of the device-resident Liar's Dice partner pool: a PPO ego against K learners, n_envs = 256, n_steps 128;
the native step (one grouped forward per partner move) and the walk (K forwards per partner move), with and without the updates.
`--ks 1,4` / `--no-walk` narrow the sweep."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecLiarPartnerPool, VecLiarsDice  # noqa: E402
from pantheonrl_amd.vec import VecOnPolicyAgent  # noqa: E402

E, T, ITERS = 256, 128, 3
_p = argparse.ArgumentParser()
_p.add_argument("--ks", default="1,2,4,8")
_p.add_argument("--no-walk", action="store_true")
_args = _p.parse_args()
KS = [int(k) for k in _args.ks.split(",")]
MODES = (True,) if _args.no_walk else (True, False)
spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()


def model(seed, n_steps=T):
    m = PPO("MlpPolicy", spaces, n_steps=n_steps, n_envs=E, batch_size=E * n_steps // 4, n_epochs=10, seed=seed)
    m.device_permutations = True
    return m


print(f"partner pool, E = {E}, ego n_steps = {T}, K learners with n_steps = max(16, {T} // K) (robin), {ITERS} timed iterations after one "
      "warm-up")
for K in KS:
    figures = {}
    for native in MODES:
        ego = VecOnPolicyAgent(model(0))
        # a member sits at 1 / K of a table's games: n_steps / K rows per column keep every learner updating about once an iteration
        members = [RaggedVecOnPolicyAgent(model(1 + k, max(16, T // K))) for k in range(K)]
        sp = VecLiarPartnerPool(E, ego, members, seed=3, native=native)
        sp.rollout_and_learn(T)
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            sp.rollout_and_learn(T)
        th.cuda.synchronize()
        dt = (time.perf_counter() - t0) / ITERS
        t1 = time.perf_counter()
        for _ in range(T):
            sp.step()
        th.cuda.synchronize()
        dr = time.perf_counter() - t1
        sp.ego.learn_from_buffer()
        th.cuda.synchronize()
        figures[native] = (E * T / dt, E * T / dr)
        print(f"K={K} native={native}: iteration (rollout + updates) {dt * 1e3:.1f} ms -> {E * T / dt:,.0f} ego steps/s; rollout alone "
              f"{dr / T * 1e6:.0f} us per vector step -> {E * T / dr:,.0f} ego steps/s; episodes {sp.episodes}, learner updates "
              f"{[m.iteration for m in members]}", flush=True)
    if len(figures) == 2:
        print(f"K={K} native over walk: {figures[True][0] / figures[False][0]:.2f}x with the updates, "
              f"{figures[True][1] / figures[False][1]:.2f}x rollout alone", flush=True)
