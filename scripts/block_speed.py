"""throughput of the device-resident block-world self-play (PPO planner vs PPO constructor, n_envs = 256): ego steps/s of the
native step (`ph_block_selfplay_step`, one engine call per vectorised step) and of the per-call walk of the same step"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecBlockSelfPlay, VecBlockWorld  # noqa: E402
from pantheonrl_amd.vec import VecOnPolicyAgent  # noqa: E402

E, T = 256, 128
for variant in (1, 0):
    for native in (True, False):
        seats = VecBlockWorld.seat_spaces(variant)
        models = [PPO("MlpPolicy", seats[i], n_steps=T, n_envs=E, batch_size=E * T // 4, n_epochs=10, seed=i) for i in (0, 1)]
        for m in models:
            m.device_permutations = True
        ego, alt = VecOnPolicyAgent(models[0]), RaggedVecOnPolicyAgent(models[1])
        sp = VecBlockSelfPlay(variant, E, ego, alt, seed=3, native=native)
        sp.rollout_and_learn(T)                     # sizes the workspaces
        th.cuda.synchronize()
        iters = 3
        t0 = time.perf_counter()
        for _ in range(iters):
            sp.rollout_and_learn(T)
        th.cuda.synchronize()
        dt = time.perf_counter() - t0
        t1 = time.perf_counter()
        for _ in range(T):
            sp.step()
        th.cuda.synchronize()
        dr = time.perf_counter() - t1
        print(f"{VecBlockWorld.GAMES[variant]} native={native}: rollout alone {dr / T * 1e6:.0f} us per vector step -> "
              f"{E * T / dr:,.0f} ego steps/s; {iters} iterations (rollout + updates) {dt / iters * 1e3:.1f} ms each -> "
              f"{E * T * iters / dt:,.0f} ego steps/s; episodes {sp.episodes}, partner updates {alt.iteration}", flush=True)
