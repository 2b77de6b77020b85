"""ADAP in device-resident Liar's Dice self-play beside the PPO pairing, one GPU.

256 tables x 128 steps.  Host clock around a device synchronise, median of REPS blocks, the variants of one process alternating:

  * `ADAP vs ADAP`   VecLiarSelfPlay with an ADAP learner in both seats (ph_liar_selfplay_step_adap: the PPO step's launches plus
                     three row builds and two redraws);
  * `PPO vs PPO`     the same game with the 64-wide PPO agents launch by launch (LIAR_PERSISTENT=0, no iteration graph): the
                     yardstick -- ph_liar_selfplay_step.

Per variant: microseconds per 256-table step of the launch-by-launch rollout (128 `_native_call`s per block), and ego steps per
second of whole iterations with both updates (`rollout_and_learn`).  Then, once, ego steps per second of the host-stepped
`trainer LiarsDice-v0 ADAP ADAP` (one table, every step a Python env.step).

`python scripts/adap_vec_speed.py yardstick` prints only the PPO-vs-PPO lines: run with PYTHONPATH at another checkout it measures
that checkout's library (the parent commit's, to show the yardstick's sequence unchanged).  `python scripts/adap_vec_speed.py
kernels` runs eight ADAP-vs-ADAP steps and nothing else, for a kernel trace."""
import os
import sys
import time

sys.path.insert(0, os.environ.get("ADAP_VEC_SPEED_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd.envs.vec import VecLiarsDice, VecLiarSelfPlay, ragged_agent_for  # noqa: E402
from pantheonrl_amd.vec import vec_agent_for  # noqa: E402

E, T = 256, 128
REPS = int(os.environ.get("ADAP_VEC_SPEED_REPS", "7"))
SPACES = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                            _is_dummy_space_env=True))()


def timed(fn):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    th.cuda.synchronize()
    return time.perf_counter() - t0


def model(kind, seed):
    kw = dict(n_steps=T, n_envs=E, batch_size=E * T // 4, n_epochs=10, seed=seed)
    if kind == "ADAP":
        from pantheonrl_amd.adap import ADAP, AdapPolicy
        m = ADAP(AdapPolicy, SPACES, **kw)
    else:
        m = PPO("MlpPolicy", SPACES, **kw)
    m.device_permutations = True
    return m


def variant(label, kind):
    os.environ["LIAR_PERSISTENT"] = "0"
    ego, alt = vec_agent_for(model(kind, 0)), ragged_agent_for(model(kind, 1))
    play = VecLiarSelfPlay(E, ego, alt, seed=3)
    assert not play.persistent
    return dict(label=label, play=play, roll=[], it=[])


def measure(variants):
    for v in variants:                                    # warm-up: sizes the workspaces, trains both learners once
        v["play"].rollout_and_learn(T)
    for _ in range(REPS):
        for v in variants:
            v["it"].append(timed(lambda: v["play"].rollout_and_learn(T)))
    for _ in range(REPS):
        for v in variants:
            play = v["play"]

            def steps():
                for t in range(T):
                    play._native_call(t + 1, ego_pos=t)
            v["roll"].append(timed(steps))
            if play.alt.full():                           # outside the clock: the next block records the partner's rows again
                play.alt.learn_from_buffer()
    for v in variants:
        it, roll = np.asarray(v["it"]), np.asarray(v["roll"])
        print(f"{v['label']:28s} {np.median(roll) / T * 1e6:8.1f} us per {E}-table step launch by launch (min "
              f"{roll.min() / T * 1e6:.1f}, max {roll.max() / T * 1e6:.1f});  iteration with both updates {np.median(it) * 1e3:7.2f} ms "
              f"(min {it.min() * 1e3:.2f}, max {it.max() * 1e3:.2f}) -> {E * T / np.median(it):12,.0f} ego steps/s;  partner updates "
              f"{v['play'].alt.iteration}", flush=True)


def host_stepped(total=4096):
    from pantheonrl_amd.trainer import run
    argv = ["LiarsDice-v0", "ADAP", "ADAP", "-t", str(total), "--seed", "0", "--ego-config", '{"n_steps": 1024, "verbose": 0}',
            "--alt-config", '{"n_steps": 1024}']
    secs = timed(lambda: run(argv))
    print(f"host-stepped trainer LiarsDice-v0 ADAP ADAP, {total} ego steps with their updates: {secs:6.2f} s -> "
          f"{total / secs:10,.0f} ego steps/s", flush=True)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode == "kernels":
        play = variant("ADAP vs ADAP", "ADAP")["play"]
        for t in range(8):
            play._native_call(t + 1, ego_pos=t)
        th.cuda.synchronize()
        return
    print(f"Liar's Dice self-play, {E} tables x {T} steps, {REPS} blocks per variant, variants alternating"
          + ("  [yardstick only]" if mode == "yardstick" else ""), flush=True)
    variants = [variant("PPO vs PPO (LIAR_PERSISTENT=0)", "PPO")]
    if mode != "yardstick":
        variants.insert(0, variant("ADAP vs ADAP", "ADAP"))
    measure(variants)
    if mode != "yardstick":
        host_stepped()


if __name__ == "__main__":
    main()
