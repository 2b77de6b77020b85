"""PPO.train() of towers of a run-time shape (policy_kwargs net_arch, ph_arch.hip) beside the 64-wide kernels, one process, one GPU.

The Overcooked shape of the headline benchmark (Box(62) observations, Discrete(6) actions, n_envs 1024, n_steps 128, batch 32 768,
10 epochs, device permutations).  Per variant: PPO.train() timed with device events after a warm-up call, REPS repetitions with the
variants alternating, median and spread of microseconds per minibatch step (gradient + reduce + clip + Adam), the multiply-adds
per row computed from the shapes, and 6 * MAC * rows / time as a share of the 157.3 TFLOP/s float32 matrix peak (the README's
roofline convention: forward 2, backward 4 flops per multiply-add).

Variants: the default policy with PH_GEMM_MODE=0 (the exact-float32 64-wide kernels: the yardstick, the same arithmetic class as
the tower kernels), the default policy in mode 2 (split bf16, for context), ArchActorCriticPolicy at (64, 64), (128, 128),
(256, 256), (64, 64, 64).

`python scripts/arch_speed.py rollout` measures the device-resident rollouts of towers instead (host clock around a device
synchronise, median of REPS, variants of one table alternating):
  * Overcooked shape, 1024 envs x 128 steps: TowerVecOnPolicyAgent.rollout_scripted (ONE launch, tower_rollout_kernel) against the
    per-step walk of the same agent (128 x get_action + update) at (64, 64), (128, 128), (256, 256), and as the yardstick
    VecOnPolicyAgent.rollout_scripted of the 64-wide kernels -- with PH_ROLLOUT_LEAN at its default here, and with PH_ROLLOUT_LEAN=0
    in a child process of its own (the switch is read once per process);
  * Liar's Dice, 256 tables x 128 steps: tower agents in both seats at (64, 64) and (128, 128) through LiarIterationGraph (6 x 128
    launches + the ego's update as one graph, the partner's update after it) and the 64-wide agents under LIAR_PERSISTENT=0 the
    same way: microseconds per 256-table step of the launch-by-launch rollout, and ego steps per second of whole iterations."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch as th  # noqa: E402

from pantheonrl_amd import PPO  # noqa: E402
from pantheonrl_amd import spaces as sp  # noqa: E402
from pantheonrl_amd.ppo import ActorCriticPolicy, ArchActorCriticPolicy, RolloutBuffer  # noqa: E402

E, T, BATCH, EPOCHS, F, L = 1024, 128, 32768, 10, 62, 6
REPS = int(os.environ.get("ARCH_SPEED_REPS", "7"))
PEAK = 157.3e12


def macs_per_row(widths):
    tower, fin = 0, F
    for w in widths:
        tower += fin * w
        fin = w
    return 2 * tower + widths[-1] * L + widths[-1]


def make(label, widths, gemm_mode, arch_class):
    env = type("Env", (), dict(observation_space=sp.Box(-np.inf, np.inf, (F,)), action_space=sp.Discrete(L), _is_dummy_space_env=True))()
    os.environ["PH_GEMM_MODE"] = str(gemm_mode)
    model = PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=BATCH, n_epochs=EPOCHS, seed=0)
    if arch_class:
        model.policy = ArchActorCriticPolicy(env.observation_space, env.action_space, net_arch=widths, device="cuda", seed=0)
        model.rollout_buffer = RolloutBuffer(T, env.observation_space, env.action_space, model.device, model.policy.ctx,
                                             model.policy.spec, n_envs=E)
    else:
        assert type(model.policy) is ActorCriticPolicy and model.policy.gemm_mode == gemm_mode
    model.device_permutations = True
    g = th.Generator(device="cuda").manual_seed(1)
    rb = model.rollout_buffer
    rb.observations.normal_(generator=g)
    rb.actions.copy_(th.randint(0, L, rb.actions.shape, generator=g, device="cuda").float())
    for a in (rb.values, rb.advantages, rb.returns):
        a.normal_(generator=g)
    rb.log_probs.fill_(-float(np.log(L)))
    rb.pos, rb.full = T, True
    return dict(label=label, widths=widths, model=model, us=[])


def main():
    variants = [make("ActorCriticPolicy (64, 64), PH_GEMM_MODE=0", (64, 64), 0, False),
                make("ActorCriticPolicy (64, 64), PH_GEMM_MODE=2", (64, 64), 2, False)]
    for w in ((64, 64), (128, 128), (256, 256), (64, 64, 64)):
        variants.append(make(f"ArchActorCriticPolicy {w}", w, 0, True))
    steps = EPOCHS * ((E * T + BATCH - 1) // BATCH)
    ev0, ev1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    for v in variants:
        v["model"].train(sync_stats=False)          # warm-up: sizes the workspaces
    th.cuda.synchronize()
    for _ in range(REPS):
        for v in variants:
            ev0.record()
            v["model"].train(sync_stats=False)
            ev1.record()
            ev1.synchronize()
            v["us"].append(ev0.elapsed_time(ev1) * 1e3 / steps)
    print(f"PPO.train(), Box({F}) x Discrete({L}), {E} envs x {T} steps, batch {BATCH}, {EPOCHS} epochs: {steps} minibatch steps per "
          f"call, {REPS} calls per variant, variants alternating")
    base = float(np.median(variants[0]["us"]))
    for v in variants:
        us = np.asarray(v["us"])
        med = float(np.median(us))
        mac = macs_per_row(v["widths"])
        share = 6.0 * mac * BATCH / (med * 1e-6) / PEAK
        ok = bool(np.isfinite(v["model"].policy.get_flat_params()).all())
        print(f"{v['label']:48s} {med:9.1f} us per minibatch step (min {us.min():.1f}, max {us.max():.1f})  x{med / base:5.2f} of the "
              f"mode-0 yardstick  {mac:7d} MAC/row  {100 * share:5.2f} % of the f32 matrix peak  parameters finite: {ok}", flush=True)


# ---- rollouts ----------------------------------------------------------------------------------------------------------------------
def tower_model(env, widths, n_steps, n_envs, seed, n_epochs=10):
    """PPO on ArchActorCriticPolicy at `widths` -- (64, 64) included, which policy_kwargs would hand to the 64-wide kernels"""
    model = PPO("MlpPolicy", env, n_steps=n_steps, n_envs=n_envs, batch_size=n_envs * n_steps // 4, n_epochs=n_epochs, seed=seed,
                _init_setup_model=False)
    if widths is not None:
        model._policy_args = {"net_arch": tuple(widths)}
    model._setup_model()
    model.device_permutations = True
    return model


def timed(fn):
    th.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    th.cuda.synchronize()
    return time.perf_counter() - t0


def scripted_variants(lean0_child):
    from pantheonrl_amd.vec import SyntheticRollouts, vec_agent_for
    env = type("Env", (), dict(observation_space=sp.Box(-np.inf, np.inf, (F,)), action_space=sp.Discrete(L), _is_dummy_space_env=True))()
    data = SyntheticRollouts(env.observation_space, E, T, horizon=400, seed=0, device="cuda")
    out = []

    def add(label, widths, one_launch):
        agent = vec_agent_for(tower_model(env, widths, T, E, 0))
        agent.bind_stream()

        def run():
            if one_launch:
                agent.rollout_scripted(data)
            else:
                for t in range(T):
                    agent.get_action(data.obs[t])
                    agent.update(data.rewards[t], data.dones[t])
                agent.flush_rewards()
            agent.finish_update()       # the buffer starts over, nothing is trained
        out.append(dict(label=label, run=run, secs=[]))

    if lean0_child:
        add("VecOnPolicyAgent (64, 64) rollout_scripted, PH_ROLLOUT_LEAN=0", None, True)
        return out
    add("VecOnPolicyAgent (64, 64) rollout_scripted (64-wide yardstick)", None, True)
    for w in ((64, 64), (128, 128), (256, 256)):
        add(f"TowerVecOnPolicyAgent {w} rollout_scripted (one launch)", w, True)
        add(f"TowerVecOnPolicyAgent {w} walk: {T} x (get_action + update)", w, False)
    return out


def rollout_scripted_section(lean0_child=False):
    variants = scripted_variants(lean0_child)
    for v in variants:
        v["run"]()
    for _ in range(REPS):
        for v in variants:
            v["secs"].append(timed(v["run"]))
    if not lean0_child:
        print(f"scripted rollouts, Box({F}) x Discrete({L}), {E} envs x {T} steps, {REPS} runs per variant, variants alternating")
    for v in variants:
        us = np.asarray(v["secs"]) * 1e6
        print(f"{v['label']:64s} {np.median(us):9.1f} us per rollout = {np.median(us) / T:7.2f} us per step "
              f"(min {us.min():.1f}, max {us.max():.1f})", flush=True)


def liar_section():
    from pantheonrl_amd.envs.vec import LiarIterationGraph, VecLiarsDice, VecLiarSelfPlay, ragged_agent_for
    from pantheonrl_amd.vec import vec_agent_for
    El, Tl = 256, 128
    spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                                _is_dummy_space_env=True))()
    variants = []
    for label, widths in (("64-wide agents, LIAR_PERSISTENT=0", None), ("tower agents (64, 64)", (64, 64)),
                          ("tower agents (128, 128)", (128, 128))):
        ego, alt = vec_agent_for(tower_model(spaces, widths, Tl, El, 0)), ragged_agent_for(tower_model(spaces, widths, Tl, El, 1))
        saved = os.environ.get("LIAR_PERSISTENT")
        os.environ["LIAR_PERSISTENT"] = "0"
        try:
            play = VecLiarSelfPlay(El, ego, alt, seed=3)
        finally:
            if saved is None:
                del os.environ["LIAR_PERSISTENT"]
            else:
                os.environ["LIAR_PERSISTENT"] = saved
        assert not play.persistent
        variants.append(dict(label=label, play=play, graph=LiarIterationGraph(play, Tl), it=[], roll=[]))
    for v in variants:
        v["graph"].launch()
    for _ in range(REPS):
        for v in variants:
            v["it"].append(timed(v["graph"].launch))
    for _ in range(REPS):
        for v in variants:
            def steps(play=v["play"]):
                for t in range(Tl):
                    play._native_call(t + 1, ego_pos=t)
            with th.cuda.stream(v["graph"].stream):
                v["roll"].append(timed(steps))
                if v["play"].alt.full():        # outside the clock: the next rollout records the partner's rows again
                    v["play"].alt.learn_from_buffer()
    print(f"Liar's Dice self-play, {El} tables x {Tl} steps, LiarIterationGraph (launch-by-launch form captured as one graph), {REPS} "
          "runs per variant, variants alternating")
    for v in variants:
        it, roll = np.asarray(v["it"]), np.asarray(v["roll"])
        print(f"{v['label']:36s} {np.median(roll) / Tl * 1e6:8.1f} us per {El}-table step launch by launch (min "
              f"{roll.min() / Tl * 1e6:.1f}, max {roll.max() / Tl * 1e6:.1f});  iteration with both updates {np.median(it) * 1e3:7.2f} ms "
              f"(min {it.min() * 1e3:.2f}, max {it.max() * 1e3:.2f}) -> {El * Tl / np.median(it):12,.0f} ego steps/s;  partner updates "
              f"{v['play'].alt.iteration}", flush=True)


def rollout_main():
    import subprocess
    rollout_scripted_section()
    env = dict(os.environ, PH_ROLLOUT_LEAN="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "rollout-lean0"], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout.strip() if r.returncode == 0 else f"PH_ROLLOUT_LEAN=0 child failed: {r.stderr[-500:]}", flush=True)
    liar_section()


if __name__ == "__main__":
    if sys.argv[1:2] == ["rollout"]:
        rollout_main()
    elif sys.argv[1:2] == ["rollout-lean0"]:
        rollout_scripted_section(lean0_child=True)
    else:
        main()
