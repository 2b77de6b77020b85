"""PPO.train() of towers of a run-time shape (policy_kwargs net_arch, ph_arch.hip) beside the 64-wide kernels, one process, one GPU.

The Overcooked shape of the headline benchmark (Box(62) observations, Discrete(6) actions, n_envs 1024, n_steps 128, batch 32 768,
10 epochs, device permutations).  Per variant: PPO.train() timed with device events after a warm-up call, REPS repetitions with the
variants alternating, median and spread of microseconds per minibatch step (gradient + reduce + clip + Adam), the multiply-adds
per row computed from the shapes, and 6 * MAC * rows / time as a share of the 157.3 TFLOP/s float32 matrix peak (the README's
roofline convention: forward 2, backward 4 flops per multiply-add).

Variants: the default policy with PH_GEMM_MODE=0 (the exact-float32 64-wide kernels: the yardstick, the same arithmetic class as
the tower kernels), the default policy in mode 2 (split bf16, for context), ArchActorCriticPolicy at (64, 64), (128, 128),
(256, 256), (64, 64, 64)."""
import os
import sys

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


if __name__ == "__main__":
    main()
