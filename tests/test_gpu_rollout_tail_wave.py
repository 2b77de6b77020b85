"""The one-launch rollout (policy_fwd16_rollout_kernel) runs its row tail on a fifth wave, one step behind the four layer waves
(csrc/ph_policy.hip, policy_fwd16_body with TW = 4).  Every case here runs the one launch and the per-step walk from the same
state and compares every buffer array, the cached outputs of the last step and the RNG counter EXACTLY, at the smallest shapes at
which that schedule can go wrong: T = 1 (no overlapped tail), 2 (exactly one), 3 and 5 (both uniform slots, the last tail after the
loop); E = 16 (one workgroup per net), 17 (a second workgroup with ONE live row: fifteen dead lanes in its tail wave, which must
still arrive at every barrier), 48 (three full workgroups); every logit count the tail's switch is reached with; the bench's
observation width, a small one, and one-hot observations (whose rows the four layer waves build, with a barrier of their own that
the tail wave has to count); the lean and the general form of the kernel; a captured graph replayed twice.

The one-launch entry point (ph_scripted_rollout) takes no action masks, no teacher-forced uniforms and no `deterministic` flag, and
the tail-wave forms of the kernel are built WITHOUT those paths: policy_fwd16_body pins the fields to constants beside a tail wave and
launch_policy_fwd16_rollout refuses a record that carries one.  They are served by the per-step and the exchange entry points, whose
kernels keep wave 0's tail and are unchanged, so there is no case for them here and no code of theirs in the 320-thread schedule."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

BOX62_L6 = ("box", 62, 6)


def _spaces(obs, act_n):
    from pantheonrl_amd import spaces as sp
    kind = obs[0]
    if kind == "box":
        space = sp.Box(-np.inf, np.inf, (obs[1],))
    else:
        space = sp.MultiDiscrete(list(obs[1]))
    return space, sp.Discrete(act_n)


def _setup(obs, act_n, T, E, seed=11):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.vec import SyntheticRollouts, VecOnPolicyAgent
    obs_space, act_space = _spaces(obs, act_n)
    env = type("S", (), dict(observation_space=obs_space, action_space=act_space, _is_dummy_space_env=True))()
    model = PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=T * E, n_epochs=1, seed=seed)
    p = model.policy.get_flat_params()
    model.policy.set_flat_params(p + 0.3 * np.random.default_rng(seed).standard_normal(p.shape).astype(np.float32))   # logits far from uniform
    model.device_permutations = True
    agent = VecOnPolicyAgent(model)
    data = SyntheticRollouts(obs_space, E, T, horizon=3, seed=seed, device=model.device)
    return model, agent, data


def _general_form(model, E):
    """a debug stamp buffer on the context: the argument record is then not lean, and the launch takes the general form"""
    from pantheonrl_amd import _native as nat
    stamps = th.zeros(2 * ((E + 15) // 16) * 16, dtype=th.int64, device=model.device)
    nat.check(model.policy.ctx.lib.ph_debug_set_profile_buffer(model.policy.ctx.handle, stamps.data_ptr()))
    return stamps


def _rollout(agent, data, scripted):
    agent.bind_stream()
    if scripted:
        agent.rollout_scripted(data)
    else:
        for t in range(data.T):
            agent.get_action(data.obs[t])
            agent.update(data.rewards[t], data.dones[t])
        agent.flush_rewards()
    th.cuda.synchronize()


def _snapshot(model, agent):
    snap = {k: v.copy() for k, v in model.rollout_buffer.host().items() if k not in ("advantages", "returns")}
    snap.update(act=agent.actions.cpu().numpy(), val=agent.values.cpu().numpy(), lp=agent.log_probs.cpu().numpy(),
                es=agent._last_episode_starts.cpu().numpy(), counter=np.int64(model.policy._counter))
    return snap


def _assert_one_launch_is_the_walk(obs, act_n, T, E, general=False, iterations=1):
    runs = []
    for scripted in (False, True):
        model, agent, data = _setup(obs, act_n, T, E)
        keep = _general_form(model, E) if (general and scripted) else None
        snaps = []
        for _ in range(iterations):
            _rollout(agent, data, scripted)
            snaps.append(_snapshot(model, agent))
            if iterations > 1:
                agent.learn_from_buffer()
                th.cuda.synchronize()
                snaps[-1]["params"] = model.policy.get_flat_params()
        runs.append(snaps)
        del keep
    for a, b in zip(*runs):
        assert set(a) >= {"observations", "actions", "values", "log_probs", "rewards", "episode_starts"}, sorted(a)
        for key in a:
            assert np.array_equal(a[key], b[key]), (key, obs, act_n, T, E, general)
    assert len(np.unique(runs[1][0]["actions"])) > 1 or act_n == 1     # the sampler did sample


@pytest.mark.parametrize("E", [16, 17, 48])
@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_lean_rollout_is_bitwise_the_walk_at_every_step_and_tile_count(T, E):
    _assert_one_launch_is_the_walk(BOX62_L6, 6, T, E)


@pytest.mark.parametrize("act_n", [1, 8])
def test_every_logit_count_of_the_tail(act_n):
    """(6 logits: every other case)"""
    _assert_one_launch_is_the_walk(("box", 62), act_n, 3, 17)
    _assert_one_launch_is_the_walk(("box", 62), act_n, 5, 48, general=True)


def test_small_observation_width():
    _assert_one_launch_is_the_walk(("box", 5), 6, 3, 17)
    _assert_one_launch_is_the_walk(("box", 5), 6, 2, 48, general=True)


@pytest.mark.parametrize("general", [False, True])
def test_one_hot_observations_beside_the_tail_wave(general):
    """the rows of a step are built by the 256 threads of the layer waves (XStage<16, 256>); the fifth wave only counts their barrier"""
    for T, E in ((1, 17), (3, 17), (5, 48)):
        _assert_one_launch_is_the_walk(("onehot", (3, 4, 5, 2, 6)), 3, T, E, general=general)


@pytest.mark.parametrize("T,E", [(1, 17), (2, 16), (3, 17), (5, 48)])
def test_general_form_is_bitwise_the_walk(T, E):
    _assert_one_launch_is_the_walk(BOX62_L6, 6, T, E, general=True)


def test_second_launch_starts_clean():
    """two iterations: the second rollout starts from the first one's last dones and its updated parameters"""
    _assert_one_launch_is_the_walk(BOX62_L6, 6, 5, 17, iterations=2)


def test_captured_rollout_replayed_twice_is_two_eager_iterations():
    """IterationGraph(scripted=True): the captured iteration replayed twice against the same iteration run eagerly, step by step,
    twice, under the same RNG epochs -- nothing of the tail wave's state may survive a launch."""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.vec import IterationGraph, run_iteration_eager
    T, E = 5, 17
    out = []
    for replay in (True, False):
        model, agent, data = _setup(BOX62_L6, 6, T, E)
        stream = th.cuda.Stream()
        graph = IterationGraph(agent, data, stream, scripted=True)     # two eager warm-up iterations, then the capture
        pol = model.policy
        snaps = []
        with th.cuda.stream(stream):
            for _ in range(2):
                if replay:
                    graph.launch()
                else:        # the captured body, launch by launch and step by step, from the counters the capture baked in
                    pol._counter -= T
                    model.permutation_seed -= 1
                    run_iteration_eager(agent, data, scripted=False)
                    nat.check(pol.ctx.lib.ph_rng_epoch_advance(pol.ctx.handle))
                stream.synchronize()
                snap = {k: v.copy() for k, v in model.rollout_buffer.host().items()}
                snap["params"] = pol.get_flat_params()
                snaps.append(snap)
        assert int(graph.epoch_word.item()) == 2
        out.append(snaps)
    for a, b in zip(*out):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    assert not np.array_equal(out[0][0]["actions"], out[0][1]["actions"])     # a replay draws fresh random numbers
