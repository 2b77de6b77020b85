"""The one-launch rollouts stage the rows of steps t > 0 with waves 1..3 only (csrc/ph_policy.hip: RowStage3 -- wave w owns rows
w - 1, w + 2, ... of the workgroup's sixteen, wave 0 owns the row tail and fetches nothing) and the value workgroup stores a step's
observation copy from those registers.  Every case compares the one launch bitwise with the launch-per-step walk, whose single
fetch is the prologue's (XStage, all four waves): every array of the rollout buffer, the cached outputs of the last step, and the
advantages after GAE.  A row that is dropped, shifted or committed twice changes an observation row of the buffer and, through the
networks, the actions, values and log-probs of its environment (checked once with such builds: CHANGELOG.md).

Shapes: the smallest at which the split can go wrong -- E = 40 (one full tile and one of 8 rows: the rows behind `n` fall into
different waves' shares), E = 16 with T = 2 (the first in-loop fetch, and the hand-over from the prologue's rows), E = 96 with T = 5;
D = 62 (the bench), 64 (no padding lanes), 1 (63 lanes of every wave own nothing); a MultiDiscrete observation, whose rows are one-hot
(built by the whole workgroup; copy_obs_rows); action masks, which select the general form of the kernel; the exchange rollout of
two local agents."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu


def _env(obs_space, act_space):
    return type("S", (), dict(observation_space=obs_space, action_space=act_space, _is_dummy_space_env=True))()


def _scripted_and_walk(obs_space, act_space, E, T, seed=3):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.vec import SyntheticRollouts, VecOnPolicyAgent
    runs = []
    for scripted in (False, True):
        model = PPO("MlpPolicy", _env(obs_space, act_space), n_steps=T, n_envs=E, batch_size=T * E // 2, n_epochs=1, seed=seed)
        model.device_permutations = True
        agent = VecOnPolicyAgent(model)
        data = SyntheticRollouts(obs_space, E, T, horizon=3, seed=seed, device=model.device)
        agent.bind_stream()
        if scripted:
            agent.rollout_scripted(data)
        else:
            for t in range(T):
                agent.get_action(data.obs[t])
                agent.update(data.rewards[t], data.dones[t])
            agent.flush_rewards()
        th.cuda.synchronize()
        snap = {k: v.copy() for k, v in model.rollout_buffer.host().items() if k not in ("advantages", "returns")}
        snap.update(act=agent.actions.cpu().numpy(), val=agent.values.cpu().numpy(), lp=agent.log_probs.cpu().numpy())
        agent.learn_from_buffer()
        th.cuda.synchronize()
        snap.update(adv=model.rollout_buffer.advantages.cpu().numpy(), ret=model.rollout_buffer.returns.cpu().numpy(),
                    params=model.policy.get_flat_params())
        runs.append(snap)
    walk, one = runs
    # the walk is the reference: it must have seen the script (a buffer of zeros would compare equal, too)
    assert np.array_equal(walk["observations"].reshape(T, E, -1), data.obs.cpu().numpy())
    assert np.isfinite(walk["adv"]).all() and np.abs(walk["values"]).max() > 0
    for key in walk:
        assert np.array_equal(walk[key], one[key]), key


@pytest.mark.parametrize("E,T,D", [(40, 3, 62), (16, 2, 62), (96, 5, 62), (40, 3, 64), (40, 3, 1)])
def test_box_rows_fetched_by_waves_1_to_3_are_bitwise_the_per_step_walk(E, T, D):
    from pantheonrl_amd import spaces as sp
    _scripted_and_walk(sp.Box(-np.inf, np.inf, (D,)), sp.Discrete(6), E, T)


def test_one_hot_rows_keep_the_whole_workgroup_fetch_and_copy_obs_rows():
    """MultiDiscrete observation (3 + 4 + 5 = 12 one-hot features, one chunk): not staged by RowStage3; the copy is copy_obs_rows"""
    from pantheonrl_amd import spaces as sp
    _scripted_and_walk(sp.MultiDiscrete([3, 4, 5]), sp.Discrete(4), 40, 3)


@pytest.mark.parametrize("n_agents,mask_mode", [(2, None), (2, 1)])
def test_exchange_rollout_rows_are_bitwise_the_per_step_walk(n_agents, mask_mode):
    """two local agents at E = 40 in one process: the lean form (no masks) and, with Bernoulli(0.8) action masks offered to the
    policy and the environment (mask_mode 1), the general form, which is built for three waves per SIMD"""
    from pantheonrl_amd import PPO, spaces as sp
    from pantheonrl_amd import dist as pdist
    from pantheonrl_amd.vec import FusedSelfPlayRollout, SyntheticRollouts, VecOnPolicyAgent
    E, T = 40, 3
    masked = mask_mode is not None
    obs_space, act_space = sp.Box(-np.inf, np.inf, (48 if masked else 62,)), sp.Discrete(5 if masked else 6)

    def run(persistent):
        agents, datas, masks = [], [], []
        for seed in range(5, 5 + n_agents):
            m = PPO("MlpPolicy", _env(obs_space, act_space), n_steps=T, n_envs=E, batch_size=E * T // 2, n_epochs=1, seed=seed)
            agents.append(VecOnPolicyAgent(m))
            datas.append(SyntheticRollouts(obs_space, E, T, 3, seed, m.device))
            if masked:
                rng = np.random.default_rng(seed)
                mk = (rng.random((T, E, act_space.n)) < 0.8).astype(np.uint8)
                mk[..., 0] |= mk.sum(-1) == 0                      # at least one legal action
                masks.append(th.as_tensor(mk).to(m.device))
        ex = pdist.ActionExchange(len(agents), E, agents[0].model.device)
        ex.want_p2p = True
        stream = th.cuda.Stream()
        snaps = []
        with th.cuda.stream(stream):
            steps = FusedSelfPlayRollout(agents, datas, ex, stream, masks=masks if masked else None,
                                         mask_mode=mask_mode if masked else 2, persistent=persistent)
            for it in range(2):                                     # the second iteration starts from the first's last dones
                steps.run_iteration(it)
                assert steps.last_rollout_mode == ("persistent" if persistent else "p2p")
                th.cuda.synchronize()
                snaps.append({f"rb{i}_{k}": v.copy() for i, a in enumerate(agents) for k, v in a.model.rollout_buffer.host().items()})
        assert ex.p2p_timeouts() == 0
        return snaps, [a.model.policy.get_flat_params() for a in agents], [d.obs.cpu().numpy() for d in datas]

    walk, w_params, obs = run(False)
    one, o_params, _ = run(True)
    for i in range(n_agents):
        assert np.array_equal(walk[-1][f"rb{i}_observations"].reshape(T, E, -1), obs[i])
    for x, y in zip(walk, one):
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    for x, y in zip(w_params, o_params):
        assert np.array_equal(x, y)
