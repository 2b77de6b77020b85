"""gpu: episode returns and lengths of device-resident training (`ph_episode_stats`, `EpisodeStats`) against the NumPy oracle
(tests/episode_stats_oracle.py): synthetic planes with and without member replay, the real partner pool credited on the host step
by step, the self-play forms against each other, RPS and the block world, a mid-run attach, ABI refusals and the command line."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from tests import liar_cases as LC
from tests.episode_stats_oracle import EpisodeOracle

pytestmark = pytest.mark.gpu


# ---- driving the entry point on planes of the test's own ----------------------------------------------------------------------
class _Planes:
    """a context, a rollout buffer description over synthetic (T, E) planes and the scan's carries"""

    def __init__(self, E, T, K=1, member=None, rule="robin", pool_seed=0, valid=True):
        self.ctx = nat.Context(0)
        self.ctx.set_stream(th.cuda.current_stream().cuda_stream)
        self.E, self.T, self.K = E, T, K
        self.rew = th.zeros((T, E), dtype=th.float32, device="cuda")
        self.es = th.zeros((T, E), dtype=th.float32, device="cuda")
        self.last = th.zeros(E, dtype=th.float32, device="cuda")
        self.rb = nat.PhRollout()
        self.rb.T, self.rb.E = T, E
        for k in ("observations", "actions", "values", "log_probs", "advantages", "returns"):
            setattr(self.rb, k, self.rew.data_ptr())            # checked for NULL only: the scan reads two planes
        self.rb.rewards, self.rb.episode_starts = self.rew.data_ptr(), self.es.data_ptr()
        self.carry_return = th.zeros(E, dtype=th.float32, device="cuda")
        self.carry_length = th.zeros(E, dtype=th.int32, device="cuda")
        self.carry_valid = th.full((E,), int(valid), dtype=th.uint8, device="cuda")
        self.member = None if member is None else th.as_tensor(np.asarray(member, np.int32)).cuda()
        self.stats = th.zeros((K, nat.EPISODE_NSTAT), dtype=th.float64, device="cuda")
        s = self.desc = nat.PhEpisodeScan()
        s.rb, s.T, s.last_dones = C.pointer(self.rb), T, self.last.data_ptr()
        s.carry_return, s.carry_length, s.carry_valid = (t.data_ptr() for t in (self.carry_return, self.carry_length, self.carry_valid))
        s.n_members, s.member, s.resample, s.pool_seed = K, nat.ptr(self.member), nat.POOL_RESAMPLE[rule], pool_seed
        s.stats = self.stats.data_ptr()

    def scan(self, rew, es, last, counter0=0):
        self.rew.copy_(th.as_tensor(rew))
        self.es.copy_(th.as_tensor(es))
        self.last.copy_(th.as_tensor(last))
        self.desc.counter0 = counter0
        nat.check(self.ctx.lib.ph_episode_stats(self.ctx.handle, C.byref(self.desc)))

    def state(self):
        th.cuda.synchronize()
        return dict(stats=self.stats.cpu().numpy().copy(), ret=self.carry_return.cpu().numpy().copy(),
                    len=self.carry_length.cpu().numpy().copy(), valid=self.carry_valid.cpu().numpy().copy(),
                    member=None if self.member is None else self.member.cpu().numpy().copy())


def _synthetic(E, T, scans, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((T, E), dtype=np.float32), (rng.random((T, E)) < 0.3).astype(np.float32),
             (rng.random(E) < 0.3).astype(np.float32)) for _ in range(scans)]


def _assert_against(o, got):
    """device state against the oracle's: counts, length sums and carries exact, float64 sums within the summation-order bound"""
    want, bound = o.stats(), o.bounds()
    stats = got["stats"]
    assert np.array_equal(stats[:, 0], want[:, 0]) and np.array_equal(stats[:, 3], want[:, 3]), (stats, want)
    assert (np.abs(stats[:, 1] - want[:, 1]) <= bound[:, 0]).all(), (stats[:, 1] - want[:, 1], bound[:, 0])
    assert (np.abs(stats[:, 2] - want[:, 2]) <= bound[:, 1]).all(), (stats[:, 2] - want[:, 2], bound[:, 1])
    assert np.array_equal(got["ret"].view(np.uint32), o.ret.view(np.uint32)) and np.array_equal(got["len"], o.len)
    assert np.array_equal(got["valid"].astype(bool), o.valid)


# ---- 1. synthetic planes, no members -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,T", [(1, 1), (70, 9), (300, 5), (130, 35), (40, 150)])
def test_synthetic_planes_without_members(E, T):
    """(1, 1): one table, one row; (70, 9): a partial last workgroup (32 tables each); (300, 5): ten workgroups, so the last phase's
    eight ranges hold two workgroups, one or none; (130, 35): the walk's 16-row blocks twice plus a 3-row tail; (40, 150): a second
    staged block of 128 rows, 22 rows long.  Three scans share the carries; a second run gives the same bits."""
    data = _synthetic(E, T, 3, seed=E * 100 + T)
    runs = []
    for _ in range(2):
        p, o = _Planes(E, T), EpisodeOracle(E)
        for i, (rew, es, last) in enumerate(data):
            p.scan(rew, es, last)
            o.scan(rew, es, last)
            _assert_against(o, p.state())
        runs.append(p.state())
    assert len(o.episodes) > 0 or E == 1
    for key in ("stats", "ret", "len", "valid"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes(), key


def test_zeroed_statistics_give_one_rollouts_figures_and_dropped_tables_come_back():
    E, T = 70, 9
    (rew, es, last), = _synthetic(E, T, 1, seed=3)
    p, o = _Planes(E, T, valid=False), EpisodeOracle(E, valid=False)
    p.scan(rew, es, last)
    o.scan(rew, es, last)
    _assert_against(o, p.state())
    ends = es[1:].sum(axis=0) + last
    assert o.stats()[0, 0] == np.maximum(ends - 1, 0).sum()          # the first end of every table is not an episode
    first = p.state()["stats"]
    p.stats.zero_()
    p.scan(rew, es, last)
    o2 = EpisodeOracle(E)
    o2.ret, o2.len, o2.valid = o.ret.copy(), o.len.copy(), o.valid.copy()
    o2.scan(rew, es, last)
    _assert_against(o2, p.state())                                  # a zeroed block: the second scan's figures alone
    assert p.state()["stats"][0, 0] >= first[0, 0] > 0


# ---- 2. member replay on synthetic planes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", [None, 5])
@pytest.mark.parametrize("rule", ["robin", "random"])
@pytest.mark.parametrize("K", [3, 8])
def test_member_replay_on_synthetic_planes(K, rule, epoch):
    E, T, pool_seed, counter0 = 70, 9, 0x1234567890ABCDEF & 0x7FFFFFFFFFFFFFFF, 41
    rng = np.random.default_rng(K * 7 + (rule == "random"))
    member = rng.integers(0, K, E)
    data = _synthetic(E, T, 3, seed=K)
    p, o = _Planes(E, T, K, member, rule, pool_seed), EpisodeOracle(E, K, member, rule, pool_seed)
    word = None
    if epoch is not None:
        word = th.full((1,), epoch, dtype=th.int64, device="cuda")
        nat.check(p.ctx.lib.ph_ctx_set_rng_epoch(p.ctx.handle, word.data_ptr()))
    for i, (rew, es, last) in enumerate(data):
        p.scan(rew, es, last, counter0 + i * T)
        o.scan(rew, es, last, counter0 + i * T, epoch)
        got = p.state()
        _assert_against(o, got)
        assert np.array_equal(got["member"], o.member)
    assert (o.stats()[:, 0] > 0).all()
    if rule == "random" and epoch is not None:        # the epoch word is part of the key: without it other members are drawn
        q = EpisodeOracle(E, K, member, rule, pool_seed)
        for i, (rew, es, last) in enumerate(data):
            q.scan(rew, es, last, counter0 + i * T, None)
        assert not np.array_equal(q.member, o.member)


def test_misuse_is_refused_by_name():
    p = _Planes(16, 4, 3, np.zeros(16), "robin")
    lib, h, s = p.ctx.lib, p.ctx.handle, p.desc

    def refused(match, **change):
        saved = {k: getattr(s, k) for k in change}
        for k, v in change.items():
            setattr(s, k, v)
        assert lib.ph_episode_stats(h, C.byref(s)) != 0
        assert match in lib.ph_last_error().decode(), lib.ph_last_error()
        for k, v in saved.items():
            setattr(s, k, v)

    refused("n_members must be 1..PH_MAX_POOL", n_members=0)
    refused("n_members must be 1..PH_MAX_POOL", n_members=nat.PH_MAX_POOL + 1)
    refused("needs the member array", member=None)
    refused("T must be 1..rb->T", T=0)
    refused("T must be 1..rb->T", T=5)
    refused("unknown resample rule", resample=2)
    refused("incomplete description", stats=None)
    nat.check(lib.ph_episode_stats(h, C.byref(s)))            # and the description itself is fine
    s.n_members, s.member = 1, None                           # no attribution: the member array may be NULL
    nat.check(lib.ph_episode_stats(h, C.byref(s)))
    th.cuda.synchronize()


# ---- the real environments -----------------------------------------------------------------------------------------------------
def _ppo(spaces, E, T, seed):
    from pantheonrl_amd import PPO
    model = PPO("MlpPolicy", spaces, n_steps=T, n_envs=E, batch_size=max(8, E * T // 2), n_epochs=2, seed=seed)
    model.device_permutations = True
    return model


def _selfplay(E, T, seed=5, persistent=None):
    sp, ego, alt = LC.selfplay(E, _ppo(LC.spaces(), E, T, seed), _ppo(LC.spaces(), E, 6, seed + 1), seed=seed)
    if persistent is not None:
        sp.persistent = persistent
    return sp, ego, alt


# ---- 3. the real pool ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", ["robin", "random"])
def test_pool_episodes_are_credited_to_the_member_that_sat(resample):
    """The test drives env.step() itself: `partnerid` before every step, the done mask and the flushed reward row after it, credited
    on the host.  Liar's Dice rewards are small integers, so every figure per member is exactly equal."""
    from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecLiarDefaultPartner, VecLiarPartnerPool
    from pantheonrl_amd.episode_stats import EpisodeStats
    from pantheonrl_amd.vec import VecOnPolicyAgent
    E, T, K = 48, 8, 3
    ego = VecOnPolicyAgent(_ppo(LC.spaces(), E, T, 2))
    members = [VecLiarDefaultPartner(), VecLiarDefaultPartner(), RaggedVecOnPolicyAgent(_ppo(LC.spaces(), E, 6, 3))]
    env = VecLiarPartnerPool(E, ego, members, seed=9, resample=resample)
    stats = EpisodeStats(ego, env)
    assert env.episode_stats is stats and ego.episode_stats is stats and stats.K == K
    rb = ego.model.rollout_buffer
    want = np.zeros((K, 4))
    ret, length = np.zeros(E, np.float32), np.zeros(E, np.int64)
    for step in range(3 * T):
        pid = env.partnerid.cpu().numpy().copy()
        done = env.step().cpu().numpy().astype(bool)
        if step and step % T == 0:
            # the step's own roll-over scanned rows that end at step - 1, then this step dealt and resampled: a read right here
            # must not mistake the members the scan stands behind for a lost replay
            assert stats._covered_step == env.steps_done - 1 and not np.array_equal(pid, env.partnerid.cpu().numpy())
            assert stats.read(reset_window=False)["total"]["count"] == int(want[:, 0].sum())
        ego.flush_rewards()
        row = rb.rewards[rb.pos - 1].cpu().numpy()
        ret = ret + row
        length += 1
        for e in np.flatnonzero(done):
            x = np.float64(ret[e])
            want[pid[e]] += (1.0, x, x * x, float(length[e]))
        ret[done], length[done] = 0.0, 0
        for m in env.learners:
            if m.full():
                m.learn_from_buffer()
    ego.learn_from_buffer()                     # the third rollout's scan (the first two ran at the step's own roll-over)
    assert stats._covered_step == env.steps_done
    rep = stats.read()                          # compares the replayed members with env.partnerid, too
    got = stats.stats.cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(stats.member.cpu().numpy(), env.partnerid.cpu().numpy())
    assert rep["total"]["count"] == env.episodes == int(want[:, 0].sum()) and (want[:, 0] > 0).all()
    assert [m["count"] for m in rep["total"]["members"]] == want[:, 0].astype(int).tolist()
    assert np.array_equal(stats.carry_return.cpu().numpy(), ret) and np.array_equal(stats.carry_length.cpu().numpy(), length)
    # the self-check: a replay that has lost step is reported with its first table
    stats.member[5] = (stats.member[5] + 1) % K
    with pytest.raises(nat.NativeError, match="table 5"):
        stats.read()


# ---- 4. the self-play forms agree ----------------------------------------------------------------------------------------------
def _totals(stats):
    th.cuda.synchronize()
    return dict(stats=stats.stats.cpu().numpy().tobytes(), ret=stats.carry_return.cpu().numpy().tobytes(),
                len=stats.carry_length.cpu().numpy().tobytes())


def test_selfplay_forms_agree_bitwise():
    """rollout_and_learn with the one-launch rollout against its walk: the running totals are the same bits (the persistent rollout
    is bitwise its walk).  LiarIterationGraph (two warm-up iterations, two replays), in either rollout form: captured against launch
    by launch the same bits (a captured scan replays against fixed pointers), and every game the environment counted is in the
    totals.  The graph's two rollout forms are NOT compared with each other: they play different games with or without statistics
    attached -- the stepwise form draws the partner's minibatch order behind the epoch advance, the split form in front of it
    (measured at these shapes: 784 against 783 episodes after four iterations, other parameters of both learners)."""
    from pantheonrl_amd.envs.vec import LiarIterationGraph
    from pantheonrl_amd.episode_stats import EpisodeStats
    E, T = 32, 8
    plain = []
    for persistent in (True, False):
        sp, ego, alt = _selfplay(E, T, persistent=persistent)
        stats = EpisodeStats(ego, sp)
        for _ in range(4):
            sp.rollout_and_learn(T)
        plain.append((_totals(stats), stats.read()["total"]["count"], sp.episodes))
    assert plain[0][0] == plain[1][0] and plain[0][1] > E
    carried = np.count_nonzero(np.frombuffer(plain[0][0]["len"], np.int32))
    assert plain[0][1] == plain[0][2]                   # every game that ended was counted; `carried` tables are mid-game
    assert carried > 0
    for persistent in (True, False):
        forms = []
        for capture in (True, False):
            sp, ego, alt = _selfplay(E, T, persistent=persistent)
            stats = EpisodeStats(ego, sp)
            g = LiarIterationGraph(sp, T, capture=capture, warmup=2)
            assert (g.graph_id is not None) == capture and g.split == persistent
            for _ in range(2):
                g.launch()
            forms.append((_totals(stats), stats.read()["total"]["count"], sp.episodes, ego.model.policy.get_flat_params().tobytes()))
        assert forms[0][0] == forms[1][0] and forms[0][3] == forms[1][3], persistent
        assert forms[0][1] == forms[0][2] > E


def test_attached_statistics_leave_the_training_bits_alone():
    """the same four iterations with and without an EpisodeStats on the ego: the same parameters and the same games"""
    from pantheonrl_amd.episode_stats import EpisodeStats
    E, T = 32, 8
    runs = []
    for attach in (True, False):
        sp, ego, alt = _selfplay(E, T)
        if attach:
            EpisodeStats(ego, sp)
        for _ in range(3):
            sp.rollout_and_learn(T)
        th.cuda.synchronize()
        runs.append((ego.model.policy.get_flat_params().tobytes(), alt.model.policy.get_flat_params().tobytes(), sp.episodes,
                     ego.model.rollout_buffer.host()["returns"].tobytes()))
    assert runs[0] == runs[1]


# ---- 5. RPS and the block world ------------------------------------------------------------------------------------------------
def test_rps_every_step_is_an_episode():
    from pantheonrl_amd.envs.vec import VecRPS, selfplay_iteration
    from pantheonrl_amd.episode_stats import EpisodeStats
    from pantheonrl_amd.vec import VecOnPolicyAgent
    E, T = 16, 4
    spaces = type("S", (), dict(observation_space=VecRPS.observation_space, action_space=VecRPS.action_space, _is_dummy_space_env=True))()
    ego, alt = VecOnPolicyAgent(_ppo(spaces, E, T, 1)), VecOnPolicyAgent(_ppo(spaces, E, T, 2))
    env = VecRPS(E, ego.model.policy.ctx, ego.model.policy.device)
    stats = EpisodeStats(ego, env)
    selfplay_iteration(env, ego, alt, T)
    tot = stats.read()["total"]
    rew = ego.model.rollout_buffer.rewards.cpu().numpy().astype(np.float64)
    assert tot["count"] == E * T == 64 and tot["mean_length"] == 1.0
    assert tot["mean"] * 64 == rew.sum() and stats.stats.cpu().numpy()[0, 2] == (rew ** 2).sum()
    assert env.episode_stats is stats and len(tot["members"]) == 1


def test_block_world_counts_its_episodes():
    from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecBlockSelfPlay, VecBlockWorld
    from pantheonrl_amd.episode_stats import EpisodeStats
    from pantheonrl_amd.vec import VecOnPolicyAgent
    E, T = 16, 8
    s_ego, s_alt = VecBlockWorld.seat_spaces(0)
    ego, alt = VecOnPolicyAgent(_ppo(s_ego, E, T, 1)), RaggedVecOnPolicyAgent(_ppo(s_alt, E, 6, 2))
    env = VecBlockSelfPlay(0, E, ego, alt, seed=4)
    stats, o = EpisodeStats(ego, env), EpisodeOracle(E)
    rb = ego.model.rollout_buffer
    for _ in range(2):
        for _ in range(T):
            env.step()
        ego.compute_returns()                        # the scan, with the buffer full and the late rewards in place
        th.cuda.synchronize()
        o.scan(rb.rewards.cpu().numpy(), rb.episode_starts.cpu().numpy(), ego._last_episode_starts.cpu().numpy())
        ego.model.train(sync_stats=False)
        ego.finish_update()
        if alt.full():
            alt.learn_from_buffer()
    tot = stats.read()["total"]
    got = dict(stats=stats.stats.cpu().numpy(), ret=stats.carry_return.cpu().numpy(), len=stats.carry_length.cpu().numpy(),
               valid=stats.carry_valid.cpu().numpy())
    _assert_against(o, got)
    assert tot["count"] == env.episodes == len(o.episodes)


# ---- 6. attached mid-run -------------------------------------------------------------------------------------------------------
def test_attached_mid_run_drops_the_game_in_progress():
    from pantheonrl_amd.episode_stats import EpisodeStats
    E, T = 32, 8
    sp, ego, alt = _selfplay(E, T, persistent=False)
    for _ in range(3):
        sp.step()
    stats, o = EpisodeStats(ego, sp), EpisodeOracle(E, valid=False)
    assert not stats.carry_valid.any().item()
    rb = ego.model.rollout_buffer
    ends = np.zeros(E)
    for _ in range(2):
        while ego.n_steps < T:
            sp.step()
        ego.compute_returns()
        th.cuda.synchronize()
        es, last = rb.episode_starts.cpu().numpy(), ego._last_episode_starts.cpu().numpy()
        o.scan(rb.rewards.cpu().numpy(), es, last)
        ends += es[1:].sum(axis=0) + last
        ego.model.train(sync_stats=False)
        ego.finish_update()
    got = dict(stats=stats.stats.cpu().numpy(), ret=stats.carry_return.cpu().numpy(), len=stats.carry_length.cpu().numpy(),
               valid=stats.carry_valid.cpu().numpy())
    _assert_against(o, got)
    # the first game a table finishes is absent from the counts
    assert stats.read()["total"]["count"] == np.maximum(ends - 1, 0).sum() > 0


# ---- 7. the command line -------------------------------------------------------------------------------------------------------
def test_trainer_logs_the_pool_per_member(capsys):
    from pantheonrl_amd import trainer
    ego, members, env = trainer.run(["LiarsDice-v0", "PPO", "PPO", "DEFAULT", "--n-envs", "16", "-t", "256", "--seed", "1",
                                     "--ego-config", '{"n_steps": 8}', "--env-config", '{"log_interval": 1}'])
    out = capsys.readouterr().out
    for key in ("rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/episodes", "rollout/ep_rew_mean_vs_0",
                "rollout/ep_rew_mean_vs_1", "rollout/episodes_vs_1", "time/fps", "time/iterations", "time/total_timesteps"):
        assert key in out, key
    assert out.count("rollout/ep_rew_mean ") == 2                         # 256 / (16 x 8) iterations, one record each
    tot = env.episode_stats.read()["total"]
    counts = [m["count"] for m in tot["members"]]
    assert len(counts) == 2 and min(counts) > 0 and sum(counts) == tot["count"] == env.episodes


def test_trainer_logs_rps_and_log_interval_zero_never_reads(capsys):
    from pantheonrl_amd import trainer
    ego, _, env = trainer.run(["RPS-v0", "PPO", "PPO", "--n-envs", "16", "-t", "128", "--seed", "1", "--ego-config", '{"n_steps": 4}',
                               "--env-config", '{"log_interval": 1}'])
    out = capsys.readouterr().out
    assert "rollout/ep_rew_mean" in out and "rollout/ep_rew_mean_vs_0" not in out
    tot = env.episode_stats.read()["total"]
    assert tot["count"] == 128 and tot["mean_length"] == 1.0 and len(tot["members"]) == 1
    trainer.run(["RPS-v0", "PPO", "PPO", "--n-envs", "16", "-t", "128", "--seed", "1", "--ego-config", '{"n_steps": 4}',
                 "--env-config", '{"log_interval": 0}'])
    assert "rollout/" not in capsys.readouterr().out
