"""gpu: device-resident Liar's Dice against a pool of partners -- the scripted rule, the grouped forward against the untouched
per-member entry points, the native step against the walk, the walk against the host MultiAgentEnv, K = 1 against the
single-partner self-play, graph capture, ABI misuse and the trainer."""
import ctypes as C
import json
import os
from collections import deque

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- 1. the scripted rule ------------------------------------------------------------------------------------------------------
def test_scripted_rule_is_the_reference_default_agent_on_active_rows_only():
    ref = json.load(open(os.path.join(GOLD, "ref_default_agents.json")))
    obs = th.as_tensor(np.asarray(ref["liar_obs"], np.float32)).cuda().contiguous()
    want = np.asarray(ref["liar_actions"], np.int32)
    n = obs.shape[0]
    assert n == 400
    ctx = LC.ctx_of(LC.pool(4, 2, 2, ["scripted"])[1])
    active = th.as_tensor((np.arange(n) % 3 != 1).astype(np.uint8)).cuda()
    out = th.full((n, 2), -7, dtype=th.int32, device="cuda")
    nat.check(ctx.lib.ph_liar_default_actions(ctx.handle, obs.data_ptr(), active.data_ptr(), out.data_ptr(), n))
    got, act = out.cpu().numpy(), active.cpu().numpy().astype(bool)
    assert np.array_equal(got[act], want[act]) and (got[~act] == -7).all()
    nat.check(ctx.lib.ph_liar_default_actions(ctx.handle, obs.data_ptr(), None, out.data_ptr(), n))      # NULL = every row
    assert np.array_equal(out.cpu().numpy(), want)


# ---- 2. the grouped forward on its own ---------------------------------------------------------------------------------------
def _forward_case(name):
    """-> (kinds, partnerid, active)"""
    if name == "mixed50":       # member row counts [0, 1, 16, 17, 16], interleaved
        pid = np.array([2, 3, 4] * 16 + [3, 1], np.int32)
        assert np.bincount(pid, minlength=5).tolist() == [0, 1, 16, 17, 16]
        return ["learner", "frozen", "learner", "learner", "scripted"], pid, np.ones(50, np.uint8)
    if name == "one50":
        return ["frozen", "scripted", "learner"], np.full(50, 2, np.int32), np.ones(50, np.uint8)
    if name == "seven":
        return ["learner", "frozen", "scripted"], np.array([0, 1, 2, 0, 1, 2, 0], np.int32), np.array([1, 1, 1, 0, 1, 0, 1], np.uint8)
    kinds = {"all_frozen": "frozen", "all_scripted": "scripted"}[name]
    return [kinds, "learner"], np.zeros(23, np.int32), (np.arange(23) % 5 != 0).astype(np.uint8)


@pytest.mark.parametrize("case", ["mixed50", "one50", "seven", "all_frozen", "all_scripted"])
def test_grouped_forward_is_bitwise_the_per_member_entry_points(case):
    from pantheonrl_amd.vec import VecOnPolicyAgent
    kinds, pid_h, active_h = _forward_case(case)
    n, K, T, counter = len(pid_h), len(kinds), 4, 9
    rng = np.random.default_rng(5)
    obs_space = LC.spaces().observation_space
    obs = th.as_tensor((rng.random((n, 30)) * np.asarray(obs_space.nvec)).astype(np.int64).astype(np.float32)).cuda()
    pid, active = th.as_tensor(pid_h).cuda(), th.as_tensor(active_h).cuda()
    host = VecOnPolicyAgent(LC.ppo(n, 2, 0))
    ctx = LC.ctx_of(host)
    lib, h, spec = ctx.lib, ctx.handle, C.byref(host.model.policy.spec)
    sets = []
    for _ in range(2):                                    # two identical sets: one for the grouped launch, one for the yardstick
        members = [LC.member(kind, n, T, 20 + k) for k, kind in enumerate(kinds)]
        fill = np.random.default_rng(6)
        for k, m in enumerate(members):
            if kinds[k] != "learner":
                continue
            rb = m.model.rollout_buffer
            for key in LC.RB_KEYS:
                t = getattr(rb, key)
                t.copy_(th.as_tensor(fill.standard_normal(tuple(t.shape)).astype(np.float32)))
            m.pos.copy_(th.as_tensor(((2 * np.arange(n) + k) % (T + 1)).astype(np.int32)))   # every fill level, full columns included
            m.boundary.copy_(th.as_tensor(fill.integers(0, 2, n).astype(np.uint8)))
            m.values.fill_(-3.0)
            m.log_probs.fill_(-5.0)
        sets.append(members)
    grouped, plain = sets
    # episode_start of a row = the boundary flag of the member that sits at the table
    es = th.zeros(n, dtype=th.float32, device="cuda")
    for k, m in enumerate(grouped):
        if kinds[k] == "learner":
            es = th.where(pid == k, m.boundary.to(th.float32), es)
    es = es.contiguous()
    arr = (nat.PhPoolMember * K)()
    keep = []
    for k, m in enumerate(grouped):
        arr[k].kind = {"learner": nat.PH_POOL_LEARNER, "frozen": nat.PH_POOL_FROZEN, "scripted": nat.PH_POOL_SCRIPTED}[kinds[k]]
        if kinds[k] == "scripted":
            continue
        pol = m.model.policy if kinds[k] == "learner" else m.policy
        arr[k].params, arr[k].seed = pol.params.data_ptr(), pol._seed
        if kinds[k] == "learner":
            keep.append(m.model.rollout_buffer.c_struct())
            arr[k].rb = C.pointer(keep[-1])
            arr[k].pos, arr[k].boundary, arr[k].term, arr[k].open = (t.data_ptr() for t in (m.pos, m.boundary, m.term, m.open))
            arr[k].values, arr[k].log_probs = m.values.data_ptr(), m.log_probs.data_ptr()
    actions = th.full((n, 2), -7, dtype=th.int32, device="cuda")
    nat.check(lib.ph_pool_forward(h, spec, arr, K, obs.data_ptr(), pid.data_ptr(), active.data_ptr(), counter, actions.data_ptr(),
                                  es.data_ptr(), n))
    th.cuda.synchronize()
    got = actions.cpu().numpy()
    act = active_h.astype(bool)
    assert (got[~act] == -7).all()
    for k, (g, p) in enumerate(zip(grouped, plain)):
        mine = act & (pid_h == k)
        if kinds[k] == "scripted":
            want = th.full((n, 2), -7, dtype=th.int32, device="cuda")
            rows = th.as_tensor(mine.astype(np.uint8)).cuda()
            nat.check(lib.ph_liar_default_actions(h, obs.data_ptr(), rows.data_ptr(), want.data_ptr(), n))
            assert np.array_equal(got[mine], want.cpu().numpy()[mine])
            continue
        if kinds[k] == "frozen":
            p.policy._counter = counter - 1
            want = p.get_action(obs).cpu().numpy()            # ph_policy_forward without a buffer
            assert np.array_equal(got[mine], want[mine])
            continue
        pol, rb = p.model.policy, p.model.rollout_buffer
        want = th.zeros((n, 2), dtype=th.int32, device="cuda")
        mask = th.as_tensor(mine.astype(np.uint8)).cuda()
        nat.check(lib.ph_policy_forward_ragged(h, spec, pol.params.data_ptr(), obs.data_ptr(), None, pol._seed, counter, 0,
                                               want.data_ptr(), p.values.data_ptr(), p.log_probs.data_ptr(),
                                               C.byref(rb.c_struct()), p.pos.data_ptr(), mask.data_ptr(), es.data_ptr()))
        th.cuda.synchronize()
        assert np.array_equal(got[mine], want.cpu().numpy()[mine]), k
        assert np.array_equal(g.values.cpu().numpy(), p.values.cpu().numpy()), k               # cached for recorded rows only
        glp, plp = g.log_probs.cpu().numpy(), p.log_probs.cpu().numpy()
        assert np.array_equal(glp[mine], plp[mine]) and (glp[~mine] == -5.0).all(), k
        recorded = mine & (p.pos.cpu().numpy() < T)
        assert (g.values.cpu().numpy()[~recorded] == -3.0).all()
        if mine.sum() >= 10:
            assert recorded.any() and (mine & ~recorded).any()     # the case covers columns with room and full ones
        gb, pb = g.model.rollout_buffer.host(), rb.host()
        for key in gb:                                        # every recorded row, and nothing else anywhere in the buffer
            assert np.array_equal(gb[key], pb[key]), (k, key)
        assert np.array_equal(g.pos.cpu().numpy(), p.pos.cpu().numpy())                        # the forward does not advance


# ---- 3. the native step is bitwise the walk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", ["robin", "random"])
def test_native_pool_step_is_bitwise_the_walk(resample):
    kinds = ["learner", "frozen", "scripted", "learner"]
    a, b = (LC.run_pool(native, resample, kinds, E=48, T_ego=8, T_alt=4, steps=32) for native in (True, False))
    assert min(a["trained"]) >= 1 and a["trained"] == b["trained"], a["trained"]      # each learner trained: nothing vacuous
    assert a["ego_it"] >= 3 and a["episodes"] > 48
    assert a["pid"].min() >= 0 and a["pid"].max() == 3 and len(np.unique(a["pid"])) == 4
    LC.same_state(a, b)             # (only the recorded rows of a ragged buffer are defined: the snapshot holds no others)


# ---- 4. per-table replay through the host MultiAgentEnv ------------------------------------------------------------------------
@pytest.mark.parametrize("resample", ["robin", "random"])
def test_pool_walk_matches_the_host_multiagentenv_table_by_table(resample):
    from pantheonrl_amd.common import Agent, Observation
    from pantheonrl_amd.envs.liar import LiarDefaultAgent, LiarEnv

    class Shadow(LiarEnv):
        def __init__(self):
            super().__init__()
            self.deals = deque()

        def n_reset(self):
            ego_first, hands, pid = self.deals.popleft()
            if resample == "random":
                self.partnerids = [int(pid)]              # the device's draw; robin: the shadow's own resample_round_robin
            self.ego_next = bool(ego_first)
            self.history, self.egohand, self.althand = [], [int(x) for x in hands[:6]], [int(x) for x in hands[6:]]
            return (0 if self.ego_next else 1,), (Observation(self.getObs(self.ego_next)),)

    class Replay(Agent):
        """plays the moves the device sampled and keeps OnPolicyAgent's book (agents.py:172-198)"""
        def __init__(self):
            self.moves, self.rows, self.last_done = deque(), [], True

        def get_action(self, obs, record=True):
            act = self.moves.popleft()
            self.rows.append(dict(obs=np.asarray(obs.obs, np.float32), act=act, rew=0.0, start=float(self.last_done)))
            return act

        def update(self, reward, done):
            self.rows[-1]["rew"] += float(reward)
            self.last_done = bool(done)

    E, K, T, steps = 24, 4, 32, 32
    kinds = ["learner", "frozen", "scripted", "learner"]
    calls = {k: [] for k in range(K) if kinds[k] != "scripted"}

    def log_moves(members):
        for k in calls:
            def logged(obs, rec_mask, _inner=members[k].get_action, _log=calls[k]):
                acts = _inner(obs, rec_mask)
                _log.append((acts.cpu().numpy().copy(), rec_mask.cpu().numpy().astype(bool)))
                return acts
            members[k].get_action = logged
    sp, ego, members = LC.pool(E, T, 64, kinds, seed=2, native=False, resample=resample, before=log_moves)
    shadows = [Shadow() for _ in range(E)]
    partners = [[LiarDefaultAgent() if kinds[k] == "scripted" else Replay() for k in range(K)] for _ in range(E)]
    for s, ps in zip(shadows, partners):
        for p in ps:
            s.add_partner_agent(p)
        s.set_resample_policy("robin")

    def feed(reset_mask):
        hands, first, pid = sp.env.hands.cpu().numpy(), sp.ego_first.cpu().numpy(), sp.partnerid.cpu().numpy()
        for k, log in calls.items():
            for acts, mask in log:
                for e in np.nonzero(mask)[0]:
                    partners[e][k].moves.append(acts[e].copy())
            log.clear()
        for e in np.nonzero(reset_mask)[0]:
            shadows[e].deals.append((first[e], hands[e].copy(), pid[e]))

    pid0 = sp.partnerid.cpu().numpy()
    assert (pid0 == 1 % K).all() if resample == "robin" else ((pid0 >= 0) & (pid0 < K)).all()
    feed(np.ones(E, bool))              # the constructor's deal and the moves of the members that opened
    cur = [s.reset() for s in shadows]
    ego_rows, games, used = [], np.zeros(E, int), set()
    for t in range(steps):
        before = sp.obs_ego.cpu().numpy().copy()
        pid_now = sp.partnerid.cpu().numpy().copy()
        done = sp.step().cpu().numpy().astype(bool)
        a_ego = ego.actions.cpu().numpy().copy()
        feed(done)
        after = sp.obs_ego.cpu().numpy()
        used |= set(pid_now.tolist())
        assert (pid_now >= 0).all() and (pid_now < K).all()
        for e in range(E):
            assert np.array_equal(before[e], np.asarray(cur[e], np.float32)), (t, e)
            o, r, d, info = shadows[e].step(a_ego[e])
            assert info["_partnerid"] == [pid_now[e]], (t, e)
            assert bool(d) == bool(done[e]), (t, e)
            ego_rows.append((t, e, float(r), bool(d)))
            if d:
                games[e] += 1
                o = shadows[e].reset()
            cur[e] = o
            assert np.array_equal(after[e], np.asarray(o, np.float32)), (t, e)
            assert not any(p.moves for p in partners[e] if isinstance(p, Replay))
    assert games.min() >= 2 * K, games.min()                  # every table seats every member of a robin pool twice
    assert games.sum() == sp.episodes and used == set(range(K))
    th.cuda.synchronize()
    be = ego.model.rollout_buffer.host()
    for t, e, r, d in ego_rows:
        assert be["rewards"][t, e] == r
        if t + 1 < T:
            assert be["episode_starts"][t + 1, e] == float(d)
    for k, m in enumerate(members):
        if kinds[k] != "learner":
            continue
        ba, pos = m.model.rollout_buffer.host(), m.pos.cpu().numpy()
        term, opened = m.term.cpu().numpy(), m.open.cpu().numpy()
        assert m.iteration == 0 and len(set(pos.tolist())) > 1
        for e in range(E):
            rows = partners[e][k].rows
            assert pos[e] == len(rows), (k, e)
            if resample == "robin":
                assert len(rows) >= 2
            for i, row in enumerate(rows):
                assert np.array_equal(ba["observations"][i, e], row["obs"]), (k, e, i)
                assert np.array_equal(ba["actions"][i, e], row["act"].astype(np.float32))
                assert ba["rewards"][i, e] == row["rew"] and ba["episode_starts"][i, e] == row["start"], (k, e, i)
                assert np.isfinite(ba["values"][i, e]) and ba["log_probs"][i, e] < 0
            if rows:
                assert opened[e] == 1 and bool(term[e]) == partners[e][k].last_done
                assert rows[0]["start"] == 1.0


# ---- 5. K = 1 ------------------------------------------------------------------------------------------------------------------
def test_pool_of_one_learner_is_bitwise_the_single_partner_selfplay(monkeypatch):
    from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecLiarSelfPlay
    from pantheonrl_amd.vec import VecOnPolicyAgent
    monkeypatch.setenv("LIAR_PERSISTENT", "0")
    E, T_ego, T_alt, steps = 32, 8, 6, 24
    runs = []
    for pool in (True, False):
        if pool:
            sp, ego, members = LC.pool(E, T_ego, T_alt, ["learner"], seed=4)
            alt = members[0]
            assert alt.min_full == E
        else:
            ego, alt = VecOnPolicyAgent(LC.ppo(E, T_ego, 4)), RaggedVecOnPolicyAgent(LC.ppo(E, T_alt, 5))
            sp = VecLiarSelfPlay(E, ego, alt, seed=4 + 7, native=True)
            assert not sp.persistent
        for _ in range(steps // T_ego):
            sp.rollout_and_learn(T_ego)
        th.cuda.synchronize()
        out = dict(hands=sp.env.hands.cpu().numpy(), hist=sp.env.history.cpu().numpy(), obs=sp.obs_ego.cpu().numpy(),
                   pos=alt.pos.cpu().numpy(), flags=np.stack([t.cpu().numpy() for t in (alt.boundary, alt.term, alt.open)]),
                   acted=sp.alt_acted.cpu().numpy(), episodes=sp.episodes, it=(ego.iteration, alt.iteration),
                   values=alt.values.cpu().numpy(), pe=ego.model.policy.get_flat_params(), pa=alt.model.policy.get_flat_params())
        out.update({"e_" + k: v for k, v in ego.model.rollout_buffer.host().items() if k in LC.RB_KEYS})
        out.update({"a_" + k: v for k, v in alt.model.rollout_buffer.host().items() if k in LC.RB_KEYS})
        runs.append(out)
    a, b = runs
    assert a["it"][0] == 3 and a["it"][1] >= 1
    for key in a:
        x, y = a[key], b[key]
        if key.startswith("a_"):
            x, y = LC.recorded_rows(x, a["pos"]), LC.recorded_rows(y, a["pos"])
        assert np.array_equal(x, y), key


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------
def test_native_pool_step_does_no_host_work_and_captures():
    sp, ego, members = LC.pool(32, 8, 8, ["learner", "frozen", "scripted", "learner"], seed=3)
    stream = th.cuda.Stream(device=sp.dev)
    th.cuda.synchronize()
    with th.cuda.stream(stream):
        for c in (1, 2):
            sp._native_call(c, ego_pos=c - 1)
        stream.synchronize()
        ctx = sp.env.ctx
        sp._bind()
        nat.check(ctx.lib.ph_graph_begin(ctx.handle))
        try:
            for c in (3, 4, 5, 6):
                sp._native_call(c, ego_pos=c - 1)
        finally:
            gid = C.c_int(-1)
            nat.check(ctx.lib.ph_graph_end(ctx.handle, C.byref(gid)))
        assert gid.value >= 0
        before = sum(m.pos.clone().sum() for m in sp.learners)
        episodes = sp.episodes
        nat.check(ctx.lib.ph_graph_launch(ctx.handle, gid.value))
        stream.synchronize()
    th.cuda.synchronize()
    assert int((sum(m.pos.sum() for m in sp.learners) - before).item()) > 0 and sp.episodes > episodes
    assert np.isfinite(ego.model.rollout_buffer.host()["values"][:6]).all()


# ---- 7. ABI misuse ---------------------------------------------------------------------------------------------------------------
def test_pool_abi_misuse_is_reported_not_fatal():
    from pantheonrl_amd import spaces as sps
    sp, ego, members = LC.pool(16, 4, 4, ["learner", "frozen", "scripted"], seed=1)
    ctx = sp.env.ctx
    sp._bind()
    lib, h, d = ctx.lib, ctx.handle, sp._desc
    err = lambda: lib.ph_last_error()  # noqa: E731
    assert lib.ph_liar_pool_step(h, None, 0, 1, 0) != 0 and b"null" in err()
    for field, bad, word in (("n_members", 0, b"1..PH_MAX_POOL"), ("n_members", 9, b"1..PH_MAX_POOL"), ("resample", 5, b"resample"),
                             ("n", 0, b"incomplete"), ("n", 8, b"E = n"), ("partnerid", None, b"incomplete")):
        good = getattr(d, field)
        setattr(d, field, bad)
        assert lib.ph_liar_pool_step(h, C.byref(d), 0, 1, 0) != 0 and word in err(), field
        setattr(d, field, good)
    assert lib.ph_liar_pool_step(h, C.byref(d), 4, 1, 0) != 0 and b"ego_pos" in err()
    arr = sp._member_arr
    for field, word in (("rb", b"rollout buffer"), ("pos", b"learner needs"), ("params", b"null params")):
        # (a pointer-typed field reads back as a view of the structure's own bytes: the learner's buffer is restored from its record)
        good = C.pointer(sp._member_rbc[0]) if field == "rb" else getattr(arr[0], field)
        setattr(arr[0], field, None)
        assert lib.ph_liar_pool_step(h, C.byref(d), 0, 1, 0) != 0 and word in err(), field
        setattr(arr[0], field, good)
    arr[1].kind = 7
    assert lib.ph_liar_pool_step(h, C.byref(d), 0, 1, 0) != 0 and b"unknown kind" in err()
    arr[1].kind = nat.PH_POOL_FROZEN
    # a spec outside the 16-row one-hot class of the game: RPS, and a Box observation
    rps = sps.make_spec(sps.Discrete(1), sps.Discrete(3))
    box = sps.make_spec(sps.Box(-1, 1, (30,)), sps.MultiDiscrete([7, 12]))
    good = C.pointer(ego.model.policy.spec)
    for spec in (rps, box):
        d.spec = C.pointer(spec)
        assert lib.ph_liar_pool_step(h, C.byref(d), 0, 1, 0) != 0 and b"one-hot" in err()
    d.spec = good
    E = 16
    pid, act = sp.partnerid, sp.ones8
    out = th.zeros((E, 2), dtype=th.int32, device=sp.dev)
    es = th.zeros(E, dtype=th.float32, device=sp.dev)
    fwd = lambda spec=good, mem=arr, K=3, obs=sp.obs_alt.data_ptr(), esp=es.data_ptr(): lib.ph_pool_forward(  # noqa: E731
        h, spec, mem, K, obs, pid.data_ptr(), act.data_ptr(), 1, out.data_ptr(), esp, E)
    assert fwd(K=0) != 0 and b"1..PH_MAX_POOL" in err()
    assert fwd(K=9) != 0 and b"1..PH_MAX_POOL" in err()
    assert fwd(mem=None) != 0 and b"null member" in err()
    assert fwd(obs=None) != 0 and b"null" in err()
    assert fwd(esp=None) != 0 and b"episode_start_in" in err()
    assert fwd(spec=C.pointer(rps)) != 0 and b"one-hot" in err()
    assert lib.ph_liar_default_actions(h, None, None, out.data_ptr(), E) != 0 and b"null" in err()
    assert lib.ph_liar_default_actions(h, sp.obs_alt.data_ptr(), None, out.data_ptr(), 0) != 0 and b"positive" in err()
    # ... and the process is alive and the pool still steps
    assert fwd() == 0
    sp.step()
    th.cuda.synchronize()
    assert np.isfinite(ego.model.rollout_buffer.host()["values"][0]).all()
    from pantheonrl_amd.envs.vec import VecLiarDefaultPartner, VecLiarPartnerPool
    with pytest.raises(nat.NativeError, match="1..8"):
        VecLiarPartnerPool(16, ego, [VecLiarDefaultPartner()] * 9)
    with pytest.raises(nat.NativeError, match="resample"):
        VecLiarPartnerPool(16, ego, [VecLiarDefaultPartner()], resample="sticky")


# ---- 8. the trainer --------------------------------------------------------------------------------------------------------------
def test_trainer_runs_a_pool_of_ppo_fixed_and_default_partners(tmp_path):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import FrozenVecPartner, VecLiarDefaultPartner, VecLiarPartnerPool
    from pantheonrl_amd.trainer import run
    old = LC.ppo(32, 8, 9)
    old.save(str(tmp_path / "old"))
    fixed = json.dumps({"type": "PPO", "location": str(tmp_path / "old")})
    ego, partners, env = run(["LiarsDice-v0", "PPO", "PPO", "FIXED", "DEFAULT", "--n-envs", "32", "-t", "8192", "--seed", "1",
                              "--ego-config", '{"n_steps": 16, "n_epochs": 2}',
                              "--alt-config", '{"n_steps": 4, "n_epochs": 2}', fixed, "{}",
                              "--ego-save", str(tmp_path / "ego"), "--alt-save", str(tmp_path / "alt")])
    assert isinstance(env, VecLiarPartnerPool) and env.native and env.K == 3 and env.resample == "robin"
    assert isinstance(partners[1], FrozenVecPartner) and isinstance(partners[2], VecLiarDefaultPartner)
    assert env.ego.iteration == 16 and partners[0].iteration >= 1                      # both learners update
    assert partners[0].min_full == 32 // 3
    assert np.array_equal(partners[1].policy.get_flat_params(), old.policy.get_flat_params())     # frozen stays frozen
    for path, model in (("ego", ego), ("alt", partners[0].model)):
        again = PPO.load(str(tmp_path / path))
        assert np.array_equal(again.policy.get_flat_params(), model.policy.get_flat_params())
    # several learners: one checkpoint each under DIR/i; random resampling through --env-config
    ego, partners, env = run(["LiarsDice-v0", "PPO", "PPO", "DEFAULT", "PPO", "--n-envs", "32", "-t", "2048", "--seed", "2",
                              "--ego-config", '{"n_steps": 16, "n_epochs": 1}',
                              "--alt-config", '{"n_steps": 4, "n_epochs": 1}', "{}", '{"n_steps": 4, "n_epochs": 1}',
                              "--env-config", '{"resample": "random", "probegostart": 0.25}', "--alt-save", str(tmp_path / "many")])
    assert env.resample == "random" and env.probegostart == 0.25 and [m.iteration >= 1 for m in env.learners] == [True, True]
    assert sorted(os.listdir(tmp_path / "many")) == ["0.zip", "2.zip"]
    for i in (0, 2):
        again = PPO.load(str(tmp_path / "many" / str(i)))
        assert np.array_equal(again.policy.get_flat_params(), partners[i].model.policy.get_flat_params())
