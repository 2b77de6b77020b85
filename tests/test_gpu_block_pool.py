"""gpu: the block worlds against a pool of constructors on the device -- the grouped constructor forward with learner tiles against
the members' own entry points, the native step against its walk after every step, the walk against the host MultiAgentEnv table by
table, a pool of one learner against VecBlockSelfPlay, graph capture, ABI misuse, the per-member episode statistics and the command
lines.  Every comparison is exact."""
import ctypes as C
import json
import os
from collections import deque

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from pantheonrl_amd.envs import blockworld as bw
from tests import block_pool_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOL4 = ["learner", "frozen", "scripted", "learner"]


# ---- 1. the grouped forward -----------------------------------------------------------------------------------------------------------
def _forward_case(name, n=72):
    """-> (kinds, member_of, active): about a third of the rows inactive; in "mixed" member 0 (a learner) holds more than 16 active
    rows -- a full tile and a partial one; in "absent" member 3 (a learner) has rows but none of them is active"""
    rng = np.random.RandomState(3)
    kinds = {"mixed": POOL4, "absent": POOL4, "learners": ["learner"] * 4, "frozen": ["frozen"] * 4, "scripted": ["scripted"] * 4}[name]
    ids = np.array([0] * 33 + [1] * 13 + [2] * 13 + [3] * 13, np.int32)
    active = np.ones(n, bool)
    for k in range(4):
        rows = np.nonzero(ids == k)[0]
        active[rng.choice(rows, len(rows) // 3, replace=False)] = False
    if name == "absent":
        active[ids == 3] = False
    perm = rng.permutation(n)
    return kinds, ids[perm], active[perm]


def _member_array(variant, kinds, members, keep):
    arr = (nat.PhPoolMember * len(kinds))()
    for k, m in enumerate(members):
        arr[k].kind = BC.KINDS[kinds[k]]
        if kinds[k] == "scripted":
            arr[k].seed = m.rule
            continue
        pol = m.model.policy if kinds[k] == "learner" else m.policy
        arr[k].params, arr[k].seed = pol.params.data_ptr(), pol._seed
        if kinds[k] == "learner":
            keep.append(m.model.rollout_buffer.c_struct())
            arr[k].rb = C.pointer(keep[-1])
            arr[k].pos, arr[k].boundary, arr[k].term, arr[k].open = (t.data_ptr() for t in (m.pos, m.boundary, m.term, m.open))
            arr[k].values, arr[k].log_probs = m.values.data_ptr(), m.log_probs.data_ptr()
    return arr


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", ["mixed", "absent", "learners", "frozen", "scripted"])
def test_grouped_forward_is_bitwise_the_members_own_entry_points(variant, case):
    from pantheonrl_amd.envs.vec import VecBlockWorld
    from pantheonrl_amd.spaces import make_spec
    kinds, ids_h, active_h = _forward_case(case)
    n, K, T, counter = len(ids_h), len(kinds), 4, 9
    counts = np.bincount(ids_h[active_h], minlength=K)
    assert counts[0] > 16 and 20 <= (~active_h).sum() <= 36 and (case != "absent" or counts[3] == 0)
    spaces = VecBlockWorld.seat_spaces(variant)[1]
    spec = make_spec(spaces.observation_space, spaces.action_space)
    nvec = np.asarray(spaces.observation_space.nvec)
    A = len(spaces.action_space.nvec)
    obs = th.as_tensor((np.random.RandomState(variant).rand(n, len(nvec)) * nvec).astype(np.int64).astype(np.float32)).to(DEV)
    ids, active = th.as_tensor(ids_h).to(DEV), th.as_tensor(active_h.astype(np.uint8)).to(DEV)
    sets = []
    for _ in range(2):                                    # two identical sets: one for the grouped launch, one for the yardstick
        members = [BC.member(variant, kind, n, T, 20 + k) for k, kind in enumerate(kinds)]
        fill = np.random.default_rng(6)
        for k, m in enumerate(members):
            if kinds[k] != "learner":
                continue
            rb = m.model.rollout_buffer
            for key in BC.RB_KEYS:
                t = getattr(rb, key)
                t.copy_(th.as_tensor(fill.standard_normal(tuple(t.shape)).astype(np.float32)))
            m.pos.copy_(th.as_tensor(((2 * np.arange(n) + k) % (T + 1)).astype(np.int32)))   # every fill level, full columns included
            m.boundary.copy_(th.as_tensor(fill.integers(0, 2, n).astype(np.uint8)))
            m.values.fill_(-3.0)
            m.log_probs.fill_(-5.0)
        sets.append(members)
    grouped, plain = sets
    es = th.zeros(n, dtype=th.float32, device=DEV)          # episode_start of a row = the boundary flag of the member at the table
    for k, m in enumerate(grouped):
        if kinds[k] == "learner":
            es = th.where(ids == k, m.boundary.to(th.float32), es)
    es = es.contiguous()
    keep = []
    arr = _member_array(variant, kinds, grouped, keep)
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
    lib, h = ctx.lib, ctx.handle
    actions = th.full((n, A), -7, dtype=th.int32, device=DEV)
    nat.check(lib.ph_block_pool_forward(h, C.byref(spec), arr, K, obs.data_ptr(), ids.data_ptr(), active.data_ptr(), counter,
                                        actions.data_ptr(), es.data_ptr(), n))
    th.cuda.synchronize()
    got = actions.cpu().numpy()
    assert (got[~active_h] == -7).all()
    for k, (g, p) in enumerate(zip(grouped, plain)):
        mine = active_h & (ids_h == k)
        if kinds[k] == "scripted":
            want = th.full((n, A), -7, dtype=th.int32, device=DEV)
            rows = th.as_tensor(mine.astype(np.uint8)).to(DEV)
            nat.check(lib.ph_block_scripted_actions(h, variant, p.rule, obs.data_ptr(), rows.data_ptr(), want.data_ptr(), n))
            assert np.array_equal(got[mine], want.cpu().numpy()[mine]), k
            continue
        if kinds[k] == "frozen":
            p.policy._counter = counter - 1
            want = p.get_action(obs).cpu().numpy()            # ph_policy_forward without a buffer
            assert np.array_equal(got[mine], want[mine]), k
            continue
        pol, rb = p.model.policy, p.model.rollout_buffer
        want = th.zeros((n, A), dtype=th.int32, device=DEV)
        mask = th.as_tensor(mine.astype(np.uint8)).to(DEV)
        pol._bind()
        nat.check(pol.ctx.lib.ph_policy_forward_ragged(pol.ctx.handle, C.byref(spec), pol.params.data_ptr(), obs.data_ptr(), None, pol._seed,
                                                       counter, 0, want.data_ptr(), p.values.data_ptr(), p.log_probs.data_ptr(),
                                                       C.byref(rb.c_struct()), p.pos.data_ptr(), mask.data_ptr(), es.data_ptr()))
        th.cuda.synchronize()
        assert np.array_equal(got[mine], want.cpu().numpy()[mine]), k
        assert np.array_equal(g.values.cpu().numpy(), p.values.cpu().numpy()), k               # cached for recorded rows only
        glp, plp = g.log_probs.cpu().numpy(), p.log_probs.cpu().numpy()
        assert np.array_equal(glp[mine], plp[mine]) and (glp[~mine] == -5.0).all(), k
        recorded = mine & (p.pos.cpu().numpy() < T)
        assert (g.values.cpu().numpy()[~recorded] == -3.0).all() and (g.values.cpu().numpy()[recorded] != -3.0).all()
        if mine.sum() >= 8:
            assert recorded.any() and (mine & ~recorded).any()     # the case covers columns with room and full ones
        gb, pb = g.model.rollout_buffer.host(), rb.host()
        for key in gb:                                        # every recorded row, and nothing else anywhere in the buffer
            assert np.array_equal(gb[key], pb[key]), (k, key)
        assert np.array_equal(g.pos.cpu().numpy(), p.pos.cpu().numpy())                        # the forward does not advance
        assert np.array_equal(g.pos.cpu().numpy(), ((2 * np.arange(n) + k) % (T + 1)).astype(np.int32))


# ---- 2. the native step is bitwise the walk, after every step -------------------------------------------------------------------------
@pytest.mark.parametrize("resample", ["robin", "random"])
@pytest.mark.parametrize("variant", [0, 1])
def test_native_pool_step_is_bitwise_the_walk_after_every_step(variant, resample):
    E, steps = 48, 32
    runs = []
    for native in (True, False):
        sp, ego, members = BC.pool(variant, E, 8, 4, POOL4, seed=11, native=native, resample=resample)
        snaps, seated = [BC.snapshot(sp, ego, members)], set()
        for _ in range(steps):
            seated |= set(sp.partnerid.cpu().numpy().tolist())
            sp.step()
            for m in sp.learners:
                if m.full():
                    m.learn_from_buffer()
            snaps.append(BC.snapshot(sp, ego, members))
        runs.append((snaps, seated, [m.iteration for m in sp.learners], sp.episodes, ego.iteration))
    (a, _, _, _, _), (b, seated, trained, episodes, ego_it) = runs
    # judged on the walk alone, nothing is vacuous
    assert min(trained) >= 1 and seated == set(range(4)) and episodes > E and ego_it >= 3, (trained, seated, episodes, ego_it)
    for t, (x, y) in enumerate(zip(a, b)):
        BC.same_state(x, y, t)


# ---- 3. the walk against the host MultiAgentEnv, table by table -----------------------------------------------------------------------
@pytest.mark.parametrize("resample", ["robin", "random"])
@pytest.mark.parametrize("variant", [0, 1])
def test_pool_walk_matches_the_host_multiagentenv_table_by_table(variant, resample):
    """Every table of the walk is shadowed by a host game driven through MultiAgentEnv.step with the device's worlds (and, for
    `random`, its draws) and the moves the learners and the frozen member sampled; the host scripted agent plays its own moves.
    With p(end) >= 0.40 per token the chance that one table ends fewer than 8 games in 64 tokens is below 1e-5; the seeds are fixed."""
    from pantheonrl_amd.common import Agent, Observation
    game = (bw.SimpleBlockEnv, bw.BlockEnv)[variant]
    scripted_agent = (bw.SBWDefaultAgent, bw.DefaultConstructorAgent)[variant]

    class Shadow(game):
        def __init__(self):
            super().__init__()
            self.worlds = deque()

        def n_reset(self):
            world, pid = self.worlds.popleft()
            if resample == "random":
                self.partnerids = [int(pid)]              # the device's draw; robin: the shadow's own resample_round_robin
            self.ego_next = True
            if variant:
                self.gridworld, self.constructor_obs = world.astype(float), np.zeros((7, 7))
            else:
                self.gridworld = [[int(v) for v in b] for b in world]
                self.constructor_obs = [[b[0], b[1], b[2], 0] for b in self.gridworld]
            self.last_token = 0
            return (0,), (Observation(self.get_obs(True)),)

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

    E, K, T, steps = 24, 4, 64, 64
    kinds = POOL4
    calls = {k: [] for k in range(K) if kinds[k] != "scripted"}

    def log_moves(members):
        for k in calls:
            def logged(obs, rec_mask, _inner=members[k].get_action, _log=calls[k]):
                acts = _inner(obs, rec_mask)
                _log.append((acts.cpu().numpy().copy(), rec_mask.cpu().numpy().astype(bool)))
                return acts
            members[k].get_action = logged
    sp, ego, members = BC.pool(variant, E, T, 64, kinds, seed=2, native=False, resample=resample, before=log_moves)
    shadows = [Shadow() for _ in range(E)]
    partners = [[scripted_agent() if kinds[k] == "scripted" else Replay() for k in range(K)] for _ in range(E)]
    for s, ps in zip(shadows, partners):
        for p in ps:
            s.add_partner_agent(p)
        s.set_resample_policy("robin")

    def feed(reset_mask):
        state, pid = sp.env.state.cpu().numpy(), sp.partnerid.cpu().numpy()
        for k, log in calls.items():
            for acts, mask in log:
                for e in np.nonzero(mask)[0]:
                    partners[e][k].moves.append(acts[e].copy())
            log.clear()
        for e in np.nonzero(reset_mask)[0]:
            world, view, token = bw.unpack_state(variant, state[e])
            assert token == 0 and not np.asarray(view).any()
            shadows[e].worlds.append((world, pid[e]))

    pid0 = sp.partnerid.cpu().numpy()
    assert (pid0 == 1 % K).all() if resample == "robin" else ((pid0 >= 0) & (pid0 < K)).all()
    feed(np.ones(E, bool))
    cur = [s.reset() for s in shadows]
    ego_rows, games, used = [], np.zeros(E, int), set()
    for t in range(steps):
        before = sp.obs_ego.cpu().numpy().copy()
        pid_now = sp.partnerid.cpu().numpy().copy()
        done = sp.step().cpu().numpy().astype(bool)
        tokens = ego.actions.cpu().numpy().copy()
        feed(done)
        after = sp.obs_ego.cpu().numpy()
        used |= set(pid_now.tolist())
        assert (pid_now >= 0).all() and (pid_now < K).all()
        for e in range(E):
            assert np.array_equal(before[e], np.asarray(cur[e], np.float32)), (t, e)
            o, r, d, info = shadows[e].step(tokens[e])
            assert info["_partnerid"] == [pid_now[e]], (t, e)
            assert bool(d) == bool(done[e]), (t, e)
            ego_rows.append((t, e, np.float32(r), bool(d)))
            if d:
                games[e] += 1
                o = shadows[e].reset()
            cur[e] = o
            assert np.array_equal(after[e], np.asarray(o, np.float32)), (t, e)
            assert not any(p.moves for p in partners[e] if isinstance(p, Replay))
    if resample == "robin":
        assert games.min() >= 2 * K, games.min()              # every table seats every member twice
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
                assert len(rows) >= 1
            for i, row in enumerate(rows):
                assert np.array_equal(ba["observations"][i, e], row["obs"]), (k, e, i)
                assert np.array_equal(ba["actions"][i, e], np.asarray(row["act"], np.float32))
                assert ba["rewards"][i, e] == np.float32(row["rew"]) and ba["episode_starts"][i, e] == row["start"], (k, e, i)
                assert np.isfinite(ba["values"][i, e]) and ba["log_probs"][i, e] < 0
            if rows:
                assert opened[e] == 1 and bool(term[e]) == partners[e][k].last_done
                assert rows[0]["start"] == 1.0


# ---- 4. K = 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_pool_of_one_learner_is_bitwise_the_block_selfplay(variant):
    from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecBlockSelfPlay
    from pantheonrl_amd.vec import VecOnPolicyAgent
    E, T_ego, T_alt, steps = 32, 8, 6, 32
    runs = []
    for pool in (True, False):
        if pool:
            sp, ego, members = BC.pool(variant, E, T_ego, T_alt, ["learner"], seed=4)
            alt = members[0]
            assert alt.min_full == E and sp.K == 1
        else:
            ego = VecOnPolicyAgent(BC.ppo(variant, 0, E, T_ego, 4))
            BC.bias_end_token(ego.model.policy)
            alt = RaggedVecOnPolicyAgent(BC.ppo(variant, 1, E, T_alt, 5))
            sp = VecBlockSelfPlay(variant, E, ego, alt, seed=4 + 7, native=True)
        for _ in range(steps // T_ego):
            sp.rollout_and_learn(T_ego)
        th.cuda.synchronize()
        pos = alt.pos.cpu().numpy()
        out = dict(state=sp.env.state.cpu().numpy(), obs=sp.obs_ego.cpu().numpy(), pos=pos,
                   flags=np.stack([t.cpu().numpy() for t in (alt.boundary, alt.term, alt.open)]),
                   acted=sp.alt_acted.cpu().numpy(), episodes=sp.episodes, it=(ego.iteration, alt.iteration),
                   values=alt.values.cpu().numpy(), pe=ego.model.policy.get_flat_params(), pa=alt.model.policy.get_flat_params())
        out.update({"e_" + k: v for k, v in ego.model.rollout_buffer.host().items() if k in BC.RB_KEYS})
        out.update({"a_" + k: BC.recorded_rows(v, pos) for k, v in alt.model.rollout_buffer.host().items() if k in BC.RB_KEYS})
        runs.append(out)
    a, b = runs
    assert a["it"][0] == 4 and a["it"][1] >= 1 and a["episodes"] > E
    BC.same_state(a, b)


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------------
def test_native_pool_step_does_no_host_work_and_its_replay_is_the_launch_by_launch_steps():
    """after two eager steps have sized the workspaces and uploaded the member table, four ph_block_pool_step calls are captured
    into a hipGraph (an allocation, an upload or a synchronisation inside a capture is an error); the replay leaves what six
    launch-by-launch steps leave"""
    snaps = []
    for capture in (False, True):
        sp, ego, members = BC.pool(1, 32, 8, 8, POOL4, seed=3)
        stream = th.cuda.Stream(device=sp.dev)
        th.cuda.synchronize()
        with th.cuda.stream(stream):
            for c in (1, 2):
                sp._native_call(c, ego_pos=c - 1)
            stream.synchronize()
            if not capture:
                for c in (3, 4, 5, 6):
                    sp._native_call(c, ego_pos=c - 1)
            else:
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
                before = sum(int(m.pos.sum().item()) for m in sp.learners)
                nat.check(ctx.lib.ph_graph_launch(ctx.handle, gid.value))
                stream.synchronize()
                assert sum(int(m.pos.sum().item()) for m in sp.learners) > before
            stream.synchronize()
        snaps.append(BC.snapshot(sp, ego, members))
    assert snaps[0]["episodes"] > 0 and np.isfinite(snaps[0]["e_observations"][:6]).all()
    BC.same_state(snaps[0], snaps[1])


# ---- 6. ABI misuse --------------------------------------------------------------------------------------------------------------------
def test_pool_abi_misuse_is_reported_not_fatal():
    from pantheonrl_amd.envs.vec import VecBlockPartnerPool, VecBlockScriptedPartner, VecBlockWorld
    from pantheonrl_amd.spaces import make_spec
    E = 16
    sp, ego, members = BC.pool(1, E, 4, 4, ["learner", "frozen", "scripted"], seed=1)
    ctx = sp.env.ctx
    sp._bind()
    th.cuda.synchronize()
    before = BC.snapshot(sp, ego, members)
    lib, h, d = ctx.lib, ctx.handle, sp._desc
    err = lambda: lib.ph_last_error()  # noqa: E731
    step = lambda: lib.ph_block_pool_step(h, C.byref(d), 0, 1, 0)  # noqa: E731
    assert lib.ph_block_pool_step(h, None, 0, 1, 0) != 0 and b"null" in err()
    other = VecBlockWorld.seat_spaces(0)
    wrong_alt = make_spec(other[1].observation_space, other[1].action_space)
    wrong_ego = make_spec(other[0].observation_space, other[0].action_space)
    for field, bad, word in (("variant", 2, b"variant"), ("n", 0, b"positive"), ("n", 8, b"E = n"), ("n_members", 0, b"1..PH_MAX_POOL"),
                             ("n_members", 9, b"1..PH_MAX_POOL"), ("resample", 5, b"resample"), ("state", None, b"incomplete"),
                             ("partnerid", None, b"incomplete"), ("alt_acted", None, b"incomplete"), ("ego_rb", None, b"incomplete"),
                             ("state", sp.env.state.data_ptr() + 4, b"16-byte aligned"),
                             ("alt_spec", C.pointer(wrong_alt), b"planner / constructor spaces"),
                             ("ego_spec", C.pointer(wrong_ego), b"planner / constructor spaces"),
                             ("variant", 0, b"planner / constructor spaces")):
        good = {"ego_rb": C.pointer(sp._ego_rbc), "alt_spec": C.pointer(sp._alt_spec),
                "ego_spec": C.pointer(ego.model.policy.spec)}.get(field, getattr(d, field))
        setattr(d, field, bad)
        assert step() != 0 and word in err(), (field, err())
        setattr(d, field, good)
    assert lib.ph_block_pool_step(h, C.byref(d), 4, 1, 0) != 0 and b"ego_pos" in err()
    arr = sp._member_arr
    for field, word in (("rb", b"rollout buffer"), ("pos", b"learner needs"), ("params", b"null params")):
        good = C.pointer(sp._member_rbc[0]) if field == "rb" else getattr(arr[0], field)
        setattr(arr[0], field, None)
        assert step() != 0 and word in err(), field
        setattr(arr[0], field, good)
    arr[1].kind = nat.PH_POOL_CLONE
    assert step() != 0 and b"PH_POOL_CLONE" in err()
    arr[1].kind = 7
    assert step() != 0 and b"unknown kind" in err()
    arr[1].kind = nat.PH_POOL_FROZEN
    arr[2].seed = nat.PH_BLOCK_RULE_EASY                      # EASY on BlockEnv-v1
    assert step() != 0 and b"BlockEnv-v0 only" in err()
    arr[2].seed = nat.PH_BLOCK_RULE_DEFAULT
    # the grouped forward on its own
    out = th.full((E, 3), -7, dtype=th.int32, device=sp.dev)
    es = th.zeros(E, dtype=th.float32, device=sp.dev)
    ones = th.ones(E, dtype=th.uint8, device=sp.dev)
    good_spec = C.pointer(sp._alt_spec)
    fwd = lambda spec=good_spec, mem=arr, K=3, obs=sp.obs_alt.data_ptr(), esp=es.data_ptr(), n=E: lib.ph_block_pool_forward(  # noqa: E731
        h, spec, mem, K, obs, sp.partnerid.data_ptr(), ones.data_ptr(), 1, out.data_ptr(), esp, n)
    assert fwd(K=0) != 0 and b"1..PH_MAX_POOL" in err()
    assert fwd(K=9) != 0 and b"1..PH_MAX_POOL" in err()
    assert fwd(mem=None) != 0 and b"null member" in err()
    assert fwd(obs=None) != 0 and b"null" in err()
    assert fwd(esp=None) != 0 and b"episode_start_in" in err()
    assert fwd(n=8) != 0 and b"E = n" in err()
    # a learner in a table whose spec is off the 16-row one-hot class: the BlockEnv-v1 planner's 98 components run on the 32-row body
    assert fwd(spec=C.pointer(ego.model.policy.spec), K=1) != 0 and b"16-row one-hot" in err()
    # ph_block_group_forward keeps refusing learners, in its own words
    assert lib.ph_block_group_forward(h, good_spec, arr, 3, sp.obs_alt.data_ptr(), sp.partnerid.data_ptr(), ones.data_ptr(), 1,
                                      out.data_ptr(), E) != 0 and b"an evaluation seats frozen and scripted members only" in err()
    # nothing was launched: the pool is where it was and the actions are untouched
    th.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    BC.same_state(before, BC.snapshot(sp, ego, members))
    # ... and the process is alive and the pool still steps
    sp.step()
    th.cuda.synchronize()
    assert ego.model.rollout_buffer.pos == 1 and np.isfinite(ego.model.rollout_buffer.host()["values"][0]).all()
    with pytest.raises(nat.NativeError, match="1..8"):
        VecBlockPartnerPool(1, E, ego, [VecBlockScriptedPartner(1)] * 9)
    with pytest.raises(nat.NativeError, match="resample"):
        VecBlockPartnerPool(1, E, ego, [VecBlockScriptedPartner(1)], resample="sticky")


# ---- 7. episode statistics per member -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", ["robin", "random"])
@pytest.mark.parametrize("variant", [0, 1])
def test_episode_statistics_are_credited_to_the_member_that_sat(variant, resample):
    """EpisodeStats attaches to the block pool unchanged.  The recomputation reads the ego's reward and episode-start planes after
    every rollout and the `partnerid` logged in front of every step.  A game's return is an f32 sum in row order on both sides;
    count, the f64 sum of returns (f32 values of one binade range: exact in f64 in any order) and the sum of lengths are compared
    exactly, and for BlockEnv-v0, whose rewards are multiples of 20, the f64 sum of squares as well."""
    from pantheonrl_amd.episode_stats import EpisodeStats
    E, T, K, iters = 32, 16, 4, 3
    sp, ego, members = BC.pool(variant, E, T, 4, POOL4, seed=6, resample=resample)
    stats = EpisodeStats(ego, sp)
    assert sp.episode_stats is stats and stats.K == K and stats.pool
    rb = ego.model.rollout_buffer
    want = np.zeros((K, 4))
    ret, length = np.zeros(E, np.float32), np.zeros(E, np.int64)
    for _ in range(iters):
        pids = []
        for _ in range(T):
            pids.append(sp.partnerid.cpu().numpy().copy())
            sp.step()
        th.cuda.synchronize()
        planes = rb.host()
        rewards, starts = planes["rewards"], planes["episode_starts"]
        last = ego._last_episode_starts.cpu().numpy()
        for t in range(T):
            ended = (starts[t + 1] if t + 1 < T else last) != 0
            ret = ret + rewards[t]
            length += 1
            for e in np.flatnonzero(ended):
                x = np.float64(ret[e])
                want[pids[t][e]] += (1.0, x, x * x, float(length[e]))
            ret[ended], length[ended] = 0.0, 0
        ego.learn_from_buffer()                 # the rollout's scan
        for m in sp.learners:
            if m.full():
                m.learn_from_buffer()
    rep = stats.read()                          # compares the replayed members with the pool's partnerid, too
    got = stats.stats.cpu().numpy()
    cols = [0, 1, 2, 3] if variant == 0 else [0, 1, 3]
    assert np.array_equal(got[:, cols], want[:, cols]), (got, want)
    assert np.array_equal(stats.member.cpu().numpy(), sp.partnerid.cpu().numpy())
    assert rep["total"]["count"] == sp.episodes == int(want[:, 0].sum()) and (want[:, 0] > 0).all()
    assert [m["count"] for m in rep["total"]["members"]] == want[:, 0].astype(int).tolist()
    assert np.array_equal(stats.carry_return.cpu().numpy(), ret) and np.array_equal(stats.carry_length.cpu().numpy(), length)


# ---- 8. the command lines -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_trainer_and_crossplay_command_lines(variant, tmp_path, capsys):
    from pantheonrl_amd import PPO, crossplay
    from pantheonrl_amd.envs.vec import FrozenVecPartner, VecBlockPartnerPool, VecBlockScriptedPartner
    from pantheonrl_amd.trainer import run
    game = f"BlockEnv-v{variant}"
    old = BC.ppo(variant, 1, 16, 8, 9)
    old.save(str(tmp_path / "old"))
    fixed = json.dumps({"type": "PPO", "location": str(tmp_path / "old")})
    ego, partners, env = run([game, "PPO", "PPO", "FIXED", "DEFAULT", "--partner-pool", "--n-envs", "16", "-t", "512", "--seed", "1",
                              "--ego-config", '{"n_steps": 16, "n_epochs": 2}',
                              "--alt-config", '{"n_steps": 2, "n_epochs": 2}', fixed, "{}",
                              "--env-config", '{"resample": "random", "log_interval": 1}',
                              "--ego-save", str(tmp_path / "ego"), "--alt-save", str(tmp_path / "alt")])
    out = capsys.readouterr().out
    assert isinstance(env, VecBlockPartnerPool) and env.native and env.K == 3 and env.resample == "random" and env.variant == variant
    assert isinstance(partners[1], FrozenVecPartner) and isinstance(partners[2], VecBlockScriptedPartner)
    assert env.ego.iteration == 2 and partners[0].min_full == 16 // 3
    assert "ep_rew_mean_vs_2" in out
    assert np.array_equal(partners[1].policy.get_flat_params(), old.policy.get_flat_params())     # frozen stays frozen
    assert sorted(os.listdir(tmp_path / "alt")) == ["0.zip"]
    for path, model in (("ego", ego), (os.path.join("alt", "0"), partners[0].model)):
        again = PPO.load(str(tmp_path / path))
        assert np.array_equal(again.policy.get_flat_params(), model.policy.get_flat_params())
    res = crossplay.run([game, "--agents", str(tmp_path / "ego"), "--partners", str(tmp_path / "alt" / "0"), "DEFAULT",
                         "--n-envs", "16", "-t", "16", "--max-steps", "24", "--out", str(tmp_path / "x.npz")])
    z = np.load(str(tmp_path / "x.npz"))
    assert z["mean"].shape == (1, 2) and z["pairs"].tolist() == [[0, 0], [0, 1]] and z["partners"].tolist()[1] == "DEFAULT"
    assert int(z["unfinished"]) == res.unfinished
    if variant == 0:
        ego, partners, env = run([game, "PPO", "DEFAULT", "DEFAULT", "--partner-pool", "--n-envs", "16", "-t", "256", "--seed", "2",
                                  "--ego-config", '{"n_steps": 16, "n_epochs": 1}', "--alt-config", "{}", '{"rule": "EASY"}',
                                  "--env-config", '{"log_interval": 0}'])
        assert [p.rule for p in partners] == [nat.PH_BLOCK_RULE_DEFAULT, nat.PH_BLOCK_RULE_EASY] and env.episodes >= 0
