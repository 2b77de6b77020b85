"""gpu: `policy_kwargs net_arch` towers (ArchActorCriticPolicy) as members of the device-resident Liar's Dice pool and cross-play --
the tower tiles of the grouped forward (pool_tower_kernel) against `ph_arch_forward` / `ph_arch_forward_ragged`, the native steps
against the walk, recorded games replayed through the host game, graph capture, misuse, and the command lines end to end.  Every
comparison is exact.  The grouped forward takes no gemm_mode, so only the MFMA instantiation (mode 0) of pool_tower_kernel is built
and that is the one every case here runs."""
import ctypes as C
import json

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat

pytestmark = pytest.mark.gpu

RB_KEYS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs")
XSTATE = ("hands", "history", "nmoves", "obs_ego", "obs_alt", "games", "playing", "tables_left", "returns", "lengths", "ep_return",
          "ep_length")
# member kinds of this file: (PH_POOL_* kind, tower widths or None)
KINDS = dict(learner=(nat.PH_POOL_LEARNER, None), frozen=(nat.PH_POOL_FROZEN, None), scripted=(nat.PH_POOL_SCRIPTED, None),
             clone=(nat.PH_POOL_CLONE, None), ltower32=(nat.PH_POOL_LEARNER, (32,)), ftower32=(nat.PH_POOL_FROZEN, (32,)),
             ftower128=(nat.PH_POOL_FROZEN, (128, 128)), ftower256=(nat.PH_POOL_FROZEN, (256, 128)),
             ftower64x3=(nat.PH_POOL_FROZEN, (64, 64, 64)))


def _spaces():
    from pantheonrl_amd.envs.vec import VecLiarsDice
    return type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                              _is_dummy_space_env=True))()


def _ppo(E, T, seed, arch=None):
    from pantheonrl_amd import PPO
    kwargs = dict(policy_kwargs=dict(net_arch=[dict(pi=list(arch), vf=list(arch))])) if arch else {}
    model = PPO("MlpPolicy", _spaces(), n_steps=T, n_envs=E, batch_size=max(8, E * T // 2), n_epochs=2, seed=seed, **kwargs)
    model.device_permutations = True
    model.rollout_buffer.gae_mode = 1
    return model


def _sharpen(policy, seed):
    """parameters of order one, so that the moves spread and a wrong bit moves a sample; the same seed gives the same parameters"""
    policy.set_flat_params(0.4 * np.random.default_rng(seed).standard_normal(policy.layout.P).astype(np.float32))
    return policy


def _member(kind, E, T_alt, seed, sharpen=False):
    from pantheonrl_amd.bc import FeedForward32Policy
    from pantheonrl_amd.envs.vec import ClonedVecPartner, VecLiarDefaultPartner, frozen_partner_for, ragged_agent_for
    pool_kind, arch = KINDS[kind]
    if pool_kind == nat.PH_POOL_SCRIPTED:
        return VecLiarDefaultPartner()
    if pool_kind == nat.PH_POOL_CLONE:
        s = _spaces()
        return ClonedVecPartner(_sharpen(FeedForward32Policy(s.observation_space, s.action_space, seed=1000 + seed), seed))
    if pool_kind == nat.PH_POOL_LEARNER:
        m = ragged_agent_for(_ppo(E, T_alt, seed, arch))
        pol = m.model.policy
    else:
        m = frozen_partner_for(_ppo(E, 2, seed, arch).policy)
        pol = m.policy
    if sharpen:
        _sharpen(pol, seed)
    return m


def _pool(E, T_ego, T_alt, kinds, ego_arch=(128, 128), seed=0, native=True, resample="robin", record=0):
    from pantheonrl_amd.envs.vec import liar_pool_for
    from pantheonrl_amd.vec import vec_agent_for
    ego = vec_agent_for(_ppo(E, T_ego, seed, ego_arch))
    members = [_member(kind, E, T_alt, seed + 1 + k) for k, kind in enumerate(kinds)]
    return liar_pool_for(E, ego, members, seed=seed + 7, resample=resample, native=native, record=record), ego, members


def _xplay(E, kinds, G, pairs=None, seed=5, native=True, record=0):
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    members = [_member(kind, 4, 2, 20 + k) for k, kind in enumerate(kinds)]
    return VecLiarCrossPlay(E, members, pairs=pairs, episodes_per_table=G, seed=seed, native=native, record=record)


def _ctx_of(agent):
    ctx = agent.model.policy.ctx
    ctx.set_stream(th.cuda.current_stream(agent.model.policy.device).cuda_stream)
    return ctx


def _arch_array(members):
    """member_archs of the `_arch` entry points: a pointer where the member plays a tower, else NULL"""
    from pantheonrl_amd.envs.vec import VecLiarStep
    from pantheonrl_amd.vec import is_tower
    archs = (C.POINTER(nat.PhArch) * len(members))()
    for k, m in enumerate(members):
        p = VecLiarStep._policy_of(m)
        if p is not None and is_tower(p):
            archs[k] = C.pointer(p.arch)
    return archs


# ---- 1. the grouped forward on its own -------------------------------------------------------------------------------------------
def _interleave(counts):
    """member ids with the given counts, interleaved by table index (round robin over the members that still have rows left)"""
    left, out = list(counts), []
    while any(left):
        for k in range(len(left)):
            if left[k]:
                out.append(k)
                left[k] -= 1
    return np.asarray(out, np.int32)


def _forward_case(name):
    """-> (kinds, partnerid, active).  The mixed case has active-row counts [17, 16, 1, 0, 16] per member, interleaved by table
    index: a full tower tile plus one row, a one-row tower tile (a learner), a member without a tile, tower tiles beside tiles of
    every other kind.  `mixed54`: the same active rows with four inactive ones in between."""
    mixed = ["ftower128", "frozen", "ltower32", "scripted", "learner"]
    if name == "mixed50":
        return mixed, _interleave([17, 16, 1, 0, 16]), np.ones(50, np.uint8)
    if name == "mixed54":
        pid, active = _interleave([17, 16, 1, 0, 16]).tolist(), [1] * 50
        for at, k in ((3, 0), (17, 3), (30, 2), (41, 4)):
            pid.insert(at, k)
            active.insert(at, 0)
        pid, active = np.asarray(pid, np.int32), np.asarray(active, np.uint8)
        assert np.bincount(pid[active != 0], minlength=5).tolist() == [17, 16, 1, 0, 16] and len(pid) == 54
        return mixed, pid, active
    if name == "tower3clone":  # a three-layer tower beside a clone: the tower and the clone kernels, no 64-wide launch
        return ["ftower64x3", "clone"], _interleave([12, 11]), np.ones(23, np.uint8)
    if name == "learner19":    # a learner tower alone: a full tile plus three rows, every recorded field
        return ["ltower32"], np.zeros(19, np.int32), np.ones(19, np.uint8)
    assert name == "tile16"    # exactly one full tile of the widest arch
    return ["ftower256"], np.zeros(16, np.int32), np.ones(16, np.uint8)


@pytest.mark.parametrize("case", ["mixed50", "mixed54", "tile16", "tower3clone", "learner19"])
def test_grouped_forward_is_bitwise_the_per_member_entry_points(case):
    from pantheonrl_amd.vec import VecOnPolicyAgent
    kinds, pid_h, active_h = _forward_case(case)
    n, K, T, counter = len(pid_h), len(kinds), 4, 9
    rng = np.random.default_rng(5)
    obs_space = _spaces().observation_space
    obs = th.as_tensor((rng.random((n, 30)) * np.asarray(obs_space.nvec)).astype(np.int64).astype(np.float32)).cuda()
    pid, active = th.as_tensor(pid_h).cuda(), th.as_tensor(active_h).cuda()
    host = VecOnPolicyAgent(_ppo(n, 2, 0))
    ctx = _ctx_of(host)
    lib, h, spec = ctx.lib, ctx.handle, C.byref(host.model.policy.spec)
    sets = []
    for _ in range(2):                                    # two identical sets: one for the grouped launch, one for the yardstick
        members = [_member(kind, n, T, 20 + k, sharpen=True) for k, kind in enumerate(kinds)]
        fill = np.random.default_rng(6)
        for k, m in enumerate(members):
            if KINDS[kinds[k]][0] == nat.PH_POOL_FROZEN:  # caches, so that floats are compared and not only sampled integers
                m.values = th.full((n,), -3.0, dtype=th.float32, device="cuda")
                m.log_probs = th.full((n,), -5.0, dtype=th.float32, device="cuda")
            if KINDS[kinds[k]][0] != nat.PH_POOL_LEARNER:
                continue
            rb = m.model.rollout_buffer
            for key in RB_KEYS:
                t = getattr(rb, key)
                t.copy_(th.as_tensor(fill.standard_normal(tuple(t.shape)).astype(np.float32)))
            m.pos.copy_(th.as_tensor(((2 * np.arange(n) + k) % (T + 1)).astype(np.int32)))   # every fill level, full columns included
            m.boundary.copy_(th.as_tensor(fill.integers(0, 2, n).astype(np.uint8)))
            m.values.fill_(-3.0)
            m.log_probs.fill_(-5.0)
        sets.append(members)
    grouped, plain = sets
    es = th.zeros(n, dtype=th.float32, device="cuda")
    for k, m in enumerate(grouped):
        if KINDS[kinds[k]][0] == nat.PH_POOL_LEARNER:
            es = th.where(pid == k, m.boundary.to(th.float32), es)
    es = es.contiguous()
    arr = (nat.PhPoolMember * K)()
    keep = []
    for k, m in enumerate(grouped):
        kind = KINDS[kinds[k]][0]
        arr[k].kind = kind
        if kind == nat.PH_POOL_SCRIPTED:
            continue
        pol = m.model.policy if kind == nat.PH_POOL_LEARNER else m.policy
        arr[k].params, arr[k].seed = pol.params.data_ptr(), pol._seed
        if kind == nat.PH_POOL_FROZEN:
            arr[k].values, arr[k].log_probs = m.values.data_ptr(), m.log_probs.data_ptr()
        if kind == nat.PH_POOL_LEARNER:
            keep.append(m.model.rollout_buffer.c_struct())
            arr[k].rb = C.pointer(keep[-1])
            arr[k].pos, arr[k].boundary, arr[k].term, arr[k].open = (t.data_ptr() for t in (m.pos, m.boundary, m.term, m.open))
            arr[k].values, arr[k].log_probs = m.values.data_ptr(), m.log_probs.data_ptr()
    archs = _arch_array(grouped)
    assert sum(bool(a) for a in archs) == sum(KINDS[kind][1] is not None for kind in kinds) >= 1
    actions = th.full((n, 2), -7, dtype=th.int32, device="cuda")
    nat.check(lib.ph_pool_forward_arch(h, spec, arr, K, obs.data_ptr(), pid.data_ptr(), active.data_ptr(), counter, actions.data_ptr(),
                                       es.data_ptr(), n, archs))
    th.cuda.synchronize()
    got = actions.cpu().numpy()
    act = active_h.astype(bool)
    assert (got[~act] == -7).all()                          # inactive rows keep their sentinel
    for k, (g, p) in enumerate(zip(grouped, plain)):
        mine = act & (pid_h == k)
        kind, arch = KINDS[kinds[k]]
        if kind == nat.PH_POOL_SCRIPTED:
            want = th.full((n, 2), -7, dtype=th.int32, device="cuda")
            rows = th.as_tensor(mine.astype(np.uint8)).cuda()
            nat.check(lib.ph_liar_default_actions(h, obs.data_ptr(), rows.data_ptr(), want.data_ptr(), n))
            assert np.array_equal(got[mine], want.cpu().numpy()[mine])
            continue
        if kind == nat.PH_POOL_CLONE:
            p.policy._counter = counter - 1
            want = p.get_action(obs).cpu().numpy()            # ONE ph_bc_forward over all n rows
            assert np.array_equal(got[mine], want[mine]), k
            continue
        if kind == nat.PH_POOL_FROZEN:
            # ONE forward over all n rows (row index = table) on the identical second policy: ph_arch_forward for a tower
            p.policy._counter = counter - 1
            want = p.get_action(obs).cpu().numpy()
            values, logp = (t.cpu().numpy() for t in p._out[n][1:])
            assert (want >= 0).all() and np.array_equal(got[mine], want[mine]), k
            gv, gl = g.values.cpu().numpy(), g.log_probs.cpu().numpy()
            assert np.array_equal(gv[mine], values[mine]) and np.array_equal(gl[mine], logp[mine]), k
            assert (gv[~mine] == -3.0).all() and (gl[~mine] == -5.0).all(), k
            assert np.isfinite(values).all() and (logp <= 0).all()
            if mine.sum() >= 10:
                assert len(np.unique(want[mine], axis=0)) > 3          # a spread of moves: nothing vacuous
            continue
        pol, rb = p.model.policy, p.model.rollout_buffer
        want = th.zeros((n, 2), dtype=th.int32, device="cuda")
        mask = th.as_tensor(mine.astype(np.uint8)).cuda()
        tail = (pol.params.data_ptr(), obs.data_ptr(), None, pol._seed, counter, 0, want.data_ptr(), p.values.data_ptr(),
                p.log_probs.data_ptr(), C.byref(rb.c_struct()), p.pos.data_ptr(), mask.data_ptr(), es.data_ptr())
        if arch:
            nat.check(lib.ph_arch_forward_ragged(h, spec, C.byref(pol.arch), *tail, 0))
        else:
            nat.check(lib.ph_policy_forward_ragged(h, spec, *tail))
        th.cuda.synchronize()
        want = want.cpu().numpy()
        assert np.array_equal(got[mine], want[mine]), k
        assert np.array_equal(g.values.cpu().numpy(), p.values.cpu().numpy()), k               # cached for recorded rows only
        glp, plp = g.log_probs.cpu().numpy(), p.log_probs.cpu().numpy()
        assert np.array_equal(glp[mine], plp[mine]) and (glp[~mine] == -5.0).all(), k
        recorded = mine & (p.pos.cpu().numpy() < T)
        assert (g.values.cpu().numpy()[~recorded] == -3.0).all()
        if mine.sum() >= 10:
            assert recorded.any() and (mine & ~recorded).any()
            assert len(np.unique(want[mine], axis=0)) > 3
        gb, pb = g.model.rollout_buffer.host(), rb.host()
        for key in gb:                                        # every recorded row, and nothing else anywhere in the buffer
            assert np.array_equal(gb[key], pb[key]), (k, key)
        before = ((2 * np.arange(n) + k) % (T + 1)).astype(np.int32)                           # what was written in front of the calls
        assert np.array_equal(g.pos.cpu().numpy(), before) and np.array_equal(p.pos.cpu().numpy(), before)   # no forward advances `pos`


# ---- 2. the native step is bitwise the walk --------------------------------------------------------------------------------------
def _pool_state(sp, ego):
    th.cuda.synchronize()
    out = dict(hands=sp.env.hands.cpu().numpy(), hist=sp.env.history.cpu().numpy(), nmoves=sp.env.nmoves.cpu().numpy(),
               obs=sp.obs_ego.cpu().numpy(), pid_now=sp.partnerid.cpu().numpy(), acted=sp.alt_acted.cpu().numpy(), episodes=sp.episodes,
               ego_it=ego.iteration, pe=ego.model.policy.get_flat_params())
    be = ego.model.rollout_buffer.host()
    out.update({"e_" + k: v for k, v in be.items() if k in RB_KEYS})          # values and log-probs too: the ego's forward is a tower's
    for i, m in enumerate(sp.learners):
        out[f"pos{i}"] = m.pos.cpu().numpy()
        out[f"flags{i}"] = np.stack([t.cpu().numpy() for t in (m.boundary, m.term, m.open)])
        out[f"values{i}"] = m.values.cpu().numpy()
        out[f"p{i}"] = m.model.policy.get_flat_params()
        out.update({f"a{i}_" + k: v for k, v in m.model.rollout_buffer.host().items() if k in RB_KEYS})
    return out


def _same_pool_state(a, b, ego_rows=None):
    for key in a:
        x, y = a[key], b[key]
        if key[0] == "a" and key[1].isdigit() and getattr(x, "ndim", 0) >= 2:       # only the recorded rows of a ragged buffer are defined
            rows = np.arange(x.shape[0])[:, None] < a["pos" + key[1]][None, :]
            x, y = x[rows], y[rows]
        if key.startswith("e_") and ego_rows is not None:
            x, y = x[:ego_rows], y[:ego_rows]
        assert np.array_equal(x, y), key


def _run_pool(native, resample, kinds, E, T_ego, T_alt, steps, seed=11):
    sp, ego, members = _pool(E, T_ego, T_alt, kinds, seed=seed, native=native, resample=resample)
    trained = [0] * len(sp.learners)
    pids = []
    for _ in range(steps):
        sp.step()
        pids.append(sp.partnerid.cpu().numpy().copy())
        for i, m in enumerate(sp.learners):
            if m.full():
                m.learn_from_buffer()
                trained[i] += 1
    out = _pool_state(sp, ego)
    out.update(pid=np.stack(pids), trained=trained)
    return out


@pytest.mark.parametrize("resample", ["robin", "random"])
def test_native_pool_step_with_towers_is_bitwise_the_walk(resample):
    from pantheonrl_amd.envs.vec import TowerVecLiarPartnerPool
    kinds = ["ltower32", "ftower64x3", "scripted", "learner"]
    a, b = (_run_pool(native, resample, kinds, E=50, T_ego=8, T_alt=4, steps=24) for native in (True, False))
    assert len(a["trained"]) == 2 and min(a["trained"]) >= 1 and a["trained"] == b["trained"], a["trained"]
    assert a["ego_it"] >= 2 and a["episodes"] > 50
    assert len(np.unique(a["pid"])) == 4                   # every member sat somewhere
    _same_pool_state(a, b)
    assert isinstance(_pool(8, 2, 2, kinds)[0], TowerVecLiarPartnerPool)


def _xstate(xp):
    th.cuda.synchronize()
    out = {k: getattr(xp.env if k in ("hands", "history", "nmoves") else xp, k).cpu().numpy().copy() for k in XSTATE}
    out["ego_first"] = xp.ego_first.cpu().numpy().copy()
    return out


def test_native_crossplay_step_with_towers_is_bitwise_the_walk_after_every_step():
    E, G, kinds = 32, 2, ["ftower128", "ftower32", "frozen", "scripted"]          # all 16 pairs on 32 tables
    a, b = (_xplay(E, kinds, G, native=native) for native in (True, False))
    assert a.P == 16 and a.towers
    steps = 0
    while True:
        sa, sb = _xstate(a), _xstate(b)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (steps, key)
        if sb["tables_left"][0] == 0:
            break
        assert steps < 7 * G
        a.step()
        b.step()
        steps += 1
    assert (sb["games"] == G).all() and sb["lengths"].min() >= 1 and sb["lengths"].max() >= 2
    ra, rb = a.run(), b.run()
    assert a.left() == 0 and b.left() == 0 and ra.steps == rb.steps == steps
    for name in ("count", "sum", "sumsq", "sum_length", "mean", "std", "mean_length"):
        assert np.array_equal(getattr(ra, name), getattr(rb, name)), name
    assert set(np.unique(ra.returns).tolist()) == {-1.0, 1.0}


# ---- 3. the games are real games: recording needs no change ------------------------------------------------------------------------
def test_recorded_tower_pool_games_replay_through_the_reference_recorder():
    """the native pool step with tower members logs moves like any member's: every table's log is what TurnBasedRecorder(LiarEnv)
    produces when it is dealt the device's hands and fed the logged moves (tests/test_gpu_record.py's replay)"""
    from tests.test_gpu_record import _replay_through_the_reference_recorder
    E, steps = 12, 10
    kinds = ["ftower128", "ltower32", "scripted"]
    sp, ego, members = _pool(E, 16, 16, kinds, seed=2, record=3 * steps + 1)
    events = [[] for _ in range(E)]                         # per table, as one-table events of the replay

    def dealt(mask):
        th.cuda.synchronize()
        hands, first = sp.env.hands.cpu().numpy(), sp.ego_first.cpu().numpy().astype(bool)
        for e in np.nonzero(mask)[0]:
            events[e].append(("deal", np.ones(1, bool), hands[e:e + 1].copy(), first[e:e + 1].copy()))
    dealt(np.ones(E, bool))
    for _ in range(steps):
        dealt(sp.step().cpu().numpy().astype(bool))
    rec = sp.recorded()
    rows, member, off = rec.rows.cpu().numpy(), rec.member.cpu().numpy(), rec.table_offsets
    assert not rec.dropped.any() and len(rows) == off[-1]
    total = tower_moves = 0
    for e in range(E):
        mine, who = rows[off[e]:off[e + 1]], member[off[e]:off[e + 1]]
        for row in mine:
            events[e].append(("move", row[None, 30:32].astype(np.int64), np.array([int(row[32]) % 2 == 0]), np.ones(1, bool)))
        tr, games = _replay_through_the_reference_recorder(events[e], 0)
        assert len(tr.flags) == len(mine), e
        assert np.array_equal(np.asarray(tr.obs), mine[:, :30]), e
        assert np.array_equal(np.asarray(tr.acts), mine[:, 30:32]), e
        assert np.array_equal(np.asarray(tr.flags), mine[:, 32]), e
        assert (mine[:, 32] >= 2).sum() == games
        seat1 = mine[:, 32].astype(int) % 2 == 1
        assert (who[~seat1] == 0).all() and ((who[seat1] >= 0) & (who[seat1] < 3)).all()
        tower_moves += int((seat1 & (who < 2)).sum())
        total += games
    assert total == sp.episodes == (rows[:, 32] >= 2).sum() and total >= E
    assert tower_moves >= E                                 # logged moves that belong to tower members


# ---- 4. no host work ---------------------------------------------------------------------------------------------------------------
def test_native_pool_step_with_towers_does_no_host_work_and_captures():
    kinds = ["ltower32", "ftower64x3", "scripted", "learner"]
    (eager, ego_e, _), (sp, ego, _) = (_pool(32, 8, 8, kinds, seed=3) for _ in range(2))
    for c in range(1, 7):
        eager._native_call(c, ego_pos=c - 1)
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
        episodes = sp.episodes
        nat.check(ctx.lib.ph_graph_launch(ctx.handle, gid.value))
        stream.synchronize()
    th.cuda.synchronize()
    assert sp.episodes > episodes
    _same_pool_state(_pool_state(sp, ego), _pool_state(eager, ego_e), ego_rows=6)


# ---- 5. misuse ---------------------------------------------------------------------------------------------------------------------
def test_tower_misuse_is_an_error_string_and_nothing_is_launched():
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    from pantheonrl_amd.envs.vec import (FrozenVecPartner, TowerFrozenVecPartner, TowerVecLiarPartnerPool, VecLiarPartnerPool,
                                         frozen_partner_for, liar_pool_for)
    from pantheonrl_amd.vec import vec_agent_for
    kinds = ["ftower128", "clone", "scripted", "frozen"]
    sp, ego, members = _pool(16, 4, 4, kinds, seed=1)
    assert type(sp) is TowerVecLiarPartnerPool and type(members[0]) is TowerFrozenVecPartner and type(members[3]) is FrozenVecPartner
    ctx = sp.env.ctx
    sp._bind()
    lib, h, d = ctx.lib, ctx.handle, sp._desc
    err = lambda: lib.ph_last_error()  # noqa: E731
    th.cuda.synchronize()
    before = {k: getattr(sp.env, k).cpu().numpy().copy() for k in ("hands", "history", "nmoves")}
    arr, archs, ego_arch = sp._member_arr, sp._member_arch_arr, sp._ego_arch
    tower = C.pointer(members[0].policy.arch)                # (archs[0] itself would be a view of the slot, not a copy of it)
    step =lambda: lib.ph_liar_pool_step_arch(h, C.byref(d), ego_arch, archs, 0, 1, 0)  # noqa: E731
    for k in (1, 2):                                         # an arch on a clone, on a scripted member
        archs[k] = tower
        assert step() != 0 and b"not to a scripted one or a clone" in err(), err()
        archs[k] = None
    bad = nat.make_arch([128, 48])                           # an arch ph_arch_fits refuses
    assert lib.ph_arch_fits(C.byref(sp.ego.model.policy.spec), C.byref(bad)) != 0
    archs[0] = C.pointer(bad)
    assert step() != 0 and b"multiple of 32" in err(), err()
    archs[0] = tower
    assert lib.ph_liar_pool_step_arch(h, C.byref(d), C.pointer(bad), archs, 0, 1, 0) != 0 and b"multiple of 32" in err()
    good = arr[0].params
    arr[0].params = good + 4                                 # a tower member's params off the 16-byte grid
    assert step() != 0 and b"16-byte aligned" in err(), err()
    arr[0].params = good
    # the same refusals from the other two entry points
    n = 16
    obs, pid, act8 = sp.obs_alt, sp.partnerid, sp.ones8
    out = th.zeros((n, 2), dtype=th.int32, device="cuda")
    spec = C.byref(sp.ego.model.policy.spec)
    archs[2] = tower
    assert lib.ph_pool_forward_arch(h, spec, arr, 4, obs.data_ptr(), pid.data_ptr(), act8.data_ptr(), 1, out.data_ptr(), None, n,
                                    archs) != 0 and b"not to a scripted one or a clone" in err()
    archs[2] = None
    xp = _xplay(16, ["ftower32", "scripted"], 1)
    xp._bind()
    xp._member_arch_arr[1] = xp._member_arch_arr[0]
    assert xp.ctx.lib.ph_liar_xplay_step_arch(xp.ctx.handle, C.byref(xp._desc), xp._member_arch_arr, 1, 0) != 0
    assert b"not to a scripted one or a clone" in xp.ctx.lib.ph_last_error()
    xp._member_arch_arr[1] = None
    th.cuda.synchronize()
    for k, v in before.items():                              # refused in front of the first launch: the game did not move
        assert np.array_equal(getattr(sp.env, k).cpu().numpy(), v), k
    # the plain classes keep refusing towers; the factories pick the classes
    plain_ego = vec_agent_for(_ppo(16, 4, 3))
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        VecLiarPartnerPool(16, plain_ego, [members[0]])
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        VecLiarPartnerPool(16, ego, [members[3]])
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        FrozenVecPartner(members[0].policy)
    with pytest.raises(nat.NativeError, match="tower"):
        TowerFrozenVecPartner(members[3].policy)
    assert type(frozen_partner_for(members[0].policy)) is TowerFrozenVecPartner
    assert type(frozen_partner_for(members[3].policy)) is FrozenVecPartner
    assert type(liar_pool_for(16, plain_ego, [members[3], members[2]])) is VecLiarPartnerPool
    assert type(liar_pool_for(16, plain_ego, [members[0]])) is TowerVecLiarPartnerPool
    with pytest.raises(nat.NativeError, match="learners train in VecLiarPartnerPool"):
        VecLiarCrossPlay(8, [_member("ltower32", 8, 2, 3)])
    # ... and the contexts still step
    sp.step()
    xp.step()
    th.cuda.synchronize()
    assert np.isfinite(ego.model.rollout_buffer.host()["values"][0]).all()
    assert not np.array_equal(sp.env.nmoves.cpu().numpy(), before["nmoves"]) or sp.episodes > 0


def test_all_null_member_archs_is_bitwise_the_entry_point_it_extends():
    kinds = ["learner", "frozen", "scripted"]
    (old, ego_o, _), (new, ego_n, _) = (_pool(32, 4, 4, kinds, ego_arch=None, seed=6) for _ in range(2))
    archs = (C.POINTER(nat.PhArch) * 3)()
    for sp, arch_form in ((old, False), (new, True)):
        sp._bind()
        ctx = sp.env.ctx
        for c in (1, 2, 3):
            if arch_form:
                nat.check(ctx.lib.ph_liar_pool_step_arch(ctx.handle, C.byref(sp._desc), None, archs if c % 2 else None, c - 1, c, 0))
            else:
                nat.check(ctx.lib.ph_liar_pool_step(ctx.handle, C.byref(sp._desc), c - 1, c, 0))
    a, b = _pool_state(old, ego_o), _pool_state(new, ego_n)
    assert a["episodes"] > 0
    _same_pool_state(a, b, ego_rows=3)
    for i, m in enumerate(old.learners):
        assert (a[f"pos{i}"] > 0).any()
    # cross-play: the same for ph_liar_xplay_step
    xa, xb = (_xplay(16, ["frozen", "scripted"], 2) for _ in range(2))
    for xp in (xa, xb):
        xp._bind()
    nat.check(xa.ctx.lib.ph_liar_xplay_step(xa.ctx.handle, C.byref(xa._desc), 1, 0))
    nat.check(xb.ctx.lib.ph_liar_xplay_step_arch(xb.ctx.handle, C.byref(xb._desc), (C.POINTER(nat.PhArch) * 2)(), 1, 0))
    sa, sb = _xstate(xa), _xstate(xb)
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------
TOWER = {"policy_kwargs": {"net_arch": [{"pi": [128, 128], "vf": [128, 128]}]}}
SMALL = {"policy_kwargs": {"net_arch": [{"pi": [32], "vf": [32]}]}}


def test_train_a_tower_pool_and_crossplay_tower_checkpoints(tmp_path, monkeypatch):
    from pantheonrl_amd import crossplay, trainer
    from pantheonrl_amd.envs.vec import (TowerFrozenVecPartner, TowerRaggedVecOnPolicyAgent, TowerVecLiarPartnerPool,
                                         VecLiarDefaultPartner)
    from pantheonrl_amd.ppo import ArchActorCriticPolicy
    monkeypatch.chdir(tmp_path)
    cfg = lambda extra, steps=8: json.dumps(dict(n_steps=steps, n_epochs=2, **extra))  # noqa: E731
    trainer.run(["LiarsDice-v0", "PPO", "PPO", "--n-envs", "16", "-t", "256", "--seed", "1", "--ego-config", cfg(TOWER),
                 "--alt-config", cfg({}), "--ego-save", "m/tower", "--alt-save", "m/plain"])
    fixed = json.dumps({"type": "PPO", "location": "m/tower"})
    ego, partners, env = trainer.run(["LiarsDice-v0", "PPO", "PPO", "FIXED", "DEFAULT", "--n-envs", "16", "-t", "512", "--seed", "2",
                                      "--ego-config", cfg(TOWER), "--alt-config", cfg(SMALL, 4), fixed, "{}"])
    assert type(env) is TowerVecLiarPartnerPool and env.native and env.K == 3
    assert type(ego.policy) is ArchActorCriticPolicy and ego.policy.net_arch == (128, 128)
    assert type(partners[0]) is TowerRaggedVecOnPolicyAgent and partners[0].model.policy.net_arch == (32,)
    assert type(partners[1]) is TowerFrozenVecPartner and partners[1].policy.net_arch == (128, 128)
    assert isinstance(partners[2], VecLiarDefaultPartner)
    assert env.ego.iteration >= 4 and env.episodes > 0 and partners[0].iteration >= 1
    for pol in (ego.policy, partners[0].model.policy):
        assert np.isfinite(pol.get_flat_params()).all()
    res = crossplay.run(["LiarsDice-v0", "--agents", "m/tower", "m/plain", "DEFAULT", "--n-envs", "18", "-t", "4", "--seed", "0",
                         "--out", "x.npz"])
    z = np.load("x.npz")
    assert z["mean"].shape == z["std"].shape == z["count"].shape == (3, 3)
    assert np.isfinite(z["mean"]).all() and np.isfinite(z["std"]).all() and (z["count"] >= 4).all()
    assert np.array_equal(z["mean"], res.matrix("mean"))
