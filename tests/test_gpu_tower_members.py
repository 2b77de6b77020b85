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
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu


def _pool(E, T_ego, T_alt, kinds, ego_arch=(128, 128), **kw):
    """this file's pools have a tower ego unless told otherwise"""
    return LC.pool(E, T_ego, T_alt, kinds, ego_arch=ego_arch, **kw)


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
def _forward_case(name):
    """-> (kinds, partnerid, active).  The mixed case has active-row counts [17, 16, 1, 0, 16] per member, interleaved by table
    index: a full tower tile plus one row, a one-row tower tile (a learner), a member without a tile, tower tiles beside tiles of
    every other kind.  `mixed54`: the same active rows with four inactive ones in between."""
    mixed = ["ftower128", "frozen", "ltower32", "scripted", "learner"]
    if name == "mixed50":
        return mixed, LC.interleave([17, 16, 1, 0, 16]), np.ones(50, np.uint8)
    if name == "mixed54":
        pid, active = LC.interleave([17, 16, 1, 0, 16]).tolist(), [1] * 50
        for at, k in ((3, 0), (17, 3), (30, 2), (41, 4)):
            pid.insert(at, k)
            active.insert(at, 0)
        pid, active = np.asarray(pid, np.int32), np.asarray(active, np.uint8)
        assert np.bincount(pid[active != 0], minlength=5).tolist() == [17, 16, 1, 0, 16] and len(pid) == 54
        return mixed, pid, active
    if name == "tower3clone":  # a three-layer tower beside a clone: the tower and the clone kernels, no 64-wide launch
        return ["ftower64x3", "clone"], LC.interleave([12, 11]), np.ones(23, np.uint8)
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
    obs_space = LC.spaces().observation_space
    obs = th.as_tensor((rng.random((n, 30)) * np.asarray(obs_space.nvec)).astype(np.int64).astype(np.float32)).cuda()
    pid, active = th.as_tensor(pid_h).cuda(), th.as_tensor(active_h).cuda()
    host = VecOnPolicyAgent(LC.ppo(n, 2, 0))
    ctx = LC.ctx_of(host)
    lib, h, spec = ctx.lib, ctx.handle, C.byref(host.model.policy.spec)
    sets = []
    for _ in range(2):                                    # two identical sets: one for the grouped launch, one for the yardstick
        members = [LC.member(kind, n, T, 20 + k, sharp=True) for k, kind in enumerate(kinds)]
        fill = np.random.default_rng(6)
        for k, m in enumerate(members):
            if LC.KINDS[kinds[k]][0] == nat.PH_POOL_FROZEN:  # caches, so that floats are compared and not only sampled integers
                m.values = th.full((n,), -3.0, dtype=th.float32, device="cuda")
                m.log_probs = th.full((n,), -5.0, dtype=th.float32, device="cuda")
            if LC.KINDS[kinds[k]][0] != nat.PH_POOL_LEARNER:
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
    es = th.zeros(n, dtype=th.float32, device="cuda")
    for k, m in enumerate(grouped):
        if LC.KINDS[kinds[k]][0] == nat.PH_POOL_LEARNER:
            es = th.where(pid == k, m.boundary.to(th.float32), es)
    es = es.contiguous()
    arr = (nat.PhPoolMember * K)()
    keep = []
    for k, m in enumerate(grouped):
        kind = LC.KINDS[kinds[k]][0]
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
    assert sum(bool(a) for a in archs) == sum(LC.KINDS[kind][1] is not None for kind in kinds) >= 1
    actions = th.full((n, 2), -7, dtype=th.int32, device="cuda")
    nat.check(lib.ph_pool_forward_arch(h, spec, arr, K, obs.data_ptr(), pid.data_ptr(), active.data_ptr(), counter, actions.data_ptr(),
                                       es.data_ptr(), n, archs))
    th.cuda.synchronize()
    got = actions.cpu().numpy()
    act = active_h.astype(bool)
    assert (got[~act] == -7).all()                          # inactive rows keep their sentinel
    for k, (g, p) in enumerate(zip(grouped, plain)):
        mine = act & (pid_h == k)
        kind, arch = LC.KINDS[kinds[k]]
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
@pytest.mark.parametrize("resample", ["robin", "random"])
def test_native_pool_step_with_towers_is_bitwise_the_walk(resample):
    from pantheonrl_amd.envs.vec import TowerVecLiarPartnerPool
    kinds = ["ltower32", "ftower64x3", "scripted", "learner"]
    a, b = (LC.run_pool(native, resample, kinds, E=50, T_ego=8, T_alt=4, steps=24, ego_arch=(128, 128))
            for native in (True, False))
    assert len(a["trained"]) == 2 and min(a["trained"]) >= 1 and a["trained"] == b["trained"], a["trained"]
    assert a["ego_it"] >= 2 and a["episodes"] > 50
    assert len(np.unique(a["pid"])) == 4                   # every member sat somewhere
    LC.same_state(a, b)
    assert isinstance(_pool(8, 2, 2, kinds)[0], TowerVecLiarPartnerPool)


def test_native_crossplay_step_with_towers_is_bitwise_the_walk_after_every_step():
    E, G, kinds = 32, 2, ["ftower128", "ftower32", "frozen", "scripted"]          # all 16 pairs on 32 tables
    a, b = (LC.xplay(E, kinds, G, native=native) for native in (True, False))
    assert a.P == 16 and a.towers
    steps = 0
    while True:
        sa, sb = LC.xstate(a), LC.xstate(b)
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
    produces when it is dealt the device's hands and fed the logged moves (tests/liar_cases.py's replay)"""
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
        tr, games = LC.replay_through_the_reference_recorder(events[e], 0)
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
    LC.same_state(LC.train_state(sp, ego), LC.train_state(eager, ego_e), ego_rows=6)


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
    xp = LC.xplay(16, ["ftower32", "scripted"], 1)
    xp._bind()
    xp._member_arch_arr[1] = xp._member_arch_arr[0]
    assert xp.ctx.lib.ph_liar_xplay_step_arch(xp.ctx.handle, C.byref(xp._desc), xp._member_arch_arr, 1, 0) != 0
    assert b"not to a scripted one or a clone" in xp.ctx.lib.ph_last_error()
    xp._member_arch_arr[1] = None
    th.cuda.synchronize()
    for k, v in before.items():                              # refused in front of the first launch: the game did not move
        assert np.array_equal(getattr(sp.env, k).cpu().numpy(), v), k
    # the plain classes keep refusing towers; the factories pick the classes
    plain_ego = vec_agent_for(LC.ppo(16, 4, 3))
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
        VecLiarCrossPlay(8, [LC.member("ltower32", 8, 2, 3)])
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
    a, b = LC.train_state(old, ego_o), LC.train_state(new, ego_n)
    assert a["episodes"] > 0
    LC.same_state(a, b, ego_rows=3)
    for i, m in enumerate(old.learners):
        assert (a[f"pos{i}"] > 0).any()
    # cross-play: the same for ph_liar_xplay_step
    xa, xb = (LC.xplay(16, ["frozen", "scripted"], 2) for _ in range(2))
    for xp in (xa, xb):
        xp._bind()
    nat.check(xa.ctx.lib.ph_liar_xplay_step(xa.ctx.handle, C.byref(xa._desc), 1, 0))
    nat.check(xb.ctx.lib.ph_liar_xplay_step_arch(xb.ctx.handle, C.byref(xb._desc), (C.POINTER(nat.PhArch) * 2)(), 1, 0))
    sa, sb = LC.xstate(xa), LC.xstate(xb)
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
