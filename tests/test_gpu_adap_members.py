"""gpu: frozen ADAP checkpoints (AdapFrozenVecPartner: a stated latent, or a context per table sampled on the device) as members of
the device-resident Liar's Dice pool and cross-play -- the ADAP tiles of the grouped forward (pool_adap_kernel) against the
per-member entry points (`ph_adap_rows` + `ph_policy_forward`) and the host policy, the native steps against the walk, the sampled
contexts against ph_adap_vec_host, recorded games against the host game and the host policy, launch counts, capture, misuse, and
the command lines end to end.  Every comparison is exact."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu


def _any_member(kind, E, T_alt, seed):
    """a member of any kind; every policy that does not learn is sharpened"""
    return LC.member(kind, E, T_alt, seed, sharp=lambda k: k != "learner")


def _apool(E, kinds, resample="robin", native=True, seed=11, record=0, T_ego=8, T_alt=4):
    return LC.pool(E, T_ego, T_alt, kinds, seed=seed, native=native, resample=resample, record=record, sharp=lambda k: k != "learner")


def _arrays(members):
    """the member, arch and ADAP arrays of the entry points, built by the classes' own code"""
    from pantheonrl_amd.envs.vec import VecLiarStep
    holder = types.SimpleNamespace(_policy_of=VecLiarStep._policy_of)
    return (VecLiarStep._member_array(holder, members), VecLiarStep._member_archs(holder, members),
            VecLiarStep._member_adaps(holder, members), holder)


def _host_ctx(n):
    from pantheonrl_amd.vec import VecOnPolicyAgent
    host = VecOnPolicyAgent(LC.ppo(n, 2, 0))
    return host, LC.ctx_of(host)


# ---- 1. the grouped forward on its own -------------------------------------------------------------------------------------------
CASES = {
    # kinds, active rows per member, inactive rows inserted (position, member)
    "mixed50": (["frozen", "scripted", "adapS3", "adapR3"], [12, 5, 17, 16], [(3, 2), (17, 3), (30, 0), (41, 2)]),
    "tile16": (["adapS3"], [16], []),
    "tile17": (["adapS3"], [17], []),
    "no_table": (["frozen", "adapS3"], [9, 0], []),
    "alone": (["adapR3", "adapS3"], [11, 12], [(4, 0)]),
    "c1": (["adapS1"], [20], []),
    "c52": (["adapR52", "frozen"], [19, 7], []),
    "clone_tower": (["clone", "ftower32", "adapS3", "adapC4"], [9, 10, 18, 5], []),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_grouped_forward_is_bitwise_the_per_member_entry_points(case):
    from pantheonrl_amd.envs.vec import AdapFrozenVecPartner, attach_adap_members
    kinds, counts, holes = CASES[case]
    pid_l = LC.interleave(counts).tolist()
    active_l = [1] * len(pid_l)
    for at, k in holes:
        pid_l.insert(at, k)
        active_l.insert(at, 0)
    pid_h, active_h = np.asarray(pid_l, np.int32), np.asarray(active_l, np.uint8)
    n, K, counter = len(pid_h), len(kinds), 9
    act = active_h.astype(bool)
    assert np.bincount(pid_h[act], minlength=K).tolist() == counts
    rng = np.random.default_rng(5)
    obs_h = (rng.random((n, 30)) * np.asarray(LC.spaces().observation_space.nvec)).astype(np.int64).astype(np.float32)
    adap_rows = np.nonzero(act & np.isin(pid_h, [k for k, kind in enumerate(kinds) if kind in LC.ADAPS]))[0]
    if len(adap_rows):                                      # out-of-range components in rows an ADAP member moves in: clamped
        obs_h[adap_rows[0], 7], obs_h[adap_rows[-1], 0], obs_h[adap_rows[len(adap_rows) // 2], 29] = 99.0, -3.0, 12.0
    obs, pid, active = th.as_tensor(obs_h).cuda(), th.as_tensor(pid_h).cuda(), th.as_tensor(active_h).cuda()
    host, ctx = _host_ctx(n)
    lib, h, spec = ctx.lib, ctx.handle, C.byref(host.model.policy.spec)
    sets = []
    for _ in range(2):                                      # two identical sets: one for the grouped launch, one for the yardstick
        members = [_any_member(kind, n, 4, 20 + k) for k, kind in enumerate(kinds)]
        attach_adap_members(members, n)
        for m in members:
            if isinstance(m, AdapFrozenVecPartner):
                m.redraw(None, 5)                           # a sampled member: every table's context, drawn at counter 5
        sets.append(members)
    grouped, plain = sets
    arr, archs, adaps, keep = _arrays(grouped)
    assert sum(bool(a) for a in adaps) == sum(kind in LC.ADAPS for kind in kinds) >= 1
    actions = th.full((n, 2), -7, dtype=th.int32, device="cuda")
    nat.check(lib.ph_pool_forward_adap(h, spec, arr, K, obs.data_ptr(), pid.data_ptr(), active.data_ptr(), counter, actions.data_ptr(),
                                       None, n, archs, adaps))
    th.cuda.synchronize()
    got = actions.cpu().numpy()
    assert (got[~act] == -7).all()                          # inactive tables' actions are untouched
    for k, (g, p) in enumerate(zip(grouped, plain)):
        mine = act & (pid_h == k)
        if kinds[k] == "scripted":
            want = th.full((n, 2), -7, dtype=th.int32, device="cuda")
            rows = th.as_tensor(mine.astype(np.uint8)).cuda()
            nat.check(lib.ph_liar_default_actions(h, obs.data_ptr(), rows.data_ptr(), want.data_ptr(), n))
            assert np.array_equal(got[mine], want.cpu().numpy()[mine])
            continue
        if kinds[k] in LC.ADAPS:
            assert np.array_equal(g.contexts.cpu().numpy().view(np.uint32), p.contexts.cpu().numpy().view(np.uint32))
            if LC.ADAPS[kinds[k]][1] == "sample":
                cs, _, sampler = LC.ADAPS[kinds[k]]
                host_ctx, _ = nat.adap_vec_host(cs, n, sampler=sampler, seed=g.seed, counter=5)
                assert np.array_equal(g.contexts.cpu().numpy().view(np.uint32), host_ctx.view(np.uint32))
                assert len(np.unique(host_ctx, axis=0)) > min(n, LC.ADAPS[kinds[k]][0]) // 2      # a context per table
        p.policy._counter = counter - 1
        want = p.get_action(obs).cpu().numpy()              # ONE per-member forward over all n rows (row index = table)
        assert (want >= 0).all() and np.array_equal(got[mine], want[mine]), (k, kinds[k])
        if mine.sum() >= 10:
            assert len(np.unique(want[mine], axis=0)) > 3   # a spread of moves: nothing vacuous
        if kinds[k] in LC.ADAPS and mine.any():                # the rows the member saw: one_hot(clamped observation) ++ its context
            cs = LC.ADAPS[kinds[k]][0]
            _, rows = nat.adap_vec_host(cs, n, contexts=p.contexts.cpu().numpy(), env_space=p.env_space, obs=obs_h)
            assert np.array_equal(p.rows.cpu().numpy().view(np.uint32), rows.view(np.uint32))
            assert (rows[:, :270].sum(axis=1) == 30).all()


# ---- 2. a stated member is the host policy under set_context ---------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [3, 52])
def test_stated_member_is_bitwise_the_loaded_host_policy_under_set_context(cs, tmp_path):
    from pantheonrl_amd.adap import ADAP
    from pantheonrl_amd.envs.vec import AdapFrozenVecPartner, attach_adap_members
    n, counter = 37, 13
    model = LC.adap_model(cs, 31)
    model.save(str(tmp_path / "m"))
    latent = LC.latent(cs, 31)
    member = AdapFrozenVecPartner(model.policy, latent)
    attach_adap_members([member], n)
    rng = np.random.default_rng(8)
    obs_h = (rng.random((n, 30)) * np.asarray(LC.spaces().observation_space.nvec)).astype(np.int64).astype(np.float32)
    obs = th.as_tensor(obs_h).cuda()
    host, ctx = _host_ctx(n)
    arr, archs, adaps, keep = _arrays([member])
    actions = th.full((n, 2), -7, dtype=th.int32, device="cuda")
    pid, active = th.zeros(n, dtype=th.int32, device="cuda"), th.ones(n, dtype=th.uint8, device="cuda")
    nat.check(ctx.lib.ph_pool_forward_adap(ctx.handle, C.byref(host.model.policy.spec), arr, 1, obs.data_ptr(), pid.data_ptr(),
                                           active.data_ptr(), counter, actions.data_ptr(), None, n, archs, adaps))
    th.cuda.synchronize()
    loaded = ADAP.load(str(tmp_path / "m"), device="cuda").policy
    assert np.array_equal(loaded.get_flat_params(), model.policy.get_flat_params())
    loaded.set_context(latent)                              # trainer.py:140-147
    loaded._seed, loaded._counter = member.seed, counter - 1
    want, _, _ = loaded.forward(obs_h)
    assert np.array_equal(actions.cpu().numpy(), want.cpu().numpy().astype(np.int32).reshape(n, 2))
    assert len(np.unique(actions.cpu().numpy(), axis=0)) > 3


# ---- 3. / 4. / 5. the native steps against the walk, and the sampled contexts --------------------------------------------------------
def _contexts(members):
    from pantheonrl_amd.envs.vec import AdapFrozenVecPartner
    th.cuda.synchronize()
    return [m.contexts.cpu().numpy().copy() if isinstance(m, AdapFrozenVecPartner) else None for m in members]


def _same_contexts(a, b, where):
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (where, k)


@pytest.mark.parametrize("resample", ["robin", "random"])
def test_native_pool_step_with_adap_members_is_bitwise_the_walk(resample):
    from pantheonrl_amd.envs.vec import AdapVecLiarPartnerPool
    kinds = ["learner", "adapS3", "adapR3", "scripted"]
    (a, ego_a, ma), (b, ego_b, mb) = (_apool(50, kinds, resample, native) for native in (True, False))
    assert type(a) is AdapVecLiarPartnerPool and a.native and not b.native
    _same_contexts(_contexts(ma), _contexts(mb), "first deal")
    pids, trained = [], 0
    for step in range(40):
        da, db = a.step(), b.step()
        for sp in (a, b):
            for m in sp.learners:
                if m.full():
                    m.learn_from_buffer()
                    trained += sp is a
        assert np.array_equal(da.cpu().numpy(), db.cpu().numpy()), step
        _same_contexts(_contexts(ma), _contexts(mb), step)
        pids.append(a.partnerid.cpu().numpy().copy())
    sa, sb = LC.train_state(a, ego_a), LC.train_state(b, ego_b)
    LC.same_state(sa, sb)
    assert trained >= 1 and sa["ego_it"] >= 2 and sa["episodes"] > 50 and len(np.unique(np.stack(pids))) == 4
    assert np.array_equal(a.alt_actions.cpu().numpy(), b.alt_actions.cpu().numpy())
    lat = _contexts(ma)[1]
    assert (lat == LC.latent(3, 11 + 2)[None, :]).all()       # the stated member's contexts never move


def test_native_crossplay_step_with_adap_members_is_bitwise_the_walk_after_every_step():
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    E, G, kinds = 32, 2, ["adapS3", "adapR3", "frozen", "scripted"]               # all 16 pairs: ADAP in the ego seat of 8
    xs = []
    for native in (True, False):
        members = [_any_member(kind, 4, 2, 20 + k) for k, kind in enumerate(kinds)]
        xs.append((VecLiarCrossPlay(E, members, episodes_per_table=G, seed=5, native=native), members))
    (a, ma), (b, mb) = xs
    assert a.P == 16 and a.adaps and not a.towers
    steps = 0
    while True:
        sa, sb = LC.xstate(a), LC.xstate(b)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (steps, key)
        _same_contexts(_contexts(ma), _contexts(mb), steps)
        if sb["tables_left"][0] == 0:
            break
        assert steps < 7 * G
        a.step()
        b.step()
        steps += 1
    assert (sb["games"] == G).all() and sb["lengths"].max() >= 2
    ra, rb = a.run(), b.run()
    for name in ("count", "sum", "sumsq", "sum_length", "mean", "std", "mean_length"):
        assert np.array_equal(getattr(ra, name), getattr(rb, name)), name
    assert set(np.unique(ra.returns).tolist()) == {-1.0, 1.0}


def test_sampled_contexts_change_only_where_games_end_and_are_the_host_draw():
    """two sampling members that share ONE policy (the same file loaded twice): different seeds, different streams; after every
    step a table's context changed iff its game ended, and the new one is ph_adap_vec_host's draw for (member seed, counter, table)"""
    from pantheonrl_amd.envs.vec import AdapFrozenVecPartner, liar_pool_for
    from pantheonrl_amd.vec import vec_agent_for
    E = 40
    pol = LC.adap_model(3, 77).policy
    members = [AdapFrozenVecPartner(pol, "sample"), AdapFrozenVecPartner(pol, "sample"),
               AdapFrozenVecPartner(LC.adap_model(4, 78, "categorical").policy, "sample", "categorical")]
    sp = liar_pool_for(E, vec_agent_for(LC.ppo(E, 64, 1)), members, seed=4)
    assert members[0].seed == pol._seed and members[1].seed != members[0].seed
    samplers = ["l2", "l2", "categorical"]
    prev = _contexts(members)
    for k, m in enumerate(members):                         # the first deal: every table, counter 0
        want, _ = nat.adap_vec_host(m.context_size, E, sampler=samplers[k], seed=m.seed, counter=0)
        assert np.array_equal(prev[k].view(np.uint32), want.view(np.uint32)), k
    assert not np.array_equal(prev[0], prev[1])
    ended = 0
    for c in range(1, 25):
        done = sp.step().cpu().numpy().astype(bool)
        now = _contexts(members)
        for k, m in enumerate(members):
            want, _ = nat.adap_vec_host(m.context_size, E, sampler=samplers[k], seed=m.seed, counter=c, redraw=done.astype(np.uint8),
                                        contexts=prev[k])
            assert np.array_equal(now[k].view(np.uint32), want.view(np.uint32)), (c, k)
            changed = (now[k].view(np.uint32) != prev[k].view(np.uint32)).any(axis=1)
            assert not changed[~done].any()
            if samplers[k] == "l2":                         # (a categorical draw may repeat the one before)
                assert changed[done].all()
        ended += int(done.sum())
        prev = now
    assert ended > E


# ---- 6. the games are real games, and the member's moves the host policy's --------------------------------------------------------
def test_recorded_games_replay_through_the_host_game_and_the_host_policy():
    from pantheonrl_amd.common import StaticPolicyAgent
    from pantheonrl_amd.common.observation import Observation
    E, steps = 12, 10
    kinds = ["adapR3", "adapS3", "scripted"]
    sp, ego, members = _apool(E, kinds, seed=2, record=3 * steps + 1, T_ego=16)
    events = [[] for _ in range(E)]
    moves = []                                              # (table, member, obs, action, counter, context) of every ADAP move

    def dealt(mask):
        hands, first = sp.env.hands.cpu().numpy(), sp.ego_first.cpu().numpy().astype(bool)
        for e in np.nonzero(mask)[0]:
            events[e].append(("deal", np.ones(1, bool), hands[e:e + 1].copy(), first[e:e + 1].copy()))

    def log_counts():
        rec = sp.recorded()
        return rec, np.diff(rec.table_offsets)
    th.cuda.synchronize()
    dealt(np.ones(E, bool))
    seen = np.zeros(E, np.int64)
    for c in range(steps + 1):                              # c = 0: the first deal's openings
        before = _contexts(members)
        if c:
            dealt(sp.step().cpu().numpy().astype(bool))
        after = _contexts(members)
        rec, counts = log_counts()
        rows, who, off = rec.rows.cpu().numpy(), rec.member.cpu().numpy(), rec.table_offsets
        for e in range(E):
            ended = c == 0
            for i in range(off[e] + seen[e], off[e] + counts[e]):
                flag = int(rows[i, 32])
                if flag % 2 == 0:                           # the ego's move
                    ended = ended or flag >= 2
                    continue
                k = int(who[i])
                if kinds[k] in LC.ADAPS:                       # a reply reads the context before the step's redraw, an opening the new one
                    moves.append((e, k, rows[i, :30].copy(), rows[i, 30:32].copy(), 2 * c + 1 if ended else 2 * c,
                                  (after if ended else before)[k][e].copy()))
                ended = ended or flag >= 2
        seen = counts.copy()
    rec, counts = log_counts()
    rows, off = rec.rows.cpu().numpy(), rec.table_offsets
    assert not rec.dropped.any()
    total = 0
    for e in range(E):                                      # every table's log is a sequence of legal games of the host LiarEnv
        mine = rows[off[e]:off[e + 1]]
        for row in mine:
            events[e].append(("move", row[None, 30:32].astype(np.int64), np.array([int(row[32]) % 2 == 0]), np.ones(1, bool)))
        tr, games = LC.replay_through_the_reference_recorder(events[e], 0)
        assert np.array_equal(np.asarray(tr.obs), mine[:, :30]) and np.array_equal(np.asarray(tr.acts), mine[:, 30:32]), e
        assert np.array_equal(np.asarray(tr.flags), mine[:, 32]), e
        total += games
    assert total == sp.episodes >= E and len(moves) >= E
    # ... and every ADAP move is the host policy's under that table's context: a StaticPolicyAgent at table 0 (its one row is
    # Philox block 0), the policy's forward with the observation at row e elsewhere
    checked0 = 0
    for e, k, o, action, counter, context in moves:
        pol = members[k].policy
        pol._seed_keep = pol._seed
        pol._seed, pol._counter = members[k].seed, counter - 1
        if e == 0:
            pol.set_context(context[None, :])
            got = StaticPolicyAgent(pol).get_action(Observation(o))
            checked0 += 1
        else:
            batch = np.zeros((e + 1, 30), np.float32)
            batch[e] = o
            pol.set_context(np.tile(context, (e + 1, 1)))
            got = pol.forward(batch)[0].cpu().numpy().reshape(e + 1, 2)[e]
        pol._seed = pol._seed_keep
        assert np.array_equal(np.asarray(got).reshape(2).astype(np.int64), action.astype(np.int64)), (e, k, counter)
    assert checked0 >= 1
    assert {k for _, k, *_ in moves} == {0, 1}


# ---- 7. launch counts, no host work, capture ---------------------------------------------------------------------------------------
def _captured_nodes(sp, calls, first):
    """capture `calls` native steps (after two outside capture) -> (nodes of the graph, graph id)"""
    ctx = sp.env.ctx if hasattr(sp, "ego") else sp.ctx
    step = (lambda c: sp._native_call(c, ego_pos=c - 1)) if hasattr(sp, "ego") else (lambda c: sp._native_call(c))
    for c in range(first, first + 2):
        step(c)
    th.cuda.current_stream().synchronize()
    sp._bind()
    nat.check(ctx.lib.ph_graph_begin(ctx.handle))
    try:
        for c in range(first + 2, first + 2 + calls):
            step(c)
    finally:
        gid = C.c_int(-1)
        nat.check(ctx.lib.ph_graph_end(ctx.handle, C.byref(gid)))
    nodes = C.c_int(-1)
    nat.check(ctx.lib.ph_graph_nodes(ctx.handle, gid.value, C.byref(nodes)))
    return nodes.value, gid.value


def test_launch_counts_and_capture():
    """pantheon_hip.h: the pool step is 8 launches, the cross-play step 9; a table with ADAP members beside others adds one launch
    per grouped forward (two in the pool step, three in cross-play) and one per sampling member"""
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    stream = th.cuda.Stream()
    th.cuda.synchronize()
    with th.cuda.stream(stream):
        plain, _, _ = _apool(32, ["learner", "frozen", "scripted"], seed=3)
        base, _ = _captured_nodes(plain, 1, 1)
        assert base == 8
        for kinds, extra in ((["learner", "adapS3", "scripted"], 2), (["learner", "adapS3", "adapR3"], 2 + 1),
                             (["adapR3", "adapC4"], 0 + 2), (["adapS3"], 0)):
            sp, _, _ = _apool(32, kinds, seed=3)
            assert _captured_nodes(sp, 1, 1)[0] == base + extra, kinds
        xbase = None
        for kinds, extra in ((["frozen", "scripted"], 0), (["frozen", "adapS3"], 3), (["adapR3", "adapS3"], 1), (["frozen", "adapR3"], 3 + 1)):
            xp = VecLiarCrossPlay(16, [_any_member(kind, 4, 2, 20 + k) for k, kind in enumerate(kinds)], episodes_per_table=50, seed=5)
            nodes, _ = _captured_nodes(xp, 1, 1)
            xbase = nodes if xbase is None else xbase
            assert xbase == 9 and nodes == xbase + extra, kinds
        # a captured graph of four steps replays: the same state as the eager calls
        kinds = ["learner", "adapS3", "adapR3", "scripted"]
        (eager, ego_e, me), (sp, ego, mg) = (_apool(32, kinds, seed=3) for _ in range(2))
        for c in range(1, 7):
            eager._native_call(c, ego_pos=c - 1)
        nodes, gid = _captured_nodes(sp, 4, 1)
        assert nodes == 4 * (base + 3)
        episodes = sp.episodes
        nat.check(sp.env.ctx.lib.ph_graph_launch(sp.env.ctx.handle, gid))
        stream.synchronize()
    th.cuda.synchronize()
    assert sp.episodes > episodes
    LC.same_state(LC.train_state(sp, ego), LC.train_state(eager, ego_e), ego_rows=6)
    _same_contexts(_contexts(mg), _contexts(me), "graph")


# ---- 8. misuse -----------------------------------------------------------------------------------------------------------------------
def test_adap_misuse_is_an_error_string_and_nothing_is_launched():
    from pantheonrl_amd.adap import ADAP, AdapPolicyMult
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    from pantheonrl_amd.envs.vec import (AdapFrozenVecPartner, AdapVecLiarPartnerPool, FrozenVecPartner, TowerVecLiarPartnerPool,
                                         VecLiarPartnerPool, liar_pool_for, ragged_agent_for)
    from pantheonrl_amd.vec import vec_agent_for
    kinds = ["adapS3", "learner", "scripted", "frozen", "adapR3"]
    sp, ego, members = _apool(16, kinds, seed=1)
    assert type(sp) is AdapVecLiarPartnerPool
    ctx = sp.env.ctx
    sp._bind()
    lib, h, d = ctx.lib, ctx.handle, sp._desc
    err = lambda: lib.ph_last_error()  # noqa: E731
    th.cuda.synchronize()
    before = {k: getattr(sp.env, k).cpu().numpy().copy() for k in ("hands", "history", "nmoves")}
    ctx_before = _contexts(members)
    arr, archs, adaps = sp._member_arr, sp._member_arch_arr, sp._member_adap_arr
    good = sp._member_adap_keep[0]
    step = lambda: lib.ph_liar_pool_step_adap(h, C.byref(d), None, archs, adaps, 0, 1, 0)  # noqa: E731

    def bad(words, **fields):
        s = nat.PhPoolAdap()
        for name, _ in nat.PhPoolAdap._fields_:
            setattr(s, name, getattr(good, name))
        for name, v in fields.items():
            setattr(s, name, v)
        adaps[0] = C.pointer(s)
        assert step() != 0 and words in err(), (words, err())
        adaps[0] = C.pointer(good)
    bad(b"null contexts", contexts=None)
    bad(b"context_size must be 1..64", context_size=0)
    bad(b"context_size must be 1..64", context_size=65)
    bad(b"270 + C", context_size=4)                         # the spec is a Box of 273
    bad(b"unknown context sampler", sampler=7)
    bad(b"needs context_size == 1", sampler=nat.CONTEXT_SAMPLERS["natural_numbers"])
    bad(b"null ADAP spec", spec=None)
    bad(b"270 + C", spec=C.pointer(ego.model.policy.spec))  # the one-hot spec of the game is not a Box(270 + C)
    from pantheonrl_amd import spaces as S
    from pantheonrl_amd.spaces import make_spec
    other_heads = make_spec(S.Box(-np.inf, np.inf, (273,)), S.MultiDiscrete([7, 13]))
    bad(b"(A, L) = (2, 19)", spec=C.pointer(other_heads))
    for k, words in ((1, b"PH_POOL_FROZEN"), (2, b"PH_POOL_FROZEN")):          # a description on a learner, on the scripted member
        adaps[k] = C.pointer(good)
        assert step() != 0 and words in err(), err()
        adaps[k] = None
    tower = nat.make_arch([32])
    archs[0] = C.pointer(tower)
    assert step() != 0 and b"takes no arch" in err(), err()
    archs[0] = None
    # the same refusals from the other two entry points
    out = th.zeros((16, 2), dtype=th.int32, device="cuda")
    s = nat.PhPoolAdap()
    for name, _ in nat.PhPoolAdap._fields_:
        setattr(s, name, getattr(good, name))
    s.contexts = None
    adaps[0] = C.pointer(s)
    assert lib.ph_pool_forward_adap(h, C.byref(ego.model.policy.spec), arr, 5, sp.obs_alt.data_ptr(), sp.partnerid.data_ptr(),
                                    sp.ones8.data_ptr(), 1, out.data_ptr(), sp._es_alt.data_ptr(), 16, archs, adaps) != 0
    assert b"null contexts" in err()
    adaps[0] = C.pointer(good)
    xp = VecLiarCrossPlay(16, [_any_member("adapS3", 4, 2, 3), _any_member("scripted", 4, 2, 4)], episodes_per_table=1)
    xp._bind()
    xp._member_adap_arr[1] = xp._member_adap_arr[0]
    assert xp.ctx.lib.ph_liar_xplay_step_adap(xp.ctx.handle, C.byref(xp._desc), xp._member_arch_arr, xp._member_adap_arr, 1, 0) != 0
    assert b"PH_POOL_FROZEN" in xp.ctx.lib.ph_last_error()
    xp._member_adap_arr[1] = None
    th.cuda.synchronize()
    for k, v in before.items():                             # refused in front of the first launch: the game did not move
        assert np.array_equal(getattr(sp.env, k).cpu().numpy(), v), k
    _same_contexts(_contexts(members), ctx_before, "misuse")
    # the classes: a latent of another length, a word that is not "sample", AdapPolicyMult, learners, the plain classes
    pol = members[0].policy
    with pytest.raises(nat.NativeError, match="context_size is 3"):
        AdapFrozenVecPartner(pol, [1.0, 0.0])
    with pytest.raises(nat.NativeError, match='"sample"'):
        AdapFrozenVecPartner(pol, "draw")
    with pytest.raises(nat.NativeError, match="natural_numbers"):
        AdapFrozenVecPartner(pol, "sample", "natural_numbers")
    from pantheonrl_amd.envs.vec import VecRPS             # (AdapPolicyMult takes one small Discrete head: RPS)
    rps = type("S", (), dict(observation_space=VecRPS.observation_space, action_space=VecRPS.action_space, _is_dummy_space_env=True))()
    mult = ADAP(AdapPolicyMult, rps, context_size=3, n_steps=2, n_envs=4, batch_size=4, n_epochs=1, seed=1).policy
    with pytest.raises(nat.NativeError, match="AdapPolicyMult"):
        AdapFrozenVecPartner(mult, [1.0, 0.0, 0.0])
    with pytest.raises(nat.NativeError, match="not an AdapPolicy"):
        AdapFrozenVecPartner(members[3].policy, [1.0, 0.0, 0.0])
    arched = LC.adap_model(3, 9).policy                      # an AdapPolicy that was given net_arch: refused by name
    arched.net_arch = (128, 128)
    with pytest.raises(nat.NativeError, match="net_arch"):
        AdapFrozenVecPartner(arched, [1.0, 0.0, 0.0])
    with pytest.raises(nat.NativeError, match="16 tables"):               # one object, one population: its contexts are 16 tables'
        members[0].attach(8)
    plain_ego = vec_agent_for(LC.ppo(16, 4, 3))
    for cls in (VecLiarPartnerPool, TowerVecLiarPartnerPool):
        with pytest.raises(nat.NativeError, match="AdapFrozenVecPartner"):
            cls(16, plain_ego, [members[0]])
    with pytest.raises(nat.NativeError, match="AdapFrozenVecPartner"):    # an ADAP policy without a latent is no member
        liar_pool_for(16, plain_ego, [FrozenVecPartner(pol), members[0]])
    with pytest.raises(nat.NativeError, match="ADAP learner"):            # ... nor an ADAP learner, nor an ADAP ego
        liar_pool_for(16, plain_ego, [ragged_agent_for(LC.adap_model(3, 5)), members[0]])
    with pytest.raises(nat.NativeError, match="ADAP learner"):
        liar_pool_for(16, vec_agent_for(LC.adap_model(3, 6)), [members[0]])
    assert type(liar_pool_for(16, plain_ego, [members[3], members[2]])) is VecLiarPartnerPool
    # ... and the contexts still step
    sp.step()
    xp.step()
    th.cuda.synchronize()
    assert not np.array_equal(sp.env.nmoves.cpu().numpy(), before["nmoves"]) or sp.episodes > 0


def test_all_null_member_adaps_is_bitwise_the_entry_point_it_extends():
    kinds = ["learner", "frozen", "scripted"]
    (old, ego_o, _), (new, ego_n, _) = (_apool(32, kinds, seed=6, T_ego=4) for _ in range(2))
    adaps = (C.POINTER(nat.PhPoolAdap) * 3)()
    for sp, adap_form in ((old, False), (new, True)):
        sp._bind()
        ctx = sp.env.ctx
        for c in (1, 2, 3):
            if adap_form:
                nat.check(ctx.lib.ph_liar_pool_step_adap(ctx.handle, C.byref(sp._desc), None, None, adaps if c % 2 else None, c - 1, c, 0))
            else:
                nat.check(ctx.lib.ph_liar_pool_step_arch(ctx.handle, C.byref(sp._desc), None, None, c - 1, c, 0))
    a, b = LC.train_state(old, ego_o), LC.train_state(new, ego_n)
    assert a["episodes"] > 0
    LC.same_state(a, b, ego_rows=3)


# ---- 9. end to end -------------------------------------------------------------------------------------------------------------------
def test_train_adap_crossplay_its_latents_and_train_an_ego_against_them(tmp_path, monkeypatch):
    from pantheonrl_amd import crossplay, trainer
    from pantheonrl_amd.envs.vec import AdapFrozenVecPartner, AdapVecLiarPartnerPool, VecLiarDefaultPartner
    monkeypatch.chdir(tmp_path)
    cfg = json.dumps(dict(n_steps=8, n_epochs=2))
    trainer.run(["LiarsDice-v0", "ADAP", "ADAP", "--share-latent", "--n-envs", "8", "-t", "128", "--seed", "1", "--ego-config", cfg,
                 "--alt-config", cfg, "--ego-save", "m"])
    res = crossplay.run(["LiarsDice-v0", "--agents", "ADAP:m@1,0,0", "ADAP:m@sample", "DEFAULT", "--n-envs", "18", "-t", "4", "--seed", "0",
                         "--out", "x.npz", "--record", "r.npy"])
    z = np.load("x.npz")
    assert z["mean"].shape == z["std"].shape == z["count"].shape == (3, 3)
    assert np.isfinite(z["mean"]).all() and np.isfinite(z["std"]).all() and (z["count"] >= 4).all()
    assert np.array_equal(z["mean"], res.matrix("mean"))
    assert z["latents"].shape == (3, 3) and z["latents"][0].tolist() == [1.0, 0.0, 0.0] and np.isnan(z["latents"][1:]).all()
    assert len(np.load("r.npy")) == z["table_offsets"][-1] > 0
    stated = json.dumps({"type": "ADAP", "location": "m", "latent_val": [1, 0, 0]})
    sampled = json.dumps({"type": "ADAP", "location": "m", "latent_val": "sample"})
    ego, partners, env = trainer.run(["LiarsDice-v0", "PPO", "FIXED", "FIXED", "DEFAULT", "--n-envs", "16", "-t", "256", "--seed", "2",
                                      "--ego-config", cfg, "--alt-config", stated, sampled, "{}", "--ego-save", "ego"])
    assert type(env) is AdapVecLiarPartnerPool and env.native and env.K == 3
    assert type(partners[0]) is AdapFrozenVecPartner and not partners[0].sampled and partners[0].latent.tolist() == [1.0, 0.0, 0.0]
    assert type(partners[1]) is AdapFrozenVecPartner and partners[1].sampled and partners[1].seed != partners[0].seed
    assert isinstance(partners[2], VecLiarDefaultPartner)
    assert env.ego.iteration >= 2 and env.episodes > 0 and np.isfinite(ego.policy.get_flat_params()).all()
    assert (tmp_path / "ego").exists() or list(tmp_path.glob("ego*"))
