"""gpu: cross-play evaluation of the block worlds on the device -- the scripted constructors against the host rule text, the grouped
forward against ph_policy_forward row by row, the native step against its walk after every step, budgets and idle tables, the step
cap and the command line.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "blockworld_ref.npz"))
DEV = "cuda:0"
_MODELS = {}


def _ppo(variant, seat, seed):
    """a tiny PPO model on the variant's planner (seat 0) or constructor (seat 1) spaces; one per (variant, seat, seed)"""
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import VecBlockWorld
    key = (variant, seat, seed)
    if key not in _MODELS:
        _MODELS[key] = PPO("MlpPolicy", VecBlockWorld.seat_spaces(variant)[seat], n_steps=2, n_envs=4, batch_size=8, n_epochs=1, seed=seed)
    return _MODELS[key]


def _frozen(variant, seat, seed):
    from pantheonrl_amd.envs.vec import FrozenVecPartner
    return FrozenVecPartner(_ppo(variant, seat, seed).policy)


def _biased_planner(variant, seed, bias=3.0):
    """a fresh planner of that seed whose end-token logit bias is raised: games end within a few tokens"""
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import FrozenVecPartner, VecBlockWorld
    model = PPO("MlpPolicy", VecBlockWorld.seat_spaces(variant)[0], n_steps=2, n_envs=4, batch_size=8, n_epochs=1, seed=seed)
    pol = model.policy
    with th.no_grad():
        pol.params[pol.layout.act_b + pol.layout.L - 1] += bias
    return FrozenVecPartner(pol)


def _constructors(variant):
    from pantheonrl_amd.envs.vec import VecBlockScriptedPartner
    third = VecBlockScriptedPartner(0, "EASY") if variant == 0 else _frozen(variant, 1, 14)
    return [_frozen(variant, 1, 13), VecBlockScriptedPartner(variant, "DEFAULT"), third]


def _xplay(variant, planners, native, E=72, G=3, seed=5):
    from pantheonrl_amd.envs.crossplay import VecBlockCrossPlay
    return VecBlockCrossPlay(variant, E, planners, _constructors(variant), games=G, seed=seed, native=native)


KEYS = ("state", "ego_actions", "alt_actions", "obs_ego", "obs_alt", "games", "playing", "ep_return", "ep_length", "returns", "lengths",
        "tables_left", "running")


def _snapshot(xp):
    return {k: getattr(xp, k).cpu().numpy().copy() for k in KEYS}


# ---- 1. the scripted rules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,rule,key", [(1, 0, "ctor_obs"), (0, 0, "sbw_obs"), (0, 1, "sbw_obs")])
def test_scripted_actions_kernel_is_the_host_rule_and_leaves_masked_rows_alone(variant, rule, key):
    from pantheonrl_amd.envs.vec import VecBlockScriptedPartner
    rows = np.ascontiguousarray(Z[key].reshape(-1, Z[key].shape[-1]).astype(np.float32))
    n, A = len(rows), 3 if variant else 2
    want = nat.block_scripted_actions_host(variant, rule, rows)
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
    obs = th.as_tensor(rows).to(DEV)
    member = VecBlockScriptedPartner(variant, rule)
    on = (np.arange(n) % 3 != 1)
    out = th.full((n, A), -7, dtype=th.int32, device=DEV)
    got = member.get_action(obs, th.as_tensor(on.astype(np.uint8)).to(DEV), out, ctx).cpu().numpy()
    assert np.array_equal(got[on], want[on]) and (got[~on] == -7).all()
    out.fill_(-7)
    assert np.array_equal(member.get_action(obs, None, out, ctx).cpu().numpy(), want)


# ---- 2. the grouped forward -----------------------------------------------------------------------------------------------------------
def _group_case(n=72):
    """member 0 holds 36 active rows (two full 16-row tiles and a partial one -- more than one 32-row body), member 1 holds one, member
    2 the rest; ten rows are inactive, some of every member"""
    rng = np.random.RandomState(7)
    ids = np.array([0] * 40 + [1] * 3 + [2] * 29)
    active = np.ones(n, bool)
    for k, off in ((0, 4), (1, 2), (2, 4)):
        rows = np.nonzero(ids == k)[0]
        active[rng.choice(rows, off, replace=False)] = False
    perm = rng.permutation(n)
    return ids[perm].astype(np.int32), active[perm]


@pytest.mark.parametrize("variant,seat", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_grouped_forward_rows_are_the_members_own_forward_rows(variant, seat):
    from pantheonrl_amd.envs.vec import VecBlockScriptedPartner, VecBlockWorld
    n, counter = 72, 11
    ids, active = _group_case(n)
    assert np.bincount(ids[active]).tolist() == [36, 1, 25] and (~active).sum() == 10
    spaces = VecBlockWorld.seat_spaces(variant)[seat]
    nvec = np.asarray(spaces.observation_space.nvec)
    rng = np.random.RandomState(variant * 2 + seat)
    obs_h = (rng.rand(n, len(nvec)) * nvec).astype(np.int64).astype(np.float32)
    obs = th.as_tensor(obs_h).to(DEV)
    # the planner's seat takes no scripted member: three frozen ones there, two frozen and the scripted rule at the constructor's
    members = [_frozen(variant, seat, 21), _frozen(variant, seat, 22)]
    members.append(VecBlockScriptedPartner(variant, "DEFAULT") if seat == 1 else _frozen(variant, seat, 23))
    assert members[0].policy._seed != members[1].policy._seed
    pol = members[0].policy
    A = pol.layout.A
    arr = (nat.PhPoolMember * 3)()
    for c, m in zip(arr, members):
        c.kind = m.kind
        if m.kind == nat.PH_POOL_SCRIPTED:
            c.seed = m.rule
        else:
            c.params, c.seed = m.policy.params.data_ptr(), m.policy._seed
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
    out = th.full((n, A), -7, dtype=th.int32, device=DEV)
    ids_d, active_d = th.as_tensor(ids).to(DEV), th.as_tensor(active.astype(np.uint8)).to(DEV)
    nat.check(ctx.lib.ph_block_group_forward(ctx.handle, C.byref(pol.spec), arr, 3, obs.data_ptr(), ids_d.data_ptr(), active_d.data_ptr(),
                                             counter, out.data_ptr(), n))
    got = out.cpu().numpy()
    assert (got[~active] == -7).all()
    for k, m in enumerate(members):
        rows = active & (ids == k)
        if m.kind == nat.PH_POOL_SCRIPTED:
            want = nat.block_scripted_actions_host(variant, m.rule, obs_h)
        else:
            m.policy._counter = counter - 1
            want = m.get_action(obs).cpu().numpy()                      # ph_policy_forward of this member over all rows
            assert want.dtype == np.int32 and want.shape == (n, A)
        assert np.array_equal(got[rows], want[rows]), (variant, seat, k)
    # two frozen members of different parameters and seeds do not play the same rows alike: the member index reached the tile
    members[0].policy._counter = members[1].policy._counter = counter - 1
    assert not np.array_equal(members[0].get_action(obs).cpu().numpy(), members[1].get_action(obs).cpu().numpy())


def test_grouped_forward_refuses_what_it_does_not_seat():
    n = 8
    pol_p, pol_c = _frozen(0, 0, 21).policy, _frozen(0, 1, 21).policy
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
    ids, active = th.zeros(n, dtype=th.int32, device=DEV), th.ones(n, dtype=th.uint8, device=DEV)
    out = th.full((n, 2), -7, dtype=th.int32, device=DEV)

    def call(pol, kind, seed=0):
        arr = (nat.PhPoolMember * 1)()
        arr[0].kind, arr[0].params, arr[0].seed = kind, pol.params.data_ptr(), seed
        obs = th.zeros((n, pol.layout.D), dtype=th.float32, device=DEV)
        nat.check(ctx.lib.ph_block_group_forward(ctx.handle, C.byref(pol.spec), arr, 1, obs.data_ptr(), ids.data_ptr(), active.data_ptr(), 1,
                                                 out.data_ptr(), n))

    with pytest.raises(nat.NativeError, match="PH_POOL_LEARNER"):
        call(pol_c, nat.PH_POOL_LEARNER)
    with pytest.raises(nat.NativeError, match="PH_POOL_CLONE"):
        call(pol_c, nat.PH_POOL_CLONE)
    with pytest.raises(nat.NativeError, match="scripted member needs a block-world constructor spec"):
        call(pol_p, nat.PH_POOL_SCRIPTED)
    with pytest.raises(nat.NativeError, match="unknown rule"):
        call(pol_c, nat.PH_POOL_SCRIPTED, seed=2)
    with pytest.raises(nat.NativeError, match="BlockEnv-v0 only"):
        call(_frozen(1, 1, 21).policy, nat.PH_POOL_SCRIPTED, seed=1)
    assert (out.cpu().numpy() == -7).all()                                 # nothing was launched


# ---- 3. the native step is bitwise its walk -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_native_step_is_bitwise_the_walk_after_every_step(variant):
    planners = [_frozen(variant, 0, 11), _frozen(variant, 0, 12)]
    a, b = (_xplay(variant, planners, native) for native in (True, False))
    assert a.P == 6 and a.pairs.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2]]
    assert np.array_equal(a.ego_id.cpu().numpy(), a.pairs[np.arange(72) % 6, 0])
    assert np.array_equal(a.alt_id.cpu().numpy(), a.pairs[np.arange(72) % 6, 1])
    for step in range(49):
        sa, sb = _snapshot(a), _snapshot(b)
        for key in KEYS:
            assert np.array_equal(sa[key], sb[key]), (step, key)
        assert np.array_equal(sb["playing"], (sb["games"] < 3).astype(np.uint8)) and sb["tables_left"][0] == sb["playing"].sum()
        if step < 48:
            a.step()
            b.step()
    # nothing vacuous, judged on the walk alone: games ended, constructors of every kind moved, worlds were regenerated
    assert sb["games"].sum() > 0 and sb["lengths"].max() >= 2
    assert len(np.unique(sb["alt_actions"], axis=0)) > 3


# ---- 4. budgets and idle tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_budget_idling_statistics_and_repeatability(variant):
    """each planner's end-token bias is raised by 3: at the near-zero logits of a fresh policy p(end) is about 0.57 (v0: e^3 / (e^3 +
    15)) and 0.41 (v1: e^3 / (e^3 + 29)), so the chance that one game outlasts 40 tokens is below 0.59^40 < 1e-9"""
    from pantheonrl_amd.envs.crossplay import crossplay_stats
    G, E = 3, 72
    planners = [_biased_planner(variant, 11), _biased_planner(variant, 12)]
    xp = _xplay(variant, planners, True)
    res = xp.run(max_steps=40 * G, chunk=8)
    s = _snapshot(xp)
    assert xp.left() == 0 and (s["games"] == G).all() and not s["playing"].any() and not s["running"].any() and res.unfinished == 0
    assert res.steps <= 40 * G
    for _ in range(4):                                                     # idle means idle
        xp.step()
    after = _snapshot(xp)
    for key in KEYS:
        assert np.array_equal(s[key], after[key]), key
    # the statistics are a float64 reduction of the logs per pair
    want = crossplay_stats(s["returns"], s["lengths"], xp.pair_of_table, xp.P, games=s["games"])
    st = xp.stats()
    assert st["unfinished"] == 0 and np.array_equal(st["count"], np.full(6, 12 * G, np.float64))
    for key in ("count", "mean", "std", "mean_length"):
        assert np.array_equal(st[key], want[key]), key
    # returns are what the games pay
    if variant == 0:
        assert set(np.unique(s["returns"]).tolist()) <= {0.0, 20.0, 40.0, 60.0, 80.0, 100.0}
    else:
        assert s["returns"].min() >= 0.0 and s["returns"].max() <= 1.0
    assert s["lengths"].min() >= 1 and s["lengths"].max() <= 40
    # two runs give equal bits, and the walk of the same evaluation ends where the native step does
    again = _xplay(variant, planners, True)
    again.run(max_steps=40 * G, chunk=5)
    walk = _xplay(variant, planners, False)
    for _ in range(res.steps):
        walk.step()
    for other in (again, walk):
        so = _snapshot(other)
        for key in ("state", "games", "playing", "returns", "lengths", "ep_return", "ep_length", "tables_left"):
            assert np.array_equal(s[key], so[key]), key


# ---- 5. the step cap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_step_cap_reports_unfinished_games_and_counts_the_logged_ones(variant):
    xp = _xplay(variant, [_frozen(variant, 0, 11), _frozen(variant, 0, 12)], True)
    res = xp.run(max_steps=8)
    games = xp.games.cpu().numpy()
    assert res.steps == 8 and res.unfinished > 0 and res.unfinished == 72 * 3 - games.sum()
    assert res.count.sum() == games.sum() and xp.stats()["unfinished"] == res.unfinished
    assert np.array_equal(res.count, np.bincount(xp.pair_of_table, weights=games, minlength=6))


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_crossplay_command_line_on_saved_checkpoints(variant, tmp_path, capsys):
    from pantheonrl_amd import crossplay
    _ppo(variant, 0, 31).save(str(tmp_path / "planner"))
    _ppo(variant, 1, 32).save(str(tmp_path / "constructor"))
    capsys.readouterr()
    res = crossplay.run([f"BlockEnv-v{variant}", "--agents", str(tmp_path / "planner"), "--partners", str(tmp_path / "constructor"), "DEFAULT",
                         "--n-envs", "16", "-t", "16", "--max-steps", "24", "--out", str(tmp_path / "x.npz")])
    out = capsys.readouterr().out
    assert "Average Reward (row = planner, column = constructor)" in out and "Standard Deviation" in out
    z = np.load(str(tmp_path / "x.npz"))
    assert z["mean"].shape == z["std"].shape == z["count"].shape == z["length"].shape == (1, 2)
    assert z["pairs"].tolist() == [[0, 0], [0, 1]] and z["pair_of_table"].tolist() == [0, 1] * 8
    assert z["returns"].shape == z["lengths"].shape == (16, 2) and z["games"].shape == (16,)          # 8 tables per pair: ceil(16 / 8) games
    assert int(z["unfinished"]) == res.unfinished == 32 - z["games"].sum() and z["count"].sum() == z["games"].sum()
    assert ("WARNING" in out) == (res.unfinished > 0)
    assert z["partners"].tolist()[1] == "DEFAULT"
