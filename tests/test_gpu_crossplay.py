"""gpu: device-resident cross-play evaluation of Liar's Dice -- the native step against the walk after every step, idle tables,
the walk against the host MultiAgentEnv table by table, the statistics kernel, graph capture, ABI misuse and the two command
lines."""
import ctypes as C
import re
from collections import deque

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu


def _ppo(seed, **kw):
    from pantheonrl_amd import PPO
    return PPO("MlpPolicy", LC.spaces(), n_steps=2, n_envs=4, batch_size=8, n_epochs=1, seed=seed, **kw)


# ---- 1. the native step is bitwise the walk --------------------------------------------------------------------------------------
def test_native_crossplay_step_is_bitwise_the_walk_after_every_step():
    E, G, kinds = 50, 3, ["frozen", "frozen", "scripted", "frozen"]        # 16 pairs on 50 tables: 3 or 4 tables each
    a, b = (LC.xplay(E, kinds, G, native=native) for native in (True, False))
    assert a.P == 16 and np.bincount(a.pair_of_table).tolist() == [4, 4] + [3] * 14
    assert np.array_equal(a.ego_id.cpu().numpy(), a.pairs[np.arange(E) % 16, 0])
    assert np.array_equal(a.alt_id.cpu().numpy(), a.pairs[np.arange(E) % 16, 1])
    finished_at = np.full(E, -1)
    partner_opened = False
    steps = 0
    while True:
        sa, sb = LC.xstate(a), LC.xstate(b)
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (steps, key)
        assert np.array_equal(sb["playing"], (sb["games"] < G).astype(np.uint8))
        assert sb["tables_left"][0] == sb["playing"].sum()
        fresh = (sb["nmoves"] <= 1) & (sb["playing"] != 0)
        partner_opened |= bool((fresh & (sb["ego_first"] == 0) & (sb["nmoves"] == 1)).any())
        finished_at[(finished_at < 0) & (sb["playing"] == 0)] = steps
        if sb["tables_left"][0] == 0:
            break
        assert steps < 7 * G
        a.step()
        b.step()
        steps += 1
    # nothing vacuous -- judged on the walk alone
    assert sb["games"].sum() == E * G and (sb["games"] == G).all() and steps <= 7 * G
    assert sb["lengths"].min() >= 1 and sb["lengths"].max() >= 2 and sb["lengths"].max() <= 7
    assert partner_opened
    assert len(set(finished_at.tolist())) > 1 and finished_at.min() >= G
    assert set(np.unique(sb["returns"]).tolist()) == {-1.0, 1.0}


# ---- 2. idle means idle ------------------------------------------------------------------------------------------------------------
def test_a_table_that_spent_its_budget_never_changes_again():
    xp = LC.xplay(20, ["frozen", "scripted"], 2)
    res = xp.run(chunk=3)
    assert xp.left() == 0 and res.steps <= 14 and (res.count == 2 * 5).all()
    scratch = ("ego_actions", "alt_actions", "_running", "_alt_opens", "_ego_opens", "_done")
    before = LC.xstate(xp)
    before.update({k: getattr(xp, k).cpu().numpy().copy() for k in scratch})
    for _ in range(4):
        xp.step()
    after = LC.xstate(xp)
    after.update({k: getattr(xp, k).cpu().numpy().copy() for k in scratch})
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert after["tables_left"][0] == 0 and not after["playing"].any() and not after["_running"].any()


# ---- 3. the walk against the host MultiAgentEnv, table by table --------------------------------------------------------------------
def test_crossplay_walk_matches_the_host_multiagentenv_table_by_table():
    from pantheonrl_amd.common import Agent, Observation
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    from pantheonrl_amd.envs.liar import LiarDefaultAgent, LiarEnv

    class Shadow(LiarEnv):
        def __init__(self):
            super().__init__()
            self.deals = deque()

        def n_reset(self):
            ego_first, hands = self.deals.popleft()
            self.ego_next = bool(ego_first)
            self.history, self.egohand, self.althand = [], [int(x) for x in hands[:6]], [int(x) for x in hands[6:]]
            return (0 if self.ego_next else 1,), (Observation(self.getObs(self.ego_next)),)

    class Replay(Agent):
        """plays the moves the device sampled"""
        def __init__(self):
            self.moves = deque()

        def get_action(self, obs, record=True):
            return self.moves.popleft()

        def update(self, reward, done):
            pass

    class Logged(VecLiarCrossPlay):
        def _seat_act(self, seat, obs, mask, counter):
            out = super()._seat_act(seat, obs, mask, counter)
            self.__dict__.setdefault("log", []).append((seat, out.cpu().numpy().copy(), mask.cpu().numpy().astype(bool)))
            return out

    E, G, kinds = 24, 3, ["frozen", "scripted", "frozen"]
    pairs = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1)]          # a diagonal pair, the scripted member in seat 0, in seat 1, in both
    xp = LC.xplay(E, kinds, G, pairs=pairs, seed=2, native=False, cls=Logged)
    ego_kind = [kinds[pairs[e % 5][0]] for e in range(E)]
    alt_kind = [kinds[pairs[e % 5][1]] for e in range(E)]
    shadows = [Shadow() for _ in range(E)]
    partners = [LiarDefaultAgent() if alt_kind[e] == "scripted" else Replay() for e in range(E)]
    for s, p in zip(shadows, partners):
        s.add_partner_agent(p)
    a_ego = np.zeros((E, 2), np.int64)

    def feed(dealt):
        hands, first = xp.env.hands.cpu().numpy(), xp.ego_first.cpu().numpy()
        for seat, acts, mask in xp.log:
            for e in np.nonzero(mask)[0]:
                if seat == 0:
                    a_ego[e] = acts[e]
                elif alt_kind[e] == "frozen":
                    partners[e].moves.append(acts[e].copy())
        xp.log.clear()
        for e in np.nonzero(dealt)[0]:
            shadows[e].deals.append((first[e], hands[e].copy()))

    feed(np.ones(E, bool))                  # the constructor's deal and the openings
    cur = [s.reset() for s in shadows]
    ret, ln = np.zeros(E, np.float32), np.zeros(E, np.int64)
    logged = [[] for _ in range(E)]
    steps = 0
    while xp.left() > 0:
        before, games0, playing0 = xp.obs_ego.cpu().numpy().copy(), xp.games.cpu().numpy().copy(), xp.playing.cpu().numpy().copy()
        xp.step()
        steps += 1
        games1, playing1, after = xp.games.cpu().numpy(), xp.playing.cpu().numpy(), xp.obs_ego.cpu().numpy()
        feed((games1 > games0) & (playing1 != 0))
        for e in range(E):
            if not playing0[e]:
                assert games1[e] == G and np.array_equal(before[e], after[e])
                continue
            assert np.array_equal(before[e], np.asarray(cur[e], np.float32)), (steps, e)
            if ego_kind[e] == "scripted":          # the device's scripted seat 0 plays LiarDefaultAgent's move
                assert np.array_equal(LiarDefaultAgent().get_action(Observation(np.asarray(cur[e]))), a_ego[e]), (steps, e)
            o, r, d, _ = shadows[e].step(a_ego[e])
            ret[e] += np.float32(r)               # tester.py:41-63: reward += newreward
            ln[e] += 1
            assert bool(d) == bool(games1[e] > games0[e]), (steps, e)
            if d:
                logged[e].append((float(ret[e]), int(ln[e])))
                ret[e], ln[e] = 0.0, 0
                if not playing1[e]:
                    continue
                o = shadows[e].reset()
            cur[e] = o
            assert np.array_equal(after[e], np.asarray(o, np.float32)), (steps, e)
            assert not (isinstance(partners[e], Replay) and partners[e].moves), (steps, e)
    assert steps <= 7 * G
    returns, lengths = xp.returns.cpu().numpy(), xp.lengths.cpu().numpy()
    for e in range(E):
        assert len(logged[e]) == G and not shadows[e].deals
        assert [g[0] for g in logged[e]] == returns[e].tolist() and [g[1] for g in logged[e]] == lengths[e].tolist(), e
    assert lengths.max() >= 2 and set(np.unique(returns).tolist()) == {-1.0, 1.0}


# ---- 4. the statistics kernel --------------------------------------------------------------------------------------------------
def test_statistics_kernel_is_the_host_statement_and_runs_are_bitwise_repeatable():
    from pantheonrl_amd.envs.crossplay import crossplay_stats
    E, G, kinds = 40, 5, ["frozen", "scripted", "frozen"]           # 9 pairs on 40 tables: 5 or 4 tables each
    runs = []
    for seed in (5, 5, 6):
        xp = LC.xplay(E, kinds, G, seed=seed)
        res = xp.run()
        runs.append((res, xp.stats.cpu().numpy().copy()))
    res, raw = runs[0]
    assert res.steps <= 7 * G and set(np.unique(res.returns).tolist()) == {-1.0, 1.0}
    want = crossplay_stats(res.returns, res.lengths, res.pair_of_table, 9)
    assert want["count"].tolist() == [5.0 * G] * 4 + [4.0 * G] * 5
    for i, key in enumerate(("count", "sum", "sumsq", "sum_length")):      # +-1 returns: every sum is an integer, so exact
        assert np.array_equal(raw[:, i], want[key]), key
        assert np.array_equal(getattr(res, key), want[key])
    for key in ("mean", "std", "mean_length"):
        assert np.array_equal(getattr(res, key), want[key]), key
    for p in range(9):
        r = res.returns[res.pair_of_table == p].astype(np.float64)
        assert res.mean[p] == r.mean() and abs(res.std[p] - r.std()) < 1e-14
    m = res.matrix("mean")
    assert m.shape == (3, 3) and np.array_equal(m.reshape(-1), res.mean) and not np.isnan(m).any()
    # a partial pair list leaves nan where nothing was played
    part = LC.xplay(8, kinds, 1, pairs=[(0, 1), (2, 2)]).run().matrix("count")
    assert part[0, 1] == 4 and part[2, 2] == 4 and np.isnan(part).sum() == 7
    # the same seeds: the same bits; another dice seed: other games
    again, raw_again = runs[1]
    assert np.array_equal(res.returns, again.returns) and np.array_equal(res.lengths, again.lengths) and np.array_equal(raw, raw_again)
    other, _ = runs[2]
    assert not (np.array_equal(res.returns, other.returns) and np.array_equal(res.lengths, other.lengths))


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------
def test_a_captured_chunk_of_crossplay_steps_replays_with_no_host_work():
    kinds = ["frozen", "scripted", "frozen"]
    xp, eager = LC.xplay(32, kinds, 6), LC.xplay(32, kinds, 6)
    for c in range(1, 7):
        eager.step()
    stream = th.cuda.Stream(device=xp.dev)
    th.cuda.synchronize()
    with th.cuda.stream(stream):
        for c in (1, 2):
            xp._native_call(c)
        stream.synchronize()
        xp._bind()
        nat.check(xp.ctx.lib.ph_graph_begin(xp.ctx.handle))
        try:
            for c in (3, 4, 5, 6):
                xp._native_call(c)
        finally:
            gid = C.c_int(-1)
            nat.check(xp.ctx.lib.ph_graph_end(xp.ctx.handle, C.byref(gid)))
        assert gid.value >= 0
        games = int(xp.games.sum().item())
        nat.check(xp.ctx.lib.ph_graph_launch(xp.ctx.handle, gid.value))
        stream.synchronize()
    th.cuda.synchronize()
    assert int(xp.games.sum().item()) > games                       # games advance across the replay
    sa, sb = LC.xstate(xp), LC.xstate(eager)
    for key in sa:                                                   # and the replay is the four eager steps
        assert np.array_equal(sa[key], sb[key]), key


# ---- 6. ABI misuse -------------------------------------------------------------------------------------------------------------------
def test_crossplay_abi_misuse_is_reported_not_fatal():
    from pantheonrl_amd import spaces as sps
    from pantheonrl_amd.envs.crossplay import VecLiarCrossPlay
    from pantheonrl_amd.envs.vec import VecLiarDefaultPartner
    xp = LC.xplay(16, ["frozen", "scripted", "frozen"], 2)
    xp._bind()
    lib, h, d = xp.ctx.lib, xp.ctx.handle, xp._desc
    err = lambda: lib.ph_last_error()  # noqa: E731
    call = lambda: lib.ph_liar_xplay_step(h, C.byref(d), 1, 0)  # noqa: E731
    assert lib.ph_liar_xplay_step(h, None, 1, 0) != 0 and b"null" in err()
    for field, bad, word in (("n_members", 0, b"1..PH_MAX_POOL"), ("n_members", 9, b"1..PH_MAX_POOL"), ("episodes_per_table", 0, b"at least 1"),
                             ("n", 0, b"incomplete"), ("n_pairs", 0, b"pairs"), ("n_pairs", 17, b"pairs"), ("games", None, b"incomplete"),
                             ("tables_left", None, b"incomplete"), ("ego_id", None, b"incomplete"), ("returns", None, b"incomplete"),
                             ("hands", xp.env.hands.data_ptr() + 4, b"16-byte")):
        good = getattr(d, field)
        setattr(d, field, bad)
        assert call() != 0 and word in err(), field
        setattr(d, field, good)
    arr = xp._member_arr
    arr[0].kind = nat.PH_POOL_LEARNER
    assert call() != 0 and b"PH_POOL_LEARNER" in err() and b"member 0" in err()
    arr[0].kind = nat.PH_POOL_FROZEN
    good = arr[2].params
    arr[2].params = None
    assert call() != 0 and b"null params" in err()
    arr[2].params = good
    for slot, bad in ((1, 3), (4, -1)):
        keep = xp._pairs_arr[slot]
        xp._pairs_arr[slot] = bad
        assert call() != 0 and b"out of range" in err() and b"pair" in err()
        xp._pairs_arr[slot] = keep
    rps = sps.make_spec(sps.Discrete(1), sps.Discrete(3))
    box = sps.make_spec(sps.Box(-1, 1, (30,)), sps.MultiDiscrete([7, 12]))
    good = C.pointer(xp.spec)
    for spec in (rps, box):
        d.spec = C.pointer(spec)
        assert call() != 0 and b"one-hot" in err()
    d.spec = good
    st = lambda **kw: lib.ph_xplay_stats(h, *[kw.get(k, v) for k, v in (  # noqa: E731
        ("returns", xp.returns.data_ptr()), ("lengths", xp.lengths.data_ptr()), ("games", xp.games.data_ptr()), ("n", 16), ("G", 2),
        ("P", 9), ("stats", xp.stats.data_ptr()))])
    assert st(returns=None) != 0 and b"null" in err()
    assert st(P=17) != 0 and b"pairs" in err()
    assert st(G=0) != 0 and b"positive" in err()
    assert st(stats=xp.stats.data_ptr() + 8) != 0 and b"16-byte" in err()
    # ... and the process is alive and the evaluation still runs to its end
    assert st() == 0
    res = xp.run()
    assert xp.left() == 0 and (res.count >= 2).all() and res.count.sum() == 32
    with pytest.raises(nat.NativeError, match="1..8"):
        VecLiarCrossPlay(128, [VecLiarDefaultPartner()] * 9)
    with pytest.raises(nat.NativeError, match="at least as many tables"):
        VecLiarCrossPlay(3, [VecLiarDefaultPartner()] * 2)
    with pytest.raises(nat.NativeError, match="episodes_per_table"):
        VecLiarCrossPlay(4, [VecLiarDefaultPartner()] * 2, episodes_per_table=0)


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
def test_tester_and_crossplay_command_lines(tmp_path, capsys):
    from pantheonrl_amd import crossplay, tester
    for name, seed in (("a", 3), ("b", 4)):
        _ppo(seed).save(str(tmp_path / name))
    capsys.readouterr()
    rewards = tester.run(["LiarsDice-v0", "PPO", "PPO", "--ego-load", str(tmp_path / "a"), "--alt-load", str(tmp_path / "b"),
                          "--n-envs", "32", "-t", "100", "--seed", "1"])
    out = capsys.readouterr().out
    assert len(rewards) == 32 * 4 and set(rewards) == {-1.0, 1.0}         # G = ceil(100 / 32) = 4
    mean = float(re.search(r"^Average Reward: (\S+)$", out, flags=re.M).group(1))
    std = float(re.search(r"^Standard Deviation: (\S+)$", out, flags=re.M).group(1))
    assert mean == np.mean(rewards) and abs(std - np.std(rewards)) < 1e-14
    assert re.search(r"^Games played: 128 ", out, flags=re.M)
    rewards = tester.run(["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", str(tmp_path / "a"), "--n-envs", "8", "-t", "16"])
    assert len(rewards) == 16
    capsys.readouterr()
    res = crossplay.run(["LiarsDice-v0", "--agents", str(tmp_path / "a"), str(tmp_path / "b"), "DEFAULT", "--n-envs", "32", "-t", "6",
                         "--out", str(tmp_path / "x.npz")])
    out = capsys.readouterr().out
    assert "Average Reward" in out and "Standard Deviation" in out
    z = np.load(str(tmp_path / "x.npz"))
    assert z["mean"].shape == z["std"].shape == z["count"].shape == z["mean_length"].shape == (3, 3)
    assert np.array_equal(z["mean"], res.matrix("mean")) and (z["count"] >= 6).all() and (np.abs(z["mean"]) <= 1).all()
    assert z["returns"].shape == (32, 2) and z["agents"].tolist()[2] == "DEFAULT"          # 3 tables per pair: ceil(6 / 3) games
    # a tower checkpoint is refused by name
    _ppo(5, policy_kwargs={"net_arch": [{"pi": [32], "vf": [32]}]}).save(str(tmp_path / "tower"))
    with pytest.raises(nat.NativeError, match="ArchActorCriticPolicy does not run on the fused MLP kernels"):
        tester.run(["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", str(tmp_path / "tower"), "--n-envs", "8"])
