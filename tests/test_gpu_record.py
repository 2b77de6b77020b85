"""gpu: the device-resident move log of the vectorised Liar's Dice step (csrc/ph_record.h) -- the native log against the walk's in
self-play, the pool and cross-play; the log against the reference recorder (TurnBasedRecorder around the host LiarEnv) table by
table; capacity; the export's seat filters; graph capture; the persistent rollout's refusal; the command lines end to end.
Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu

POOL_KINDS = ["learner", "frozen", "scripted", "learner"]


def _selfplay(E, T_ego, T_alt, native, record, towers=False, seed=4):
    ego, alt = LC.ppo(E, T_ego, seed, (128, 128) if towers else None), LC.ppo(E, T_alt, seed + 1, (32,) if towers else None)
    return LC.selfplay(E, ego, alt, seed=seed, native=native, record=record)[0]


def _pool(E, T_ego, T_alt, native, record, resample="robin", seed=11, kinds=POOL_KINDS):
    return LC.pool(E, T_ego, T_alt, kinds, seed=seed, native=native, resample=resample, record=record)[0]


def _xplay(E, G, native, record, kinds=("frozen", "frozen", "scripted"), seed=5):
    return LC.xplay(E, kinds, G, seed=seed, native=native, record=record)


def _train_state(sp):
    """the end state of a training run: the game, both seats' recorded rows, the parameters after the updates"""
    return LC.train_state(sp, sp.ego)


def _train_steps(sp, steps):
    """`steps` vectorised steps; a partner-side learner trains whenever it is full (the ego trains inside the step)"""
    for _ in range(steps):
        sp.step()
        for m in sp.learners:
            if m.full():
                m.learn_from_buffer()
    th.cuda.synchronize()


def _log(sp, seat=None):
    rec = sp.recorded(seat)
    return dict(rows=rec.rows.cpu().numpy(), member=rec.member.cpu().numpy(), offsets=rec.table_offsets, dropped=rec.dropped)


def _check_log_shape(log, E):
    rows, off = log["rows"], log["offsets"]
    assert rows.shape == (off[-1], 33) and off.shape == (E + 1,) and off[0] == 0 and (np.diff(off) >= 0).all()
    assert log["member"].shape == (len(rows),) and log["dropped"].shape == (E,)
    assert set(np.unique(rows[:, 32]).tolist()) == {0.0, 1.0, 2.0, 3.0}          # every kind of move happened: nothing vacuous


# ---- 1. the native log is the walk's, and recording does not perturb the run -------------------------------------------------------
@pytest.mark.parametrize("towers", [False, True], ids=["mlp64", "towers"])
def test_selfplay_native_log_is_the_walks_and_the_recorder_only_reads(towers):
    E, steps = 48, 24
    cap = 3 * steps + 1
    runs = {}
    for name, native, record in (("native", True, cap), ("walk", False, cap), ("plain", True, 0)):
        sp = _selfplay(E, 8, 6, native, record, towers=towers)
        assert sp.persistent is False or name == "plain"                  # launch by launch while recording
        assert sp.towers == towers
        _train_steps(sp, steps)
        runs[name] = (_train_state(sp), _log(sp) if record else None)
    LC.same_state(runs["native"][1], runs["walk"][1], "log")
    LC.same_state(runs["native"][0], runs["plain"][0], "state, recorder attached vs none")
    log, state = runs["native"][1], runs["native"][0]
    _check_log_shape(log, E)
    assert not log["dropped"].any() and not log["member"].any()
    assert (log["rows"][:, 32] >= 2).sum() == state["episodes"] > E and state["ego_it"] >= 2 and state["it0"] >= 1
    assert (np.diff(log["offsets"]) >= steps).all()                        # the ego moves in every table at every step


@pytest.mark.parametrize("resample", ["robin", "random"])
def test_pool_native_log_is_the_walks_and_the_recorder_only_reads(resample):
    E, steps = 48, 32
    cap = 3 * steps + 1
    runs = {}
    for name, native, record in (("native", True, cap), ("walk", False, cap), ("plain", True, 0)):
        sp = _pool(E, 8, 4, native, record, resample=resample)
        _train_steps(sp, steps)
        runs[name] = (_train_state(sp), _log(sp) if record else None)
    LC.same_state(runs["native"][1], runs["walk"][1], "log")
    LC.same_state(runs["native"][0], runs["plain"][0], "state, recorder attached vs none")
    log, state = runs["native"][1], runs["native"][0]
    _check_log_shape(log, E)
    assert not log["dropped"].any()
    seat1 = log["rows"][:, 32].astype(int) % 2 == 1
    assert not log["member"][~seat1].any() and set(np.unique(log["member"][seat1]).tolist()) == {0, 1, 2, 3}
    assert (log["rows"][:, 32] >= 2).sum() == state["episodes"] and min(state["it0"], state["it1"]) >= 1


def test_crossplay_native_log_is_the_walks_and_the_recorder_only_reads():
    from pantheonrl_amd.envs.crossplay import MAX_STEPS_PER_GAME
    E, G = 24, 3
    cap = 3 * MAX_STEPS_PER_GAME * G
    runs = {}
    for name, native, record in (("native", True, cap), ("walk", False, cap), ("plain", True, 0)):
        xp = _xplay(E, G, native, record)
        assert xp.P == 9
        res = xp.run(chunk=3)
        assert (res.count >= 2 * G).all()
        runs[name] = (LC.xstate(xp), _log(xp) if record else None, xp)
    LC.same_state(runs["native"][1], runs["walk"][1], "log")
    LC.same_state(runs["native"][0], runs["plain"][0], "state, recorder attached vs none")
    state, log, xp = runs["native"]
    _check_log_shape(log, E)
    assert not log["dropped"].any() and state["games"].sum() == E * G == (log["rows"][:, 32] >= 2).sum()
    # who moved: the table's pair, by seat
    seat = log["rows"][:, 32].astype(int) % 2
    table = np.repeat(np.arange(E), np.diff(log["offsets"]))
    want = np.where(seat == 0, xp.pairs[xp.pair_of_table[table], 0], xp.pairs[xp.pair_of_table[table], 1])
    assert np.array_equal(log["member"], want)
    # idle tables log nothing: further steps leave the log as it is
    for _ in range(3):
        xp.step()
    LC.same_state(_log(xp), log, "idle")


# ---- 2. the log is the reference recorder's ------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """every move the walk plays and every deal it makes, in order, from the game's own entry points (not from the recorder)"""
    from pantheonrl_amd.envs.vec import VecLiarsDice, VecLiarStep
    events = []
    inner_step, inner_deal = VecLiarsDice.player_step, VecLiarStep._deal

    def player_step(self, actions, is_ego, active=None):
        on = np.ones(self.E, bool) if active is None else active.cpu().numpy().astype(bool)
        events.append(("move", actions.cpu().numpy().reshape(self.E, 2).copy(), is_ego.cpu().numpy().astype(bool), on))
        return inner_step(self, actions, is_ego, active)

    def deal(self, reset_mask, c):
        at = len(events)                     # the deal stands in front of the opening it makes
        inner_deal(self, reset_mask, c)
        events.insert(at, ("deal", reset_mask.cpu().numpy().astype(bool), self.env.hands.cpu().numpy().copy(),
                           self.ego_first.cpu().numpy().astype(bool)))
    monkeypatch.setattr(VecLiarsDice, "player_step", player_step)
    monkeypatch.setattr(VecLiarStep, "_deal", deal)
    return events


@pytest.mark.parametrize("mode", ["pool-robin", "pool-random", "crossplay"])
def test_walk_log_is_the_reference_recorders_table_by_table(mode, monkeypatch):
    from pantheonrl_amd.envs.crossplay import MAX_STEPS_PER_GAME
    E = 24
    events = _spy(monkeypatch)
    if mode == "crossplay":
        G = 3
        sp = _xplay(E, G, False, 3 * MAX_STEPS_PER_GAME * G)
        sp.run(chunk=4)
        finished = int(sp.games.sum().item())
        assert finished == E * G
    else:
        steps = 32
        sp = _pool(E, 32, 64, False, 3 * steps + 1, resample=mode.split("-")[1], seed=2)
        for _ in range(steps):
            sp.step()
        finished = sp.episodes
    th.cuda.synchronize()
    rec = sp.recorded()
    rows, off = rec.rows.cpu().numpy(), rec.table_offsets
    assert not rec.dropped.any() and len(rows) == off[-1]
    total = 0
    for e in range(E):
        tr, games = LC.replay_through_the_reference_recorder(events, e)
        mine = rows[off[e]:off[e + 1]]
        assert games >= 2, (e, games)
        assert len(tr.flags) == len(mine), e
        assert np.array_equal(np.asarray(tr.obs), mine[:, :30]), e
        assert np.array_equal(np.asarray(tr.acts), mine[:, 30:32]), e
        assert np.array_equal(np.asarray(tr.flags), mine[:, 32]), e
        assert (mine[:, 32] >= 2).sum() == games
        total += games
    assert total == finished == (rows[:, 32] >= 2).sum()
    # seat 1's opening of a fresh game (nothing bid yet) never ends it, whatever it proposed
    opening = (rows[:, 6] == 6) & (rows[:, 32].astype(int) % 2 == 1)
    assert opening.sum() >= E // 4 and (rows[opening, 32] == 1).all()


# ---- 3. capacity -------------------------------------------------------------------------------------------------------------------------
def test_a_full_table_drops_and_counts_and_nothing_is_written_past_it(monkeypatch):
    from pantheonrl_amd.envs.vec import VecLiarStep
    E, cap, steps, guard, sentinel = 16, 7, 12, 4096, -12345
    guards = {}

    def alloc(self, c):
        rows = th.full((E * c * 33 + guard,), float(sentinel), dtype=th.float32, device=self.dev)
        member = th.full((E * c + guard,), sentinel, dtype=th.int32, device=self.dev)
        rows[:E * c * 33] = 0
        member[:E * c] = 0
        guards[c] = (rows, member)
        return rows[:E * c * 33].view(E, c, 33), member[:E * c].view(E, c)
    monkeypatch.setattr(VecLiarStep, "_record_alloc", alloc)
    small, ample, walk = _pool(E, 16, 8, True, cap), _pool(E, 16, 8, True, 3 * steps + 1), _pool(E, 16, 8, False, cap)
    for sp in (small, ample, walk):
        for _ in range(steps):
            sp.step()
    a, b = _log(small), _log(ample)
    LC.same_state(a, _log(walk), "the walk drops and counts the same moves")
    nb = np.diff(b["offsets"])
    assert (nb > cap).all() and not b["dropped"].any()
    assert np.array_equal(a["offsets"], cap * np.arange(E + 1))
    assert np.array_equal(a["dropped"], nb - cap)
    for e in range(E):                      # a prefix of the table's stream
        lo = b["offsets"][e]
        assert np.array_equal(a["rows"][cap * e:cap * (e + 1)], b["rows"][lo:lo + cap]), e
        assert np.array_equal(a["member"][cap * e:cap * (e + 1)], b["member"][lo:lo + cap]), e
    assert np.array_equal(small._rec_count.cpu().numpy(), np.full(E, cap))
    for c, (rows, member) in guards.items():
        assert (rows[E * c * 33:] == sentinel).all().item() and (member[E * c:] == sentinel).all().item(), c
    LC.same_state(_train_state(small), _train_state(ample), "a full log does not perturb the run")


# ---- 4. the export -----------------------------------------------------------------------------------------------------------------------
def test_export_seat_filters_are_the_hosts_selection_in_order():
    from pantheonrl_amd.envs.vec import export_recording
    E, steps = 37, 9                         # not a multiple of the wave size
    sp = _pool(E, 16, 8, True, 3 * steps + 1, kinds=["frozen", "scripted"])
    for _ in range(steps):
        sp.step()
    empty = [0, 17, 35, 36]                  # the first table, one in the middle, the last two
    for e in empty:
        sp._rec_count[e] = 0
        sp._rec_count_alt[e] = 0
    full = sp.recorded()
    rows, member, off = full.rows.cpu().numpy(), full.member.cpu().numpy(), full.table_offsets
    raw_rows, raw_count = sp._rec_rows.cpu().numpy(), sp._rec_count.cpu().numpy()
    want, want_off = export_recording(raw_rows, raw_count)
    assert np.array_equal(rows, want) and np.array_equal(off, want_off) and len(rows) > 3 * E
    assert all(off[e] == off[e + 1] for e in empty) and (np.diff(off) > 0).sum() == E - len(empty)
    table = np.repeat(np.arange(E), np.diff(off))
    for seat, side in ((0, full.transitions.get_ego_transitions()), (1, full.transitions.get_alt_transitions())):
        part = sp.recorded(seat)
        sel = rows[:, 32].astype(int) % 2 == seat
        assert sel.any() and np.array_equal(part.rows.cpu().numpy(), rows[sel])
        assert np.array_equal(part.member.cpu().numpy(), member[sel])
        assert np.array_equal(part.table_offsets, np.concatenate([[0], np.cumsum(np.bincount(table[sel], minlength=E))]))
        assert np.array_equal(part.transitions.obs, side.obs) and np.array_equal(part.transitions.acts, side.acts)
        assert np.array_equal(part.table_offsets, export_recording(raw_rows, raw_count, seat)[1])
    # N = 0
    sp._rec_count.zero_()
    sp._rec_count_alt.zero_()
    for seat in (None, 0, 1):
        none = sp.recorded(seat)
        assert len(none) == 0 and none.rows.shape == (0, 33) and not none.table_offsets.any()
        assert none.transitions.obs.shape == (0, 30)


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------------
def test_a_recording_pool_step_captures_and_attaching_inside_capture_is_refused():
    E = 32
    eager, sp = (_pool(E, 8, 8, True, 64, seed=3) for _ in range(2))
    for c in range(1, 7):
        eager._native_call(c, ego_pos=c - 1)
    lib, h = sp.env.ctx.lib, sp.env.ctx.handle
    stream = th.cuda.Stream(device=sp.dev)
    th.cuda.synchronize()
    graph = th.cuda.CUDAGraph()
    with th.cuda.stream(stream):
        for c in (1, 2):
            sp._native_call(c, ego_pos=c - 1)
        stream.synchronize()
    with th.cuda.graph(graph, stream=stream):
        sp._bind()
        assert lib.ph_liar_record_attach(h, C.byref(sp._rec_desc)) != 0 and b"capture" in lib.ph_last_error()
        assert lib.ph_liar_record_attach(h, None) != 0 and b"capture" in lib.ph_last_error()
        for c in (3, 4, 5, 6):
            sp._native_call(c, ego_pos=c - 1)
    th.cuda.synchronize()
    before = int(sp._rec_count.sum().item())
    graph.replay()
    th.cuda.synchronize()
    assert int(sp._rec_count.sum().item()) >= before + 4 * E
    LC.same_state(_log(sp), _log(eager), "replayed log vs eager log")
    assert sp.recording and sp.episodes == eager.episodes


# ---- 6. the persistent rollout ------------------------------------------------------------------------------------------------------------
def test_the_one_launch_rollout_is_refused_while_recording(monkeypatch):
    monkeypatch.delenv("LIAR_PERSISTENT", raising=False)
    E, T = 32, 8
    sp = _selfplay(E, T, 6, True, 3 * T + 1)
    assert sp.recording and sp.persistent is False
    ctx = sp.env.ctx
    sp._bind()
    assert ctx.lib.ph_liar_selfplay_rollout(ctx.handle, C.byref(sp._desc), 0, T, 1) != 0
    assert b"recorder is attached" in ctx.lib.ph_last_error()
    with pytest.raises(nat.NativeError, match="recorder is attached"):
        sp.rollout_persistent(T, 1, 0)
    th.cuda.synchronize()
    assert sp.episodes == 0 and len(sp.recorded()) == int((~sp.ego_first.bool()).sum().item())     # nothing ran: the openings only
    sp.stop_recording()
    assert sp.persistent is True
    sp.rollout_persistent(T, 1, 0)
    th.cuda.synchronize()
    assert sp.episodes > 0 and np.isfinite(sp.ego.model.rollout_buffer.host()["values"]).all()
    # a recorder of another size is refused by the step, by name
    other = _pool(16, 4, 4, True, 8, kinds=["scripted"])
    desc = other._rec_desc
    desc.n = 8
    octx = other.env.ctx
    other._bind()
    nat.check(octx.lib.ph_liar_record_attach(octx.handle, C.byref(desc)))
    with pytest.raises(nat.NativeError, match="recorder holds 8 tables, the step 16"):
        other.step()
    for field, bad, word in (("cap", 0, b"cap"), ("rows", desc.rows + 4, b"aligned"), ("count", None, b"incomplete"), ("n", 0, b"positive")):
        good = getattr(desc, field)
        setattr(desc, field, bad)
        assert octx.lib.ph_liar_record_attach(octx.handle, C.byref(desc)) != 0 and word in octx.lib.ph_last_error(), field
        setattr(desc, field, good)
    nat.check(octx.lib.ph_liar_record_attach(octx.handle, None))


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------
def test_record_clone_and_test_pipeline_on_device_resident_tables(tmp_path, monkeypatch):
    from pantheonrl_amd import bctrainer, crossplay, tester, trainer
    from pantheonrl_amd.bc import BC
    from pantheonrl_amd.common.trajsaver import TurnBasedTransitions
    from pantheonrl_amd.envs.vec import VecLiarsDice
    monkeypatch.chdir(tmp_path)
    osp, asp = VecLiarsDice.observation_space, VecLiarsDice.action_space
    cfg = '{"n_steps": 8, "n_epochs": 2}'

    def check_file(name, rec):
        tr = TurnBasedTransitions.read_transition(name, osp, asp)
        table = np.load(name)
        assert table.ndim == 2 and table.shape[1] == 33 and len(table) > 0
        assert set(np.unique(tr.flags).tolist()) <= {0.0, 1.0, 2.0, 3.0}
        if rec is not None:
            assert np.array_equal(table, rec.rows.cpu().numpy())          # the file is what recorded() returned
        return tr

    # self-play: four iterations (two launch by launch, two replayed from the iteration graph), and a pool
    ego, partners, env = trainer.run(["LiarsDice-v0", "PPO", "PPO", "--n-envs", "32", "-t", str(4 * 32 * 8), "--seed", "1",
                                      "--ego-config", cfg, "--alt-config", cfg, "--record", "f.npy", "--ego-save", "m/ego"])
    assert env.recording and env.persistent is False and env.steps_done == 32
    rec = env.recorded()
    tr = check_file("f.npy", rec)
    assert not rec.dropped.any() and (np.diff(rec.table_offsets) >= 32).all() and (tr.flags >= 2).sum() == env.episodes
    _, _, penv = trainer.run(["LiarsDice-v0", "PPO", "PPO", "DEFAULT", "--n-envs", "32", "-t", str(2 * 32 * 8), "--seed", "2",
                              "--ego-config", cfg, "--alt-config", cfg, "{}", "--record", "p.npy"])
    check_file("p.npy", penv.recorded())
    # the evaluation: the tester's vectorised run records (its command line keeps refusing the combination), and so does crossplay
    argv = ["LiarsDice-v0", "PPO", "DEFAULT", "--ego-load", "m/ego", "--n-envs", "16", "-t", "64", "--record", "g.npy"]
    with pytest.raises(trainer.EnvException, match="--record"):
        tester.run(argv)
    args = tester.build_parser().parse_args(argv)
    tester.input_check(args)
    rewards = tester.run_vectorised(args)
    assert len(rewards) == 64
    tg = check_file("g.npy", None)
    assert (tg.flags >= 2).sum() == 64
    res = crossplay.run(["LiarsDice-v0", "--agents", "m/ego", "DEFAULT", "--n-envs", "16", "-t", "8", "--record", "x.npy",
                         "--out", "x.npz"])
    tx, z = check_file("x.npy", None), np.load("x.npz")
    assert z["table_offsets"].shape == (17,) and z["table_offsets"][-1] == len(tx.flags) == len(z["member"])
    assert np.array_equal(z["pair_of_table"], res.pair_of_table) and (tx.flags >= 2).sum() == res.count.sum()
    # the clone
    clone = bctrainer.run(["LiarsDice-v0", "g.npy", "--total-epochs", "2"])
    assert np.isfinite(clone.policy.get_flat_params()).all() and np.isfinite(clone.last_stats).all()
    # BC fed the device result is BC fed the file
    rec0 = env.recorded(seat=0)
    data = tr.get_ego_transitions()
    n = len(data)
    assert n == len(rec0) > 0
    orders = np.stack([np.random.default_rng(ep).permutation(n) for ep in range(2)])
    clones = []
    for source in (data, rec0):
        bc = BC(osp, asp, policy_kwargs=dict(seed=3))
        if clones:
            bc.policy.set_flat_params(clones[0][1])
        start = bc.policy.get_flat_params()
        bc.set_expert_data_loader(source)
        bc.train(n_epochs=2, orders=orders)
        clones.append((bc.policy.get_flat_params(), start))
    assert np.array_equal(clones[0][1], clones[1][1]) and not np.array_equal(clones[0][0], clones[0][1])
    assert np.array_equal(clones[0][0], clones[1][0])
