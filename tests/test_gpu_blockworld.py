"""gpu: BlockEnv-v0 / BlockEnv-v1 on the device -- the per-call kernels against the reference's traces
(tests/golden/blockworld_ref.npz), the vectorised self-play against the Python MultiAgentEnv step loop, the one-call native
step against the per-call walk, the trainer.  Every comparison is exact."""
import ctypes as C
import os
from collections import deque

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from pantheonrl_amd.envs import blockworld as bw

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "blockworld_ref.npz"))
DEV = "cuda:0"


def _world(variant, n):
    from pantheonrl_amd.envs.vec import VecBlockWorld
    return VecBlockWorld(variant, n, nat.Context(0), th.device(DEV))


@pytest.mark.parametrize("variant", [0, 1])
def test_device_kernels_replay_the_reference_traces(variant):
    """ph_block_step / ph_block_obs on the fixture's 256 tables, every second table masked out of every call: the active tables
    reproduce the reference bit for bit, the others -- state and output rows -- stay untouched"""
    k = f"v{variant}_"
    n, rounds = Z[k + "tokens"].shape
    env = _world(variant, n)
    state0 = np.stack([bw.pack_state(variant, w) for w in Z[k + "world"]])
    env.load(state0)
    active = th.as_tensor((np.arange(n) % 2 == 0).astype(np.uint8)).to(DEV)
    on = active.cpu().numpy().astype(bool)
    env.obs_next_alt.fill_(-7.0)
    env.obs_next_ego.fill_(-7.0)
    env.rewards.fill_(-7.0)
    probe_e = th.full((n, env.D_ego), -7.0, device=DEV)
    probe_a = th.full((n, env.D_alt), -7.0, device=DEV)
    for r in range(rounds):
        tok = th.as_tensor(Z[k + "tokens"][:, r].astype(np.int32)).to(DEV)
        o, rew, done = env.player_step(tok, True, active)
        assert np.array_equal(o.cpu().numpy()[on], Z[k + "alt_obs"][on, r].astype(np.float32)), r
        assert np.array_equal(rew.cpu().numpy()[on], Z[k + "rew"][on, r]) and np.array_equal(done.cpu().numpy()[on], Z[k + "done"][on, r])
        assert np.array_equal(env.observe(False, probe_a, active).cpu().numpy()[on], Z[k + "alt_obs"][on, r].astype(np.float32))
        act = th.as_tensor(np.ascontiguousarray(Z[k + "acts"][:, r].astype(np.int32))).to(DEV)
        o, rew, done = env.player_step(act, False, active)
        assert np.array_equal(o.cpu().numpy()[on], Z[k + "ego_obs"][on, r].astype(np.float32)), r
        assert not rew.cpu().numpy()[on].any() and not done.cpu().numpy()[on].any()
        assert np.array_equal(env.observe(True, probe_e, active).cpu().numpy()[on], Z[k + "ego_obs"][on, r].astype(np.float32))
    assert np.array_equal(env.state.cpu().numpy()[~on], state0[~on])
    for t in (env.obs_next_alt, env.obs_next_ego, env.rewards, probe_e, probe_a):
        assert (t.cpu().numpy()[~on] == -7.0).all()
    # all tables in one call (no mask) from the start: the whole file
    env.load(state0)
    for r in range(rounds):
        o, rew, done = env.player_step(th.as_tensor(Z[k + "tokens"][:, r].astype(np.int32)).to(DEV), True)
        assert np.array_equal(o.cpu().numpy(), Z[k + "alt_obs"][:, r].astype(np.float32))
        assert np.array_equal(rew.cpu().numpy(), Z[k + "rew"][:, r]) and np.array_equal(done.cpu().numpy(), Z[k + "done"][:, r])
        o, _, _ = env.player_step(th.as_tensor(np.ascontiguousarray(Z[k + "acts"][:, r].astype(np.int32))).to(DEV), False)
        assert np.array_equal(o.cpu().numpy(), Z[k + "ego_obs"][:, r].astype(np.float32))


@pytest.mark.parametrize("variant", [0, 1])
def test_device_reset_gives_the_worlds_of_the_host_replay(variant):
    env = _world(variant, 300)
    for seed, counter in ((5, 0), (5, 9), (2 ** 40 + 3, 2 ** 33 + 1)):
        env.state.fill_(-1)
        env.reset(seed, counter)
        want = nat.block_replay_host(variant, n=300, seed=seed, counter=counter)["state"]
        assert np.array_equal(env.state.cpu().numpy(), want)
    mask = th.as_tensor((np.arange(300) % 3 == 0).astype(np.uint8)).to(DEV)
    before = env.state.cpu().numpy().copy()
    env.reset(11, 4, mask)
    after, want = env.state.cpu().numpy(), nat.block_replay_host(variant, n=300, seed=11, counter=4)["state"]
    m = mask.cpu().numpy().astype(bool)
    assert np.array_equal(after[m], want[m]) and np.array_equal(after[~m], before[~m])


def _selfplay(variant, E, T_ego, T_alt, seed=0, native=True):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecBlockSelfPlay, VecBlockWorld
    from pantheonrl_amd.vec import VecOnPolicyAgent
    planner, constructor = VecBlockWorld.seat_spaces(variant)
    me = PPO("MlpPolicy", planner, n_steps=T_ego, n_envs=E, batch_size=E * T_ego // 2, n_epochs=2, seed=seed)
    ma = PPO("MlpPolicy", constructor, n_steps=T_alt, n_envs=E, batch_size=E * T_alt // 2, n_epochs=2, seed=seed + 1)
    me.device_permutations = ma.device_permutations = True
    ego, alt = VecOnPolicyAgent(me), RaggedVecOnPolicyAgent(ma)
    calls = []
    inner = alt.get_action

    def logged(obs, rec_mask):
        acts = inner(obs, rec_mask)
        calls.append((acts.cpu().numpy().copy(), rec_mask.cpu().numpy().astype(bool)))
        return acts
    alt.get_action = logged
    return VecBlockSelfPlay(variant, E, ego, alt, seed=seed + 7, native=native), ego, alt, calls


@pytest.mark.parametrize("variant", [0, 1])
def test_vec_block_selfplay_matches_the_python_step_loop(variant):
    """Every table of the device self-play is shadowed by a host game driven through MultiAgentEnv.step with the device's worlds
    and sampled moves: the planner's and the constructor's recorded transitions are identical, row by row.  An untrained planner
    ends a game with probability 1/30 (1/16) per step, so the run is 150 steps long for several games per table."""
    from pantheonrl_amd.common import Agent, Observation
    game = (bw.SimpleBlockEnv, bw.BlockEnv)[variant]

    class Shadow(game):
        def __init__(self):
            super().__init__()
            self.worlds = deque()

        def n_reset(self):
            world = self.worlds.popleft()
            self.ego_next = True
            if variant:
                self.gridworld, self.constructor_obs = world.astype(float), np.zeros((7, 7))
            else:
                self.gridworld = [[int(v) for v in b] for b in world]
                self.constructor_obs = [[b[0], b[1], b[2], 0] for b in self.gridworld]
            self.last_token = 0
            return (0,), (Observation(self.get_obs(True)),)

    class Replay(Agent):
        """partner that plays the moves the device sampled and keeps OnPolicyAgent's book (agents.py:172-198)"""
        def __init__(self):
            self.moves, self.rows, self.last_done = deque(), [], True

        def get_action(self, obs, record=True):
            act = self.moves.popleft()
            self.rows.append(dict(obs=np.asarray(obs.obs, np.float32), act=act, rew=0.0, start=float(self.last_done)))
            return act

        def update(self, reward, done):
            self.rows[-1]["rew"] += float(reward)
            self.last_done = bool(done)

    E, steps = 24, 150
    sp, ego, alt, calls = _selfplay(variant, E, steps, steps, native=False)
    shadows, partners = [Shadow() for _ in range(E)], [Replay() for _ in range(E)]
    for s, p in zip(shadows, partners):
        s.add_partner_agent(p)

    def feed(reset_mask):
        state = sp.env.state.cpu().numpy()
        for acts, mask in calls:
            for e in np.nonzero(mask)[0]:
                partners[e].moves.append(acts[e].copy())
        calls.clear()
        for e in np.nonzero(reset_mask)[0]:
            world, view, token = bw.unpack_state(variant, state[e])
            assert token == 0 and not np.asarray(view).any()
            shadows[e].worlds.append(world)

    feed(np.ones(E, bool))
    cur = [s.reset() for s in shadows]
    ego_rows, games = [], np.zeros(E, int)
    for t in range(steps):
        before = sp.obs_ego.cpu().numpy().copy()
        done = sp.step().cpu().numpy().astype(bool)
        tokens = ego.actions.cpu().numpy().copy()
        feed(done)
        after = sp.obs_ego.cpu().numpy()
        for e in range(E):
            assert np.array_equal(before[e], np.asarray(cur[e], np.float32)), (t, e)
            o, r, d, _ = shadows[e].step(tokens[e])
            assert bool(d) == bool(done[e]), (t, e)
            ego_rows.append((t, e, np.float32(r), bool(d)))
            if d:
                games[e] += 1
                o = shadows[e].reset()
            cur[e] = o
            assert np.array_equal(after[e], np.asarray(o, np.float32)), (t, e)
            assert not partners[e].moves            # the Python loop consumed exactly the moves the device made
    assert games.sum() == sp.episodes and games.sum() > 2 * E         # several games per table
    th.cuda.synchronize()
    be, ba = ego.model.rollout_buffer.host(), alt.model.rollout_buffer.host()
    for t, e, r, d in ego_rows:
        assert be["rewards"][t, e] == r
        if t + 1 < steps:
            assert be["episode_starts"][t + 1, e] == float(d)
    pos = alt.pos.cpu().numpy()
    term, opened = alt.term.cpu().numpy(), alt.open.cpu().numpy()
    assert pos.min() >= 1 and len(set(pos.tolist())) > 1      # the columns really are ragged
    for e in range(E):
        rows = partners[e].rows
        assert pos[e] == len(rows)
        for i, row in enumerate(rows):
            assert np.array_equal(ba["observations"][i, e], row["obs"]), (e, i)
            assert np.array_equal(ba["actions"][i, e], np.asarray(row["act"], np.float32))
            assert ba["rewards"][i, e] == np.float32(row["rew"]) and ba["episode_starts"][i, e] == row["start"], (e, i)
            assert np.isfinite(ba["values"][i, e]) and ba["log_probs"][i, e] < 0
        assert opened[e] == 1 and bool(term[e]) == partners[e].last_done


@pytest.mark.parametrize("variant", [0, 1])
def test_vec_block_native_step_is_bitwise_the_per_call_step(variant):
    """ph_block_selfplay_step (one engine call per vectorised step, masks on the device) against the per-call / torch-mask walk
    with the same RNG counters: identical game state, observations, both rollout buffers, partner book-keeping and -- after
    both learners have trained -- identical parameters.  The native run steps through ph_block_selfplay_step itself; a third run
    makes the driver's own call, ph_block_selfplay_step_arch(NULL, NULL), and holds the same bits."""
    E, T_ego, T_alt = 48, 8, 6
    runs = []
    for native, plain in ((True, True), (False, False), (True, False)):
        sp, ego, alt, _ = _selfplay(variant, E, T_ego, T_alt, seed=11, native=native)
        if plain:
            def plain_step(counter, ego_pos=-1, sp=sp, rb=ego.model.rollout_buffer):
                sp._bind()
                nat.check(sp.env.ctx.lib.ph_block_selfplay_step(sp.env.ctx.handle, C.byref(sp._desc),
                                                                int(rb.pos if ego_pos < 0 else ego_pos), int(counter)))
            assert sp._archs == (None, None)
            sp._native_call = plain_step
        alt.model.rollout_buffer.gae_mode = ego.model.rollout_buffer.gae_mode = 1
        trained = 0
        for _ in range(3 * T_ego):
            sp.step()
            if alt.full():
                alt.learn_from_buffer()
                trained += 1
        th.cuda.synchronize()
        be, ba = ego.model.rollout_buffer.host(), alt.model.rollout_buffer.host()
        runs.append(dict(state=sp.env.state.cpu().numpy(), obs=sp.obs_ego.cpu().numpy(), obs_alt=sp.obs_alt.cpu().numpy(),
                         pos=alt.pos.cpu().numpy(), flags=np.stack([t.cpu().numpy() for t in (alt.boundary, alt.term, alt.open)]),
                         acted=sp.alt_acted.cpu().numpy(), episodes=sp.episodes, trained=trained, ego_it=ego.iteration,
                         pe=ego.model.policy.get_flat_params(), pa=alt.model.policy.get_flat_params(),
                         **{"e_" + k: v for k, v in be.items() if k in ("observations", "actions", "rewards", "episode_starts")},
                         **{"a_" + k: v for k, v in ba.items()}))
    a = runs[0]
    assert a["trained"] >= 1 and a["ego_it"] >= 2
    pos = a["pos"]
    for b in runs[1:]:
        for key in a:
            x, y = a[key], b[key]
            if key.startswith("a_") and getattr(x, "ndim", 0) >= 2:      # only the recorded rows of the ragged buffer are defined
                rows = np.arange(x.shape[0])[:, None] < pos[None, :]
                x, y = x[rows], y[rows]
            assert np.array_equal(x, y), key


def test_native_step_does_no_host_work_and_captures():
    """after two eager steps have sized the workspaces, four ph_block_selfplay_step calls are captured into a hipGraph (an
    allocation or a synchronisation inside a capture is an error) and the graph replays"""
    sp, ego, alt, _ = _selfplay(1, 32, 8, 8, seed=3)
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
        before = alt.pos.clone()
        nat.check(ctx.lib.ph_graph_launch(ctx.handle, gid.value))
        stream.synchronize()
    th.cuda.synchronize()
    assert int((alt.pos - before).sum().item()) > 0 and np.isfinite(ego.model.rollout_buffer.host()["values"][:6]).all()


@pytest.mark.parametrize("game", ["BlockEnv-v1", "BlockEnv-v0"])
def test_trainer_n_envs_runs_device_selfplay(game, tmp_path):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.trainer import run
    ego, partners, env = run([game, "PPO", "PPO", "--n-envs", "32", "-t", "2048", "--seed", "1",
                              "--ego-config", '{"n_steps": 16, "n_epochs": 2}', "--alt-config", '{"n_steps": 8, "n_epochs": 2}',
                              "--ego-save", str(tmp_path / "ego"), "--alt-save", str(tmp_path / "alt")])
    assert env.ego.iteration == 4 and partners[0].iteration >= 1
    for path, model in (("ego", ego), ("alt", partners[0].model)):
        again = PPO.load(str(tmp_path / path))
        assert np.array_equal(again.policy.get_flat_params(), model.policy.get_flat_params())


def test_trainer_default_partner_runs_on_the_host_stepped_path():
    from pantheonrl_amd.trainer import run
    ego, partners, env = run(["BlockEnv-v0", "PPO", "DEFAULT", "-t", "256", "--seed", "2",
                              "--ego-config", '{"n_steps": 64, "batch_size": 64, "n_epochs": 2}'])
    assert isinstance(partners[0], bw.SBWDefaultAgent) and isinstance(env, bw.SimpleBlockEnv)
    assert ego.num_timesteps >= 256 and np.isfinite(ego.policy.get_flat_params()).all()


def test_abi_misuse_is_reported_not_fatal():
    sp, ego, alt, _ = _selfplay(1, 16, 4, 4, seed=1)
    ctx, lib, h = sp.env.ctx, sp.env.ctx.lib, sp.env.ctx.handle
    st, f, u8 = sp.env.state, sp.env.obs_next_alt, sp.env.done
    tok = th.zeros(16, dtype=th.int32, device=sp.dev)
    assert lib.ph_block_reset(h, 1, None, None, 0, 0, 16) != 0 and b"null" in lib.ph_last_error()
    assert lib.ph_block_reset(h, 2, st.data_ptr(), None, 0, 0, 16) != 0 and b"variant" in lib.ph_last_error()
    assert lib.ph_block_reset(h, 1, st.data_ptr(), None, 0, 0, 0) != 0 and b"positive" in lib.ph_last_error()
    assert lib.ph_block_step(h, -1, st.data_ptr(), tok.data_ptr(), 1, None, f.data_ptr(), sp.env.rewards.data_ptr(), u8.data_ptr(), 16) != 0
    assert b"variant" in lib.ph_last_error()
    assert lib.ph_block_step(h, 1, st.data_ptr(), None, 1, None, f.data_ptr(), sp.env.rewards.data_ptr(), u8.data_ptr(), 16) != 0
    assert lib.ph_block_step(h, 1, st.data_ptr(), tok.data_ptr(), 1, None, f.data_ptr(), sp.env.rewards.data_ptr(), u8.data_ptr(), -3) != 0
    assert lib.ph_block_obs(h, 1, st.data_ptr(), 1, None, None, 16) != 0 and b"null" in lib.ph_last_error()
    assert lib.ph_block_obs(h, 3, st.data_ptr(), 1, None, f.data_ptr(), 16) != 0
    assert lib.ph_block_selfplay_step(h, None, 0, 1) != 0 and b"null" in lib.ph_last_error()
    d = sp._desc
    for field, bad, word in (("variant", 2, b"variant"), ("n", 0, b"positive"), ("n", 8, b"E = n")):
        good = getattr(d, field)
        setattr(d, field, bad)
        assert lib.ph_block_selfplay_step(h, C.byref(d), 0, 1) != 0 and word in lib.ph_last_error(), field
        setattr(d, field, good)
    good = d.state
    d.state = None
    assert lib.ph_block_selfplay_step(h, C.byref(d), 0, 1) != 0 and b"incomplete" in lib.ph_last_error()
    d.state = good
    assert lib.ph_block_selfplay_step(h, C.byref(d), 99, 1) != 0 and b"ego_pos" in lib.ph_last_error()
    # the context and the description are still usable afterwards
    sp.step()
    th.cuda.synchronize()
    assert ego.model.rollout_buffer.pos == 1
