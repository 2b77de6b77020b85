"""-m gpu: `policy_kwargs net_arch` towers in the device-resident paths -- the ragged tower forward, the `_arch` forms of the native
self-play steps, the vectorised tower agents, LiarIterationGraph with towers, the one-launch tower rollout
(tower_rollout_kernel) and the trainer's `--n-envs` runs.

Tolerances are the project's own from the header of tests/test_gpu_arch.py (values / log-probs against the checker: 2e-5 * s,
s = max(1, w_last / 64)); none are new.  Everything else -- a native step against its per-call walk, the one-launch rollout against
the per-step calls, gemm_mode 1 / 2 against 0, a captured graph against its body -- is bit-exact."""
import ctypes as C
from collections import deque

import numpy as np
import pytest
import torch as th

from pantheonrl_amd import _native as nat
from tests import arch_oracle as A
from tests import helpers as H
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RB_KEYS = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs")
SENTINEL = -777.0


def _scale(arch):
    return max(1.0, arch[-1] / 64.0)


def _model(env, arch, T, E, seed, **kw):
    """PPO on `env`'s spaces: a tower of `arch`, or the default 64-wide policy when arch is None"""
    from pantheonrl_amd import PPO
    m = PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=E * T // 2, n_epochs=2, seed=seed,
            policy_kwargs=A.kwargs_of(arch) if arch else None, **kw)
    m.device_permutations = True
    return m


def _fill(rb, value=SENTINEL):
    for k in RB_KEYS:
        getattr(rb, k).fill_(value)


def _dev(a, dtype=None):
    t = th.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- 1. ragged forward ---------------------------------------------------------------------------------------------------------
def _ragged_run(name, arch, gemm_mode):
    E, T, calls = 37, 5, 7
    orac = A.oracle_policy(name, arch, seed=4)
    pol = A.device_policy(name, orac)
    obs_s, act_s = H.CONFIGS[name]
    Aa = act_s.stored_len
    rb = H.make_device_buffer(name, pol, T, E)
    _fill(rb)
    lib, h = pol.ctx.lib, pol.ctx.handle
    pol._bind()
    rng = np.random.default_rng(17)
    pos_h = rng.integers(0, T + 1, E).astype(np.int32)
    pos_h[:4] = T                                              # columns that are full from the start
    pos = _dev(pos_h)
    acts, vals, lps = (th.zeros((E, Aa), dtype=th.int32, device=DEV), th.full((E,), SENTINEL, device=DEV),
                       th.zeros(E, device=DEV))
    r_acts, r_vals, r_lps = th.zeros_like(acts), th.zeros_like(vals), th.zeros_like(lps)
    want = {k: np.full(tuple(getattr(rb, k).shape), SENTINEL, np.float32) for k in RB_KEYS}
    want_cache = np.full(E, SENTINEL, np.float32)
    outs = []
    for c in range(1, calls + 1):
        obs_h = H.sample_obs(obs_s, E, rng)
        rec_h = (rng.random(E) < 0.6).astype(np.uint8)
        rec_h[5] = 0
        es_h = (rng.random(E) < 0.3).astype(np.float32)
        obs, rec, es = _dev(obs_h), _dev(rec_h), _dev(es_h)
        nat.check(lib.ph_arch_forward_ragged(h, C.byref(pol.spec), C.byref(pol.arch), pol.params.data_ptr(), obs.data_ptr(), None,
                                             99, c, 0, acts.data_ptr(), vals.data_ptr(), lps.data_ptr(), C.byref(rb.c_struct()),
                                             pos.data_ptr(), rec.data_ptr(), es.data_ptr(), gemm_mode))
        nat.check(lib.ph_arch_forward(h, C.byref(pol.spec), C.byref(pol.arch), pol.params.data_ptr(), obs.data_ptr(), E, None, None,
                                      None, 99, c, 0, r_acts.data_ptr(), None, r_vals.data_ptr(), r_lps.data_ptr(), None, None, None, 0,
                                      None, None, 0))
        a_h, v_h, lp_h = r_acts.cpu().numpy(), r_vals.cpu().numpy(), r_lps.cpu().numpy()
        assert np.array_equal(acts.cpu().numpy(), a_h) and np.array_equal(lps.cpu().numpy(), lp_h), c
        can = rec_h.astype(bool) & (pos_h < T)
        for e in np.nonzero(can)[0]:
            p = pos_h[e]
            want["observations"][p, e] = obs_h[e]
            want["actions"][p, e] = a_h[e].astype(np.float32).reshape(want["actions"][p, e].shape)
            want["rewards"][p, e] = 0.0
            want["episode_starts"][p, e] = es_h[e]
            want["values"][p, e] = v_h[e]
            want["log_probs"][p, e] = lp_h[e]
        want_cache[can] = v_h[can]
        assert np.array_equal(vals.cpu().numpy(), want_cache), c      # the cache moves for recorded tables only
        nat.check(lib.ph_ragged_advance(h, C.byref(rb.c_struct()), pos.data_ptr(), rec.data_ptr()))
        pos_h = pos_h + can.astype(np.int32)
        assert np.array_equal(pos.cpu().numpy(), pos_h)
        outs.append((a_h.copy(), v_h.copy(), lp_h.copy()))
    got = rb.host()
    for k in RB_KEYS:
        assert np.array_equal(got[k], want[k].reshape(got[k].shape)), k
    assert (want["values"] == SENTINEL).any() and (want["values"] != SENTINEL).any()
    return got, outs, vals.cpu().numpy()


@pytest.mark.parametrize("name,arch", [("liar", (256, 128)), ("rps", (32,))])
def test_ragged_tower_forward_writes_exactly_the_recorded_rows(name, arch):
    base = _ragged_run(name, arch, 0)
    for mode in (1, 2):
        got, outs, cache = _ragged_run(name, arch, mode)
        for k in RB_KEYS:
            assert np.array_equal(got[k], base[0][k]), (mode, k)
        assert np.array_equal(cache, base[2])
        for x, y in zip(outs, base[1]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), mode


# ---- 2. / 3. Liar's Dice ---------------------------------------------------------------------------------------------------------
def _liar_selfplay(E, T_ego, T_alt, ego_arch, alt_arch, seed=0, native=True):
    """-> (self-play, ego, alt, the partner's forwards of the walk); a seat's arch None: the default 64-wide policy"""
    calls, spaces = [], LC.spaces()
    sp, ego, alt = LC.selfplay(E, _model(spaces, ego_arch, T_ego, E, seed), _model(spaces, alt_arch, T_alt, E, seed + 1), seed=seed,
                               native=native, calls=calls)
    return sp, ego, alt, calls


def _liar_state(sp, ego, alt, **more):
    return dict(LC.train_state(sp, ego), **more)


@pytest.mark.parametrize("ego_arch,alt_arch", [((128, 128), (32,)), ((96, 160, 32), None), (None, (256, 128))],
                         ids=["128x128-32", "96x160x32-default", "default-256x128"])
def test_liar_native_arch_step_is_bitwise_the_per_call_walk(ego_arch, alt_arch):
    from pantheonrl_amd.envs.vec import TowerRaggedVecOnPolicyAgent
    from pantheonrl_amd.vec import TowerVecOnPolicyAgent
    E, T_ego, T_alt = 48, 8, 6
    runs = []
    for native in (True, False):
        sp, ego, alt, _ = _liar_selfplay(E, T_ego, T_alt, ego_arch, alt_arch, seed=11, native=native)
        assert isinstance(ego, TowerVecOnPolicyAgent) == (ego_arch is not None)
        assert isinstance(alt, TowerRaggedVecOnPolicyAgent) == (alt_arch is not None)
        assert sp.persistent is False
        alt.model.rollout_buffer.gae_mode = ego.model.rollout_buffer.gae_mode = 1
        trained = LC.train_steps(sp, 3 * T_ego)[0]
        runs.append(_liar_state(sp, ego, alt, trained=trained))
    a, b = runs
    assert a["trained"] >= 1 and a["ego_it"] >= 2 and a["episodes"] > E
    LC.same_state(a, b)


def test_liar_arch_step_with_two_null_arches_is_the_plain_step():
    """the driver's own call -- always ph_liar_selfplay_step_arch, (NULL, NULL) without a tower -- against a run that steps
    through ph_liar_selfplay_step itself"""
    E, T_ego, T_alt = 48, 8, 6
    runs = []
    for through_arch in (False, True):
        sp, ego, alt, _ = _liar_selfplay(E, T_ego, T_alt, None, None, seed=3)
        assert not sp.towers and sp._archs == (None, None)
        if not through_arch:
            LC.step_through_the_plain_entry_point(sp)
        alt.model.rollout_buffer.gae_mode = ego.model.rollout_buffer.gae_mode = 1
        trained = LC.train_steps(sp, 2 * T_ego)[0]
        runs.append(_liar_state(sp, ego, alt, trained=trained))
    LC.same_state(*runs)


def test_liar_walk_with_towers_matches_the_python_step_loop():
    """Every table of the device self-play with towers in both seats is replayed through the Python MultiAgentEnv step loop (same
    dice, same first mover, same sampled moves): both seats' recorded transitions are identical, row by row."""
    from pantheonrl_amd.common import Agent, Observation
    from pantheonrl_amd.envs.liar import LiarEnv

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
        def __init__(self):
            self.moves, self.rows, self.last_done = deque(), [], True

        def get_action(self, obs, record=True):
            act = self.moves.popleft()
            self.rows.append(dict(obs=np.asarray(obs.obs, np.float32), act=act, rew=0.0, start=float(self.last_done)))
            return act

        def update(self, reward, done):
            self.rows[-1]["rew"] += float(reward)
            self.last_done = bool(done)

    E, T, steps = 24, 20, 20
    sp, ego, alt, calls = _liar_selfplay(E, T, 64, (128, 128), (32,), native=False)
    shadows, partners = [Shadow() for _ in range(E)], [Replay() for _ in range(E)]
    for s, p in zip(shadows, partners):
        s.add_partner_agent(p)

    def feed(reset_mask):
        hands, first = sp.env.hands.cpu().numpy(), sp.ego_first.cpu().numpy()
        for acts, mask in calls:
            for e in np.nonzero(mask)[0]:
                partners[e].moves.append(acts[e].copy())
        calls.clear()
        for e in np.nonzero(reset_mask)[0]:
            shadows[e].deals.append((first[e], hands[e].copy()))

    feed(np.ones(E, bool))
    cur = [s.reset() for s in shadows]
    ego_rows, n_games = [], 0
    for t in range(steps):
        before = sp.obs_ego.cpu().numpy().copy()
        done = sp.step().cpu().numpy().astype(bool)
        a_ego = ego.actions.cpu().numpy().copy()
        feed(done)
        after = sp.obs_ego.cpu().numpy()
        for e in range(E):
            assert np.array_equal(before[e], np.asarray(cur[e], np.float32)), (t, e)
            o, r, d, _ = shadows[e].step(a_ego[e])
            assert bool(d) == bool(done[e]), (t, e)
            ego_rows.append((t, e, float(r), bool(d)))
            if d:
                n_games += 1
                o = shadows[e].reset()
            cur[e] = o
            assert np.array_equal(after[e], np.asarray(o, np.float32)), (t, e)
            assert not partners[e].moves
    assert n_games == sp.episodes and n_games > E
    th.cuda.synchronize()
    be, ba = ego.model.rollout_buffer.host(), alt.model.rollout_buffer.host()
    for t, e, r, d in ego_rows:
        assert be["rewards"][t, e] == r
        if t + 1 < T:
            assert be["episode_starts"][t + 1, e] == float(d)
    pos = alt.pos.cpu().numpy()
    term, opened = alt.term.cpu().numpy(), alt.open.cpu().numpy()
    assert pos.min() >= 1 and len(set(pos.tolist())) > 1
    for e in range(E):
        rows = partners[e].rows
        assert pos[e] == len(rows)
        for k, row in enumerate(rows):
            assert np.array_equal(ba["observations"][k, e], row["obs"]), (e, k)
            assert np.array_equal(ba["actions"][k, e], row["act"].astype(np.float32))
            assert ba["rewards"][k, e] == row["rew"] and ba["episode_starts"][k, e] == row["start"], (e, k)
            assert np.isfinite(ba["values"][k, e]) and ba["log_probs"][k, e] < 0
        assert opened[e] == 1 and bool(term[e]) == partners[e].last_done


# ---- 4. block worlds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tower_seat", ["ego", "alt"])
@pytest.mark.parametrize("variant", [0, 1])
def test_block_native_arch_step_is_bitwise_the_per_call_walk(variant, tower_seat):
    from pantheonrl_amd.envs.vec import VecBlockSelfPlay, VecBlockWorld, ragged_agent_for
    from pantheonrl_amd.vec import vec_agent_for
    E, T_ego, T_alt = 48, 8, 6
    ego_arch, alt_arch = ((128, 128), None) if tower_seat == "ego" else (None, (96, 160, 32))
    runs = []
    for native in (True, False):
        planner, constructor = VecBlockWorld.seat_spaces(variant)
        ego = vec_agent_for(_model(planner, ego_arch, T_ego, E, 11))
        alt = ragged_agent_for(_model(constructor, alt_arch, T_alt, E, 12))
        sp = VecBlockSelfPlay(variant, E, ego, alt, seed=18, native=native)
        assert sp.towers
        alt.model.rollout_buffer.gae_mode = ego.model.rollout_buffer.gae_mode = 1
        trained = LC.train_steps(sp, 3 * T_ego, [alt])[0]
        be, ba, pos = ego.model.rollout_buffer.host(), alt.model.rollout_buffer.host(), alt.pos.cpu().numpy()
        runs.append(dict(state=sp.env.state.cpu().numpy(), obs=sp.obs_ego.cpu().numpy(), obs_alt=sp.obs_alt.cpu().numpy(),
                         pos=pos, flags=np.stack([t.cpu().numpy() for t in (alt.boundary, alt.term, alt.open)]),
                         acted=sp.alt_acted.cpu().numpy(), episodes=sp.episodes, trained=trained, ego_it=ego.iteration,
                         pe=ego.model.policy.get_flat_params(), pa=alt.model.policy.get_flat_params(),
                         **{"e_" + k: v for k, v in be.items() if k in ("observations", "actions", "rewards", "episode_starts")},
                         **{"a_" + k: LC.recorded_rows(v, pos) for k, v in ba.items()}))
    a, b = runs
    assert a["trained"] >= 1 and a["ego_it"] >= 2
    LC.same_state(a, b)


# ---- 5. LiarIterationGraph ---------------------------------------------------------------------------------------------------------
def test_liar_iteration_graph_with_towers_replays_its_body_bitwise():
    from pantheonrl_amd.envs.vec import LiarIterationGraph
    E, T_ego, T_alt = 48, 8, 6
    runs = []
    for capture in (True, False):
        sp, ego, alt, _ = _liar_selfplay(E, T_ego, T_alt, (128, 128), (32,), seed=5)
        assert sp.persistent is False
        g = LiarIterationGraph(sp, T_ego, capture=capture)
        assert (g.graph_id is not None) == capture and not g.split
        snaps = []
        for _ in range(4):
            g.launch()
            snaps.append(ego.model.rollout_buffer.host()["actions"].copy())
        th.cuda.synchronize()
        runs.append(dict(hands=sp.env.hands.cpu().numpy(), hist=sp.env.history.cpu().numpy(), obs=sp.obs_ego.cpu().numpy(),
                         pos=alt.pos.cpu().numpy(), episodes=sp.episodes, alt_it=alt.iteration, ego_it=ego.iteration,
                         steps=sp.steps_done, pe=ego.model.policy.get_flat_params(), pa=alt.model.policy.get_flat_params(),
                         snaps=np.stack(snaps), epoch=int(g.epoch_word.item())))
    a, b = runs
    assert a["ego_it"] == 6 and a["alt_it"] >= 1 and a["episodes"] > E and a["epoch"] == 6 and a["steps"] == 6 * T_ego
    assert not np.array_equal(a["snaps"][0], a["snaps"][1])           # a replay draws fresh random numbers
    for key in a:
        assert np.array_equal(a[key], b[key]), key


# ---- 6. / 7. the one-launch tower rollout ------------------------------------------------------------------------------------------
ROLLOUT_CASES = [("overcooked", (128, 128)), ("liar", (256, 256, 256)), ("rps", (32,))]


def _tower_agent(name, arch, T, E, orac, gemm_mode=0):
    from pantheonrl_amd.vec import TowerVecOnPolicyAgent
    model = _model(A.space_env(name), arch, T, E, seed=2)
    model.policy.set_flat_params(orac.flat_params())
    model.policy.gemm_mode = gemm_mode
    return TowerVecOnPolicyAgent(model)


def _agent_state(agent):
    th.cuda.synchronize()
    rb = agent.model.rollout_buffer.host()
    out = {k: rb[k] for k in RB_KEYS}
    out.update(actions_out=agent.actions.cpu().numpy(), values_out=agent.values.cpu().numpy(),
               log_probs_out=agent.log_probs.cpu().numpy(), last_starts=agent._last_episode_starts.cpu().numpy(),
               counter=agent.model.policy._counter, pos=agent.model.rollout_buffer.pos, n_steps=agent.n_steps)
    return out


@pytest.fixture(scope="module")
def rollouts():
    """(spec, arch, n) -> (checker, data, state after the per-step calls, state after rollout_scripted), computed once"""
    from pantheonrl_amd.vec import SyntheticRollouts
    T, out = 6, {}
    for name, arch in ROLLOUT_CASES:
        orac = A.oracle_policy(name, arch, seed=9)
        for n in (37, 64):
            walk = _tower_agent(name, arch, T, n, orac)
            data = SyntheticRollouts(walk.model.observation_space, n, T, horizon=3, seed=n, device=walk.model.device)
            data.rewards[T - 1, :5] = -0.0                      # a plain store of the last reward would leave -0.0 in its row
            data.rewards[2, :5] = -0.0
            walk.bind_stream()
            for t in range(T):
                walk.get_action(data.obs[t])
                walk.update(data.rewards[t], data.dones[t])
            walk.flush_rewards()
            one = _tower_agent(name, arch, T, n, orac)
            one.bind_stream()
            one.rollout_scripted(data)
            out[(name, arch, n)] = (orac, data, _agent_state(walk), _agent_state(one))
    return out


@pytest.mark.parametrize("n", [37, 64])
@pytest.mark.parametrize("name,arch", ROLLOUT_CASES, ids=[c[0] for c in ROLLOUT_CASES])
def test_scripted_tower_rollout_is_bitwise_the_per_step_calls(rollouts, name, arch, n):
    orac, data, walk, one = rollouts[(name, arch, n)]
    assert walk["pos"] == one["pos"] == data.T and walk["n_steps"] == one["n_steps"] == data.T
    for k in walk:
        assert np.array_equal(walk[k], one[k]), k
    assert not np.signbit(one["rewards"][data.T - 1, :5]).any() and not np.signbit(one["rewards"][2, :5]).any()
    for mode in (1, 2):
        other = _tower_agent(name, arch, data.T, n, orac, gemm_mode=mode)
        other.bind_stream()
        other.rollout_scripted(data)
        got = _agent_state(other)
        for k in one:
            assert np.array_equal(got[k], one[k]), (mode, k)


@pytest.mark.parametrize("name,arch", ROLLOUT_CASES, ids=[c[0] for c in ROLLOUT_CASES])
def test_scripted_tower_rollout_stays_close_to_the_checker(rollouts, name, arch):
    """teacher-forced by the recorded action, so no row sits on a CDF edge: none is excluded"""
    s = _scale(arch)
    for n in (37, 64):
        orac, data, _, one = rollouts[(name, arch, n)]
        obs = data.obs.cpu().numpy()
        for t in range(data.T):
            with th.no_grad():
                v_ref, lp_ref, _ = orac.evaluate_actions(th.as_tensor(obs[t]), th.as_tensor(one["actions"][t].reshape(n, -1)))
            dv = np.abs(one["values"][t] - v_ref.numpy().reshape(-1)).max()
            dl = np.abs(one["log_probs"][t] - lp_ref.numpy().reshape(-1)).max()
            print(name, arch, n, t, "values", dv, "log_probs", dl, "bound", 2e-5 * s)
            assert dv <= 2e-5 * s and dl <= 2e-5 * s, (n, t, dv, dl)


def test_scripted_tower_rollout_through_ctypes_touches_its_rows_only():
    from pantheonrl_amd.vec import SyntheticRollouts
    name, arch, n, T, pos0, steps = "liar", (256, 128), 37, 6, 2, 4
    orac = A.oracle_policy(name, arch, seed=1)
    pol = A.device_policy(name, orac)
    obs_s, act_s = H.CONFIGS[name]
    data = SyntheticRollouts(H.to_space(obs_s), n, steps, horizon=3, seed=5, device=pol.device)
    lib, h = pol.ctx.lib, pol.ctx.handle
    pol._bind()
    es0 = _dev((np.arange(n) % 3 == 0).astype(np.float32))
    states = []
    for one_launch in (True, False):
        rb = H.make_device_buffer(name, pol, T, n)
        _fill(rb)
        acts = th.zeros((n, act_s.stored_len), dtype=th.int32, device=DEV)
        vals, lps = th.zeros(n, device=DEV), th.zeros(n, device=DEV)
        spec, ar, rbc = C.byref(pol.spec), C.byref(pol.arch), C.byref(rb.c_struct())
        if one_launch:
            nat.check(lib.ph_arch_scripted_rollout(h, spec, ar, pol.params.data_ptr(), data.obs.data_ptr(), data.rewards.data_ptr(),
                                                   data.dones.data_ptr(), n, steps, es0.data_ptr(), 7, 100, acts.data_ptr(),
                                                   vals.data_ptr(), lps.data_ptr(), rbc, pos0, 0))
        else:
            for t in range(steps):
                nat.check(lib.ph_arch_forward(h, spec, ar, pol.params.data_ptr(), data.obs[t].data_ptr(), n, None, None, None, 7,
                                              100 + t, 0, acts.data_ptr(), None, vals.data_ptr(), lps.data_ptr(), None, None, rbc,
                                              pos0 + t, (data.dones[t - 1] if t else es0).data_ptr(),
                                              data.rewards[t - 1].data_ptr() if t else None, 0))
            nat.check(lib.ph_buffer_add_reward(h, rbc, pos0 + steps - 1, data.rewards[steps - 1].data_ptr(), None))
        th.cuda.synchronize()
        got = rb.host()
        states.append(dict({k: got[k] for k in RB_KEYS}, a=acts.cpu().numpy(), v=vals.cpu().numpy(), lp=lps.cpu().numpy()))
    one, walk = states
    for k in one:
        assert np.array_equal(one[k], walk[k]), k
    for k in RB_KEYS:
        assert (one[k][:pos0] == SENTINEL).all() and (one[k][pos0 + steps:] == SENTINEL).all(), k
        assert (one[k][pos0:pos0 + steps] != SENTINEL).any(), k


# ---- 8. trainer --------------------------------------------------------------------------------------------------------------------
TOWER = '"policy_kwargs": {"net_arch": [{"pi": [128, 128], "vf": [128, 128]}]}'
SMALL = '"policy_kwargs": {"net_arch": [{"pi": [32], "vf": [32]}]}'


@pytest.mark.parametrize("game,ego_extra,alt_extra", [("LiarsDice-v0", TOWER, None), ("LiarsDice-v0", TOWER, SMALL),
                                                      ("BlockEnv-v0", TOWER, SMALL), ("RPS-v0", TOWER, SMALL)],
                         ids=["liar-ego-tower", "liar-both-towers", "block-v0", "rps"])
def test_trainer_n_envs_runs_towers_on_the_device_paths(game, ego_extra, alt_extra, tmp_path):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.ppo import ActorCriticPolicy, ArchActorCriticPolicy
    from pantheonrl_amd.trainer import run
    alt_steps = 16 if game == "RPS-v0" else 8
    ego_steps = 16 if game == "RPS-v0" else 8
    cfg = lambda steps, extra: '{"n_steps": %d, "n_epochs": 2%s}' % (steps, ", " + extra if extra else "")  # noqa: E731
    ego, partners, env = run([game, "PPO", "PPO", "--n-envs", "32", "-t", str(4 * 32 * ego_steps), "--seed", "1",
                              "--ego-config", cfg(ego_steps, ego_extra), "--alt-config", cfg(alt_steps, alt_extra),
                              "--ego-save", str(tmp_path / "ego"), "--alt-save", str(tmp_path / "alt")])
    alt = partners[0]
    assert type(ego.policy) is ArchActorCriticPolicy and ego.policy.net_arch == (128, 128)
    assert type(alt.model.policy) is (ArchActorCriticPolicy if alt_extra else ActorCriticPolicy)
    assert alt.iteration >= 1
    # four iterations x 2 epochs x 4 minibatches (batch_size defaults to E * n_steps / 4), counted on the device: the Liar's Dice
    # run replays its last two iterations from LiarIterationGraph
    assert int(ego.policy.opt_step.item()) == 4 * 2 * 4
    for m in (ego, alt.model):
        assert np.isfinite(m.policy.get_flat_params()).all()
    if game == "LiarsDice-v0":
        assert env.persistent is False and env.towers
    for path, m in ((tmp_path / "ego", ego), (tmp_path / "alt", alt.model)):
        again = PPO.load(str(path))
        assert type(again.policy) is type(m.policy)
        assert np.array_equal(again.policy.get_flat_params(), m.policy.get_flat_params())


# ---- 9. refusals and misuse ----------------------------------------------------------------------------------------------------
def test_paths_built_around_the_64_wide_blocks_still_refuse_towers():
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import (RaggedVecOnPolicyAgent, TowerRaggedVecOnPolicyAgent, VecLiarPartnerPool, VecLiarsDice,
                                         ragged_agent_for)
    from pantheonrl_amd.vec import FusedSelfPlayRollout, SyntheticRollouts, TowerVecOnPolicyAgent, VecOnPolicyAgent, vec_agent_for
    E, T = 16, 8
    spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                                _is_dummy_space_env=True))()
    tower_ego, plain_ego = vec_agent_for(_model(spaces, (128, 128), T, E, 0)), vec_agent_for(_model(spaces, None, T, E, 0))
    tower_alt, plain_alt = ragged_agent_for(_model(spaces, (32,), T, E, 1)), ragged_agent_for(_model(spaces, None, T, E, 1))
    assert type(tower_ego) is TowerVecOnPolicyAgent and type(plain_ego) is VecOnPolicyAgent
    assert type(tower_alt) is TowerRaggedVecOnPolicyAgent and type(plain_alt) is RaggedVecOnPolicyAgent
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        VecLiarPartnerPool(E, tower_ego, [plain_alt])
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        VecLiarPartnerPool(E, plain_ego, [plain_alt, tower_alt])
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        VecOnPolicyAgent(tower_ego.model)
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        RaggedVecOnPolicyAgent(tower_alt.model)
    with pytest.raises(nat.NativeError, match="tower"):
        TowerVecOnPolicyAgent(plain_ego.model)
    data = SyntheticRollouts(spaces.observation_space, E, T, horizon=4, seed=0, device=tower_ego.model.device)
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        FusedSelfPlayRollout([tower_ego], [data], None, th.cuda.current_stream())
    with pytest.raises(nat.NativeError, match="fused MLP kernels"):
        PPO.train_joint([tower_ego.model, plain_ego.model])
    with pytest.raises(nat.NativeError, match="64-wide"):
        tower_ego.model.policy.forward_and_store_host(np.zeros((E, 30), np.float32), tower_ego.model.rollout_buffer, None)


def test_a_carve_above_the_lds_is_refused_when_the_agent_is_built():
    from pantheonrl_amd import spaces as sp
    from pantheonrl_amd.envs.vec import TowerRaggedVecOnPolicyAgent
    from pantheonrl_amd.vec import TowerVecOnPolicyAgent
    env = type("S", (), dict(observation_space=sp.MultiDiscrete([2] * 256), action_space=sp.Discrete(3), _is_dummy_space_env=True))()
    model = _model(env, (256, 256, 256), 4, 8, 0)
    with pytest.raises(nat.NativeError, match="LDS tile"):
        TowerVecOnPolicyAgent(model)
    with pytest.raises(nat.NativeError, match="LDS tile"):
        TowerRaggedVecOnPolicyAgent(model)
    pol = model.policy
    rb = model.rollout_buffer
    z = th.zeros(8 * 256, device=DEV)
    pol._bind()
    rc = pol.ctx.lib.ph_arch_scripted_rollout(pol.ctx.handle, C.byref(pol.spec), C.byref(pol.arch), pol.params.data_ptr(), z.data_ptr(),
                                              z.data_ptr(), z.data_ptr(), 8, 1, z.data_ptr(), 0, 0, None, None, None,
                                              C.byref(rb.c_struct()), 0, 0)
    assert rc != 0 and b"LDS tile" in pol.ctx.lib.ph_last_error()


def test_misuse_of_the_new_entry_points_returns_an_error_text():
    name, arch, n, T = "liar", (128, 128), 8, 4
    orac = A.oracle_policy(name, arch, seed=1)
    pol = A.device_policy(name, orac)
    lib, h = pol.ctx.lib, pol.ctx.handle
    pol._bind()
    rb = H.make_device_buffer(name, pol, T, n)
    spec, ar, rbc = C.byref(pol.spec), C.byref(pol.arch), C.byref(rb.c_struct())
    z = th.zeros(T * n * 30, device=DEV)
    zi = th.zeros(n, dtype=th.int32, device=DEV)
    zb = th.zeros(n, dtype=th.uint8, device=DEV)
    P, Z = pol.params.data_ptr(), z.data_ptr()

    def refused(rc, text):
        msg = lib.ph_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)

    # ph_arch_forward_ragged
    refused(lib.ph_arch_forward_ragged(h, spec, ar, P, Z, None, 0, 0, 0, None, None, None, rbc, None, zb.data_ptr(), Z, 0), "null argument")
    refused(lib.ph_arch_forward_ragged(h, spec, ar, P, Z, None, 0, 0, 0, None, None, None, None, zi.data_ptr(), zb.data_ptr(), Z, 0),
            "null rollout buffer")
    refused(lib.ph_arch_forward_ragged(h, spec, None, P, Z, None, 0, 0, 0, None, None, None, rbc, zi.data_ptr(), zb.data_ptr(), Z, 0),
            "null arch")
    refused(lib.ph_arch_forward_ragged(None, spec, ar, P, Z, None, 0, 0, 0, None, None, None, rbc, zi.data_ptr(), zb.data_ptr(), Z, 0),
            "null ctx")
    # ph_arch_scripted_rollout
    refused(lib.ph_arch_scripted_rollout(h, spec, ar, P, Z, Z, None, n, T, Z, 0, 0, None, None, None, rbc, 0, 0), "null argument")
    refused(lib.ph_arch_scripted_rollout(h, spec, ar, P, Z, Z, Z, n + 1, T, Z, 0, 0, None, None, None, rbc, 0, 0), "must equal")
    refused(lib.ph_arch_scripted_rollout(h, spec, ar, P, Z, Z, Z, n, T, Z, 0, 0, None, None, None, rbc, 1, 0), "must lie in the buffer")
    refused(lib.ph_arch_scripted_rollout(h, spec, ar, P, Z, Z, Z, n, T + 1, Z, 0, 0, None, None, None, rbc, 0, 0), "must lie in the buffer")
    refused(lib.ph_arch_scripted_rollout(h, spec, ar, P, Z, Z, Z, n, 0, Z, 0, 0, None, None, None, rbc, 0, 0), "must be positive")
    refused(lib.ph_arch_scripted_rollout(h, spec, None, P, Z, Z, Z, n, T, Z, 0, 0, None, None, None, rbc, 0, 0), "null arch")
    # the step calls
    refused(lib.ph_liar_selfplay_step_arch(h, None, ar, ar, 0, 1, 0), "ph_liar_selfplay_step_arch: null argument")
    refused(lib.ph_block_selfplay_step_arch(h, None, ar, ar, 0, 1), "ph_block_selfplay_step_arch: null argument")
    empty_l, empty_b = nat.PhLiarSelfPlay(), nat.PhBlockSelfPlay()
    refused(lib.ph_liar_selfplay_step_arch(h, C.byref(empty_l), ar, None, 0, 1, 0), "incomplete description")
    refused(lib.ph_block_selfplay_step_arch(h, C.byref(empty_b), None, ar, 0, 1), "n must be positive")
    # the process lives, and the context still works
    assert np.isfinite(pol.get_logits(np.zeros((3, 30), np.float32)).cpu().numpy()).all()
