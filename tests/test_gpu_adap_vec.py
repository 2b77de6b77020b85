"""gpu: ADAP learners in the device-resident games (csrc/ph_adap_vec.h / .hip, vec.py: AdapSeat).  The two kernels are held to
ph_adap_vec_host bit for bit (tests/test_adap_vec_host.py holds that to numpy), the engine-side step to the per-call walk, the walk
to the host LiarEnv and the numpy draws, the gradient kernel at the new row shape to the oracle's autograd."""
import ctypes as C
from collections import deque

import numpy as np
import pytest
import torch as th

from oracle import sb3_oracle as orc
from tests import adap_vec_ref as A
from tests import helpers as H
from tests import adap_cases as TA
from tests import liar_cases as LC

pytestmark = pytest.mark.gpu

SENTINEL = -7.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _game_spaces(game):
    from pantheonrl_amd.envs.vec import VecLiarsDice, VecRPS
    g = {"liar": VecLiarsDice, "rps": VecRPS}[game]
    return type("S", (), dict(observation_space=g.observation_space, action_space=g.action_space, _is_dummy_space_env=True))()


def _model(kind, spaces, T, E, seed, sampler="l2", cs=3):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.adap import ADAP, AdapPolicy
    kw = dict(n_steps=T, n_envs=E, batch_size=E * T // 2, n_epochs=2, seed=seed)
    m = (ADAP(AdapPolicy, spaces, context_sampler=sampler, context_size=cs, **kw) if kind == "ADAP"
         else PPO("MlpPolicy", spaces, **kw))
    m.device_permutations = True
    return m


# ---- 1. the two kernels are ph_adap_vec_host ----------------------------------------------------------------------------------------
def _shape_case(name, n, rng):
    from pantheonrl_amd import spaces as sp
    from pantheonrl_amd.envs.vec import VecLiarsDice, VecRPS
    if name == "liar":
        space = VecLiarsDice.observation_space
        nvec = np.asarray(space.nvec)
        obs = (rng.random((n, len(nvec))) * nvec).astype(np.int64).astype(np.float32)
        obs[0, 7], obs[n - 1, 0] = 99.0, -3.0                       # clamped components
    elif name == "rps":
        space, obs = VecRPS.observation_space, np.zeros((n, 1), np.float32)
    else:
        space, obs = sp.Box(-np.inf, np.inf, (6,)), rng.standard_normal((n, 6)).astype(np.float32)
    return space, obs


@pytest.mark.parametrize("n", [1, 17, 257])
@pytest.mark.parametrize("shape", ["liar", "rps", "box6"])
def test_row_kernel_is_bitwise_the_host_statement(shape, n):
    from pantheonrl_amd import _native as nat
    rng = np.random.default_rng(n)
    cs = 3
    space, obs = _shape_case(shape, n, rng)
    env = nat.env_space_of(space)
    ctxs = A.draw_contexts("l2", cs, 5, 2, np.arange(n))
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream().cuda_stream)
    for active in (None, (rng.random(n) < 0.5).astype(np.uint8)):
        W = {"liar": 270, "rps": 1, "box6": 6}[shape] + cs
        _, want = nat.adap_vec_host(cs, n, contexts=ctxs, env_space=env, obs=obs, active=active, rows=np.full((n, W), SENTINEL, np.float32))
        rows = th.full((n + 1, W), SENTINEL, dtype=th.float32, device="cuda")     # one row past the end: nothing is written there
        a = None if active is None else th.as_tensor(active).cuda()
        obs_d, ctxs_d = th.as_tensor(obs).cuda(), th.as_tensor(ctxs).cuda()
        nat.check(ctx.lib.ph_adap_rows(ctx.handle, C.byref(env), cs, obs_d.data_ptr(), ctxs_d.data_ptr(), nat.ptr(a), rows.data_ptr(), n))
        th.cuda.synchronize()
        got = rows.cpu().numpy()
        assert np.array_equal(bits(got[:n]), bits(want)) and np.all(got[n] == SENTINEL)
        if active is not None and n > 1:
            assert np.all(got[:n][active == 0] == SENTINEL)


@pytest.mark.parametrize("n", [1, 17, 257])
@pytest.mark.parametrize("sampler,cs", [("l2", 3), ("unit_square", 4), ("positive_square", 3), ("categorical", 4), ("natural_numbers", 1)])
def test_draw_kernel_is_bitwise_the_host_statement(sampler, cs, n):
    from pantheonrl_amd import _native as nat
    rng = np.random.default_rng(n + cs)
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream().cuda_stream)
    seed = 0x5EED1234ABCD
    for counter in (0, 9, 2 ** 33 + 1):
        for flags in (None, (rng.random(n) < 0.5).astype(np.uint8)):
            before = np.full((n, cs), SENTINEL, np.float32)
            want, _ = nat.adap_vec_host(cs, n, sampler=sampler, seed=seed, counter=counter, redraw=flags, contexts=before)
            dev = th.full((n + 1, cs), SENTINEL, dtype=th.float32, device="cuda")
            f = None if flags is None else th.as_tensor(flags).cuda()
            nat.check(ctx.lib.ph_adap_context_draw(ctx.handle, nat.CONTEXT_SAMPLERS[sampler], cs, seed, counter, nat.ptr(f),
                                                   dev.data_ptr(), n))
            th.cuda.synchronize()
            got = dev.cpu().numpy()
            assert np.array_equal(bits(got[:n]), bits(want)) and np.all(got[n] == SENTINEL), (sampler, counter)
            if flags is not None:
                assert np.all(got[:n][flags == 0] == SENTINEL)
    with pytest.raises(nat.NativeError, match="context_size"):
        nat.check(ctx.lib.ph_adap_context_draw(ctx.handle, 0, 65, seed, 0, None, dev.data_ptr(), n))


# ---- 2. the engine-side step is the walk ----------------------------------------------------------------------------------------------
def _adap_selfplay(E, T_ego, T_alt, kinds, share=False, seed=0, native=True, sampler="l2", calls=None):
    """calls: a list that collects the partner's forwards of the walk -- (moves, mask, the contexts it read) -- the first deal's too"""
    spaces = _game_spaces("liar")
    return LC.selfplay(E, _model(kinds[0], spaces, T_ego, E, seed, sampler), _model(kinds[1], spaces, T_alt, E, seed + 1, sampler),
                       seed=seed, native=native, calls=calls, latent_syncer=share)


def _contexts_of(sp, ego, alt):
    more = dict(obs_alt_plane=sp.obs_alt.cpu().numpy())
    for name, agent in (("ego", ego), ("alt", alt)):
        if hasattr(agent, "contexts"):
            more["ctx_" + name] = agent.contexts.cpu().numpy()
    return more


@pytest.mark.parametrize("kinds,share", [(("ADAP", "ADAP"), False), (("ADAP", "ADAP"), True), (("ADAP", "PPO"), False),
                                         (("PPO", "ADAP"), False)], ids=["adap-adap", "shared-latent", "adap-ppo", "ppo-adap"])
def test_liar_native_adap_step_is_bitwise_the_per_call_walk(kinds, share):
    from pantheonrl_amd.envs.vec import AdapRaggedVecOnPolicyAgent
    from pantheonrl_amd.vec import AdapVecOnPolicyAgent
    E, T_ego, T_alt = 48, 8, 6
    runs = []
    for native in (True, False):
        sp, ego, alt = _adap_selfplay(E, T_ego, T_alt, kinds, share, seed=11, native=native)
        assert isinstance(ego, AdapVecOnPolicyAgent) == (kinds[0] == "ADAP")
        assert isinstance(alt, AdapRaggedVecOnPolicyAgent) == (kinds[1] == "ADAP")
        assert sp.adap and sp.persistent is False
        alt.model.rollout_buffer.gae_mode = ego.model.rollout_buffer.gae_mode = 1
        trained = LC.train_steps(sp, 3 * T_ego)[0]
        runs.append(dict(LC.train_state(sp, ego), trained=trained, **_contexts_of(sp, ego, alt)))
    a, b = runs
    assert a["trained"] >= 1 and a["ego_it"] >= 2 and a["episodes"] > E
    assert ("ctx_ego" in a) == (kinds[0] == "ADAP") and ("ctx_alt" in a) == (kinds[1] == "ADAP")
    if kinds[0] == "ADAP":
        assert a["e_observations"].shape[-1] == 273
    LC.same_state(a, b)


def test_liar_adap_step_with_two_null_seats_is_the_plain_step():
    E, T_ego, T_alt = 48, 8, 6
    runs = []
    for through_adap in (False, True):
        sp, ego, alt = _adap_selfplay(E, T_ego, T_alt, ("PPO", "PPO"), seed=3)
        assert not sp.adap
        if through_adap:
            sp.adap = True                        # _native_call then goes through ph_liar_selfplay_step_adap(NULL, NULL)
        else:
            LC.step_through_the_plain_entry_point(sp)         # ph_liar_selfplay_step itself, not the driver's _arch(NULL, NULL)
        sp.persistent = False
        alt.model.rollout_buffer.gae_mode = ego.model.rollout_buffer.gae_mode = 1
        trained = LC.train_steps(sp, 2 * T_ego)[0]
        runs.append(dict(LC.train_state(sp, ego), trained=trained))
    LC.same_state(*runs)


def test_a_bad_seat_is_an_error_string_not_a_launch():
    from pantheonrl_amd import _native as nat
    sp, ego, alt = _adap_selfplay(16, 4, 4, ("ADAP", "ADAP"), seed=1)
    ctx = sp.env.ctx

    def call(ego_seat, alt_seat):
        nat.check(ctx.lib.ph_liar_selfplay_step_adap(ctx.handle, C.byref(sp._desc), C.byref(ego_seat), C.byref(alt_seat), 0, 1, 0))
    th.cuda.synchronize()
    before = sp.env.nmoves.clone()
    bad = ego.seat_struct()
    bad.context_size = 4                                   # the Box spec says 273 = 270 + 3
    with pytest.raises(nat.NativeError, match="F \\+ C"):
        call(bad, alt.seat_struct())
    bad = alt.seat_struct()
    bad.sampler = nat.CONTEXT_SAMPLERS["natural_numbers"]  # draws one integer: context_size 1 only
    with pytest.raises(nat.NativeError, match="context_size == 1"):
        call(ego.seat_struct(), bad)
    both = ego.seat_struct(), alt.seat_struct()
    both[0].shared = both[1].shared = 1                    # somebody has to draw
    with pytest.raises(nat.NativeError, match="shared"):
        call(*both)
    bad = ego.seat_struct()
    bad.rows = None
    with pytest.raises(nat.NativeError, match="rows"):
        call(bad, alt.seat_struct())
    th.cuda.synchronize()
    assert th.equal(before, sp.env.nmoves)
    with pytest.raises(nat.NativeError, match="ADAP"):
        sp.rollout_persistent(4, 1)
    from pantheonrl_amd.envs.vec import LiarIterationGraph
    with pytest.raises(nat.NativeError, match="ADAP"):
        LiarIterationGraph(sp, 4)


# ---- 3. the walk means what the reference means -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True], ids=["own-contexts", "shared-latent"])
def test_liar_walk_with_adap_seats_shows_the_host_games_observations_under_the_drawn_contexts(share):
    from pantheonrl_amd.common import Agent, Observation
    from pantheonrl_amd.envs.liar import LiarEnv
    from pantheonrl_amd.envs.vec import VecLiarsDice

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
        """partner that plays the moves the device sampled and keeps what the host game showed it"""
        def __init__(self):
            self.moves, self.seen = deque(), []

        def get_action(self, obs, record=True):
            self.seen.append(np.asarray(obs.obs, np.float32))
            return self.moves.popleft()

        def update(self, reward, done):
            pass

    E, steps, cs = 24, 40, 3
    nvec = [int(v) for v in VecLiarsDice.observation_space.nvec]
    calls = []
    sp, ego, alt = _adap_selfplay(E, steps, 3 * steps, ("ADAP", "ADAP"), share, seed=21, native=False, calls=calls)
    seeds = ego.model.policy._seed, alt.model.policy._seed
    shadows, partners = [Shadow() for _ in range(E)], [Replay() for _ in range(E)]
    for s, p in zip(shadows, partners):
        s.add_partner_agent(p)
    alt_ctx_rows = [[] for _ in range(E)]                           # per table: the context under which each recorded row was made

    def feed(reset_mask):
        hands, first = sp.env.hands.cpu().numpy(), sp.ego_first.cpu().numpy()
        for acts, mask, ctxs in calls:
            for e in np.nonzero(mask)[0]:
                partners[e].moves.append(acts[e].copy())
                alt_ctx_rows[e].append(ctxs[e])
        calls.clear()
        for e in np.nonzero(reset_mask)[0]:
            shadows[e].deals.append((first[e], hands[e].copy()))

    tables = np.arange(E)
    want = [A.draw_contexts("l2", cs, s, 0, tables) for s in seeds]  # counter 0 before the first `done`
    feed(np.ones(E, bool))
    cur = [s.reset() for s in shadows]
    ends = np.zeros(E, np.int64)
    ego_rows = []
    for t in range(steps):
        c = t + 1
        before, ctx_before = sp.obs_ego.cpu().numpy().copy(), ego.contexts.cpu().numpy().copy()
        assert np.array_equal(bits(ctx_before), bits(want[0]))
        if not share:
            assert np.array_equal(bits(alt.contexts.cpu().numpy()), bits(want[1]))
        done = sp.step().cpu().numpy().astype(bool)
        a_ego = ego.actions.cpu().numpy().copy()
        assert len(calls) == 2                                      # reply: the contexts in front of this step's redraw; opening: behind
        for opening, (acts, mask, ctxs) in enumerate(calls):
            k = 0 if share else 1                                   # whose plane the partner reads
            ref = np.where(done[:, None], A.draw_contexts("l2", cs, seeds[k], c, tables), want[k]) if opening else want[k]
            assert np.array_equal(bits(ctxs[mask]), bits(ref[mask])), (t, opening)
            assert not opening or not (mask & ~done).any()          # the partner opens fresh games only
        feed(done)
        ends += done
        for k in range(2):                                          # both seats are paid `done` where the game ended
            want[k] = np.where(done[:, None], A.draw_contexts("l2", cs, seeds[k], c, tables), want[k])
        for e in range(E):
            assert np.array_equal(before[e], np.asarray(cur[e], np.float32)), (t, e)      # what the host game shows seat 0
            o, r, d, _ = shadows[e].step(a_ego[e])
            assert bool(d) == bool(done[e]), (t, e)
            cur[e] = shadows[e].reset() if d else o
            assert not partners[e].moves
        ego_rows.append((before, ctx_before))
    assert ends.sum() >= 2 * E and ends.min() >= 1 and ends.sum() == sp.episodes
    if share:                                                       # the partner never draws: its plane is the constructor's zeros
        assert not alt.contexts.cpu().numpy().any()
    th.cuda.synchronize()
    be, ba = ego.model.rollout_buffer.host(), alt.model.rollout_buffer.host()
    for t, (obs, ctxs) in enumerate(ego_rows):
        assert np.array_equal(bits(be["observations"][t]), bits(A.rows(nvec, obs, ctxs))), t
    pos = alt.pos.cpu().numpy()
    for e in range(E):
        seen = partners[e].seen
        assert pos[e] == len(seen) == len(alt_ctx_rows[e]) and pos[e] >= 1
        want_rows = A.rows(nvec, np.stack(seen), np.stack(alt_ctx_rows[e]))
        assert np.array_equal(bits(ba["observations"][:pos[e], e]), bits(want_rows)), e


# ---- 4. RPS ---------------------------------------------------------------------------------------------------------------------------
def test_rps_selfplay_iteration_with_two_adap_agents():
    from pantheonrl_amd.envs.vec import VecRPS, selfplay_iteration
    from pantheonrl_amd.vec import vec_agent_for
    E, T, cs = 32, 8, 3
    spaces = _game_spaces("rps")
    ego, alt = (vec_agent_for(_model("ADAP", spaces, T, E, seed)) for seed in (4, 5))
    ego.sync_stats = alt.sync_stats = True
    env = VecRPS(E, ego.model.policy.ctx, ego.model.policy.device)
    p0 = [a.model.policy.get_flat_params() for a in (ego, alt)]
    kept = []
    for a in (ego, alt):                                            # the buffers as the rollout left them, in front of the update
        inner = a.compute_returns
        a.compute_returns = (lambda a=a, inner=inner: (kept.append(a.model.rollout_buffer.host()["observations"].copy()), inner())[1])
    selfplay_iteration(env, ego, alt, T)
    th.cuda.synchronize()
    for a, obs, p in zip((ego, alt), kept, p0):
        assert obs.shape == (T, E, 1 + cs)
        for t in range(T):                                          # one-step episodes: every table redraws at every step
            want = np.concatenate([np.ones((E, 1), np.float32), A.draw_contexts("l2", cs, a.model.policy._seed, t, np.arange(E))], axis=1)
            assert np.array_equal(bits(obs[t]), bits(want)), t
        assert a.iteration == 1 and np.abs(a.model.policy.get_flat_params() - p).max() > 0
        cl = a.model.last_context_losses
        assert cl is not None and np.isfinite(cl).all() and (cl > 0).all()


# ---- 5. the gradient kernel at the Liar's Dice row shape --------------------------------------------------------------------------------
H.CONFIGS.setdefault("adap_liar", (H.SpaceSpec("box", dim=270 + 3), H.SpaceSpec("multidiscrete", nvec=(7, 12))))
TA.CTX.setdefault("adap_liar", 3)


def _liar_rows(obs, rng):
    """(E, 273) rows as the device builds them: one-hot Liar's Dice features, then an l2 context"""
    from pantheonrl_amd.envs.vec import VecLiarsDice
    nvec = np.asarray(VecLiarsDice.observation_space.nvec)
    raw = (rng.random((obs.shape[0], len(nvec))) * nvec).astype(np.int64).astype(np.float32)
    c = rng.random((obs.shape[0], 3)).astype(np.float32) * 2 - 1
    return A.rows([int(v) for v in nvec], raw, c / np.sqrt((c ** 2).sum(axis=1, keepdims=True)))


def test_context_term_gradient_at_box273_with_the_liar_heads_matches_autograd():
    T, E, nb, n_ctx, n_states = 16, 8, 64, 5, 32
    idx = np.random.default_rng(nb).permutation(T * E)[:nb]

    def fill(name, orac, T, E, seed=0):
        return H.filled_oracle_buffer(name, orac, T, E, seed=seed, obs_fn=_liar_rows)
    g, g_ref, st, st_ref, cl, _, _, lay = TA._grad_pair("adap_liar", T, E, idx, orc.PPOHyper(), n_ctx, n_states, coef=5.0, fill=fill)
    assert (lay.D, lay.A, lay.L) == (273, 2, 19)
    print("max |g - g_ref| = %.3e, max |g_ref| = %.3e, term %.6f vs %.6f" % (np.abs(g - g_ref).max(), np.abs(g_ref).max(), cl,
                                                                              st_ref["context_loss"]))
    TA._assert_grads(g, g_ref)
    assert abs(cl - st_ref["context_loss"]) <= 1e-5, (cl, st_ref["context_loss"])


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------
def test_native_adap_step_does_no_host_work_and_captures():
    from pantheonrl_amd import _native as nat
    sp, ego, alt = _adap_selfplay(32, 8, 8, ("ADAP", "ADAP"), seed=3)
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
        before, ctx_before = alt.pos.clone(), ego.contexts.clone()
        nat.check(ctx.lib.ph_graph_launch(ctx.handle, gid.value))
        stream.synchronize()
    th.cuda.synchronize()
    rows = ego.model.rollout_buffer.host()
    assert int((alt.pos - before).sum().item()) > 0 and np.isfinite(rows["values"][:6]).all()
    assert not th.equal(ctx_before, ego.contexts)                   # four steps of 32 tables: some game ended and its context moved
    assert np.all(np.abs(np.linalg.norm(rows["observations"][:6, :, 270:], axis=-1) - 1) < 1e-6)


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------------------
def test_trainer_liars_dice_adap_adap_shared_latent(tmp_path):
    from pantheonrl_amd.adap import ADAP
    from pantheonrl_amd.trainer import run
    ego, partners, env = run(["LiarsDice-v0", "ADAP", "ADAP", "--share-latent", "--n-envs", "32", "-t", "2048", "--seed", "1",
                              "--ego-config", '{"n_steps": 16, "n_epochs": 2}', "--alt-config", '{"n_steps": 8, "n_epochs": 2}',
                              "--ego-save", str(tmp_path / "ego"), "--alt-save", str(tmp_path / "alt")])
    assert env.ego.iteration == 4 and partners[0].iteration >= 1
    assert partners[0].latent_syncer is env.ego
    for path, model, plane in (("ego", ego, env.ego.contexts), ("alt", partners[0].model, env.ego.contexts)):
        again = ADAP.load(str(tmp_path / path))
        assert np.array_equal(again.policy.get_flat_params(), model.policy.get_flat_params())
        assert np.array_equal(bits(again.policy.get_context()), bits(plane.cpu().numpy()))
    assert env.episode_stats.read()["total"]["count"] > 0


def test_trainer_rps_adap_adap_runs(tmp_path):
    from pantheonrl_amd.trainer import run
    ego, partners, env = run(["RPS-v0", "ADAP", "ADAP", "--n-envs", "32", "-t", "1024", "--seed", "2",
                              "--ego-config", '{"n_steps": 16, "n_epochs": 2}', "--alt-config", '{"n_steps": 16, "n_epochs": 2}'])
    assert partners[0].iteration == 2 and partners[0].contexts.shape == (32, 3)
