"""-m gpu: every random draw of the device against the host statement of its Philox stream (tests/philox_ref.py).

A draw is a function of (key, 64-bit counter, row, component or block).  The rest of the suite compares the kernels' own draws with
each other (one launch against the per-step walk, the native step against the walk), which a wrong coordinate shared by both
sides passes.  Here the test sets the coordinates itself -- `pol._seed = KEY` with a non-zero high word, `pol._counter = c - 1` for
c in {7, 2**32 + 5} -- predicts the draw on the host and compares: integers bit for bit, sampled actions through the checker's
float64 inverse CDF on every row whose uniform is not within helpers.EDGE_MARGIN of a CDF edge of the checker (tests/sampler_cases.py;
tests/test_philox_host.py shows on the CPU that such rows are none at n <= 65 and at most 3 % above, and that a shifted row,
component, counter word or key word would move >= 20 % of the predictions).

philox_uniform / philox_uniform4 call sites under csrc/ -> the test that reaches them:
  ph_rowtail.h   discrete8_row_tail (:219)       test_categorical_heads_draw_the_host_stream[overcooked | rps | mpe8 | mpe8-masked |
                                                  overcooked-16384 (through general_row_tail) | adapmult-small (ph_adapmult.hip) |
                                                  modular-* (ph_modular.hip)]
  ph_rowtail.h   general_row_tail, categorical   ...[wide | quad16 | onehot17 | arch32-wide (ph_arch.hip)]
  ph_rowtail.h   general_row_tail, Gaussian      test_gaussian_head_draws_box_muller_on_the_host_uniforms
  ph_policy.hip  head_draw32 (:904)              ...[liar | onehot32 | discrete20 | discrete20-masked]; the grouped forward's 64-64 tiles:
                                                  test_pool_forward_clone_and_frozen_tiles_draw_the_host_stream
  ph_policy.hip  tail wave `draw` (:583)         test_one_launch_rollout_rows_hold_the_host_prediction[lean | general]
  ph_policy.hip  draw_uniforms / u_pre (:454)    test_one_launch_rollout_rows_hold_the_host_prediction[valu]
  ph_bc.hip      bc_forward_kernel (:905)        ...[bc-liar | bc-box33-3x30x7]
  ph_bc_row.h    bc_clone_tile (:176)            test_pool_forward_clone_and_frozen_tiles_draw_the_host_stream
  ph_liar.h      liar_deal (:118, :133)          test_liar_reset_deals_the_host_deal (ph_envs.hip), test_liar_drivers_deal_the_host_deal[walk |
                                                  native (ph_liar_step.h: the one step of self-play, pool and cross-play)]
  ph_liar_group.h liar_grp_deal (:140)           test_liar_rollout_launch_deals_under_the_epoch_word (the 4-lanes-per-table deal of the
                                                  one-launch rollout, liar_rollout_kernel)
  ph_adap.hip    contexts (:146, :150, :156)     test_adap_samples_are_the_host_statement[adap-*]
  ph_adapmult.hip contexts (:370, :374, :380)    test_adap_samples_are_the_host_statement[mult-*]
  ph_pool.h      the pool's resample word        tests/test_pool_host.py (already pinned to envs/vec.py::philox_word0)
  ph_block.h     BlockWorld's reset              tests/test_gpu_blockworld.py (a host replay of its __host__ __device__ source)
"""
import ctypes as C

import numpy as np
import pytest
import torch as th

from tests import helpers as H
from tests import philox_ref as R
from tests import sampler_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t, shape=None):
    a = t.detach().cpu().numpy()
    return a if shape is None else a.reshape(shape)


# ---- a. categorical heads, own draws; b. the negative control ---------------------------------------------------------------------------
def _forward(case, pol, obs, mask, c, uniforms=None):
    """one forward at (S.KEY, c): the launch advances the counter before it passes it on"""
    pol._seed, pol._counter = S.KEY, c - 1
    kw = dict(partner_idx=case.extra["partner"]) if case.family == "modular" else {}
    acts, _, logp = pol.forward(obs, action_mask=mask, uniforms=uniforms, **kw)
    assert pol._counter == c
    return _np(acts, (len(obs), -1)), _np(logp)


@pytest.mark.parametrize("cid", [c.id for c in S.CASES])
def test_categorical_heads_draw_the_host_stream(cid):
    """pol.forward(obs) with no `uniforms`: the action of row g, component k is the checker's float64 inverse CDF at
    philox_ref.uniform(KEY, c, g, k) on every row that is not near; the same rows teacher-forced with those uniforms give the same
    actions and the checker's log-prob at 2e-5.  Inside: the negative control on the host prediction.  What each case reaches:
    sampler_cases.CASES[].kernel."""
    case = S.BY_ID[cid]
    pol = S.device(case)
    A = len(S.spaces(case)[1].nvec)
    for mode in case.gemm_modes:
        if mode is not None:
            pol.gemm_mode = mode
        for n in case.rows:
            obs, mask = S.inputs(case, n)
            probs = S.probabilities64(case, obs, mask)
            for c in S.COUNTERS:
                where = (cid, case.kernel, "gemm_mode", mode, "n", n, "counter", c)
                u = S.uniforms(n, A, S.KEY, c)
                want, near = S.predict(probs, u)
                ctl = S.control(probs, n, S.KEY, c)
                S.assert_caps_and_control(cid, n, near, ctl, c)
                got, logp = _forward(case, pol, obs, mask, c)
                bad = np.nonzero((got != want).any(axis=1) & ~near)[0]
                print(where, "near", int(near.sum()), "mismatches", len(bad), "control", {k: round(v, 2) for k, v in ctl.items()})
                assert len(bad) == 0, (where, bad[:8], got[bad[:8]], want[bad[:8]], u[bad[:8]])
                lp_ref = S.log_prob64(probs, want)
                assert np.abs(logp - lp_ref)[~near].max() <= S.FORWARD_TOL, where
                # the same rows with the host's uniforms handed in: the kernel's own draw is off, the answer must not move
                got_u, logp_u = _forward(case, pol, obs, mask, c, uniforms=u)
                assert np.array_equal(got_u[~near], want[~near]), where
                assert np.abs(logp_u - lp_ref)[~near].max() <= S.FORWARD_TOL, where
                assert np.array_equal(got_u, got) and np.array_equal(logp_u, logp), where     # (the same uniform: the same bits)


def test_pool_forward_clone_and_frozen_tiles_draw_the_host_stream():
    """ph_pool_forward over 50 tables that alternate between a behavioural clone (bc_clone_tile, ph_bc_row.h) and a frozen 64-64
    policy (the grouped forward's DPP head), four tables sitting out: table e of member k plays the host prediction for
    (member key, counter, row = e, component) -- the row slot is the TABLE, not the row's place in its member's tile"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.bc import FeedForward32Policy
    obs, pid, active = S.pool_inputs()
    n = len(obs)
    obs_s, act_s = H.CONFIGS["liar"]
    clone = FeedForward32Policy(H.to_space(obs_s), H.to_space(act_s), device=DEV, seed=7)
    clone.set_flat_params(S.checker("bc-liar").flat_params())
    frozen = H.device_policy("liar", S.checker("liar"))
    arr = (nat.PhPoolMember * 2)()
    for k, (kind, pol) in enumerate(((nat.PH_POOL_CLONE, clone), (nat.PH_POOL_FROZEN, frozen))):
        arr[k].kind, arr[k].params, arr[k].seed = kind, pol.params.data_ptr(), S.POOL_KEYS[k]
    ctx = frozen.ctx
    frozen._bind()
    obs_t, pid_t, act_t = (th.as_tensor(x).to(DEV) for x in (obs, pid, active))
    es = th.zeros(n, dtype=th.float32, device=DEV)
    on = active.astype(bool)
    for c in S.COUNTERS:
        want, near, ctl = S.pool_prediction(obs, pid, c)
        S.assert_rollout_caps(("pool", c), near, ctl)
        out = th.full((n, 2), -7, dtype=th.int32, device=DEV)
        nat.check(ctx.lib.ph_pool_forward(ctx.handle, C.byref(frozen.spec), arr, 2, obs_t.data_ptr(), pid_t.data_ptr(), act_t.data_ptr(),
                                          c, out.data_ptr(), es.data_ptr(), n))
        th.cuda.synchronize()
        got = _np(out)
        assert (got[~on] == -7).all()
        for k in (0, 1):
            rows = on & (pid == k) & ~near
            assert rows.sum() >= 20 and np.array_equal(got[rows], want[rows]), (c, S.POOL_KINDS[k], got[rows], want[rows])


# ---- c. the one-launch rollouts ---------------------------------------------------------------------------------------------------------
def _rollout_setup(E, T):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.vec import VecOnPolicyAgent
    obs_s, act_s = H.CONFIGS[S.ROLLOUT_NAME]
    env = type("E", (), dict(observation_space=H.to_space(obs_s), action_space=H.to_space(act_s), _is_dummy_space_env=True))()
    model = PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=T * E, n_epochs=1, seed=0)
    model.policy.set_flat_params(S.checker(S.ROLLOUT_NAME).flat_params())
    return model, VecOnPolicyAgent(model), S.rollout_data(E, T, device=model.device)


@pytest.mark.parametrize("form", ["lean", "general", "valu"])
@pytest.mark.parametrize("E,T", S.ROLLOUT_SHAPES)
def test_one_launch_rollout_rows_hold_the_host_prediction(E, T, form):
    """ph_scripted_rollout: row t of the rollout buffer holds the action the host predicts from the STORED observation at counter
    c0 + t, row = environment, component 0 -- with the RNG epoch word at 0 and advanced once (ph_rng_epoch_advance, what
    IterationGraph captures behind an iteration): the word rides in the high half of the counter.  lean / general: the tail-wave
    forms of policy_fwd16_rollout_kernel (the tail wave's own `draw`; general = a debug stamp buffer on the context, as
    tests/test_gpu_rollout_tail_wave.py selects it); valu: gemm_mode 1, the form without a tail wave, whose wave 1 pre-draws
    `u_pre` a step ahead.  This pins counter + t + epoch_hi to the host statement, not to the per-step walk."""
    from pantheonrl_amd import _native as nat
    model, agent, data = _rollout_setup(E, T)
    pol, rb = model.policy, model.rollout_buffer
    if form == "valu":
        pol.gemm_mode = 1
    keep = None
    if form == "general":
        keep = th.zeros(2 * ((E + 15) // 16) * 16, dtype=th.int64, device=model.device)
        nat.check(pol.ctx.lib.ph_debug_set_profile_buffer(pol.ctx.handle, keep.data_ptr()))
    word = th.zeros(1, dtype=th.int64, device=model.device)
    nat.check(pol.ctx.lib.ph_ctx_set_rng_epoch(pol.ctx.handle, word.data_ptr()))
    seen = []
    for c0, epoch in S.ROLLOUT_RUNS:
        agent.bind_stream()
        while int(word.item()) < epoch:
            nat.check(pol.ctx.lib.ph_rng_epoch_advance(pol.ctx.handle))
            th.cuda.synchronize()
        assert int(word.item()) == epoch
        pol._seed, pol._counter = S.KEY, c0 - 1
        rb.pos, rb.full = 0, False
        agent.rollout_scripted(data)
        th.cuda.synchronize()
        assert pol._counter == c0 - 1 + T
        host = rb.host()
        obs = host["observations"].reshape(T, E, -1)
        assert np.array_equal(obs, _np(data.obs))
        want, near, ctl = S.rollout_prediction(obs, S.KEY, c0, epoch)
        S.assert_rollout_caps((E, T, c0, epoch), near, ctl)
        got = host["actions"].reshape(T, E)
        bad = np.argwhere((got != want) & ~near)
        print((E, T, form), "counter", c0, "epoch", epoch, "near", int(near.sum()), "mismatches", len(bad))
        assert len(bad) == 0, ((E, T, form, c0, epoch), bad[:8])
        assert np.array_equal(_np(agent.actions).reshape(-1)[~near[-1]], want[-1][~near[-1]])       # the cached last step
        probs = [S.probabilities64(S.BY_ID[S.ROLLOUT_NAME], obs[t], None) for t in range(T)]
        lp_ref = np.stack([S.log_prob64(probs[t], want[t][:, None]) for t in range(T)])
        assert np.abs(host["log_probs"].reshape(T, E) - lp_ref)[~near].max() <= S.FORWARD_TOL
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])
    if keep is not None:
        nat.check(pol.ctx.lib.ph_debug_set_profile_buffer(pol.ctx.handle, None))
    nat.check(pol.ctx.lib.ph_ctx_set_rng_epoch(pol.ctx.handle, None))


# ---- d. the Gaussian head ---------------------------------------------------------------------------------------------------------------
GAUSS_FACTOR, GAUSS_CEILING = 16.0, 1e-3


@pytest.mark.parametrize("name", ["gauss5", "gauss16"])
def test_gaussian_head_draws_box_muller_on_the_host_uniforms(name):
    """eps_dev = (a - mu) / exp(log_std) at n = 257 against Box-Muller in float64 on the host uniforms: u1 at component c, u2 at
    c + 128, max(u1, 1e-30) as the kernel clamps.  Allowance per entry: 16 x (the largest error of the same formula in numpy float32
    against float64 on the same uniforms) + the recovery rounding 2**-23 |a| / sigma, and below 1e-3 whatever is measured -- a
    wrong coordinate moves eps by order one (the control: median |delta eps| > 0.5 under every shifted coordinate).
    Measured on an MI355X (printed by the test; CHANGELOG.md): the float32 formula differs from float64 by 8.9e-7 to 9.4e-7 on these
    uniforms, the device's eps from the float64 host value by at most 1.0e-6 (gauss5) and 1.2e-6 (gauss16): 6 to 8 % of the allowance,
    which came to 1.5e-5 to 1.6e-5."""
    orac = H.oracle_policy(name, seed=3)
    pol = H.device_policy(name, orac)
    obs_s, act_s = H.CONFIGS[name]
    n, A = 257, act_s.dim
    obs = H.sample_obs(obs_s, n, np.random.default_rng(5))
    mu = _np(pol.forward(obs, deterministic=True)[0]).astype(np.float64)
    sigma = np.exp(_np(pol.log_std()).astype(np.float64))[None, :]
    assert mu.shape == (n, A) and len(np.unique(sigma)) == A

    def host_eps(key, c, row_shift=0, comp_shift=0, dtype=np.float64):
        u1 = S.uniforms(n, A, key, c, row_shift=row_shift, comp_shift=comp_shift)
        u2 = S.uniforms(n, A, key, c, row_shift=row_shift, comp_shift=comp_shift + 128)
        return R.box_muller(u1, u2, dtype).astype(np.float64)

    for c in S.COUNTERS:
        pol._seed, pol._counter = S.KEY, c - 1
        a = _np(pol.forward(obs)[0]).astype(np.float64)
        eps_dev = (a - mu) / sigma
        eps = host_eps(S.KEY, c)
        measured = np.abs(host_eps(S.KEY, c, dtype=np.float32) - eps).max()
        allowed = GAUSS_FACTOR * measured + 2.0 ** -23 * np.abs(a) / sigma
        err = np.abs(eps_dev - eps)
        print(name, "counter", c, "float32 formula vs float64: %.3g; device vs float64 host: max %.3g, largest allowance %.3g, "
              "largest share of its allowance %.3g" % (measured, err.max(), allowed.max(), (err / allowed).max()))
        assert allowed.max() < GAUSS_CEILING, allowed.max()
        assert (err <= allowed).all(), (name, c, err.max(), np.argwhere(err > allowed)[:5])
        for shift, kw in (("row + 1", dict(row_shift=1)), ("component + 1", dict(comp_shift=1))):
            assert np.median(np.abs(host_eps(S.KEY, c, **kw) - eps)) > 0.5, shift
        for shift, (k2, c2) in (("counter + 1", (S.KEY, c + 1)), ("counter + 2**32", (S.KEY, c + 2 ** 32)),
                                ("key high word cleared", (S.KEY & 0xFFFFFFFF, c))):
            assert np.median(np.abs(host_eps(k2, c2) - eps)) > 0.5, shift


# ---- e. the Liar's Dice deal --------------------------------------------------------------------------------------------------------------
DEALS = [(5, 0), (5, 9), (2 ** 40 + 3, 2 ** 33 + 1)]


@pytest.mark.parametrize("probegostart", [0.5, 0.25])
@pytest.mark.parametrize("seed,counter", DEALS)
def test_liar_reset_deals_the_host_deal(seed, counter, probegostart):
    """ph_liar_reset as VecLiarStep._deal calls it, E = 300, a third of the tables outside the reset mask: hands equal the host deal
    bit for bit (die d = word d % 4 of block d // 4 at row = table, side = min(int(float32(u) * 6), 5)), ego_first equals
    uniform(block 100) < probegostart, and the tables left out keep what they held"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.envs.vec import VecLiarsDice
    E = 300
    ctx = nat.Context(0)
    ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
    env = VecLiarsDice(E, ctx, th.device(DEV))
    rng = np.random.default_rng(counter % 97)
    mask = (rng.random(E) < 2.0 / 3.0)
    assert 60 < (~mask).sum() < 140
    env.hands.fill_(-3), env.history.fill_(9), env.nmoves.fill_(4)
    first = th.full((E,), 7, dtype=th.uint8, device=DEV)
    mask_t = th.as_tensor(mask.astype(np.uint8)).to(DEV)
    nat.check(ctx.lib.ph_liar_reset(ctx.handle, env.hands.data_ptr(), env.history.data_ptr(), env.nmoves.data_ptr(), mask_t.data_ptr(),
                                    first.data_ptr(), seed, counter, probegostart, E))
    th.cuda.synchronize()
    tables = np.arange(E)
    want = R.liar_deal(seed, counter, tables)
    # the host deal is a deal: tables differ, and so do the two hands of most tables
    assert len({tuple(r) for r in want.tolist()}) > 250 and (want[:, :6] != want[:, 6:]).any(axis=1).mean() > 0.9
    hands, hist, nm, ef = _np(env.hands), _np(env.history), _np(env.nmoves), _np(first)
    assert np.array_equal(hands[mask], want[mask]), np.argwhere(hands[mask] != want[mask])[:5]
    assert np.array_equal(ef[mask], R.liar_ego_first(seed, counter, tables, probegostart)[mask].astype(np.uint8))
    assert not hist[mask].any() and not nm[mask].any()
    assert (hands[~mask] == -3).all() and (hist[~mask] == 9).all() and (nm[~mask] == 4).all() and (ef[~mask] == 7).all()


def _liar_selfplay(E, T, seed, native):
    from pantheonrl_amd import PPO
    from pantheonrl_amd.envs.vec import RaggedVecOnPolicyAgent, VecLiarsDice, VecLiarSelfPlay
    from pantheonrl_amd.vec import VecOnPolicyAgent
    spaces = type("S", (), dict(observation_space=VecLiarsDice.observation_space, action_space=VecLiarsDice.action_space,
                                _is_dummy_space_env=True))()
    me = PPO("MlpPolicy", spaces, n_steps=T, n_envs=E, batch_size=E * T // 2, n_epochs=1, seed=1)
    ma = PPO("MlpPolicy", spaces, n_steps=4 * T, n_envs=E, batch_size=E * T, n_epochs=1, seed=2)     # never full within the test
    me.device_permutations = ma.device_permutations = True
    ego, alt = VecOnPolicyAgent(me), RaggedVecOnPolicyAgent(ma)
    return VecLiarSelfPlay(E, ego, alt, seed=seed, native=native), ego, alt


LIAR_SEED = 2 ** 40 + 3


@pytest.mark.parametrize("native", [True, False], ids=["native", "walk"])
def test_liar_drivers_deal_the_host_deal(native):
    """VecLiarSelfPlay, 64 tables, 12 steps: every table starts on the host deal of counter 0, and a table whose game ended in step c
    holds the host deal of counter c at the end of that step (native: liar_deal inside the engine's one step, ph_liar_step.h; walk:
    ph_liar_reset, launch by launch)"""
    E, steps = 64, 12
    sp, ego, alt = _liar_selfplay(E, 16, LIAR_SEED, native)
    tables = np.arange(E)
    th.cuda.synchronize()
    hands = _np(sp.env.hands).copy()
    assert np.array_equal(hands, R.liar_deal(LIAR_SEED, 0, tables))
    assert np.array_equal(_np(sp.ego_first), R.liar_ego_first(LIAR_SEED, 0, tables, 0.5).astype(np.uint8))
    ended = 0
    for c in range(1, steps + 1):
        done = _np(sp.step()).astype(bool)
        th.cuda.synchronize()
        now, ef = _np(sp.env.hands).copy(), _np(sp.ego_first)
        want = R.liar_deal(LIAR_SEED, c, tables)
        assert np.array_equal(now[done], want[done]), (c, np.nonzero(done)[0])
        assert np.array_equal(ef[done], R.liar_ego_first(LIAR_SEED, c, tables, 0.5)[done].astype(np.uint8)), c
        assert np.array_equal(now[~done], hands[~done]), c                  # a game that goes on keeps its dice
        hands, ended = now, ended + int(done.sum())
    assert ended > E // 2 and ended == sp.episodes


def test_liar_rollout_launch_deals_under_the_epoch_word():
    """ph_liar_selfplay_rollout, 16 steps of 64 tables as one launch with the RNG epoch word at 2: a table's last deal happened at the
    step its last game ended (read off the ego's episode starts), and its hands are the host deal of counter step + (2 << 32) --
    the epoch word in the high half of the dice counter; a table whose first game never ended keeps the deal of counter 0"""
    from pantheonrl_amd import _native as nat
    E, T, epoch = 64, 16, 2
    sp, ego, alt = _liar_selfplay(E, T, LIAR_SEED, True)
    ctx = sp.env.ctx
    word = th.full((1,), epoch, dtype=th.int64, device=sp.dev)
    nat.check(ctx.lib.ph_ctx_set_rng_epoch(ctx.handle, word.data_ptr()))
    sp.rollout_persistent(T, 1, 0)
    th.cuda.synchronize()
    es = ego.model.rollout_buffer.host()["episode_starts"].reshape(T, E)
    done = np.concatenate([es[1:], _np(ego._last_episode_starts).reshape(1, E)]) != 0      # done[t]: the game ended in step t + 1
    assert int(done.sum()) == sp.episodes and done.any(axis=0).sum() > E // 2
    tables = np.arange(E)
    want = R.liar_deal(LIAR_SEED, 0, tables)
    first = R.liar_ego_first(LIAR_SEED, 0, tables, 0.5)
    for t in range(T):
        c = t + 1 + (epoch << 32)
        want[done[t]] = R.liar_deal(LIAR_SEED, c, tables)[done[t]]
        first[done[t]] = R.liar_ego_first(LIAR_SEED, c, tables, 0.5)[done[t]]
    assert np.array_equal(_np(sp.env.hands), want), np.nonzero((_np(sp.env.hands) != want).any(axis=1))[0]
    assert np.array_equal(_np(sp.ego_first), first.astype(np.uint8))
    # the word matters: the same steps dealt under epoch 0 give other hands in the tables that were dealt again
    plain = R.liar_deal(LIAR_SEED, 0, tables)
    for t in range(T):
        plain[done[t]] = R.liar_deal(LIAR_SEED, t + 1, tables)[done[t]]
    assert (plain != want).any(axis=1).sum() >= 0.9 * done.any(axis=0).sum()
    nat.check(ctx.lib.ph_ctx_set_rng_epoch(ctx.handle, None))


# ---- f. ADAP's samples ------------------------------------------------------------------------------------------------------------------
ADAP_SALT = 0xADA9C0DE
SAMPLERS = ["natural_numbers", "categorical", "positive_square", "unit_square", "l2"]
ADAP_SHAPES = [("adap", 8, 4, 20), ("adap", 16, 8, 64), ("mult", 8, 4, 20)]


def host_contexts(sampler, key, n_ctx, cs):
    """-> (contexts (n_ctx, cs) float64, ulps allowed): counter 1, row = context index, component k"""
    u = R.uniform(key, 1, np.arange(n_ctx)[:, None], np.arange(cs)[None, :])
    assert u.dtype == np.float32
    if sampler in ("natural_numbers", "categorical"):
        v = np.minimum((u[:, 0] * np.float32(cs)).astype(np.int64), cs - 1)
        out = np.zeros((n_ctx, cs))
        if sampler == "natural_numbers":
            out[:, 0] = v
        else:
            out[np.arange(n_ctx), v] = 1.0
        return out, 0
    if sampler == "positive_square":
        return u.astype(np.float64), 0
    v = (u * np.float32(2.0) - np.float32(1.0)).astype(np.float32).astype(np.float64)       # exact in float32
    if sampler == "unit_square":
        return v, 0
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True)), 4        # one sqrtf, one division (and the sum of squares' order)


@pytest.mark.parametrize("epoch", [0, 3])
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("kind,T,E,nb", ADAP_SHAPES, ids=["adap-8x4-20", "adap-16x8-64", "mult-8x4-20"])
def test_adap_samples_are_the_host_statement(kind, T, E, nb, sampler, epoch):
    """ph_adap_minibatch_grad / ph_adapmult_minibatch_grad with nothing teacher-forced: used_contexts equal the host statement under
    the key epoch_key((seed ^ 0xADA9C0DE) + epoch, minibatch 0) -- integer-valued samplers bit for bit, l2 within 4 float32 ulp --
    and used_state_idx is the head of nat.feistel_indices(nb, (seed ^ 0xADA9C0DE) + epoch, 0).  natural_numbers draws ONE integer
    below the context size and the engine takes it at context size 1 only: it runs on a policy of that context size."""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd import spaces as sp
    from pantheonrl_amd.adap import AdapPolicyMult
    from pantheonrl_amd.ppo import ActorCriticPolicy, RolloutBuffer
    from oracle import sb3_oracle as orc
    from tests.adap_cases import _adap_struct
    from tests.adapmult_cases import _hyper
    obs_s, act_s = H.CONFIGS["adap_small"]
    cs = 1 if sampler == "natural_numbers" else 3
    n_ctx, n_states, seed = 5, 32, 2 ** 40 + 11
    obs_space, act_space = sp.Box(-np.inf, np.inf, (obs_s.dim,)), H.to_space(act_s)
    if kind == "mult":
        pol = AdapPolicyMult(sp.Box(-np.inf, np.inf, (obs_s.dim - cs,)), act_space, context_size=cs, device="cuda", seed=0)
        P = pol.mlayout.P
    else:
        pol = ActorCriticPolicy(obs_space, act_space, device="cuda", seed=0)
        P = pol.layout.P
    buf = RolloutBuffer(T, obs_space, act_space, pol.device, pol.ctx, pol.spec, n_envs=E)
    g = th.Generator().manual_seed(1)
    for k in ("observations", "rewards", "values", "log_probs", "advantages", "returns"):
        getattr(buf, k).copy_(th.randn(getattr(buf, k).shape, generator=g))
    buf.actions.copy_(th.randint(0, 5, buf.actions.shape, generator=g).float())
    buf.pos, buf.full = T, True
    keep = []
    ad, _, used = _adap_struct(nat, cs, n_ctx, n_states, 1.0, keep, sampler=sampler, seed=seed, want_used=True)
    idx = th.as_tensor(np.random.default_rng(nb).permutation(T * E)[:nb].astype(np.int32)).cuda()
    grad, st = th.zeros(P, device="cuda"), th.zeros(nat.PH_NSTAT, device="cuda")
    h = _hyper(nat, orc.PPOHyper())
    word = th.full((1,), epoch, dtype=th.int64, device="cuda")
    pol._bind()
    nat.check(pol.ctx.lib.ph_ctx_set_rng_epoch(pol.ctx.handle, word.data_ptr()))
    if kind == "mult":
        nat.check(pol.ctx.lib.ph_adapmult_minibatch_grad(pol.ctx.handle, C.byref(pol.spec), cs, pol.params.data_ptr(), C.byref(buf.c_struct()),
                                                         C.byref(h), idx.data_ptr(), nb, grad.data_ptr(), st.data_ptr(), C.byref(ad)))
    else:
        nat.check(pol.ctx.lib.ph_adap_minibatch_grad(pol.ctx.handle, C.byref(pol.spec), pol.params.data_ptr(), C.byref(buf.c_struct()),
                                                     C.byref(h), idx.data_ptr(), nb, grad.data_ptr(), st.data_ptr(), 0, C.byref(ad)))
    th.cuda.synchronize()
    nat.check(pol.ctx.lib.ph_ctx_set_rng_epoch(pol.ctx.handle, None))
    key = R.epoch_key((seed ^ ADAP_SALT) + epoch, 0)
    want, ulps = host_contexts(sampler, key, n_ctx, cs)
    got = _np(used[1][0]).astype(np.float64)
    if ulps == 0:
        assert np.array_equal(got, want), (got, want)
    else:
        assert (np.abs(got - want) <= ulps * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all(), (got, want)
    if sampler not in ("natural_numbers", "categorical"):
        assert len(np.unique(want)) == want.size                             # contexts and components all differ: nothing degenerate
    assert not np.array_equal(want, host_contexts(sampler, R.epoch_key((seed ^ ADAP_SALT) + epoch + 1, 0), n_ctx, cs)[0]) or cs == 1
    ns = min(n_states, nb)
    sidx = _np(used[0][0])
    assert np.array_equal(sidx[:ns], nat.feistel_indices(nb, (seed ^ ADAP_SALT) + epoch, 0)[:ns]) and (sidx[ns:] == -1).all()
    assert len(set(sidx[:ns].tolist())) == ns
