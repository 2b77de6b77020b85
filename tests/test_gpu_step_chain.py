"""-m gpu: the two-launch minibatch step (ppo_reduce_kernel -> ppo_adam_kernel, learners that share a device) against the fused
one-launch step (ppo_step_kernel, ph_set_exclusive_device), bit for bit, over small chains of steps.

The two-launch kernels consume their early loads behind the slab walk and take Adam's bias corrections from the table the call's
advantage-statistics launch wrote (AdamBias, one entry per minibatch, made for step *opt_step + 1 + mb); step_body / ppo_step_kernel
compute their own and are the independent statement.  What a stale entry, a wrong base step or a lost stop test would change is
compared here: params, adam_m, adam_v, opt_step, the weight image and every per-minibatch statistics row.

Every case runs three epochs on an on-policy buffer the policy under test filled itself (first minibatch: ratio == 1)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

from oracle.sb3_oracle import SpaceSpec
from tests import helpers as H

pytestmark = pytest.mark.gpu

# name -> (observation space, action space, n_envs, n_steps, batch, gemm_mode or None = the policy's default)
CASES = {
    # Box 62 -> Discrete 6 (the bench's spaces): register-order slabs through the table, even slab length
    "oc": (SpaceSpec("box", dim=62), SpaceSpec("discrete", nvec=(6,)), 8, 8, 32, None),
    # the same at 40 rows in minibatches of 16: the last minibatch of every epoch is ragged (8 rows)
    "oc-ragged": (SpaceSpec("box", dim=62), SpaceSpec("discrete", nvec=(6,)), 5, 8, 16, None),
    # canonical slabs (map == null: slab position = parameter index): 70 features are past the register-order kernels, and
    # gemm_mode 0 keeps the spec off the split kernels, whose slabs have their own table; 40 rows, ragged last minibatch
    "canonical": (SpaceSpec("box", dim=70), SpaceSpec("discrete", nvec=(3,)), 5, 8, 16, 0),
    # Liar's Dice: the one-hot kernel, an odd slab length (4-byte loads, four ranges in turn)
    "liar": H.CONFIGS["liar"] + (4, 8, 16, None),
}
N_EPOCHS = 3


def _mismatches(pol):
    from pantheonrl_amd import _native as nat
    n = C.c_int(-2)
    nat.check(pol.ctx.lib.ph_debug_weight_image_mismatches(pol.ctx.handle, C.byref(pol.spec), pol.params.data_ptr(), C.byref(n)))
    return n.value


def _model(case, exclusive, t0, target_kl=None):
    """a PPO model of the case on a full on-policy buffer, its optimizer loaded with step t0 (and, past step 0, seeded moments)"""
    from pantheonrl_amd.ppo import PPO
    obs_s, act_s, E, T, batch, gm = CASES[case]
    env = type("E", (), dict(observation_space=H.to_space(obs_s), action_space=H.to_space(act_s), _is_dummy_space_env=True))()
    model = PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=batch, n_epochs=N_EPOCHS, target_kl=target_kl, seed=0)
    pol, rb = model.policy, model.rollout_buffer
    pol.ctx.set_exclusive_device(exclusive)
    if gm is not None:
        pol.gemm_mode = gm
    pol.set_flat_params(_initial_params(case))
    rng = np.random.default_rng(11)
    starts = np.ones(E, np.float32)
    for _ in range(T):
        pol.forward_and_store(H.sample_obs(obs_s, E, rng), rb, starts, uniforms=rng.random((E, act_s.stored_len)).astype(np.float32))
        rb.add_reward(th.as_tensor(rng.standard_normal(E).astype(np.float32), device="cuda"))
        starts = (rng.random(E) < 0.1).astype(np.float32)
    rb.compute_returns_and_advantage(th.zeros(E, device="cuda"), th.as_tensor(starts, device="cuda"))
    if t0:
        g = np.random.default_rng(t0)
        P = pol.adam_m.numel()
        pol.adam_m.copy_(th.as_tensor((1e-3 * g.standard_normal(P)).astype(np.float32)))
        pol.adam_v.copy_(th.as_tensor((1e-5 * g.random(P)).astype(np.float32)))
    pol.opt_step.fill_(int(t0))
    model.device_permutations = True
    return model


@functools.lru_cache(maxsize=None)
def _initial_params(case):
    from pantheonrl_amd.ppo import PPO
    obs_s, act_s, E, T, batch, _ = CASES[case]
    env = type("E", (), dict(observation_space=H.to_space(obs_s), action_space=H.to_space(act_s), _is_dummy_space_env=True))()
    return PPO("MlpPolicy", env, n_steps=T, n_envs=E, batch_size=batch, n_epochs=1, seed=0).policy.get_flat_params().copy()


def _state(model):
    pol = model.policy
    th.cuda.synchronize()
    return dict(params=pol.get_flat_params().copy(), adam_m=pol.adam_m.cpu().numpy().copy(), adam_v=pol.adam_v.cpu().numpy().copy(),
                opt_step=int(pol.opt_step.item()), image_mismatches=_mismatches(pol))


def _assert_same(where, got, want):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape, (where, k, g.shape, w.shape)
            bad = np.argwhere(g != w)
            assert bad.size == 0, (where, k, "%d entries differ, the first at %s: %r against %r"
                                   % (len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]), bad[:8].tolist())
        else:
            assert g == w, (where, k, g, w)


def _n_minibatches(case):
    _, _, E, T, batch, _ = CASES[case]
    return N_EPOCHS * (-(-(E * T) // batch))


def _chain(case, exclusive, t0, target_kl=None):
    model = _model(case, exclusive, t0, target_kl)
    model.train()
    out = _state(model)
    out["stats"] = model.last_train_stats.copy()
    return out


@functools.lru_cache(maxsize=None)
def _fused(case, t0):
    return _chain(case, True, t0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_two_launch_chain_is_bitwise_the_fused_chain(case):
    """(the canonical case is the one that found the fused launch's unordered pair of stores to the gradient-norm slot: the statistics
    block's zero and block 0's norm, whichever landed last -- 4 to 9 of its 9 rows read 0.0; the slot now has one writer per launch)"""
    two, one = _chain(case, False, 0), _fused(case, 0)
    n = _n_minibatches(case)
    assert one["opt_step"] == n and (one["stats"][:, 7] == 1).all() and one["stats"].shape[0] == n, (case, one["opt_step"])
    # (-1: the context holds no weight image -- gemm_mode 0 keeps the canonical case off the split kernels that read one)
    assert one["image_mismatches"] == (-1 if CASES[case][5] == 0 else 0) and np.isfinite(one["params"]).all()
    assert not np.array_equal(one["params"], _initial_params(case))
    _assert_same(case, two, one)


@pytest.mark.parametrize("t0", [0, 7, 100000])
def test_two_launch_chain_from_a_loaded_optimizer_step(t0):
    """the table's base is the step counter as the call finds it: at 0 and 7 the bias corrections matter (a base off by one moves every
    parameter), at 100 000 both are 1"""
    two, one = _chain("oc", False, t0), _fused("oc", t0)
    assert one["opt_step"] == t0 + _n_minibatches("oc")
    _assert_same(("oc", t0), two, one)
    if t0 == 7:   # the corrections do matter there: the same chain from step 0 ends elsewhere
        assert not np.array_equal(one["params"], _fused("oc", 0)["params"])


def test_two_launch_chain_through_a_kl_stop_and_the_calls_after_it():
    """target_kl = 1e-12: the first minibatch is on-policy (approx_kl == 0) and steps, the second stops the call.  A stopped call leaves
    what the fused path leaves (zeros in the later statistics rows, opt_step = t0 + 1); the next call stops at once (the buffer is no
    longer on-policy); a third with the KL test lifted steps on from t0 + 1 -- with a table kept from an earlier call, or a base
    other than the counter, its corrections would be those of other steps."""
    t0 = 7
    states = []
    for exclusive in (False, True):
        model = _model("oc", exclusive, t0, target_kl=1e-12)
        per_call = []
        for call in range(3):
            if call == 2:
                model.target_kl = None
            model.train()
            st = _state(model)
            st["stats"] = model.last_train_stats.copy()
            per_call.append(st)
        states.append(per_call)
    two, one = states
    st = one[0]["stats"]
    print("first call: approx_kl of minibatch 0 = %.3g, of minibatch 1 = %.3g, applied = %s" % (st[0, 4], st[1, 4], st[:, 7].tolist()))
    assert st[0, 4] == 0.0 and st[0, 7] == 1 and (st[1:, 7] == 0).all() and st[1, 4] > 1.5e-12
    assert (st[2:] == 0).all()                                    # minibatches after the stop do nothing
    assert one[0]["opt_step"] == t0 + 1
    assert one[1]["opt_step"] == t0 + 1 and (one[1]["stats"][:, 7] == 0).all()
    assert one[2]["opt_step"] == t0 + 1 + _n_minibatches("oc")
    for call in range(3):
        _assert_same(("call", call), two[call], one[call])


def test_captured_train_replayed_is_bitwise_the_eager_calls():
    """train() captured once into a graph and replayed three times (what IterationGraph does with whole iterations) against three
    eager calls: the table is written by a launch inside the graph, from the step counter as every replay finds it"""
    from pantheonrl_amd import _native as nat
    t0, calls = 7, 3
    eager = _model("oc", False, t0)
    want = []
    for _ in range(calls):
        eager.permutation_seed = 5          # the graph keeps the seed of its capture: the same order in every call
        eager.train()
        st = _state(eager)
        st["stats"] = eager.last_train_stats.copy()
        want.append(st)
    model = _model("oc", False, t0)
    pol = model.policy
    start = (pol.params.clone(), pol.adam_m.clone(), pol.adam_v.clone())
    stream = th.cuda.Stream()
    got = []
    with th.cuda.stream(stream):
        model.permutation_seed = 5
        model.train()                       # outside capture: sizes the workspace
        pol.params.copy_(start[0])
        pol.adam_m.copy_(start[1])
        pol.adam_v.copy_(start[2])
        pol.opt_step.fill_(t0)
        stream.synchronize()
        model.permutation_seed = 5
        lib, h = pol.ctx.lib, pol.ctx.handle
        pol._bind()
        nat.check(lib.ph_graph_begin(h))
        try:
            model.train(sync_stats=False)
        finally:
            gid = C.c_int(-1)
            nat.check(lib.ph_graph_end(h, C.byref(gid)))
        for _ in range(calls):
            nat.check(lib.ph_graph_launch(h, gid.value))
            stream.synchronize()
            st = _state(model)
            st["stats"] = model._stats_dev.cpu().numpy().copy()
            got.append(st)
    assert want[-1]["opt_step"] == t0 + calls * _n_minibatches("oc")
    for call in range(calls):
        _assert_same(("replay", call), got[call], want[call])
