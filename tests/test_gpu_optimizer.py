"""-m gpu: every hand-written copy of "clip the gradient by its norm, then take an Adam step" against the checker, ONE optimizer
step at a time from a LOADED optimizer state: adam_scalars / adam_apply of csrc/ph_step.h through ppo_adam_kernel (two launches) and
ppo_step_kernel (one launch, exclusive device) and each of their call sites (PPO, Gaussian heads, net_arch towers, ADAP, ADAP-MULT,
ph_ppo_train_multi, the handle ABI), modular_adam_kernel, and the Adam inside both BC kernels.

The unit: n_epochs = 1, batch_size = T * E, so train() does exactly one reduce, clip and Adam.  Before it the same (p0, m0, v0, t0) is
loaded into checker and device; after it opt_step (exact), adam_m, adam_v, the parameters and the gradient norm are compared with the
checker's, every entry, under tests/optimizer_bound.one_step_bounds -- derived from the gradient tolerance (1e-6 + 2e-4 max|g|) and
the norm tolerance (1e-5 + 2e-4 n) the suite already enforces, not measured.  tests/test_optimizer_checks.py shows on the CPU that
these bounds reject a clip coefficient wrong by 2 %, a missing clamp at 1, a step count off by one, the wrong eps and an unclipped
gradient in either moment, and that they are below 10 % of the update for at least 80 % of the entries.  Scenarios: DESIGN.md section 3.

Every comparison prints its largest error beside its bound."""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from oracle import sb3_oracle as orc
from tests import arch_oracle as A
from tests import helpers as H
from tests import optimizer_bound as OB
from tests import adapmult_cases as AM
from tests import modular_cases as M
from tests import optimizer_cases as OC

pytestmark = pytest.mark.gpu

SHORT = ("fresh", "resumed-clipped", "resumed-unclipped")


def _env(name, obs_space=None):
    obs_s, act_s = H.CONFIGS[name]
    return type("E", (), dict(observation_space=obs_space or H.to_space(obs_s), action_space=H.to_space(act_s),
                             _is_dummy_space_env=True))()


def _mismatches(pol):
    from pantheonrl_amd import _native as nat
    n = C.c_int(-2)
    nat.check(pol.ctx.lib.ph_debug_weight_image_mismatches(pol.ctx.handle, C.byref(pol.spec), pol.params.data_ptr(), C.byref(n)))
    return n.value


@functools.lru_cache(maxsize=None)
def _unit(name, T, E):
    return OC.ppo_unit(name, T, E)


def _set_hyper(model, sc, max_norm, lr):
    model.max_grad_norm = max_norm
    if sc == "lr":      # the schedule reaches the step: hyper() evaluates it at the current progress
        model.learning_rate = lambda p: 1e-3 * p
        model._current_progress_remaining = 0.25
    else:
        model.learning_rate = lr


def _compare(where, pol, orac, b, t0, norm_dev, norm_ref, flat=None, state=None):
    """device state after the step against the checker's, every entry, under the bounds b"""
    m_ref, v_ref, steps = state(orac) if state else H.flat_adam_state(orac)
    p_ref = flat(orac) if flat else orac.flat_params()
    m, v, step = H.read_device_adam_state(pol)
    assert step == t0 + 1 and (steps == t0 + 1).all(), (where, step, t0)
    print(where, "gradient norm: device %.7g checker %.7g, error %.3g (bound %.3g)" % (norm_dev, norm_ref, abs(norm_dev - norm_ref), b["e_n"]))
    assert abs(norm_dev - norm_ref) <= b["e_n"], (where, norm_dev, norm_ref)
    failed = OB.check_one_step(dict(m=m, v=v, p=pol.get_flat_params()), dict(m=m_ref, v=v_ref, p=p_ref), b, where)
    assert not failed, (where, failed)


def _one_step(where, base, run, g_ref, n_ref, model, sc, train, ob, seed=1):
    """load the scenario's state into a fresh copy of the checker and into the device, one step on each, compare"""
    orac = copy.deepcopy(base)
    pol = model.policy
    p0 = orac.flat_params()
    m0, v0, t0, max_norm, lr = OB.scenario_state(sc, p0.size, n_ref, seed=seed)
    H.load_flat_adam_state(orac, m0, v0, t0)
    pol.set_flat_params(p0)
    H.load_device_adam_state(pol, m0, v0, t0)
    _set_hyper(model, sc, max_norm, lr)
    H.upload_buffer(model.rollout_buffer, ob)
    train()
    th.cuda.synchronize()
    st = model.last_train_stats
    assert st.shape[0] == 1 and st[0, 7] == 1
    ref = run(orac, max_norm, lr)
    b = OB.one_step_bounds(p0, m0, v0, t0, g_ref, max_norm, lr=lr)
    assert (b["coef"] < 1) == (sc not in ("resumed-unclipped", "never")), (where, b["coef"])
    _compare(where, pol, orac, b, t0, float(st[0, 6]), ref[0]["grad_norm"])
    return orac, (p0, m0, v0, t0, max_norm, lr), b


# ---- PPO: both step paths, every scenario ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", OB.SCENARIOS)
@pytest.mark.parametrize("exclusive", [False, True], ids=["two-launch", "one-launch"])
@pytest.mark.parametrize("name,T,E", OC.SPECS)
def test_ppo_one_step_from_a_loaded_state(name, T, E, exclusive, sc):
    from pantheonrl_amd.ppo import PPO
    base, ob, run, g_ref, n_ref = _unit(name, T, E)
    model = PPO("MlpPolicy", _env(name), n_steps=T, n_envs=E, batch_size=T * E, n_epochs=1, seed=0)
    assert model.policy.gemm_mode == 2
    model.policy.ctx.set_exclusive_device(exclusive)
    _one_step((name, "one-launch" if exclusive else "two-launch", sc), base, run, g_ref, n_ref, model, sc,
              lambda: model.train(perms=np.arange(T * E)[None]), ob)
    n = _mismatches(model.policy)       # mode 2 rewrites the bf16 weight image in the Adam step: it must be the new parameters'
    print(name, "weight image mismatches", n)
    assert n == 0 if name == "overcooked" else n in (0, -1), n


@pytest.mark.parametrize("sc", ["resumed-clipped", "resumed-unclipped"])
def test_ppo_one_step_exact_float32_products(sc):
    from pantheonrl_amd.ppo import PPO
    name, T, E = OC.SPECS[0]
    base, ob, run, g_ref, n_ref = _unit(name, T, E)
    model = PPO("MlpPolicy", _env(name), n_steps=T, n_envs=E, batch_size=T * E, n_epochs=1, seed=0)
    model.policy.gemm_mode = 0
    _one_step((name, "gemm_mode 0", sc), base, run, g_ref, n_ref, model, sc, lambda: model.train(perms=np.arange(T * E)[None]), ob)


# ---- the other call sites of ph_step.h: state, learning rate and max norm must arrive ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family(kind):
    """-> (name, T, E, unit, model factory, train(model))"""
    from pantheonrl_amd.ppo import PPO
    T, E = 16, 8
    N = T * E
    perms = np.arange(N)[None]
    if kind == "gaussian":
        name = "gauss5"
        unit = OC.ppo_unit(name, T, E, hp=orc.PPOHyper(ent_coef=0.01))
        make = lambda: PPO("MlpPolicy", _env(name), n_steps=T, n_envs=E, batch_size=N, n_epochs=1, ent_coef=0.01, seed=0)   # noqa: E731
        return name, unit, make, lambda model: model.train(perms=perms)
    if kind == "net_arch":
        name, arch = "quad16", (96, 160, 32)
        unit = OC.ppo_unit(name, T, E, make_oracle=lambda n, seed: A.oracle_policy(n, arch, seed=seed))
        make = lambda: PPO("MlpPolicy", A.space_env(name), n_steps=T, n_envs=E, batch_size=N, n_epochs=1, seed=0,     # noqa: E731
                           policy_kwargs=A.kwargs_of(arch))
        return name, unit, make, lambda model: model.train(perms=perms)
    # ADAP / ADAP-MULT: the context term on, its samples teacher-forced the way the train tests of those families do it
    from pantheonrl_amd import spaces as sp
    from pantheonrl_amd.adap import ADAP
    name, cs, n_ctx, n_states, coef = "adap_small", 3, 5, 32, 0.5
    rng = np.random.default_rng(31)
    sidx = rng.permutation(N)[:n_states].astype(np.int32)[None]
    ctxs = orc.adap_sample_contexts("l2", cs, n_ctx, rng.random((n_ctx, cs)))[None]
    term = orc.AdapTerm(cs, coef, [sidx[0]], ctxs)
    unit = OC.ppo_unit(name, T, E, adap=term, make_oracle=(lambda n, seed: AM._oracle(n, seed=seed)) if kind == "adapmult" else None)
    obs_s = H.CONFIGS[name][0]
    env = _env(name, sp.Box(-np.inf, np.inf, (obs_s.dim - cs,)))
    make = lambda: ADAP("AdapPolicyMult" if kind == "adapmult" else "AdapPolicy", env, n_steps=T, n_envs=E, batch_size=N,   # noqa: E731
                        n_epochs=1, seed=0, context_loss_coeff=coef, context_size=cs, num_context_samples=n_ctx,
                        num_state_samples=n_states)
    return name, unit, make, lambda model: model.train(perms=perms, state_idx=sidx, contexts=ctxs)


@pytest.mark.parametrize("sc", SHORT)
@pytest.mark.parametrize("kind", ["gaussian", "net_arch", "adap", "adapmult"])
def test_every_call_site_of_the_shared_step_passes_state_rate_and_norm_through(kind, sc):
    name, (base, ob, run, g_ref, n_ref), make, train = _family(kind)
    model = make()
    if kind == "net_arch":
        from pantheonrl_amd.ppo import ArchActorCriticPolicy
        assert type(model.policy) is ArchActorCriticPolicy
    if kind == "adapmult":
        from pantheonrl_amd.adap import AdapPolicyMult
        assert isinstance(model.policy, AdapPolicyMult)
    orac, _, _ = _one_step((kind, name, sc), base, run, g_ref, n_ref, model, sc, lambda: train(model), ob)
    if kind in ("adap", "adapmult"):     # the term was in the gradient: the same step without it ends somewhere else
        plain = copy.deepcopy(base)
        orc.ppo_train(plain, ob, H.unit_hyper(orc.PPOHyper(), ob.T * ob.E, 1e9), [np.arange(ob.T * ob.E)])
        assert np.abs(plain.flat_grads() - g_ref).max() > 1e-5


def test_two_learners_in_one_call_each_equal_their_own_checker():
    """ph_ppo_train_multi: different loaded states and different max_grad_norm, one learner clips and the other does not"""
    from pantheonrl_amd.ppo import PPO
    units = [_unit(*OC.SPECS[0]), OC.ppo_unit("overcooked", 16, 8, seed=22)]
    cases = [("resumed-clipped", 1), ("resumed-unclipped", 2)]
    models, streams, loaded = [], [th.cuda.Stream(), th.cuda.Stream()], []
    for (base, ob, run, g_ref, n_ref), (sc, seed), stream in zip(units, cases, streams):
        model = PPO("MlpPolicy", _env("overcooked"), n_steps=ob.T, n_envs=ob.E, batch_size=ob.T * ob.E, n_epochs=1, seed=seed)
        orac = copy.deepcopy(base)
        p0 = orac.flat_params()
        m0, v0, t0, max_norm, lr = OB.scenario_state(sc, p0.size, n_ref, seed=seed)
        H.load_flat_adam_state(orac, m0, v0, t0)
        model.policy.set_flat_params(p0)
        H.load_device_adam_state(model.policy, m0, v0, t0)
        _set_hyper(model, sc, max_norm, lr)
        H.upload_buffer(model.rollout_buffer, ob)
        with th.cuda.stream(stream):
            model.policy._bind()
        models.append(model)
        loaded.append((orac, p0, m0, v0, t0, max_norm, lr))
    th.cuda.synchronize()
    PPO.train_joint(models)
    th.cuda.synchronize()
    for (base, ob, run, g_ref, n_ref), (sc, _), model, (orac, p0, m0, v0, t0, max_norm, lr) in zip(units, cases, models, loaded):
        ref = run(orac, max_norm, lr)
        b = OB.one_step_bounds(p0, m0, v0, t0, g_ref, max_norm, lr=lr)
        assert (b["coef"] < 1) == (sc == "resumed-clipped")
        st = model._stats_dev.cpu().numpy()
        assert st.shape[0] == 1 and st[0, 7] == 1
        _compare(("multi", sc), model.policy, orac, b, t0, float(st[0, 6]), ref[0]["grad_norm"])


# ---- the handle ABI ----------------------------------------------------------------------------------------------------------------------
def test_handle_abi_optimizer_state_round_trips_and_steps():
    """ph_agent_set_optimizer(m0, v0, 7), ph_agent_get_optimizer returns the same bits, one ph_agent_train step equals the checker"""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd import spaces as sp
    name, T, E = OC.SPECS[0]
    base, ob, run, g_ref, n_ref = _unit(name, T, E)
    lib = nat.load()
    obs_s, act_s = H.CONFIGS[name]
    spec = sp.make_spec(H.to_space(obs_s), H.to_space(act_s))
    h = C.c_void_p()
    assert lib.ph_agent_create(0, C.byref(spec), E, T, 0.99, 0.95, 123, C.byref(h)) == 0, lib.ph_agent_last_error()
    try:
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
        arr = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731
        orac = copy.deepcopy(base)
        p0 = orac.flat_params()
        sc = "resumed-clipped"
        m0, v0, t0, max_norm, lr = OB.scenario_state(sc, p0.size, n_ref, seed=1)
        H.load_flat_adam_state(orac, m0, v0, t0)
        assert lib.ph_agent_set_params(h, ptr(arr(p0))) == 0
        assert lib.ph_agent_set_optimizer(h, ptr(arr(m0)), ptr(arr(v0)), t0) == 0, lib.ph_agent_last_error()
        m, v, step = np.zeros_like(m0), np.zeros_like(v0), C.c_int(-1)
        assert lib.ph_agent_get_optimizer(h, ptr(m), ptr(v), C.byref(step)) == 0
        assert step.value == t0 and np.array_equal(m, m0) and np.array_equal(v, v0)
        keys = ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")
        keep = [arr(getattr(ob, k)) for k in keys]
        assert lib.ph_agent_import_buffer(h, *[ptr(a) for a in keep], T) == 0, lib.ph_agent_last_error()
        hp = nat.PhPpoHyper()
        hp.learning_rate, hp.clip_range, hp.clip_range_vf, hp.ent_coef, hp.vf_coef = lr, 0.2, -1.0, 0.0, 0.5
        hp.max_grad_norm, hp.target_kl, hp.normalize_advantage = max_norm, -1.0, 1
        hp.adam_beta1, hp.adam_beta2, hp.adam_eps = 0.9, 0.999, 1e-5
        perms = np.arange(T * E, dtype=np.int32)[None].copy()
        stats = np.zeros((1, nat.PH_NSTAT), np.float32)
        assert lib.ph_agent_train(h, C.byref(hp), 1, T * E, ptr(perms), 0, ptr(stats)) == 0, lib.ph_agent_last_error()
        ref = run(orac, max_norm, lr)
        p = np.zeros_like(p0)
        assert lib.ph_agent_get_params(h, ptr(p)) == 0 and lib.ph_agent_get_optimizer(h, ptr(m), ptr(v), C.byref(step)) == 0
        assert step.value == t0 + 1 and stats[0, 7] == 1
        b = OB.one_step_bounds(p0, m0, v0, t0, g_ref, max_norm, lr=lr)
        assert abs(stats[0, 6] - ref[0]["grad_norm"]) <= b["e_n"]
        m_ref, v_ref, _ = H.flat_adam_state(orac)
        assert not OB.check_one_step(dict(m=m, v=v, p=p), dict(m=m_ref, v=v_ref, p=orac.flat_params()), b, ("handle ABI", sc))
    finally:
        assert lib.ph_agent_destroy(h) == 0


# ---- a KL stop leaves the state alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclusive", [False, True], ids=["two-launch", "one-launch"])
def test_a_kl_stop_leaves_parameters_and_optimizer_state_bitwise_alone(exclusive):
    """the buffer comes from a perturbed copy of the policy, so the first minibatch's approx_kl is not 0; 1.5 * target_kl is HALF of
    the checker's approx_kl (no rounding tie): train() stops before its only step"""
    from pantheonrl_amd.ppo import PPO
    name, T, E = OC.SPECS[0]
    orac = H.oracle_policy(name, seed=OC.SEED)
    other = copy.deepcopy(orac)
    g = th.Generator().manual_seed(9)
    with th.no_grad():
        for p in other.parameters():
            p.add_(0.05 * th.randn(p.shape, generator=g))
    ob = H.filled_oracle_buffer(name, other, T, E, seed=OC.SEED)
    N = T * E
    kl = orc.ppo_train(copy.deepcopy(orac), ob, H.unit_hyper(orc.PPOHyper(), N, 0.5), [np.arange(N)])[0]["approx_kl"]
    assert kl > 1e-4, kl
    target_kl = kl / 3.0
    stopped = orc.ppo_train(copy.deepcopy(orac), ob, H.unit_hyper(orc.PPOHyper(target_kl=target_kl), N, 0.5), [np.arange(N)])
    assert stopped[0].get("stopped")
    model = PPO("MlpPolicy", _env(name), n_steps=T, n_envs=E, batch_size=N, n_epochs=1, target_kl=target_kl, seed=0)
    model.policy.ctx.set_exclusive_device(exclusive)
    p0 = orac.flat_params()
    m0, v0, t0, _, _ = OB.scenario_state("resumed-clipped", p0.size, 1.0, seed=1)
    model.policy.set_flat_params(p0)
    H.load_device_adam_state(model.policy, m0, v0, t0)
    H.upload_buffer(model.rollout_buffer, ob)
    model.train(perms=np.arange(N)[None])
    th.cuda.synchronize()
    st = model.last_train_stats
    print("approx_kl: device %.6g checker %.6g, threshold %.6g" % (st[0, 4], kl, 1.5 * target_kl))
    assert st[0, 7] == 0 and abs(st[0, 4] - kl) <= 3e-6 + 2e-4 * kl
    m, v, step = H.read_device_adam_state(model.policy)
    assert step == t0 and np.array_equal(m, m0) and np.array_equal(v, v0) and np.array_equal(model.policy.get_flat_params(), p0)


# ---- checkpoint, then step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ppo", "net_arch"])
def test_a_step_on_the_loaded_checkpoint_is_bitwise_the_step_on_the_original(kind, tmp_path):
    from pantheonrl_amd.ppo import PPO
    if kind == "ppo":
        name, T, E = OC.SPECS[0]
        base, ob, run, g_ref, n_ref = _unit(name, T, E)
        model = PPO("MlpPolicy", _env(name), n_steps=T, n_envs=E, batch_size=T * E, n_epochs=1, seed=0)
        train = lambda mdl: mdl.train(perms=np.arange(T * E)[None])     # noqa: E731
    else:
        name, (base, ob, run, g_ref, n_ref), make, train = _family("net_arch")
        model = make()
    sc = "resumed-clipped"
    p0 = base.flat_params()
    m0, v0, t0, max_norm, lr = OB.scenario_state(sc, p0.size, n_ref, seed=1)
    model.policy.set_flat_params(p0)
    H.load_device_adam_state(model.policy, m0, v0, t0)
    path = str(tmp_path / "ckpt")
    model.save(path)
    again = PPO.load(path)
    assert type(again.policy) is type(model.policy)
    m, v, step = H.read_device_adam_state(again.policy)
    assert step == t0 and np.array_equal(m, m0) and np.array_equal(v, v0) and np.array_equal(again.policy.get_flat_params(), p0)
    _one_step((kind, "original", sc), base, run, g_ref, n_ref, model, sc, lambda: train(model), ob)
    _one_step((kind, "loaded checkpoint", sc), base, run, g_ref, n_ref, again, sc, lambda: train(again), ob)
    # (_one_step loads the same state into both again: what differs between the two models is only that one was built by load())
    assert np.array_equal(again.policy.get_flat_params(), model.policy.get_flat_params())
    assert th.equal(again.policy.adam_m, model.policy.adam_m) and th.equal(again.policy.adam_v, model.policy.adam_v)
    # ... and a step straight from what load() restored, with nothing written in between
    fresh = PPO.load(path)
    _set_hyper(fresh, sc, max_norm, lr)
    H.upload_buffer(fresh.rollout_buffer, ob)
    train(fresh)
    th.cuda.synchronize()
    assert np.array_equal(fresh.policy.get_flat_params(), model.policy.get_flat_params())
    assert th.equal(fresh.policy.adam_m, model.policy.adam_m) and th.equal(fresh.policy.adam_v, model.policy.adam_v)
    assert int(fresh.policy.opt_step.item()) == t0 + 1


# ---- Modular: modular_adam_kernel, per-entry step counts -----------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ["resumed-clipped", "resumed-unclipped"])
def test_modular_three_steps_from_a_loaded_state_with_per_module_step_counts(sc):
    """ModularAlgorithm.train() always walks all K partners: the unit is one call, K = 3 steps (partner 0, 1, 2).  opt_step = 7,
    mod_first = [0, 3, -1]: module 0's value side has counted 7 steps, module 1's 4, module 2's joins at the third step of this call.
    Against the checker under the chain allowance (helpers.assert_chain_moments: max(4 d, 4e-4) of the largest entry, d measured on
    the checker float32 against float64); for the parameters the same rule on the update p - p0.
    tests/test_optimizer_checks.py shows that this comparison rejects one shared step count and an untouched value side."""
    c = OC.MOD
    if sc == "resumed-clipped":
        max_norm = 0.5
    else:
        max_norm = float(np.float32(1.25 * max(OC.modular_recorded_steps(OC.modular_unit(), 1e9)[2])))
    u = OC.modular_unit()
    orac, label = u["orac"], u["label"]
    o64, _ = H.double_copy(orac)                 # the float64 copy of the checker: same state, same buffers, same order
    M._load_flat_adam_state(o64, u["m0"], u["v0"], u["steps"])
    ref64 = H.chain64_state(o64, lambda o: OC.modular_unit_run(o, u["bufs"], max_norm), flat_fn=M._flat)
    p64 = M._flat(o64).astype(np.float64)
    model = M._algo(c["name"], c["K"], c["T"], c["E"], OC.modular_hp(max_norm), c["coef"])
    pol = model.policy
    pol.set_flat_params(u["p0"])
    H.load_device_adam_state(pol, u["m0"], u["v0"], c["t0"], mod_first=c["first"])
    for rb, ob in zip(model.rollout_buffer, u["bufs"]):
        H.upload_buffer(rb, ob)
    N = c["T"] * c["E"]
    model.train(perms=np.tile(np.arange(N), (c["K"], 1, 1)))
    th.cuda.synchronize()
    M._load_flat_adam_state(orac, u["m0"], u["v0"], u["steps"])
    ref = OC.modular_unit_run(orac, u["bufs"], max_norm)
    assert all((s["grad_norm"] > max_norm) == (sc == "resumed-clipped") for s in ref), ([s["grad_norm"] for s in ref], max_norm)
    assert int(pol.opt_step.item()) == 10 and list(pol.mod_first.cpu().numpy()) == [0, 3, 9]
    m32, v32, steps = M._flat_adam_state(orac)
    assert np.array_equal(steps, np.where(label == 1, 7, np.where(label == 2, 1, 10)))
    st = model.last_train_stats.reshape(-1, 8)
    for row, s in zip(st, ref):
        print(sc, "partner", s["partner"], "gradient norm: device %.7g checker %.7g" % (row[6], s["grad_norm"]))
        assert abs(row[6] - s["grad_norm"]) <= 1e-5 + 2e-4 * s["grad_norm"]
    m, v, _ = H.read_device_adam_state(pol)
    H.assert_chain_moments(m, v, (m32, v32, steps), ref64, ("modular", sc))
    upd32, upd64, upd = M._flat(orac).astype(np.float64) - u["p0"], p64 - u["p0"], pol.get_flat_params().astype(np.float64) - u["p0"]
    allowed, d = OC.chain_allowance(upd32, upd64)
    err = np.abs(upd - upd32).max()
    print(sc, "update: checker f32 vs f64 d = %.3g, device vs checker %.3g, allowed %.3g" % (d, err, allowed))
    assert err <= allowed, (sc, err, allowed)
    untouched = label == 2       # module 2's value side: no state before its own step, one step taken
    assert np.abs(m[untouched]).max() > 0


# ---- BC: the Adam inside bc_train_mfma_kernel (and, through the child process below, bc_train_kernel) ----------------------------------
@pytest.mark.parametrize("sc", OC.BC_SCENARIOS)
@pytest.mark.parametrize("l2", [0.0, 1e-3])
@pytest.mark.parametrize("N", [32, 77])
def test_bc_one_step_from_a_loaded_state(N, l2, sc):
    """BC: no clip, torch's default eps 1e-8, lr 1e-3, optional L2; batch_size 200 > N: the whole table is one batch, one step.
    The gradient tolerance e_g = 1e-6 + 2e-4 max|g| is BORROWED from the PPO gradient tests; BC's gradient itself is bounded per
    parameter block, on every shape class, in tests/test_gpu_bc_shapes.py."""
    from pantheonrl_amd.bc import BC
    from pantheonrl_amd.common import TransitionsMinimal
    name = "overcooked"
    orac, obs, acts = OC.bc_checker(name, N)
    g_data = OC.bc_data_gradient(orac, obs, acts)
    obs_s, act_s = H.CONFIGS[name]
    clone = BC(H.to_space(obs_s), H.to_space(act_s), expert_data=TransitionsMinimal(obs, acts[:, 0]), batch_size=200, l2_weight=l2)
    p0 = orac.flat_params()
    m0, v0, t0 = OC.bc_scenario_state(sc, p0.size, seed=2)
    opt = th.optim.Adam(orac.parameters())
    H.load_flat_adam_state(orac, m0, v0, t0, opt)
    clone.policy.set_flat_params(p0)
    H.load_device_adam_state(clone, m0, v0, t0)
    order = np.arange(N)[None]
    st = clone.train(n_epochs=1, orders=order)
    ref = orc.bc_train(orac, obs, acts, order, 200, ent_weight=1e-3, l2_weight=l2, optimizer=opt)
    assert st.shape[0] == len(ref) == 1
    b = OB.one_step_bounds(p0, m0, v0, t0, g_data, 0.0, l2=l2, **OC.BC_ADAM)
    m_ref, v_ref, steps = H.flat_adam_state(orac, opt)
    m, v, step = H.read_device_adam_state(clone)
    assert step == t0 + 1 and (steps == t0 + 1).all()
    where = ("bc", "PH_BC_MFMA=" + os.environ.get("PH_BC_MFMA", "default"), N, l2, sc)
    failed = OB.check_one_step(dict(m=m, v=v, p=clone.policy.get_flat_params()), dict(m=m_ref, v=v_ref, p=orac.flat_params()), b, where)
    assert not failed, (where, failed)


def test_bc_valu_kernel_passes_the_same_one_step_tests():
    """PH_BC_MFMA=0 routes every shape through bc_train_kernel; the switch is read once per process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_optimizer.py", "-x", "-q", "-s", "-m", "gpu", "-k",
                          "test_bc_one_step_from_a_loaded_state"], cwd=root, env={**os.environ, "PH_BC_MFMA": "0"},
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-6000:])
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "16 passed" in out.stdout, out.stdout[-500:]
