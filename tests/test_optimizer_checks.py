"""CPU: what makes tests/test_gpu_optimizer.py trustworthy.  The checker's Adam state in flat layout (tests/helpers.py), the float64
statement of one clip + Adam step and its derived error bound (tests/optimizer_bound.py), the proof on the checker alone that the
bounds reject wrong optimizers, and that they are tight enough to mean something.  Also the scenario builders the GPU module shares."""
import copy

import numpy as np
import pytest
import torch as th

from oracle import sb3_oracle as orc
from tests import arch_oracle as A
from tests import helpers as H
from tests import optimizer_bound as OB
from tests import adapmult_cases as AM
from tests import modular_cases as M
from tests.optimizer_cases import (BC_ADAM, BC_SCENARIOS, MOD, SPECS, bc_checker, bc_data_gradient, bc_flat_grads,
                                   bc_scenario_state, chain_allowance, modular_recorded_steps, modular_unit, modular_unit_run,
                                   ppo_unit)


# ---- shared builders ---------------------------------------------------------------------------------------------------------------
def modular_replay(u, grads, lives, max_grad_norm, variant="right"):
    """the unit in float64 from the recorded gradients.  variant "shared-step": one step count (opt_step) for every entry;
    "untouched": a value side whose partner is not the one being trained is skipped instead of stepped with g = 0."""
    p, m, v = u["p0"].astype(np.float64), u["m0"].astype(np.float64), u["v0"].astype(np.float64)
    t = u["steps"].astype(np.float64).copy()
    shared = float(MOD["t0"])
    for k, (g, live) in enumerate(zip(grads, lives)):
        if variant == "untouched":
            live = live & ((u["label"] < 0) | (u["label"] == k))
        t_use = np.full_like(t, shared) if variant == "shared-step" else t
        p, m, v, _, _ = OB.adam_step_f64(p, m, v, t_use, g, max_grad_norm, eps=1e-5, live=live)
        t = np.where(live, t + 1, t)
        shared += 1
    return p, m, v


# ---- 1. flat_adam_state / load_flat_adam_state ----------------------------------------------------------------------------------------
def _case(kind):
    """-> (checker, optimizer, backward(), flat gradient (), flat_fn)"""
    if kind in ("mlp", "gaussian", "adapmult", "arch"):
        name = {"mlp": "overcooked", "gaussian": "gauss5", "adapmult": "adap_small", "arch": "quad16"}[kind]
        orac = (AM._oracle(name, seed=2) if kind == "adapmult" else A.oracle_policy(name, (96, 160, 32), seed=2) if kind == "arch"
                else H.oracle_policy(name, seed=2))
        ob = H.filled_oracle_buffer(name, orac, 8, 8, seed=2)
        mb = next(iter(ob.get(64, np.arange(64))))

        def backward():
            orc.ppo_minibatch_loss(orac, mb, orc.PPOHyper(ent_coef=0.01))[0].backward()
        return orac, orac.optimizer, backward, orac.flat_grads, None
    if kind in ("modular", "modular-baseline"):
        kw = {"baseline": True} if kind == "modular-baseline" else {}
        orac = M._oracle("mod_small", 3, seed=2, **kw)
        mb = next(iter(M._filled(orac, "mod_small", 1, 8, 8, seed=2).get(64, np.arange(64))))

        def backward():
            orc.modular_minibatch_loss(orac, mb, orc.PPOHyper(), 1, 0.3)[0].backward()
        return orac, orac.optimizer, backward, lambda: M._flat(orac, grads=True), M._flat
    orac, obs, acts = bc_checker("overcooked", 40)
    opt = th.optim.Adam(orac.parameters())

    def backward():
        orc.bc_loss(orac, th.as_tensor(obs), th.as_tensor(acts), 1e-3, 1e-3)[0].backward()
    return orac, opt, backward, lambda: bc_flat_grads(orac), None


KINDS = ["mlp", "gaussian", "adapmult", "arch", "modular", "modular-baseline", "bc"]


@pytest.mark.parametrize("kind", KINDS)
def test_flat_adam_state_round_trips_and_has_the_layout_of_flat_grads(kind):
    orac, opt, backward, flat_grads, flat_fn = _case(kind)
    flat = (flat_fn(orac) if flat_fn else orac.flat_params())
    P = flat.size
    m, v, steps = H.flat_adam_state(orac, opt, flat_fn)
    assert m.shape == v.shape == steps.shape == (P,) and not m.any() and not v.any() and not steps.any()     # no state yet
    # the layout: after one step from zero state without clipping m = (1 - beta1) g, v = (1 - beta2) g^2, entry by entry
    backward()
    g = np.asarray(flat_grads(), np.float64)
    if kind != "bc":
        th.nn.utils.clip_grad_norm_(orac.parameters(), 1e9)
    opt.step()
    m, v, steps = H.flat_adam_state(orac, opt, flat_fn)
    assert np.abs(g).max() > 0
    assert (np.abs(m - 0.1 * g) <= OB._ulp32(0.1 * g)).all() and (np.abs(v - 0.001 * g * g) <= 4 * OB._ulp32(0.001 * g * g)).all()
    reached = np.concatenate([np.full(p.numel(), p.grad is not None) for p in H._flat_layout(orac, flat_fn)[0]])[
        H._flat_layout(orac, flat_fn)[1]]
    assert np.array_equal(steps, reached.astype(np.int64))
    if kind == "modular":       # the value sides of the partners that were not trained have neither gradient nor state
        label = M._value_side(orac)
        assert not reached[(label == 0) | (label == 2)].any() and reached[label == 1].all() and reached[label < 0].all()
    # the round trip, bit for bit, with a step count per parameter tensor
    rng = np.random.default_rng(0)
    m1 = rng.standard_normal(P).astype(np.float32)
    v1 = (rng.standard_normal(P) ** 2).astype(np.float32)
    params, idx = H._flat_layout(orac, flat_fn)
    per_param = np.concatenate([np.full(p.numel(), 3 + i, np.int64) for i, p in enumerate(params)])[idx]
    if flat_fn is None and kind != "bc":
        assert np.array_equal(np.sort(idx), np.arange(P))        # a permutation: every parameter entry exactly once
    H.load_flat_adam_state(orac, m1, v1, per_param, opt, flat_fn)
    m2, v2, s2 = H.flat_adam_state(orac, opt, flat_fn)
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2) and np.array_equal(per_param, s2)
    before = (flat_fn(orac) if flat_fn else orac.flat_params()).copy()
    opt.zero_grad(set_to_none=False)
    backward()
    opt.step()                                                    # ... and the optimizer continues from it
    _, _, s3 = H.flat_adam_state(orac, opt, flat_fn)
    assert np.array_equal(s3, per_param + 1)
    assert not np.array_equal(before, flat_fn(orac) if flat_fn else orac.flat_params())
    H.load_flat_adam_state(orac, 0 * m1, 0 * v1, 0, opt, flat_fn)       # step 0: no state at all
    assert all(len(opt.state.get(p, {})) == 0 for p in params)


# ---- 2. adam_step_f64 is torch's step -------------------------------------------------------------------------------------------------
ROUNDING_ONLY = dict(e_g_abs=0.0, e_g_rel=0.0, e_n_abs=0.0, e_n_rel=0.0)


@pytest.mark.parametrize("name,T,E", SPECS)
def test_adam_step_f64_is_the_float32_checkers_step_up_to_rounding(name, T, E):
    """every scenario: the float32 torch checker against adam_step_f64 on the checker's own gradient and norm, within the rounding
    terms of one_step_bounds alone (no gradient tolerance, no norm tolerance)"""
    base, ob, run, g_ref, n_ref = ppo_unit(name, T, E)
    for sc in OB.SCENARIOS:
        orac = copy.deepcopy(base)
        p0 = orac.flat_params()
        m0, v0, t0, max_norm, lr = OB.scenario_state(sc, p0.size, n_ref, seed=1)
        H.load_flat_adam_state(orac, m0, v0, t0)
        stats = run(orac, max_norm, lr)
        assert stats[0]["grad_norm"] == n_ref            # the same gradient: float32, bit for bit
        b = OB.one_step_bounds(p0, m0, v0, t0, g_ref, max_norm, lr=lr, norm=n_ref, **ROUNDING_ONLY)
        m, v, steps = H.flat_adam_state(orac)
        assert (steps == t0 + 1).all()
        failed = OB.check_one_step(dict(m=m, v=v, p=orac.flat_params()), b, b, (name, sc, "rounding only"))
        assert not failed, (name, sc, failed)
        clipped = max_norm / (n_ref + 1e-6) < 1
        assert clipped == (sc not in ("resumed-unclipped", "never")), (sc, max_norm, n_ref)


def test_adam_step_f64_with_per_entry_steps_is_the_modular_checkers_step():
    """one step (partner 0) from the Modular unit's loaded state: module 1's value side steps with g = 0 and its own count (4 -> 5),
    module 2's value side has no gradient tensor and is skipped"""
    u = modular_unit()
    orac, label = u["orac"], u["label"]
    (g,), (live,), (norm,) = modular_recorded_steps(u, 0.5, n=1)
    assert np.array_equal(live, label != 2)
    assert not g[label == 1].any() and not g[label == 2].any() and np.abs(g[label == 0]).max() > 0
    b = OB.one_step_bounds(u["p0"], u["m0"], u["v0"], u["steps"], g, 0.5, norm=norm, **ROUNDING_ONLY)
    m, v, steps = M._flat_adam_state(orac)
    assert np.array_equal(steps, np.where(label == 2, 0, u["steps"] + 1))
    assert not OB.check_one_step(dict(m=m, v=v, p=M._flat(orac)), b, b, ("modular", "per-entry steps"))
    untouched = label == 2
    assert np.array_equal(M._flat(orac)[untouched], u["p0"][untouched]) and not m[untouched].any() and not v[untouched].any()
    moved = label == 1                                   # decayed and moved by its momentum
    assert (np.abs(m[moved] - 0.9 * u["m0"][moved]) <= 4 * OB._ulp32(u["m0"][moved])).all()
    assert np.abs(M._flat(orac)[moved] - u["p0"][moved]).max() > 1e-5


@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_adam_step_f64_is_the_bc_checkers_step(l2):
    """BC: no clip, eps 1e-8, lr 1e-3, the L2 term enters the gradient as l2 * p"""
    base, obs, acts = bc_checker("overcooked", 77)
    g_data = bc_data_gradient(base, obs, acts)
    for sc in BC_SCENARIOS:
        orac = copy.deepcopy(base)
        opt = th.optim.Adam(orac.parameters())
        p0 = orac.flat_params()
        m0, v0, t0 = bc_scenario_state(sc, p0.size, seed=2)
        H.load_flat_adam_state(orac, m0, v0, t0, opt)
        orc.bc_train(orac, obs, acts, [np.arange(77)], 200, ent_weight=1e-3, l2_weight=l2, optimizer=opt)
        # autograd adds the two gradient paths in float32: one rounding of the data gradient's size, as a relative term
        b = OB.one_step_bounds(p0, m0, v0, t0, g_data, 0.0, l2=l2, e_g_abs=0.0, e_g_rel=2.0 ** -23, e_n_abs=0.0, e_n_rel=0.0, **BC_ADAM)
        m, v, steps = H.flat_adam_state(orac, opt)
        assert (steps == t0 + 1).all()
        assert not OB.check_one_step(dict(m=m, v=v, p=orac.flat_params()), b, b, ("bc", sc, l2))


# ---- 3. the bounds reject wrong optimizers, and accept a right one whose inputs are at the edge of their tolerances ----------------
WRONG = {"coef x 1.02": dict(coef_scale=1.02), "no clamp at 1": dict(clamp=False), "t0 for t0+1": dict(stale_step=True),
         "eps 1e-8": dict(eps=1e-8), "unclipped g into m": dict(raw_into_m=True), "unclipped g into v": dict(raw_into_v=True)}


def _rejected(wrong, b):
    return "".join(k for k in ("m", "v", "p") if not (np.abs(wrong[k] - b[k]) <= b["e_" + k]).all())


def _informative(b, p0):
    """share of the entries whose parameter bound is below 10 % of that entry's own update"""
    return float((b["e_p"] < 0.1 * np.abs(b["p"] - np.asarray(p0, np.float64))).mean())


@pytest.mark.parametrize("name,T,E", SPECS)
def test_the_bounds_reject_every_wrong_optimizer_and_are_worth_something(name, T, E):
    orac, ob, run, g_ref, n_ref = ppo_unit(name, T, E)
    p0 = orac.flat_params()
    seen = {w: [] for w in WRONG}
    print("\n%s: gradient norm %.4g, %d parameters\n%-18s %-11s " % (name, n_ref, p0.size, "scenario", "informative")
          + " | ".join("%-18s" % w for w in WRONG))
    rng = np.random.default_rng(3)
    for sc in OB.SCENARIOS:
        m0, v0, t0, max_norm, lr = OB.scenario_state(sc, p0.size, n_ref, seed=1)
        b = OB.one_step_bounds(p0, m0, v0, t0, g_ref, max_norm, lr=lr)
        cells = []
        for w, kw in WRONG.items():
            if w == "t0 for t0+1" and t0 == 0:
                cells.append("n/a")
                continue
            args = dict(dict(lr=lr, eps=1e-5), **kw)
            p, m, v, _, _ = OB.adam_step_f64(p0, m0, v0, t0, g_ref, max_norm, **args)
            cells.append(" ".join(_rejected(dict(p=p, m=m, v=v), b)) or "-")
            if cells[-1] != "-":
                seen[w].append(sc)
        info = _informative(b, p0)
        print("%-18s %-11.2f " % (sc, info) + " | ".join("%-18s" % c for c in cells))
        # a right optimizer fed a gradient and a norm at 0.9 of their tolerances passes: the bounds are not too tight
        e_g = 0.9 * (OB.E_G_ABS + OB.E_G_REL * np.abs(g_ref).max())
        for sign in (-1.0, 1.0):
            g_edge = g_ref + e_g * rng.choice([-1.0, 1.0], size=g_ref.size)
            n_edge = n_ref + sign * 0.9 * (OB.E_N_ABS + OB.E_N_REL * n_ref)
            p, m, v, _, _ = OB.adam_step_f64(p0, m0, v0, t0, g_edge, max_norm, lr=lr, norm=n_edge)
            assert _rejected(dict(p=p, m=m, v=v), b) == "", (name, sc, sign)
        # the bound is worth something: a condition on the scenario's inputs (change the state scale, not the 80 %)
        if sc != "fresh":
            assert info >= 0.8, (name, sc, info)
    for w, where in seen.items():
        assert where, (name, w, "is rejected in no scenario")
    assert "resumed-unclipped" in seen["no clamp at 1"] and "never" in seen["no clamp at 1"]
    assert "fresh" not in seen["no clamp at 1"] and "fresh" not in seen["eps 1e-8"]      # what today's single case cannot see


def test_the_chain_comparison_rejects_the_wrong_modular_optimizers():
    """the Modular unit (three steps) on the checker alone: the float64 replay of the recorded gradients is the checker's chain, and
    the two wrong optimizers -- one shared step count for every entry; a value side whose partner is not being trained left untouched
    instead of decayed and moved by its momentum -- fall outside the chain allowance (max(4 d, 4e-4) of the largest entry; for the
    parameters: of the largest entry of the update p - p0).  t0 = 7 and the 1e-3 state scale of the other scenarios are enough:
    nothing had to be lowered or raised."""
    for sc, max_norm in (("resumed-clipped", 0.5), ("resumed-unclipped", None)):
        if max_norm is None:
            norms = modular_recorded_steps(modular_unit(), 1e9)[2]
            max_norm = float(np.float32(1.25 * max(norms)))
        u = modular_unit()
        grads, lives, norms = modular_recorded_steps(u, max_norm)
        assert all((n > max_norm) == (sc == "resumed-clipped") for n in norms), (sc, norms, max_norm)
        again = modular_unit()                                   # the written-out loop is modular_train
        M._load_flat_adam_state(again["orac"], u["m0"], u["v0"], u["steps"])
        modular_unit_run(again["orac"], again["bufs"], max_norm)
        assert np.array_equal(M._flat(again["orac"]), M._flat(u["orac"]))
        m32, v32, steps = M._flat_adam_state(u["orac"])
        label = u["label"]
        assert np.array_equal(steps, np.where(label == 1, 7, np.where(label == 2, 1, 10)))
        ref = dict(zip("pmv", modular_replay(u, grads, lives, max_norm)))
        got32 = dict(p=M._flat(u["orac"]).astype(np.float64), m=m32.astype(np.float64), v=v32.astype(np.float64))
        allow = {}
        for k in "mv":
            allow[k], d = chain_allowance(got32[k], ref[k])
            print(sc, k, "checker f32 vs f64 replay d = %.3g" % d)
        allow["p"], d = chain_allowance(got32["p"] - u["p0"], ref["p"] - u["p0"])
        print(sc, "update: d = %.3g, allowance %.3g" % (d, allow["p"]))
        assert d < 1e-4                                          # the replay IS the checker's chain
        for variant in ("shared-step", "untouched"):
            wrong = dict(zip("pmv", modular_replay(u, grads, lives, max_norm, variant)))
            rejected = "".join(k for k in "mvp" if np.abs(wrong[k] - got32[k]).max() > allow[k])
            print(sc, variant, "rejected through", rejected, {k: "%.3g / %.3g" % (np.abs(wrong[k] - got32[k]).max(), allow[k]) for k in "mvp"})
            assert rejected, (sc, variant)
            assert ("m" in rejected) == (variant == "untouched")       # a wrong step count leaves the moments alone


def test_the_bc_bounds_reject_the_other_eps():
    """BC runs Adam with torch's default eps 1e-8; PPO's 1e-5 in its place must not pass"""
    base, obs, acts = bc_checker("overcooked", 77)
    g = bc_data_gradient(base, obs, acts)
    p0 = base.flat_params()
    seen = []
    for l2 in (0.0, 1e-3):
        for sc in BC_SCENARIOS:
            m0, v0, t0 = bc_scenario_state(sc, p0.size, seed=2)
            b = OB.one_step_bounds(p0, m0, v0, t0, g, 0.0, l2=l2, **BC_ADAM)
            p, m, v, _, _ = OB.adam_step_f64(p0, m0, v0, t0, g, 0.0, **dict(BC_ADAM, eps=1e-5, l2=l2))
            r = _rejected(dict(p=p, m=m, v=v), b)
            info = _informative(b, p0)
            print("bc l2=%g %-8s informative %.2f  eps 1e-5 for 1e-8 rejected through: %s" % (l2, sc, info, r or "-"))
            if r:
                seen.append((l2, sc))
            if sc != "fresh":
                assert info >= 0.8, (l2, sc, info)
    assert seen
