"""CPU: what makes tests/test_gpu_offpolicy.py trustworthy -- the inputs and the yardstick, proven on the checker alone.

For every case of tests/offpolicy_cases.py (a drifted copy of the checker fills the buffer, the checker is differentiated):
  * class shares: each of the eight classes of helpers.offpolicy_rows -- P1 (ratio > 1+c, adv > 0: clipped), P2 (ratio > 1+c,
    adv < 0: live), P3 (ratio < 1-c, adv > 0: live), P4 (ratio < 1-c, adv < 0: clipped), P5 (inside), V1 (v - old_v > c_vf),
    V2 (v - old_v < -c_vf), V3 (inside) -- holds >= 5 % of the minibatch and >= 3 rows;
  * edge rows (within 1e-4 s relative of a ratio bound, 1e-4 s of a value bound; s = max(1, w_last / 64)) are out of the minibatch,
    and were at most 2 % of the candidates -- a cap, not a measurement;
  * ratios stay within [0.05, 20]: the comparison is about branches, not about overflow;
  * wrong tails: the loss tail restated in torch with a detached gate reproduces the checker's own gradient when the gate is the
    right one, and each wrong gate (gate = inr; no gate; the tie value everywhere; the clipped and live quadrants swapped; the
    value `pass` mask dropped; the value clamp dropped) moves the gradient by >= 10x what the GPU test allows (1e-6 + 2e-4 max|g|);
    counting clip_fraction with clip_range_vf's range instead of clip_range's changes the count.
Which kernel each case lands on: the `kernel` field of the table (printed with each case)."""
import functools

import numpy as np
import pytest
import torch as th

from oracle import sb3_oracle as orc
from tests import helpers as H
from tests import offpolicy_cases as OC

IDS = [c.id for c in OC.CASES]


@functools.lru_cache(maxsize=None)
def _built(case_id):
    c = OC.BY_ID[case_id]
    b = OC.build(c)
    b["rows"] = OC.rows(c, H.double_copy(b["orac"])[0], b["ob"], b["idx"])
    return b


# ---- the helper and the table themselves -------------------------------------------------------------------------------------------
def test_stale_buffer_comes_from_a_drifted_copy_and_leaves_the_checker_alone():
    orac = H.oracle_policy("overcooked", seed=3)
    before = orac.flat_params()
    fresh = H.filled_oracle_buffer("overcooked", orac, 8, 4, seed=3)
    stale = H.stale_oracle_buffer("overcooked", orac, 8, 4, seed=3, drift=0.03)
    again = H.stale_oracle_buffer("overcooked", orac, 8, 4, seed=3, drift=0.03)
    assert np.array_equal(orac.flat_params(), before)
    assert np.array_equal(stale.log_probs, again.log_probs) and np.array_equal(stale.actions, again.actions)
    assert np.array_equal(stale.observations, fresh.observations)            # the same synthetic inputs ...
    assert not np.array_equal(stale.values, fresh.values)                   # ... seen by another policy
    hp = orc.PPOHyper(clip_range_vf=0.1)
    mb = OC.minibatch(fresh, np.arange(32))
    on = H.offpolicy_rows(H.double_copy(orac)[0], mb, hp)
    assert np.abs(on["ratio"] - 1).max() < 1e-5 and np.abs(on["dlt"]).max() < 1e-5 and on["P5"].all() and on["V3"].all()
    off = H.offpolicy_rows(H.double_copy(orac)[0], OC.minibatch(stale, np.arange(32)), hp)
    assert np.abs(off["ratio"] - 1).max() > 0.2 and np.abs(off["dlt"]).max() > 0.1
    # the builder is the caller's: Modular's _filled through the same helper
    seen = []
    H.stale_oracle_buffer("overcooked", orac, 8, 4, seed=3, drift=0.5,
                          fill=lambda name, beh, T, E, seed=0: seen.append((name, beh.flat_params(), T, E, seed)))
    assert seen[0][0] == "overcooked" and seen[0][2:] == (8, 4, 3) and np.abs(seen[0][1] - before).max() > 0.5


def test_offpolicy_rows_classes_by_hand():
    """a checker whose log-prob and value are known: one Discrete(2) head with zero weights -> logp = log 0.5, v = value bias"""
    orac = H.oracle_policy("box1", seed=0, perturb=0.0)
    with th.no_grad():
        for p in orac.parameters():
            p.zero_()
        orac.value_net.bias.fill_(1.0)
    ratio = np.array([1.5, 1.5, 0.5, 0.5, 1.0, 1.2 * (1 + 5e-5), 0.9, 1.0], np.float64)
    adv = np.array([1.0, -1.0, 1.0, -1.0, 1.0, 1.0, 1.0, -2.0], np.float32)
    oldv = np.array([0.0, 2.0, 1.0, 1.0 - 0.3 * (1 - 5e-5), 1.0, 1.0, 1.0, 1.0], np.float32)
    mb = dict(observations=th.zeros(8, 1), actions=th.zeros(8, 1), advantages=th.as_tensor(adv), old_values=th.as_tensor(oldv),
              old_log_prob=th.as_tensor((np.log(0.5) - np.log(ratio)).astype(np.float32)), returns=th.zeros(8))
    r = H.offpolicy_rows(H.double_copy(orac)[0], mb, orc.PPOHyper(clip_range=0.2, clip_range_vf=0.3, normalize_advantage=False))
    np.testing.assert_allclose(r["ratio"], ratio, rtol=1e-6)
    want = dict(P1=[0, 5], P2=[1], P3=[2], P4=[3], P5=[4, 6, 7], V1=[0], V2=[1], V3=[2, 3, 4, 5, 6, 7], edge=[3, 5])
    for k, rows in want.items():
        assert list(np.flatnonzero(r[k])) == rows, (k, np.flatnonzero(r[k]))
    r = H.offpolicy_rows(H.double_copy(orac)[0], mb, orc.PPOHyper(clip_range=0.2))         # normalised advantages, no value clip
    assert r["V1"] is None and list(np.flatnonzero(r["edge"])) == [5]
    np.testing.assert_allclose(r["adv"], (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8), rtol=1e-6)


def test_the_table_reaches_every_tail_copy_with_small_buffers():
    cases = OC.CASES
    assert all(c.T * c.E <= 256 and 64 < c.nb <= 128 for c in cases)
    assert all(c.clip_range_vf is not None and c.clip_range_vf != c.clip_range for c in cases)
    raw = [c for c in cases if not c.normalize_advantage]
    assert all(c.clip_range == 0.1 for c in raw) and all(c.clip_range == 0.2 for c in cases if c.normalize_advantage)
    assert abs(len(raw) - len(cases) / 2) <= 2.5, (len(raw), len(cases))     # Modular's loss has no switch: its cases are "defaults"
    assert all(cases[i].nb % 64 != 0 and cases[i].nb % 16 != 0 for i in range(1, len(cases), 2))      # every second: no tile multiple
    have = {(c.family, c.config, c.arch, c.gemm_mode) for c in cases}
    for need in [("ppo", "overcooked", None, 0), ("ppo", "overcooked", None, 1), ("ppo", "overcooked", None, 2),
                 ("ppo", "box64", None, 2), ("ppo", "box1", None, 2), ("ppo", "liar", None, 0), ("ppo", "quad16", None, 0),
                 ("ppo", "wide", None, 0), ("ppo", "adap_oc", None, 0), ("ppo", "liar", None, 2), ("ppo", "onehot32", None, 2),
                 ("ppo", "discrete20", None, 2), ("ppo", "box130", None, 2), ("ppo", "gauss5", None, 0), ("ppo", "gauss16", None, 0)]:
        assert need in have, need
    for name in ("overcooked", "liar"):
        for arch in ((32,), (128, 128), (96, 160, 32)):
            assert any(c.family == "arch" and c.config == name and c.arch == arch for c in cases), (name, arch)
    assert {c.partner for c in cases if c.family == "modular" and c.K == 2 and c.coef > 0} == {0, 1}
    assert any(c.family == "adap" and c.config == "adap_oc" for c in cases) and any(c.family == "adapmult" for c in cases)
    assert all(c.kernel for c in cases)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", IDS)
def test_class_shares_edge_rows_and_ratio_range(case_id):
    c, b = OC.BY_ID[case_id], _built(case_id)
    r, n = b["rows"], len(b["idx"])
    shares = {k: int(r[k].sum()) for k in H.OFFPOLICY_CLASSES}
    print(case_id, "->", c.kernel)
    print(case_id, "rows %d of %d candidates (%d edge rows removed), ratio in [%.3f, %.3f], v - old_v in [%.3f, %.3f], classes %s"
          % (n, c.nb, int(b["edge"].sum()), r["ratio"].min(), r["ratio"].max(), r["dlt"].min(), r["dlt"].max(), shares))
    assert n == c.nb - int(b["edge"].sum()) and len(set(b["idx"].tolist())) == n
    assert b["edge"].sum() <= 0.02 * c.nb, (b["edge"].sum(), c.nb)
    assert not r["edge"].any()                                                   # what is left has no edge row
    for k, cnt in shares.items():
        assert cnt >= 3 and cnt >= 0.05 * n, (k, cnt, n)
    assert sum(shares[k] for k in ("P1", "P2", "P3", "P4", "P5")) == n - int(((r["adv"] == 0) & ~r["P5"]).sum())
    assert shares["V1"] + shares["V2"] + shares["V3"] == n
    assert 0.05 <= r["ratio"].min() and r["ratio"].max() <= 20.0, (r["ratio"].min(), r["ratio"].max())


# ---- the yardstick: wrong tails -----------------------------------------------------------------------------------------------------
POLICY_VARIANTS = ("gate_inr", "no_gate", "tie_everywhere", "quadrants_swapped")
VALUE_VARIANTS = ("pass_dropped", "clamp_dropped")


def tail_loss(logp, values, entropy, mb, hp, adv, variant="true"):
    """the row-loss tail as the kernels state it -- g_lp = -adv ratio gate / nb with a DETACHED gate, the value residual through
    `pass` -- so that a wrong gate is one changed line.  Only its gradient is meant (the policy term's value is not the loss's)."""
    c, cv = hp.clip_range, hp.clip_range_vf
    ratio = th.exp(logp - mb["old_log_prob"])
    r = ratio.detach()
    one = th.ones_like(r)
    inr = ((r >= 1 - c) & (r <= 1 + c)).to(r.dtype)
    pl1, pl2 = adv * r, adv * th.clamp(r, 1 - c, 1 + c)
    gate = th.where(pl1 < pl2, one, th.where(pl1 > pl2, inr, 0.5 + 0.5 * inr))
    if variant == "gate_inr":
        gate = inr
    elif variant == "no_gate":
        gate = one
    elif variant == "tie_everywhere":
        gate = 0.5 + 0.5 * inr
    elif variant == "quadrants_swapped":                     # P1 / P4 live, P2 / P3 clipped
        gate = th.where(inr > 0, gate, 1 - gate)
    policy = -(adv * ratio * gate).mean()
    old = mb["old_values"]
    dlt = (values - old).detach()
    vp = old + th.clamp(dlt, -cv, cv)
    passm = (dlt.abs() <= cv).to(values.dtype)
    if variant == "pass_dropped":                            # the residual of the clamped prediction, the gradient of the raw one
        passm = th.ones_like(passm)
    elif variant == "clamp_dropped":
        vp, passm = values.detach(), th.ones_like(passm)
    value = (2.0 * (vp - mb["returns"]) * passm * values).mean()          # d/dv of mean((ret - vp)^2) with dvp/dv = pass
    return policy + hp.ent_coef * (-entropy.mean()) + hp.vf_coef * value


def _tail_gradient(c, o64, mb64, hp, adv, variant):
    for p in o64.parameters():
        p.grad = None
    actions = mb64["actions"]
    if o64.act_space.kind == "discrete":
        actions = actions.long().flatten()
    with H.float64_checker():
        values, logp, ent = o64.evaluate_actions(mb64["observations"], actions, **OC.eval_kw(c))
        tail_loss(logp, values.flatten(), ent, mb64, hp, adv, variant).backward()
    return H.flat_grads_exact(o64, OC.flat_fn(c))


@pytest.mark.parametrize("case_id", IDS)
def test_wrong_tails_are_rejected_by_ten_times_the_allowance(case_id):
    c, b = OC.BY_ID[case_id], _built(case_id)
    hp, r = OC.hyper(c), b["rows"]
    mb = OC.minibatch(b["ob"], b["idx"])
    mb64 = {k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
    adv = th.as_tensor(r["adv"])
    o64 = H.double_copy(b["orac"])[0]
    # the restatement with the right gate IS the checker's PPO gradient (float64: to rounding)
    g_true = _tail_gradient(c, o64, mb64, hp, adv, "true")
    for p in o64.parameters():
        p.grad = None
    with H.float64_checker():
        if c.family == "modular":
            orc.modular_minibatch_loss(o64, mb64, hp, c.partner, 0.0)[0].backward()
        else:
            orc.ppo_minibatch_loss(o64, mb64, hp)[0].backward()
    g_chk = H.flat_grads_exact(o64, OC.flat_fn(c))
    assert np.abs(g_true - g_chk).max() <= 1e-12 * max(1.0, np.abs(g_chk).max()), np.abs(g_true - g_chk).max()
    # the allowance of the GPU test is taken on the gradient of the family's WHOLE loss (context term, regulariser included)
    g32, g64, _ = OC.checker_gradients(c, b["orac"], b["ob"], b["idx"])
    allowance = 1e-6 + 2e-4 * np.abs(g32).max()
    assert np.abs(g32 - g64).max() <= 0.1 * allowance          # float32 autograd is a sound reference at this size
    for variant in POLICY_VARIANTS + VALUE_VARIANTS:
        diff = np.abs(_tail_gradient(c, o64, mb64, hp, adv, variant) - g_true).max()
        print(case_id, "%-18s moves the gradient by %.3g = %.0f x the allowance %.3g" % (variant, diff, diff / allowance, allowance))
        assert diff >= 10 * allowance, (variant, diff, allowance)
    # clip_fraction counted with the other clip's range is another count
    right = int((np.abs(r["ratio"] - 1) > hp.clip_range).sum())
    wrong = int((np.abs(r["ratio"] - 1) > hp.clip_range_vf).sum())
    assert right == int(r["P1"].sum() + r["P2"].sum() + r["P3"].sum() + r["P4"].sum() + ((r["adv"] == 0) & ~r["P5"]).sum())
    assert right != wrong, (right, wrong)


# ---- train level -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_ref(train_id):
    return OC.train_reference(OC.TRAIN_BY_ID[train_id])


@pytest.mark.parametrize("train_id", [t.id for t in OC.TRAIN_CASES])
def test_train_cases_have_live_clips_and_no_edge_row_in_any_minibatch(train_id):
    """train() walks the whole buffer, so no row can be taken out: the case's seed is one whose minibatches hold no edge row (the
    float64 checker walks the chain; the second minibatch is judged at the parameters after the first step)"""
    t, ref = OC.TRAIN_BY_ID[train_id], _train_ref(train_id)
    n_mb = (t.K or 1) * 2
    assert len(ref["rows"]) == len(ref["stats"]) == n_mb and t.T * t.E == 2 * t.batch
    for k, (r, s) in enumerate(zip(ref["rows"], ref["stats"])):
        shares = {c: int(r[c].sum()) for c in H.OFFPOLICY_CLASSES}
        print(train_id, "minibatch", k, "classes", shares, "approx_kl %.4f" % s["approx_kl"])
        assert not r["edge"].any(), (k, np.flatnonzero(r["edge"]))
        assert all(v >= 3 for v in shares.values()), shares
        assert 0.05 <= r["ratio"].min() and r["ratio"].max() <= 20.0
        count = int((np.abs(r["ratio"] - 1) > ref["hp"].clip_range).sum())
        if "clip_fraction" in s:                                   # the float32 checker counts what the float64 one counts
            assert abs(s["clip_fraction"] - count / t.batch) <= 1e-6
    # the first step as a unit of its own is the chain's first step (Modular: a one-partner model, another checker)
    fs = OC.first_step_reference(t, ref)
    if t.family != "modular":
        assert abs(fs["n_ref"] - ref["stats"][0]["grad_norm"]) <= 1e-5 * fs["n_ref"], (fs["n_ref"], ref["stats"][0]["grad_norm"])
    assert fs["n_ref"] > ref["hp"].max_grad_norm and np.abs(fs["m_ref"]).max() > 1e-3       # the clip is live, adam_m is off zero


def test_kl_stop_case_is_far_from_a_tie():
    t, hp, ref = OC.kl_stop_reference()
    kls = [s["approx_kl"] for s in ref["stats"]]
    thr = 1.5 * hp.target_kl
    print("approx_kl per minibatch", kls, "threshold", thr)
    assert ref["stats"][-1].get("stopped") and 2 <= len(kls) - 1 < hp.n_epochs * 4       # at least two steps, then the stop
    assert kls[-1] >= 2 * thr and max(kls[:-1]) <= 0.5 * thr, (kls, thr)
    assert not any(r["edge"].any() for r in ref["rows"])
