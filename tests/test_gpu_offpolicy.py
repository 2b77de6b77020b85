"""-m gpu: every caller of the row loss (ph_ppo_loss.h) OFF-policy -- live ratio clip, live value clip -- against float32 autograd of the
checker's own loss, once per case of tests/offpolicy_cases.py and through the same ph_*_minibatch_grad entry points (and the same
_grad_pair functions) as each family's on-policy gradient test.

A drifted copy of the checker fills the buffer, the checker's parameters go to the device: every minibatch holds rows of the eight
classes P1 (ratio > 1+c, adv > 0: clipped), P2 (ratio > 1+c, adv < 0: live), P3 (ratio < 1-c, adv > 0: live), P4 (ratio < 1-c,
adv < 0: clipped), P5 (inside), V1 / V2 (v - old_v beyond +-c_vf: clipped), V3 (inside).  Rows within 1e-4 s of a clip bound (edge
rows; s = max(1, w_last / 64)) are taken out of the minibatch before either side sees it, at most 2 % of the candidates;
tests/test_offpolicy_checks.py proves on the CPU that every class is populated and that each wrong tail (gate = inr, no gate, the tie
value everywhere, swapped quadrants, `pass` dropped, the clamp dropped) misses the allowance below by 10x or more.

Asserted per case: the gradient at the project's rule 1e-6 + 2e-4 max|g|; per parameter block b (every weight matrix and bias, the
Gaussian log_std) at 1e-6 + max(2e-4 M_b, 4 d_b), M_b the block's largest float64-checker entry, d_b the checker's float32-vs-float64
difference in the block; policy / value / entropy loss and loss at 1e-5 + 1e-4 |x|; approx_kl at 3e-6 + 2e-4 |x|; clip_fraction
EXACTLY the checker's count / nb (no edge row is left to flip); gemm_mode 1 the bits of mode 0 and mode 2 within 2e-6 of the largest
entry of mode 0 where the family's own test asserts it.  The kernel each case lands on is its `kernel` field (printed).

Train level, one case per family (PPO two-launch and one-launch, net_arch, Gaussian, Modular, ADAP, ADAP-MULT): one epoch of two
minibatches on a stale buffer from a zero Adam state -- last_train_stats rows against the checker's train(), clip_fraction exact,
and adam_m after the first step under optimizer_bound.one_step_bounds; and a target_kl stop on a stale buffer that lands on the
checker's minibatch."""
import numpy as np
import pytest

from tests import helpers as H
from tests import offpolicy_cases as OC

pytestmark = pytest.mark.gpu

STAT_KEYS = ("policy_loss", "value_loss", "entropy_loss", "clip_fraction", "approx_kl", "loss")


def _device_pair(c, mode):
    """-> (g, g_ref, st, st_ref) through the family's own _grad_pair, with the case's stale buffer and edge-free rows passed in"""
    hp, fill, idx = OC.hyper(c), OC.fill(c), OC.pick_idx(c)
    if c.family == "ppo":
        from tests.parity_cases import _grad_pair
        g, g_ref, st, st_ref, _ = _grad_pair(c.config, c.T, c.E, idx, hp, seed=OC.SEED, gemm_mode=mode, fill=fill)
    elif c.family == "arch":
        from tests.arch_cases import _grad_pair
        out, g_ref, st_ref = _grad_pair(c.config, c.arch, c.T, c.E, idx, hp, seed=OC.SEED, gemm_mode=mode, fill=fill)
        g, st = out[0]
    elif c.family == "modular":
        from tests.modular_cases import _grad_pair
        g, g_ref, st, st_ref, _ = _grad_pair(c.config, c.K, c.partner, c.T, c.E, c.nb, c.coef, hp, seed=OC.SEED, gemm_mode=mode,
                                             fill=fill, idx=idx)
    elif c.family == "adap":
        from tests.adap_cases import _grad_pair
        g, g_ref, st, st_ref = _grad_pair(c.config, c.T, c.E, idx, hp, 5, 32, c.coef, seed=OC.SEED, gemm_mode=mode, fill=fill)[:4]
    else:
        from tests.adapmult_cases import _grad_pair
        assert mode == 0
        g, g_ref, st, st_ref = _grad_pair(c.config, c.T, c.E, c.nb, hp, coef=c.coef, seed=OC.SEED, fill=fill, idx=idx)[:4]
    return g, g_ref, st, st_ref


@pytest.mark.parametrize("case_id", [c.id for c in OC.CASES])
def test_offpolicy_minibatch_gradient_matches_autograd(case_id):
    c = OC.BY_ID[case_id]
    print(case_id, "->", c.kernel)
    g, g_ref, st, st_ref = _device_pair(c, c.gemm_mode)
    # the checker side once more, for what _grad_pair does not hand out: the rows, the float64 gradient, the blocks
    b = OC.build(c)
    g32, g64, _ = OC.checker_gradients(c, b["orac"], b["ob"], b["idx"])
    assert np.array_equal(g32.astype(np.float32), g_ref), "the family's _grad_pair differentiated another minibatch"
    r = OC.rows(c, H.double_copy(b["orac"])[0], b["ob"], b["idx"])
    nb = len(b["idx"])
    print(case_id, "rows", nb, "classes", {k: int(r[k].sum()) for k in H.OFFPOLICY_CLASSES})
    block, names = H.flat_blocks(b["orac"], OC.flat_fn(c))
    H.assert_block_gradients(g, g32, g64, block, names, case_id)
    # statistics
    count = int((np.abs(r["ratio"] - 1) > c.clip_range).sum())
    if "clip_fraction" in st_ref:
        assert abs(st_ref["clip_fraction"] - count / nb) <= 1e-6, (st_ref["clip_fraction"], count, nb)
    ref = dict(st_ref, clip_fraction=count / nb)
    for i, k in enumerate(STAT_KEYS):
        tol = {"clip_fraction": 1e-6, "approx_kl": 3e-6 + 2e-4 * abs(ref[k])}.get(k, 1e-5 + 1e-4 * abs(ref[k]))
        print(case_id, "%-14s device %.7g checker %.7g error %.3g allowed %.3g" % (k, st[i], ref[k], abs(st[i] - ref[k]), tol))
    for i, k in enumerate(STAT_KEYS):
        tol = {"clip_fraction": 1e-6, "approx_kl": 3e-6 + 2e-4 * abs(ref[k])}.get(k, 1e-5 + 1e-4 * abs(ref[k]))
        assert abs(st[i] - ref[k]) <= tol, (case_id, k, st[i], ref[k], tol)
    assert 0 < count < nb and abs(ref["approx_kl"]) > 1e-3          # both clips were live, the estimator is off zero
    # gemm modes, as the family's own test has them
    if c.gemm_mode != 0:
        g0 = _device_pair(c, 0)[0]
        if c.gemm_mode == 1 or c.family == "arch":
            assert np.array_equal(g, g0), np.abs(g - g0).max()
        else:
            d = np.abs(g - g0).max()
            print(case_id, "gemm_mode 2 vs 0: %.3g allowed %.3g" % (d, 2e-6 * max(np.abs(g0).max(), 1e-3)))
            assert d <= 2e-6 * max(np.abs(g0).max(), 1e-3), (d, np.abs(g0).max())


# ---- train level -------------------------------------------------------------------------------------------------------------------
def _device_train(t, T, E, hp, bufs, perms, samples, orac0):
    """the family's train() on the device from a zero Adam state -> the trained model (ppo / arch go through the family's _train_pair,
    which builds the same checker and, through `fill`, gets the same buffer)"""
    given = lambda *a, **k: bufs[0]     # noqa: E731
    if t.family == "ppo":
        from tests.parity_cases import _train_pair
        assert np.array_equal(perms, OC.train_perms(t, hp.n_epochs, N=T * E))
        return _train_pair(t.config, T, E, hp, seed=t.seed, fill=given, exclusive=t.exclusive)[0]
    if t.family == "arch":
        from tests.arch_cases import _train_pair
        assert np.array_equal(perms, OC.train_perms(t, hp.n_epochs, N=T * E))
        return _train_pair(t.config, t.arch, T, E, hp, seed=t.seed, fill=given)[0]
    if t.family == "modular":
        from tests import modular_cases as M
        model = M._algo(t.config, len(bufs), T, E, hp, t.coef)
        model.policy.set_flat_params(M._flat(orac0))
        for rb, ob in zip(model.rollout_buffer, bufs):
            H.upload_buffer(rb, ob)
        model.train(perms=np.asarray([list(perms)] * len(bufs)))
        return model
    if t.family == "adap":
        from tests.adap_cases import _adap_model
        model = _adap_model(t.config, T, E, hp, coef=t.coef, n_ctx=OC.N_CTX, n_states=OC.N_STATES)
    else:
        from tests.adapmult_cases import _model
        model = _model(t.config, T, E, hp, t.coef, n_ctx=OC.N_CTX, n_states=OC.N_STATES)
    model.policy.set_flat_params(orac0.flat_params())
    H.upload_buffer(model.rollout_buffer, bufs[0])
    model.train(perms=perms, state_idx=samples[0], contexts=samples[1])
    return model


def _assert_rows(t, st, ref, where):
    """last_train_stats rows against the checker's: the project's train rule (tests/parity_cases._assert_train_stats), with
    clip_fraction EXACT (no edge row in any minibatch: tests/test_offpolicy_checks.py)"""
    from tests.parity_cases import _assert_train_stats
    st = np.asarray(st).reshape(-1, st.shape[-1])
    st = st[np.abs(st).sum(-1) > 0]
    assert len(st) == len(ref["stats"]), (where, len(st), len(ref["stats"]))
    for i, (row, s, r) in enumerate(zip(st, ref["stats"], ref["rows"])):
        count = int((np.abs(r["ratio"] - 1) > ref["hp"].clip_range).sum())
        print(where, i, "device", [float("%.6g" % x) for x in row[:8]], "checker", {k: float("%.6g" % v) for k, v in s.items() if k != "partner"},
              "clipped rows", count)
        assert abs(row[3] - count / t.batch) <= 1e-6, (where, i, row[3], count, t.batch)
        if s.get("stopped"):
            s = dict(s, grad_norm=row[6])
        if t.family == "modular":          # ModularAlgorithm's rows: no clip_fraction on the checker's side, its own approx_kl, the regulariser
            for j, k in ((0, "policy_loss"), (1, "value_loss"), (2, "entropy_loss")):
                assert abs(row[j] - s[k]) <= 2e-5 + 2e-4 * abs(s[k]), (where, i, k, row[j], s[k])
            assert abs(row[4] - s["approx_kl"]) <= 3e-6 + 2e-4 * abs(s["approx_kl"]), (where, i, row[4], s["approx_kl"])
            assert abs(row[7] - s["marginal_reg"]) <= 2e-5 and abs(row[6] - s["grad_norm"]) <= 1e-5 + 2e-4 * s["grad_norm"]
        else:
            _assert_train_stats(row, dict(s, clip_fraction=count / t.batch), t.batch, (where, i))


@pytest.mark.parametrize("train_id", [t.id for t in OC.TRAIN_CASES])
def test_offpolicy_train_statistics_and_first_step_moment(train_id):
    from tests import optimizer_bound as OB
    t = OC.TRAIN_BY_ID[train_id]
    print(train_id, "->", t.kernel)
    ref = OC.train_reference(t)
    model = _device_train(t, t.T, t.E, ref["hp"], ref["bufs"], ref["perms"], ref["samples"], ref["orac0"])
    assert int(model.policy.opt_step.item()) == len(ref["stats"])
    _assert_rows(t, model.last_train_stats, ref, train_id)
    # the first step as a unit of its own: adam_m from a zero state is 0.1 * the clipped gradient, every entry under the derived bound
    fs = OC.first_step_reference(t, ref)
    one = _device_train(fs["t1"], t.batch, 1, fs["hp"], [fs["sub"]], fs["perms"], fs["samples"], fs["orac0"])
    assert int(one.policy.opt_step.item()) == 1
    m = H.read_device_adam_state(one.policy)[0]
    P = fs["m_ref"].size
    b = OB.one_step_bounds(np.zeros(P), np.zeros(P), np.zeros(P), 0, fs["g_ref"], fs["hp"].max_grad_norm)
    assert b["coef"] < 1                                                # the clip coefficient is in the product
    err = np.abs(m.astype(np.float64) - fs["m_ref"])
    i = int(np.argmax(err / b["e_m"]))
    print(train_id, "adam_m after the first step: largest error %.3g, largest error / bound %.3g at entry %d (error %.3g, bound %.3g), "
          "max |m| %.3g" % (err.max(), (err / b["e_m"]).max(), i, err[i], b["e_m"][i], np.abs(fs["m_ref"]).max()))
    assert (err <= b["e_m"]).all(), (train_id, err.max(), i, err[i], b["e_m"][i])
    norm_dev = float(np.asarray(one.last_train_stats).reshape(-1, one.last_train_stats.shape[-1])[0, 6])
    assert abs(norm_dev - fs["n_ref"]) <= b["e_n"], (norm_dev, fs["n_ref"], b["e_n"])


def test_offpolicy_target_kl_stop_lands_on_the_checkers_minibatch():
    t, hp, ref = OC.kl_stop_reference()
    applied = sum(0 if s.get("stopped") else 1 for s in ref["stats"])
    assert ref["stats"][-1].get("stopped") and applied == len(ref["stats"]) - 1 >= 2
    model = _device_train(t, t.T, t.E, hp, ref["bufs"], ref["perms"], None, ref["orac0"])
    st = model.last_train_stats
    print("approx_kl device", st[:applied + 1, 4], "checker", [s["approx_kl"] for s in ref["stats"]], "threshold", 1.5 * hp.target_kl)
    assert int(model.policy.opt_step.item()) == applied
    assert int((st[:, 7] > 0).sum()) == applied and (st[:applied, 7] > 0).all() and not (st[applied:, 7] > 0).any()
    for i, s in enumerate(ref["stats"]):
        assert abs(st[i, 4] - s["approx_kl"]) <= 3e-6 + 2e-4 * abs(s["approx_kl"]), (i, st[i, 4], s["approx_kl"])
    p, p_ref = model.policy.get_flat_params(), ref["orac"].flat_params()
    assert np.abs(p - p_ref).max() <= 2e-6 * applied * (hp.learning_rate / 3e-4) + 1e-6, np.abs(p - p_ref).max()
