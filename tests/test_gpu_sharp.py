"""-m gpu: every policy head and its gradient kernel on sharp (head x 8) and saturated (head x 30) policies, against the checker.

The rest of the suite runs checkers close to their initial weights: no probability below ~1e-5, no row of entropy below 0.3.  Here
one action sits at probability 1 - 1e-9 and the others at 1e-20 or under float32's smallest denormal, beside soft rows in the same
launch.  Cases, inputs, references and allowances are tests/sharp_cases.py (its docstring derives every allowance);
tests/test_sharp_checks.py proves on the CPU that the cases hold those populations, that the head as ph_rowtail.h writes it passes
every allowance, and that each wrong head -- no max subtraction, log of the softmax, entropy from the probabilities, the mask as
-inf, an unnormalised inverse CDF, saturated rows without a gradient -- misses one by 10x or more.  Which kernel a case reaches is
its `kernel` field (printed).  Every comparison prints the error, the checker's own float32-vs-float64 difference d and the
allowance; lines starting with RATIO carry the largest error / allowance of a test (CHANGELOG.md lists them per family)."""
import numpy as np
import pytest

from tests import bc_cases as B
from tests import helpers as H
from tests import offpolicy_cases as OC
from tests import sampler_cases as S
from tests import sharp_cases as SC

pytestmark = pytest.mark.gpu


def _np(t, shape=None):
    a = t.detach().cpu().numpy()
    return a if shape is None else a.reshape(shape)


class _Ratios:
    def __init__(self, where):
        self.where, self.worst = where, {}

    def check(self, what, err, allowed, d=None, extra=()):
        """print error, d and allowance; remember the largest ratio; -> whether every entry is finite and within its allowance"""
        err = np.asarray(err, np.float64)
        ratio = SC.miss(err, allowed)
        print(self.where, *extra, "%-10s error %.3g  checker f32 vs f64 d = %s  allowed %.3g  error / allowed %.3g"
              % (what, err.max() if err.size else 0.0, "%.3g" % d if d is not None else "-", float(np.max(allowed)), ratio))
        self.worst[what] = max(self.worst.get(what, 0.0), ratio)
        return ratio <= 1.0

    def report(self, family, scale):
        print("RATIO", family, "x%d" % scale, self.where, {k: float("%.3g" % v) for k, v in self.worst.items()})


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
def _kw(case):
    return dict(partner_idx=case.extra["partner"]) if case.family == "modular" else {}


def _obs_t(case, pol, obs):
    return obs if case.family == "bc" else pol._obs(obs)


def _own_draw(case, pol, obs, mask, c):
    """one forward with the device's own draws at (S.KEY, c): the launch advances the counter before it passes it on"""
    pol._seed, pol._counter = S.KEY, c - 1
    acts, v, logp = pol.forward(obs, action_mask=mask, **_kw(case))
    assert pol._counter == c
    return _np(acts, (len(obs), -1)), _np(v, -1), _np(logp)


def _deterministic(case, pol, obs, mask):
    """-> (argmax actions (n, A), logits (n, L) after the mask offset)"""
    acts, _, _, _, z = pol._launch(_obs_t(case, pol, obs), mask=mask, deterministic=True, want_logits=True, **_kw(case))
    if case.family == "modular":            # (main logits, partner logits), unmasked; no Modular case here carries a mask
        assert mask is None
        z = z[1] if pol.nomain else z[0] + z[1]
    return _np(acts, (len(obs), -1)), _np(z)


def _evaluate(case, pol, obs, mask, acts):
    """-> (values (n,), log-prob (n,), entropy (n,)) of given actions"""
    given = np.asarray(acts, np.float32)
    if case.family == "bc":
        _, v, lp, ent, _ = pol._launch(obs, given=given, mask=mask)
    else:
        v, lp, ent = pol.evaluate_actions(obs, given, action_mask=mask, **_kw(case))
    return _np(v, -1), _np(lp), _np(ent)


@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("cid", [f.id for f in SC.FORWARD])
def test_forward_heads_on_sharp_policies(cid, scale):
    """per gemm_mode and row count: one forward with the device's own draws (actions = the float64 inverse CDF off near rows, the
    drawn action's log-prob within A_lp, values within 2e-5 s); deterministic=True (logits within A_z, the argmax on rows whose top
    two logits differ by more than 2 max A_z); evaluate_actions on the most likely, least likely and one random action set (log-prob
    within A_lp, entropy within A_H and >= -A_H, value within 2e-5 s, everything finite); gemm_mode 1 the bits of mode 0"""
    from tests.sampler_cases import device as _device
    fc = SC.FORWARD_BY_ID[cid]
    case = fc.case
    print(cid, "x%d" % scale, "->", case.kernel)
    pol = _device(case, SC.checker(cid, scale))
    R = _Ratios(cid)
    ok, bits = True, {}
    for mode in case.gemm_modes:
        if mode is not None:
            pol.gemm_mode = mode
        for n in fc.rows:
            r = SC.reference(cid, scale, n)
            tag = ("gemm_mode", mode, "n", n)
            out = []
            # -- the device's own draws
            for c in S.COUNTERS:
                u, want, near = r.prediction(c)
                got, v, logp = _own_draw(case, pol, r.obs, r.mask, c)
                bad = np.nonzero((got != want).any(axis=1) & ~near)[0]
                print(cid, *tag, "counter", c, "near", int(near.sum()), "mismatches", len(bad))
                assert len(bad) == 0, (cid, tag, c, bad[:8], got[bad[:8]], want[bad[:8]], u[bad[:8]])
                assert (got >= 0).all() and (got < np.asarray(r.nvec)).all(), (cid, tag)
                lp32, _, A_lp, d_lp = r.log_probs(got)
                ok &= R.check("logp", np.abs(logp - lp32), A_lp, d_lp, tag + ("own draw",))
                ok &= R.check("value", np.abs(v - r.v32), r.A_v, float(np.abs(r.v32 - r.v64).max()), tag)
                out += [got, v, logp]
            # -- deterministic: logits and argmax
            arg, z = _deterministic(case, pol, r.obs, r.mask)
            ok &= R.check("logits", np.abs(z - r.z32), r.A_z[None, :], r.d_z, tag)
            want_arg, decided = r.decided_argmax()
            assert decided.sum() >= 0.9 * n and np.array_equal(arg[decided], want_arg[decided]), \
                (cid, tag, np.nonzero((arg != want_arg).any(axis=1) & decided)[0][:8])
            out += [arg, z]
            # -- teacher-forced: three action sets
            for name, acts in r.action_sets().items():
                v, lp, ent = _evaluate(case, pol, r.obs, r.mask, acts)
                assert np.isfinite(v).all() and np.isfinite(lp).all() and np.isfinite(ent).all(), (cid, tag, name)
                lp32, _, A_lp, d_lp = r.log_probs(acts)
                ok &= R.check("logp", np.abs(lp - lp32), A_lp, d_lp, tag + (name,))
                ok &= R.check("entropy", np.abs(ent - r.H32), r.A_H, r.d_H, tag + (name,))
                ok &= R.check("value", np.abs(v - r.v32), r.A_v, None, tag + (name,))
                assert (ent >= -r.A_H).all(), (cid, tag, name, ent.min())
                out += [v, lp, ent]
            if mode == 1:
                assert all(np.array_equal(a, b) for a, b in zip(out, bits[n])), (cid, "gemm_mode 1 is not the bits of mode 0", n)
            bits.setdefault(n, out)
    R.report("forward/" + case.family, scale)
    assert ok, (cid, scale, R.worst)


# ---- gradients -------------------------------------------------------------------------------------------------------------------------
def _device_pair(g, scale, nb, mode):
    """-> (gradient, the family's float32 checker gradient, statistics, ADAP's context loss or None) through the family's own _grad_pair"""
    hp, fill, idx, prep = SC.hyper(), SC.fill(g), SC.minibatch_rows(nb), SC.preparer(scale)
    cl = None
    if g.family == "ppo":
        from tests.parity_cases import _grad_pair
        grad, g_ref, st, _, _ = _grad_pair(g.config, SC.T, SC.E, idx, hp, seed=OC.SEED, gemm_mode=mode, fill=fill, prepare=prep)
    elif g.family == "arch":
        from tests.arch_cases import _grad_pair
        out, g_ref, _ = _grad_pair(g.config, g.arch, SC.T, SC.E, idx, hp, seed=OC.SEED, gemm_mode=mode, fill=fill, prepare=prep)
        grad, st = out[0]
    elif g.family == "modular":
        from tests.modular_cases import _grad_pair
        grad, g_ref, st, _, _ = _grad_pair(g.config, g.K, g.partner, SC.T, SC.E, nb, g.coef, hp, seed=OC.SEED, gemm_mode=mode, fill=fill,
                                           idx=idx, prepare=prep)
    elif g.family == "adap":
        from tests.adap_cases import _grad_pair
        grad, g_ref, st, _, cl = _grad_pair(g.config, SC.T, SC.E, idx, hp, 5, 32, g.coef, seed=OC.SEED, gemm_mode=mode, fill=fill,
                                            prepare=prep)[:5]
    else:
        from tests.adapmult_cases import _grad_pair
        assert mode == 0
        grad, g_ref, st, _, cl = _grad_pair(g.config, SC.T, SC.E, nb, hp, coef=g.coef, seed=OC.SEED, fill=fill, idx=idx, prepare=prep)
    return grad, g_ref, st, cl


def _bc_gradient_case(g, scale, R):
    from tests.bc_shape_cases import _assert_path, _clone, _reset
    for nb in SC.NBS:
        b = SC.bc_build(g, scale, nb)
        case, orac, obs, acts = b["case"], b["orac"], b["obs"], b["acts"]
        block, names = H.flat_blocks(orac)
        p0 = orac.flat_params()
        clone = _clone(case, obs, acts)
        path = _assert_path(case, clone)
        for ent, l2 in SC.BC_WEIGHTS:
            where = (g.id, "x%d" % scale, "path %d" % path, "nb %d" % nb, "ent %g" % ent)
            _reset(clone, p0, ent, l2)
            st = clone.train(n_epochs=1, orders=B.permutation(nb)[None])
            ref = B.reference(orac, obs, acts, ent, l2)
            m, _, step = H.read_device_adam_state(clone)
            assert step == 1 and np.isfinite(m).all() and np.isfinite(st).all(), where
            R.worst["gradient"] = max(R.worst.get("gradient", 0.0), SC.block_misses(m, ref["g32"], ref["g64"], block, names).max())
            B.assert_stats(st[0], ref["stats"], nb, where)
            H.assert_block_gradients(m, ref["g32"], ref["g64"], block, names, where)


@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("gid", [g.id for g in SC.GRAD_CASES])
def test_gradient_kernels_on_sharp_policies(gid, scale):
    """one on-policy minibatch (nb in {77, 100} of 16 x 8 rows) whose every second row holds a uniformly drawn action with the
    float32 checker's log-prob as old_log_prob: ratios stay at 1, unlikely actions (log-prob -50 and below) sit beside saturated likely
    ones, both carry gradient.  helpers.assert_block_gradients unchanged against the float32 checker and its float64 copy; policy,
    value, entropy and total loss at 1e-5 + 1e-4 |x| + 4 d_x; clip_fraction exactly 0; ADAP's context loss at the same rule; the
    device gradient finite everywhere.  BC: adam_m after one minibatch with beta1 = 0 is the gradient; bounds as in
    tests/test_gpu_bc_shapes.py.

    Two allowances were derived anew (both derivations with their figures: tests/sharp_cases.py):
    - gemm_mode 2 against gemm_mode 0: per block, 2e-6 of the largest entry of mode 0 (the off-policy test's rule) or 8 d_b where
      that is more (sharp_cases.mode2_allowances).  On these minibatches the 2e-6 rule alone rejects torch's own float32 autograd
      against float64; both kernels pass the block rule against the checker.
    - ADAP's context term at x30: the float32 checker's term is degenerate (torch's kl_divergence returns inf where a float32
      probability underflowed to 0: sharp_cases.context_term_degenerate), the device computes kl = sum p (lp - lq) as written.
      There the float64 checker is the reference for gradient, context loss and total loss, at the same rule with d = 0 -- a
      narrower allowance than 4 d, not a wider one."""
    g = SC.GRAD_BY_ID[gid]
    print(gid, "x%d" % scale, "->", g.kernel)
    R = _Ratios(gid)
    if g.family == "bc":
        _bc_gradient_case(g, scale, R)
        R.report("gradient/bc", scale)
        return
    ok = True
    for nb in SC.NBS:
        where = (gid, "x%d" % scale, "nb %d" % nb)
        grad, g_ref, st, cl = _device_pair(g, scale, nb, g.gemm_mode)
        b = SC.build(g, scale, nb)
        g32, g64, st32, st64 = SC.checker_gradients(b["c"], b["orac"], b["ob"], b["idx"])
        assert np.array_equal(g32.astype(np.float32), g_ref), "the family's _grad_pair differentiated another minibatch"
        assert np.isfinite(grad).all() and np.isfinite(st).all(), where
        block, names = H.flat_blocks(b["orac"], OC.flat_fn(b["c"]))
        ref, st_r, swapped = SC.gradient_reference(g32, g64, st32, st64)
        if swapped:
            print(*where, "the float32 checker's context term is degenerate (context loss %.6g, float64 %.6g): the float64 checker is "
                  "the reference, without the d terms" % (st32["context_loss"], st64["context_loss"]))
        R.worst["gradient"] = max(R.worst.get("gradient", 0.0), SC.block_misses(grad, ref, g64, block, names).max())
        H.assert_block_gradients(grad, ref, g64, block, names, where)
        for k in SC.STAT_KEYS:
            ok &= R.check(k, abs(st[SC.STAT_SLOT[k]] - st_r[k]), SC.stat_allowance(st_r[k], st64[k]), abs(st_r[k] - st64[k]), where)
        assert st[SC.STAT_SLOT["clip_fraction"]] == 0.0, (where, st[SC.STAT_SLOT["clip_fraction"]])
        if cl is not None:
            assert np.isfinite(cl), where
            ok &= R.check("context", abs(cl - st_r["context_loss"]), SC.stat_allowance(st_r["context_loss"], st64["context_loss"]),
                          abs(st_r["context_loss"] - st64["context_loss"]), where)
        if g.gemm_mode == 2:
            g0 = _device_pair(g, scale, nb, 0)[0]
            allowed = SC.mode2_allowances(g0, g32, g64, block, names)
            dm = np.array([np.abs(grad - g0)[block == b].max() for b in range(len(names))])
            print(*where, "gemm_mode 2 vs 0: largest difference %.3g (2e-6 of the largest entry: %.3g), largest difference / allowed "
                  "%.3g in block %s" % (dm.max(), 2e-6 * max(np.abs(g0).max(), 1e-3), (dm / allowed).max(), names[int((dm / allowed).argmax())]))
            R.worst["mode 2 vs 0"] = max(R.worst.get("mode 2 vs 0", 0.0), float((dm / allowed).max()))
            assert (dm <= allowed).all(), (where, dm, allowed)
    R.report("gradient/" + g.family, scale)
    assert ok, (gid, scale, R.worst)
