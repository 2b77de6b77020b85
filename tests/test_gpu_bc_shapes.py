"""-m gpu: behavioural cloning's kernels on every shape class they dispatch on (tests/bc_cases.py), against the checker.

The gradient is read bit for bit: with Adam's beta1 = 0, zero moments and step 0, both training kernels leave
m = m0 + (g - m0) * (1 - beta1) = g in adam_m after ONE minibatch, so adam_m is the minibatch gradient (L2 term included) and
helpers.assert_block_gradients bounds it per parameter block against autograd of oracle.bc_loss in float32, with the float64
copy giving the allowance.  Which kernel ran is asked of the library (ph_bc_train_path), not restated here.
tests/test_bc_checks.py shows on the CPU that these bounds reject a dropped entropy or L2 term, a fixed 1/32, a zeroed row or
logit column at the tile seams and skipped out-of-range rows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from tests import bc_cases as B
from tests import helpers as H
from tests.bc_shape_cases import _assert_path, _clone, _reset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAIN_IDS = [c.id for c in B.TRAINABLE]
ALL_IDS = [c.id for c in B.CASES]


def _assert_value_head(m, p0, case, l2_weight, where):
    """value_net gets no gradient from the BC loss: exactly 0 without the L2 term, exactly float32(l2) * w with it"""
    lo = B.offsets(case)["val_W"]
    if l2_weight == 0.0:
        assert not m[lo:].any(), (where, m[lo:])
    else:
        assert np.array_equal(m[lo:], np.float32(l2_weight) * p0[lo:]), where


# ---- the gradient, entry by entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", TRAIN_IDS)
def test_bc_minibatch_gradient_per_block(cid):
    """one launch of one minibatch (batch_size 128 >= N, a shuffled visiting order) for N in {1, 31, 33, 77} rows -- 31 padding rows,
    a second tile of one row, a third tile -- and (ent_weight, l2_weight) in {(1e-3, 0), (0.5, 0), (1e-3, 0.25)}: adam_m against
    autograd per parameter block, the value head exactly, the statistics row at test_gpu_bc's bound"""
    from pantheonrl_amd.common import TransitionsMinimal
    case = B.BY_ID[cid]
    orac, obs, acts = B.checker(case, max(B.N_ROWS))
    block, names = H.flat_blocks(orac)
    p0 = orac.flat_params()
    clone = _clone(case, obs, acts)
    path = _assert_path(case, clone)
    for N in B.N_ROWS:
        clone.set_expert_data_loader(TransitionsMinimal(obs[:N], acts[:N]))
        order = B.permutation(N)[None]
        for ent, l2 in B.WEIGHTS:
            where = (cid, "path %d" % path, "N %d" % N, "ent %g l2 %g" % (ent, l2))
            _reset(clone, p0, ent, l2)
            st = clone.train(n_epochs=1, orders=order)
            ref = B.reference(orac, obs[:N], acts[:N], ent, l2)
            m, _, step = H.read_device_adam_state(clone)
            assert st.shape == (1, 8) and step == 1, where
            B.assert_stats(st[0], ref["stats"], N, where)
            H.assert_block_gradients(m, ref["g32"], ref["g64"], block, names, where)
            _assert_value_head(m, p0, case, l2, where)
            assert not np.array_equal(clone.policy.get_flat_params(), p0)        # lr 1e-3: the step was taken


def test_bc_valu_kernel_passes_the_gradient_test_on_the_mfma_shapes():
    """PH_BC_MFMA=0 routes every shape through bc_train_kernel, the MFMA-class shapes included; the switch is read once per process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_bc_shapes.py", "-x", "-q", "-m", "gpu", "-k",
                          "test_bc_minibatch_gradient_per_block"], cwd=root, env={**os.environ, "PH_BC_MFMA": "0"},
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-2000:])
    assert "%d passed" % len(TRAIN_IDS) in out.stdout, out.stdout[-500:]


# ---- nothing is carried from one minibatch into the next --------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [32, 50])
@pytest.mark.parametrize("cid", B.LEAK_CASES)
def test_bc_last_minibatch_of_a_launch_equals_that_minibatch_alone(cid, batch):
    """lr = 0 keeps the parameters where they are, so after ONE launch over all minibatches of an epoch (N = 77: 32 + 32 + 13 rows,
    or 50 + 27) adam_m is the last minibatch's gradient at the initial parameters.  The callback route of BC.train launches every
    minibatch alone, the order pointer offset to its first row: its adam_m after the last one and every statistics row must be the
    single launch's bit for bit (a stale gradient, feature or logit entry, or a prefetch carried across the minibatch boundary, would
    show), and every minibatch's gradient is held against the checker."""
    case = B.BY_ID[cid]
    N = 77
    orac, obs, acts = B.checker(case, N)
    block, names = H.flat_blocks(orac)
    p0 = orac.flat_params()
    clone = _clone(case, obs, acts, batch_size=batch, lr=0.0)
    _assert_path(case, clone)
    order = B.permutation(N, seed=1)
    starts = list(range(0, N, batch))
    for ent, l2 in ((0.5, 0.0), (1e-3, 0.25)):
        where = (cid, "batch %d" % batch, "ent %g l2 %g" % (ent, l2))
        _reset(clone, p0, ent, l2)
        st_one = clone.train(n_epochs=1, orders=order[None]).copy()
        m_one, _, step = H.read_device_adam_state(clone)
        assert step == len(starts) and np.array_equal(clone.policy.get_flat_params(), p0), where
        _reset(clone, p0, ent, l2)
        snaps = []
        st_each = clone.train(n_epochs=1, orders=order[None], on_batch_end=lambda: snaps.append(clone.adam_m.cpu().numpy().copy()))
        assert len(snaps) == len(starts) and np.array_equal(clone.policy.get_flat_params(), p0), where
        for i, lo in enumerate(starts):
            rows = order[lo:lo + batch]
            ref = B.reference(orac, obs[rows], acts[rows], ent, l2)
            B.assert_stats(st_each[i], ref["stats"], len(rows), where + (i,))
            H.assert_block_gradients(snaps[i], ref["g32"], ref["g64"], block, names, where + ("minibatch %d alone" % i,))
            _assert_value_head(snaps[i], p0, case, l2, where + (i,))
        H.assert_block_gradients(m_one, ref["g32"], ref["g64"], block, names, where + ("last minibatch of one launch",))
        assert np.array_equal(st_one, st_each), (where, np.abs(st_one - st_each).max(axis=1))
        assert np.array_equal(m_one, snaps[-1]), (where, int((m_one != snaps[-1]).sum()), np.abs(m_one - snaps[-1]).max())


# ---- out-of-range entries are clamped ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", B.CLAMP_CASES)
def test_bc_clamps_out_of_range_actions_and_observation_components(cid):
    """a few rows carry expert actions -1, n and n + 5 (one-hot observations: components -1 and n): gradient and statistics are the
    checker's on the clamped table"""
    case = B.BY_ID[cid]
    N = 33
    orac, obs, acts = B.checker(case, N)
    block, names = H.flat_blocks(orac)
    p0 = orac.flat_params()
    pobs, pacts, rows = B.poison(case, obs, acts)
    cobs, cacts = B.clamp(case, pobs, pacts)
    assert len(rows) >= 3 and not np.array_equal(cacts, pacts) and (not case.onehot or not np.array_equal(cobs, pobs))
    clone = _clone(case, pobs, pacts)
    path = _assert_path(case, clone)
    for ent, l2 in ((1e-3, 0.0), (0.5, 0.0)):
        where = (cid, "path %d" % path, "ent %g" % ent)
        _reset(clone, p0, ent, l2)
        st = clone.train(n_epochs=1, orders=B.permutation(N)[None])
        ref = B.reference(orac, cobs, cacts, ent, l2)
        B.assert_stats(st[0], ref["stats"], N, where)
        H.assert_block_gradients(clone.adam_m.cpu().numpy(), ref["g32"], ref["g64"], block, names, where)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in B.REFUSED])
def test_bc_train_refuses_by_name_and_touches_nothing(cid):
    from pantheonrl_amd import _native as nat
    case = B.BY_ID[cid]
    N = 33
    orac, obs, acts = B.checker(case, N)
    clone = _clone(case, obs, acts)
    assert nat.bc_train_path(clone.policy.spec) == 0
    p0 = orac.flat_params()
    clone.policy.set_flat_params(p0)
    H.load_device_adam_state(clone, np.full_like(p0, 0.5), np.full_like(p0, 0.25), 3)
    with pytest.raises(nat.NativeError) as err:
        clone.train(n_epochs=1, orders=B.permutation(N)[None])
    assert str(err.value).startswith("ph_bc_train: working set exceeds"), str(err.value)
    clone.policy.ctx.sync()
    th.cuda.synchronize()
    m, v, step = H.read_device_adam_state(clone)
    assert step == 3 and (m == 0.5).all() and (v == 0.25).all() and np.array_equal(clone.policy.get_flat_params(), p0)


def _wide_box(F):
    return B.Case("box%d-d2" % F, B.box(F), B.disc(2), 0, "the LDS limit of bc_forward_kernel")


def test_bc_forward_refuses_by_name_exactly_when_its_lds_request_exceeds_the_cu():
    """bc_forward_kernel asks for 4 P bytes of parameters plus 16 KiB of per-lane logits.  Box 1115 -> Discrete 2 has P = 36867:
    the parameters alone are under 150 KiB, the request is over 160 KiB -- refused by name before any launch (not by the
    dynamic-LDS opt-in's bare HIP error), outputs untouched.  Box 1114 (P = 36835, 163 728 bytes) is the largest that fits: it runs and matches the checker's logits."""
    from pantheonrl_amd import _native as nat
    from pantheonrl_amd.bc import FeedForward32Policy
    n, SENT = 65, -777.0
    over, fits = _wide_box(1115), _wide_box(1114)
    pol = FeedForward32Policy(H.to_space(over.obs), H.to_space(over.act), device=DEV, seed=0)
    P = pol.layout.P
    assert 36864 < P <= 38400 and 4 * P + 16384 > 160 * 1024 and 4 * P <= 150 * 1024
    obs = th.zeros((n, over.F), dtype=th.float32, device=DEV)
    acts = th.full((n, 1), int(SENT), dtype=th.int32, device=DEV)
    outs = [th.full(s, SENT, dtype=th.float32, device=DEV) for s in ((n,), (n,), (n,), (n, 2))]
    pol.ctx.set_stream(th.cuda.current_stream(th.device(DEV)).cuda_stream)
    with pytest.raises(nat.NativeError) as err:
        nat.check(pol.ctx.lib.ph_bc_forward(pol.ctx.handle, C.byref(pol.spec), pol.params.data_ptr(), obs.data_ptr(), n, None, None,
                                            None, 1, 1, 1, acts.data_ptr(), *(t.data_ptr() for t in outs)))
    assert str(err.value).startswith("ph_bc_forward: policy too large"), str(err.value)
    pol.ctx.sync()
    th.cuda.synchronize()
    assert bool((acts == int(SENT)).all()) and all(bool((t == SENT).all()) for t in outs)
    orac, x, _ = B.checker(fits, n)
    pol = FeedForward32Policy(H.to_space(fits.obs), H.to_space(fits.act), device=DEV, seed=0)
    assert 4 * pol.layout.P + 16384 <= 160 * 1024 < 4 * (pol.layout.P + 32) + 16384          # one more feature would not fit
    pol.set_flat_params(orac.flat_params())
    with th.no_grad():
        z_ref = orac.logits(th.as_tensor(x)).numpy()
    err = np.abs(pol.get_logits(x).cpu().numpy() - z_ref).max()
    print("Box 1114 -> Discrete 2 logits: device vs checker %.3g" % err)
    assert err <= B.FORWARD_TOL


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def _policy(case, orac):
    from pantheonrl_amd.bc import FeedForward32Policy
    pol = FeedForward32Policy(H.to_space(case.obs), H.to_space(case.act), device=DEV, seed=7)
    pol.set_flat_params(orac.flat_params())
    return pol


def _np(t, shape=None):
    a = t.cpu().numpy()
    return a if shape is None else a.reshape(shape)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_bc_forward_under_a_mask_teacher_forced_sampling_and_given_actions(cid):
    """n in {1, 63, 64, 65, 300} rows under a random action mask (>= 1 allowed entry per component): logits, values, log-prob and
    entropy of given actions against the checker's logits minus 30 on masked entries at 2e-5; teacher-forced uniforms against
    orc.inverse_cdf_sample on the masked softmax (a row is left out only when a uniform lies within 1e-5 of a float64 CDF edge, at
    most 1 % of rows: test_bc_checks.py), the returned log-prob being that of the returned action; out-of-range given actions and
    one-hot components behave as clamped, bit for bit."""
    case = B.BY_ID[cid]
    orac, _, _ = B.checker(case, 1)
    pol = _policy(case, orac)
    tol = B.FORWARD_TOL
    for n in B.FORWARD_ROWS:
        inp = B.forward_inputs(case, n)
        obs, mask, given, u = inp["obs"], inp["mask"], inp["given"], inp["uniforms"]
        a, v, lp, h, z = pol._launch(obs, given=given, mask=mask, want_logits=True)
        z_ref, v_ref, lp_ref, h_ref = B.masked_evaluate(orac, obs, mask, given)
        errs = dict(logits=np.abs(_np(z) - z_ref).max(), values=np.abs(_np(v, -1) - v_ref).max(),
                    log_prob=np.abs(_np(lp) - lp_ref).max(), entropy=np.abs(_np(h) - h_ref).max())
        print(cid, "n", n, "device vs checker", {k: "%.3g" % e for k, e in errs.items()})
        assert all(e <= tol for e in errs.values()), (cid, n, errs)
        assert np.array_equal(_np(a), given.astype(np.int32))
        # teacher-forced inverse-CDF sampling
        acts, v2, lp2 = pol.forward(obs, action_mask=mask, uniforms=u)
        acts = _np(acts, (n, case.A))
        want, decided = B.sampling_reference(orac, obs, mask, u)
        assert (~decided).sum() <= 0.01 * n, (cid, n, int((~decided).sum()))
        assert np.array_equal(acts[decided], want[decided]), (cid, n, np.argwhere(acts != want)[:5])
        assert (acts >= 0).all() and (acts < np.asarray(case.act.nvec)).all()
        _, _, lp_of_returned, _ = B.masked_evaluate(orac, obs, mask, acts)
        assert np.abs(_np(lp2) - lp_of_returned).max() <= tol and np.abs(_np(v2, -1) - v_ref).max() <= tol, (cid, n)
    # out-of-range entries (n = 300 rows of the last round): as clamped
    pobs, pgiven, rows = B.poison(case, obs, given)
    cobs, cgiven = B.clamp(case, pobs, pgiven)
    out_p = pol._launch(pobs, given=pgiven, mask=mask, want_logits=True)
    out_c = pol._launch(cobs, given=cgiven, mask=mask, want_logits=True)
    assert all(np.array_equal(_np(p), _np(c)) for p, c in zip(out_p, out_c)), cid
    z_ref, v_ref, lp_ref, h_ref = B.masked_evaluate(orac, cobs, mask, cgiven)
    assert np.array_equal(_np(out_p[0]), cgiven.astype(np.int32))
    assert np.abs(_np(out_p[2]) - lp_ref).max() <= tol and np.abs(_np(out_p[4]) - z_ref).max() <= tol, cid


@pytest.mark.parametrize("cid", ALL_IDS)
def test_bc_forward_philox_sampler_draws_the_masked_softmax(cid):
    """one observation row and mask repeated 65536 times: every category's frequency within 5 sqrt(p (1 - p) / n) of its float64
    probability (the draw is a function of seed, counter, row and component: nothing here can flake); the same seed and counter
    give the same draws, another counter gives others"""
    case = B.BY_ID[cid]
    n = B.PHILOX_ROWS
    orac, _, _ = B.checker(case, 1)
    pol = _policy(case, orac)
    inp = B.forward_inputs(case, 1, seed=B.SAMPLING_SEED + 1)
    obs = th.as_tensor(inp["obs"]).to(DEV).expand(n, -1).contiguous()
    mask = th.as_tensor(inp["mask"]).to(DEV).expand(n, -1).contiguous()

    def draw(counter):
        pol._counter = counter - 1            # _launch advances the counter before it passes it on
        return _np(pol.forward(obs, action_mask=mask)[0], (n, case.A))
    a = draw(10)
    assert np.array_equal(a, draw(10))
    b = draw(11)
    probs = B.component_probabilities(orac, inp["obs"][0], inp["mask"][0])
    for c, p in enumerate(probs):
        if p.max() < 0.99:                    # a component the mask leaves one entry has one draw
            assert (a[:, c] != b[:, c]).any(), (cid, c)
        for drawn in (a, b):
            f = np.bincount(drawn[:, c], minlength=len(p)) / n
            bound = 5.0 * np.sqrt(p * (1.0 - p) / n)
            assert (np.abs(f - p) <= bound).all(), (cid, c, f, p, bound)
