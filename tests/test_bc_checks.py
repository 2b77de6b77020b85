"""CPU: what makes tests/test_gpu_bc_shapes.py trustworthy.  On the checker alone: the per-block gradient rule rejects the ways a BC
kernel could be subtly wrong on each shape class of tests/bc_cases.py, the case table's dispatch column is the library's own answer,
and the exclusion cap of the teacher-forced sampling test holds for the inputs that test uses."""
import os

import numpy as np
import pytest

from oracle import sb3_oracle as orc
from tests import bc_cases as B
from tests import helpers as H
from tests.optimizer_cases import bc_flat_grads

N = 33
IDS = [c.id for c in B.CASES]


@pytest.fixture(scope="module")
def units():
    """per case: the checker, N rows, and the references at the three weight settings -- computed once, never changed"""
    out = {}
    for case in B.CASES:
        orac, obs, acts = B.checker(case, N)
        block, names = H.flat_blocks(orac)
        out[case.id] = dict(case=case, orac=orac, obs=obs, acts=acts, block=block, names=names,
                            ref={w: B.reference(orac, obs, acts, *w) for w in B.WEIGHTS})
    return out


def _rejected(wrong, ref, u, where):
    try:
        H.assert_block_gradients(wrong, ref["g32"], ref["g64"], u["block"], u["names"], where)
    except AssertionError:
        return True
    return False


def test_the_table_names_every_path_and_its_dispatch_column_is_the_librarys():
    from pantheonrl_amd import _native as nat
    assert {c.path for c in B.CASES} == {0, 1, 2, 3}
    valu_only = os.environ.get("PH_BC_MFMA", "1").startswith("0")
    for c in B.CASES:
        assert nat.bc_train_path(B.native_spec(c)) == (min(c.path, 1) if valu_only else c.path), c.id
        assert B.offsets(c)["P"] == sum(p.numel() for p in orc.FeedForward32Oracle(c.obs, c.act).parameters())


def test_flat_gradient_has_the_layout_of_bc_flat_grads():
    """B.gradient reads the gradient through helpers.flat_grads_exact; where every parameter has one (l2_weight > 0) that is
    optimizer_cases.bc_flat_grads entry for entry"""
    import copy
    import torch as th
    case = B.BY_ID["box33-3x30x7"]
    orac, obs, acts = B.checker(case, N)
    g, _ = B.gradient(orac, obs, acts, 1e-3, 0.25)
    c = copy.deepcopy(orac)
    orc.bc_loss(c, th.as_tensor(obs), th.as_tensor(acts), 1e-3, 0.25)[0].backward()
    assert np.array_equal(g, bc_flat_grads(c))
    o = B.offsets(case)
    assert np.array_equal(g[o["val_W"]:], 0.25 * orac.flat_params().astype(np.float64)[o["val_W"]:])


@pytest.mark.parametrize("cid", IDS)
def test_the_float32_checker_passes_its_own_bound(units, cid):
    u = units[cid]
    for w in B.WEIGHTS:
        assert not _rejected(u["ref"][w]["g32"], u["ref"][w], u, (cid, w))
        assert not _rejected(u["ref"][w]["g64"], u["ref"][w], u, (cid, w, "float64"))


@pytest.mark.parametrize("cid", IDS)
def test_a_dropped_entropy_term_is_rejected_at_weight_one_half(units, cid):
    u = units[cid]
    without, _ = B.gradient(u["orac"], u["obs"], u["acts"], 0.0, 0.0, double=True)
    assert _rejected(without, u["ref"][(0.5, 0.0)], u, (cid, "no entropy term, ent_weight 0.5"))
    # at the default weight the term is about the size of the tolerance: this is why the 0.5 setting exists (figure, no assertion)
    print(cid, "entropy term dropped at ent_weight 1e-3: rejected =",
          _rejected(without, u["ref"][(1e-3, 0.0)], u, (cid, "no entropy term, ent_weight 1e-3")))


@pytest.mark.parametrize("cid", IDS)
def test_a_fixed_one_over_32_is_rejected(units, cid):
    u = units[cid]
    ref = u["ref"][(1e-3, 0.0)]
    assert _rejected(ref["g64"] * (N / 32.0), ref, u, (cid, "1/32 for 1/nb"))


@pytest.mark.parametrize("cid", IDS)
def test_a_zeroed_last_row_of_W1_is_rejected(units, cid):
    """the row next to the F -> Fpad padding"""
    u = units[cid]
    ref, o = u["ref"][(1e-3, 0.0)], B.offsets(u["case"])
    wrong = ref["g64"].copy()
    wrong[o["b1"] - orc.BC_HIDDEN:o["b1"]] = 0
    assert _rejected(wrong, ref, u, (cid, "dW1's last row zero"))


@pytest.mark.parametrize("cid", [c.id for c in B.CASES if c.L > 32])
def test_a_zeroed_logit_column_32_is_rejected(units, cid):
    """the first column of the second logit tile"""
    u = units[cid]
    ref, o, L = u["ref"][(1e-3, 0.0)], B.offsets(u["case"]), u["case"].L
    for what in ("act_W", "act_b"):
        wrong = ref["g64"].copy()
        if what == "act_W":
            wrong[o["act_W"] + 32:o["act_b"]:L] = 0
        else:
            wrong[o["act_b"] + 32] = 0
        assert _rejected(wrong, ref, u, (cid, what + " column 32 zero"))


@pytest.mark.parametrize("cid", IDS)
def test_skipping_the_rows_with_an_out_of_range_action_is_rejected(units, cid):
    """the kernels clamp an expert action into its range; one that dropped such a row instead (its 1/nb unchanged) is caught"""
    u = units[cid]
    case = u["case"]
    obs, acts, rows = B.poison(case, u["obs"], u["acts"])
    cobs, cacts = B.clamp(case, obs, acts)
    assert not np.array_equal(cacts, acts) and cacts.min() >= 0 and (cacts < np.asarray(case.act.nvec)).all()
    if case.onehot:
        assert not np.array_equal(cobs, obs) and cobs.min() >= 0 and (cobs < np.asarray(case.obs.nvec)).all()
    ref = B.reference(u["orac"], cobs, cacts, 1e-3, 0.0)
    good = np.setdiff1d(np.arange(N), rows)
    skipped, _ = B.gradient(u["orac"], cobs[good], cacts[good], 1e-3, 0.0, double=True)
    assert _rejected(skipped * (len(good) / N), ref, u, (cid, "out-of-range rows skipped"))


@pytest.mark.parametrize("cid", IDS)
def test_a_dropped_l2_term_is_rejected_at_weight_one_quarter(units, cid):
    u = units[cid]
    assert _rejected(u["ref"][(1e-3, 0.0)]["g64"], u["ref"][(1e-3, 0.25)], u, (cid, "no L2 term, l2_weight 0.25"))


@pytest.mark.parametrize("cid", IDS)
def test_sampling_inputs_leave_at_most_one_percent_of_rows_undecided(cid):
    """the teacher-forced sampling test drops a row only when a uniform lies within 1e-5 of a float64 CDF edge: with the seed of
    bc_cases.forward_inputs that is at most 1 % of the rows of every case at every row count, on the checker alone"""
    case = B.BY_ID[cid]
    orac, _, _ = B.checker(case, 1)
    for n in B.FORWARD_ROWS:
        inp = B.forward_inputs(case, n)
        lo = 0
        for k in case.act.nvec:                     # the mask leaves every component an allowed entry
            assert inp["mask"][:, lo:lo + k].any(axis=1).all()
            lo += k
        assert n < 63 or not inp["mask"].all()
        acts, decided = B.sampling_reference(orac, inp["obs"], inp["mask"], inp["uniforms"])
        assert (~decided).sum() <= 0.01 * n, (cid, n, int((~decided).sum()))
        assert acts.shape == (n, case.A) and (acts >= 0).all() and (acts < np.asarray(case.act.nvec)).all()
        # a sampled action is (almost) never a masked one: its probability carries e^-30
        lo = 0
        for c, k in enumerate(case.act.nvec):
            assert inp["mask"][np.arange(n), lo + acts[:, c]][decided].all()
            lo += k
