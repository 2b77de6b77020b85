"""CPU: what tests/sharp_cases.py claims about its cases, proven on the checker alone -- nothing of the device is involved.

Populations: the sharpened cases hold what tests/test_gpu_sharp.py is there for (probabilities under float32's smallest denormal,
rows of entropy < 1e-6 beside soft rows in the same launch, few rows near a CDF edge).  Reach: every wrong head of
sharp_cases.MUTANTS, restated in numpy float32 on the checker's float32 logits, misses the allowance of the output named by a
factor of 10 or more or hands out a non-finite value, while the restatement of the head as ph_rowtail.h writes it passes everything.
Every mutant is printed with its miss factor (run with -s).

Four forward cases cannot hold the saturated populations and are listed in NOT_SATURATING with the reason; they stay in the GPU
test (their allowances hold as for every case), the population asserts and the mutants that need an underflowed probability are
required on the others."""
import numpy as np
import pytest

from tests import helpers as H
from tests import offpolicy_cases as OC
from tests import sampler_cases as S
from tests import sharp_cases as SC

# forward cases whose checker cannot reach the saturated regime by a scaled head alone (measured here, asserted below at what they do reach)
NOT_SATURATING = {
    "rps": "one distinct observation (Discrete(1)): every row is the same row -- all saturated or none",
    "modular-rps": "one distinct observation, and the main head (not scaled) is part of the logits",
    "bc-liar": "bc_cases perturbs the head by 0.06 N(0, 1), a fifth of helpers.oracle_policy: x30 reaches 1e-19, no row below entropy 1e-6",
    "bc-box33-3x30x7": "as bc-liar: x30 reaches 1e-31",
}
SATURATING = [f.id for f in SC.FORWARD if f.id not in NOT_SATURATING]
F32_DENORMAL = 1e-45


def _big_rows(fc):
    return [n for n in fc.rows if n >= SC.POPULATION_ROWS]


def near_cap(n: int) -> int:
    """at most 3 % of the rows, and two rows where 3 % is less (n = 65, three components of 40 edges: bc-box33-3x30x7 has 2 near rows)"""
    return max(2, int(0.03 * n))


# ---- sharpen ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [f.id for f in SC.FORWARD])
def test_sharpen_moves_the_heads_alone_and_leaves_the_cached_checker(cid):
    fc = SC.FORWARD_BY_ID[cid]
    before = {k: v.clone() for k, v in S.checker(cid).state_dict().items()}
    sharp = SC.checker(cid, 30)
    after = S.checker(cid).state_dict()
    assert all((before[k] == after[k]).all() for k in before), "the cached checker moved"
    head_ids = {id(p) for h in SC.heads(sharp) for p in h.parameters()}
    for (name, p), (_, q) in zip(sharp.named_parameters(), S.checker(cid).named_parameters()):
        if id(p) in head_ids:
            assert np.array_equal(p.detach().numpy(), (q.detach() * 30.0).numpy()), name
        else:
            assert np.array_equal(p.detach().numpy(), q.detach().numpy()), name
    n = fc.rows[-1]
    obs, _ = S.inputs(fc.case, n)
    assert np.array_equal(SC.logits_values(fc.case, sharp, obs)[1], SC.logits_values(fc.case, S.checker(cid), obs)[1]), "values moved"


# ---- populations -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SATURATING)
def test_saturated_and_sharp_populations(cid):
    fc = SC.FORWARD_BY_ID[cid]
    assert _big_rows(fc), cid
    for n in _big_rows(fc):
        r30, r8 = SC.reference(cid, 30, n), SC.reference(cid, 8, n)
        pmin30, pmin8 = min(p.min() for p in r30.p64), min(p.min() for p in r8.p64)
        low, soft = int((r30.H64 < 1e-6).sum()), int((r30.H64 > 0.1).sum())
        print(cid, "n", n, "x30: smallest p %.1e, entropy < 1e-6 on %d rows, > 0.1 on %d; x8: smallest p %.1e, entropy > 1e-6 on %d rows"
              % (pmin30, low, soft, pmin8, int((r8.H64 > 1e-6).sum())))
        assert pmin30 < F32_DENORMAL, (cid, n, pmin30)
        assert low >= 3 and low >= 0.04 * n, (cid, n, low)
        assert soft >= 0.05 * n, (cid, n, soft)
        assert pmin8 < 1e-12, (cid, n, pmin8)
        assert (r8.H64 > 1e-6).sum() >= 0.5 * n, (cid, n)


@pytest.mark.parametrize("cid", sorted(NOT_SATURATING))
def test_cases_that_cannot_saturate_are_sharp_all_the_same(cid):
    """what the four other cases do reach at x30: a probability below 1e-10, five orders under anything the unsharpened suite sees"""
    fc = SC.FORWARD_BY_ID[cid]
    for n in _big_rows(fc):
        r = SC.reference(cid, 30, n)
        pmin = min(p.min() for p in r.p64)
        print(cid, "n", n, "x30: smallest p %.1e, entropy < 1e-6 on %d rows (%s)" % (pmin, int((r.H64 < 1e-6).sum()), NOT_SATURATING[cid]))
        assert pmin < 1e-10, (cid, n, pmin)


@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("cid", [f.id for f in SC.FORWARD])
def test_few_rows_are_near_a_cdf_edge(cid, scale):
    """a condition on the inputs: near rows are left out of the sampled-action comparison only, never of the teacher-forced ones"""
    fc = SC.FORWARD_BY_ID[cid]
    for n in fc.rows:
        r = SC.reference(cid, scale, n)
        for c in S.COUNTERS:
            near = r.prediction(c)[2]
            assert near.sum() <= near_cap(n), (cid, scale, n, c, int(near.sum()))


# ---- the real head passes, the wrong heads miss ------------------------------------------------------------------------------------------
def _forward_errors(r, variant="real", z=None):
    """-> dict(output -> miss factor) of tail32(variant) against the float32 checker over the three action sets, the sampled actions
    (mismatches off near rows) and the argmax (mismatches on decided rows)"""
    z = r.z32 if z is None else z
    out = {}
    for name, acts in r.action_sets().items():
        t = SC.tail32(z, r.nvec, acts=acts, variant=variant)
        lp32, _, A_lp, _ = r.log_probs(acts)
        out["logp/" + name] = SC.miss(np.abs(t["logp"].astype(np.float64) - lp32), A_lp)
        out["entropy/" + name] = SC.miss(np.abs(t["entropy"].astype(np.float64) - r.H32), r.A_H)
        if np.isfinite(t["entropy"]).all() and not (t["entropy"] >= -r.A_H).all():
            out["entropy/" + name] = float("inf")
    bad = 0
    for c in S.COUNTERS:
        u, want, near = r.prediction(c)
        t = SC.tail32(z, r.nvec, u=u, variant=variant)
        bad += int(((t["actions"] != want).any(axis=1) & ~near).sum())
    out["sampled"] = bad
    arg, ok = r.decided_argmax()
    out["argmax"] = int(((SC.tail32(z, r.nvec, variant=variant)["actions"] != arg).any(axis=1) & ok).sum())
    out["decided"] = int(ok.sum())
    return out


@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("cid", [f.id for f in SC.FORWARD])
def test_the_head_as_the_row_tail_writes_it_passes_every_allowance(cid, scale):
    fc = SC.FORWARD_BY_ID[cid]
    for n in fc.rows:
        e = _forward_errors(SC.reference(cid, scale, n))
        print(cid, "x%d" % scale, "n", n, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in e.items()})
        assert e["sampled"] == 0 and e["argmax"] == 0, (cid, scale, n, e)
        assert all(v <= 1.0 for k, v in e.items() if "/" in k), (cid, scale, n, e)
        assert e["decided"] >= 0.9 * n, (cid, scale, n, e["decided"])


def _largest(cid, scale):
    fc = SC.FORWARD_BY_ID[cid]
    return SC.reference(cid, scale, fc.rows[-1])


def test_m1_softmax_without_the_max_subtraction():
    hit = []
    for fc in SC.FORWARD:
        r = _largest(fc.id, 30)
        zmax = float(r.z32.max())
        e = _forward_errors(r, "M1")
        worst = min(max(e["logp/" + s], e["entropy/" + s]) for s in ("most", "least", "random"))
        print("M1", fc.id, "largest logit %.1f" % zmax, "log-prob miss", {s: e["logp/" + s] for s in ("most", "least", "random")},
              "entropy miss", e["entropy/most"])
        if zmax > 89.0:
            hit.append(fc.id)
            assert worst >= 10.0 and e["logp/most"] >= 10.0 and e["entropy/most"] >= 10.0, (fc.id, e)
    assert len(hit) >= len(SC.FORWARD) / 2, hit


@pytest.mark.parametrize("cid", SATURATING)
def test_m2_log_of_the_softmax_and_m3_entropy_from_the_probabilities(cid):
    r = _largest(cid, 30)
    e2, e3 = _forward_errors(r, "M2"), _forward_errors(r, "M3")
    print("M2", cid, "log-prob of the least likely set misses by", e2["logp/least"], "| M3 entropy misses by", e3["entropy/most"])
    assert e2["logp/least"] >= 10.0, (cid, e2)
    assert e3["entropy/most"] >= 10.0, (cid, e3)


def test_m2_m3_on_the_cases_that_cannot_saturate_are_reported():
    for cid in sorted(NOT_SATURATING):
        r = _largest(cid, 30)
        print("M2", cid, "misses by", _forward_errors(r, "M2")["logp/least"], "| M3 by", _forward_errors(r, "M3")["entropy/most"],
              "(not required: no probability underflows)")


@pytest.mark.parametrize("cid", SC.MASKED)
def test_m4_the_mask_as_minus_infinity(cid):
    r = _largest(cid, 30)
    on = r.mask.astype(bool)
    masked_top = int(np.any([~m[np.arange(r.n), z.argmax(axis=1)] for z, m in zip(SC.split(r.z64, r.nvec), SC.split(on, r.nvec))],
                            axis=0).sum())
    saturating = cid in SATURATING      # (the BC case's logits span less than 30: no masked logit stays on top, the argmax cannot tell)
    assert masked_top >= 3 or not saturating, (cid, masked_top)
    z = np.where(on, r.raw32, -np.inf).astype(np.float32)
    e = _forward_errors(r, "real", z=z)
    print("M4", cid, "rows whose largest logit after the offset is a masked one:", masked_top, "| log-prob of the random set misses by",
          e["logp/random"], "| argmax differs on", e["argmax"], "decided rows")
    assert e["logp/random"] >= 10.0 and (e["argmax"] >= 1 or not saturating), (cid, e)


M5_NOT_REQUIRED = ("rps",)      # one distinct row whose unnormalised sum is 1 + 1e-4: a draw lands in the gap once in 1e4 rows


@pytest.mark.parametrize("cid", [f.id for f in SC.FORWARD])
def test_m5_inverse_cdf_against_unnormalised_prefix_sums(cid):
    r = _largest(cid, 8)
    e = _forward_errors(r, "M5")
    print("M5", cid, "sampled actions off near rows differ on", e["sampled"], "of", 2 * r.n, "draws")
    if cid not in M5_NOT_REQUIRED:
        assert e["sampled"] >= 1, (cid, e)


# ---- gradient cases ------------------------------------------------------------------------------------------------------------------
def _ppo_case(gid, scale, nb):
    g = SC.GRAD_BY_ID[gid]
    b = SC.build(g, scale, nb)
    g32, g64, st32, st64 = SC.checker_gradients(b["c"], b["orac"], b["ob"], b["idx"])
    lp, ent = SC.minibatch_log_probs(b["c"], b["orac"], b["ob"], b["idx"])
    block, names = H.flat_blocks(b["orac"], OC.flat_fn(b["c"]))
    import copy
    mutant = copy.deepcopy(b["orac"])
    with SC.dead_saturated_rows(mutant):
        loss, _ = OC.checker_loss(b["c"], mutant, OC.minibatch(b["ob"], b["idx"]), OC.context_samples(b["c"], len(b["idx"])))
        loss.backward()
    gm = H.flat_grads_exact(mutant, OC.flat_fn(b["c"]))
    return g, g32, g64, st32, st64, lp, ent, block, names, gm, b["orac"]


def _bc_case(gid, scale, nb):
    from tests import bc_cases as B
    g = SC.GRAD_BY_ID[gid]
    b = SC.bc_build(g, scale, nb)
    ent_w, l2 = SC.BC_WEIGHTS[1]
    ref = B.reference(b["orac"], b["obs"], b["acts"], ent_w, l2)
    lp, ent = SC.bc_log_probs(b)
    block, names = H.flat_blocks(b["orac"])
    with SC.dead_saturated_rows(b["orac"]):
        gm, _ = B.gradient(b["orac"], b["obs"], b["acts"], ent_w, l2)
    return g, ref["g32"], ref["g64"], ref["stats"], None, lp, ent, block, names, gm, b["orac"]


@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("gid", [g.id for g in SC.GRAD_CASES])
def test_gradient_cases_hold_unlikely_actions_and_reach_every_block(gid, scale):
    """the minibatch holds actions of log-prob below -40 on at least 10 % of its rows at x30; every parameter block the loss reaches
    (sharp_cases.reached_blocks) is non-zero in the float64 gradient; both gradients and every statistic are finite; mutant G1
    (saturated rows contribute nothing) misses a block allowance by 10x or more at x30.  Two exceptions, both printed:
    - the BC checkers hold no row of entropy below 1e-6 (bc_cases perturbs the head a fifth as much): G1 has no row to kill;
    - ADAP's context term: torch's float32 kl_divergence returns inf wherever q's float32 probability is exactly 0, so at x30 the
      float32 checker's context loss departs from the float64 one by 15 to 35 % (sharp_cases.context_term_degenerate).  There the
      float64 checker is the reference, on the CPU here as in the GPU test, and G1 is held against that."""
    for nb in SC.NBS:
        g, g32, g64, st32, st64, lp, ent, block, names, gm, orac = (_bc_case if gid.startswith("bc-") else _ppo_case)(gid, scale, nb)
        unlikely = int((lp < SC.LOGP_UNLIKELY).sum())
        ref, _, swapped = SC.gradient_reference(g32, g64, st32, st64) if st64 is not None else (g32, st32, False)
        if swapped:
            gm = gm + (g64 - g32)       # the mutant's defect, carried over to the float64 reference
        misses = SC.block_misses(gm, ref, g64, block, names)
        reached = SC.reached_blocks(g, orac, names)
        print(gid, "x%d" % scale, "nb", nb, "rows with log-prob < -40:", unlikely, "smallest %.1f" % lp.min(), "entropy < 1e-6 on",
              int((ent < 1e-6).sum()), "| G1 misses its worst block by %.3g" % misses.max(), "(against the float64 checker)" if swapped else "")
        assert np.isfinite(g32).all() and np.isfinite(g64).all(), gid
        assert all(np.isfinite(v) for v in st32.values()), st32
        for b, name in enumerate(names):
            assert (np.abs(g64[block == b]).max() > 0) == bool(reached[b]), (gid, name)
        if scale == 30:
            assert unlikely >= SC.UNLIKELY_SHARE * nb, (gid, nb, unlikely)
            if gid.startswith("bc-"):
                assert not (ent < 1e-6).any(), gid
            else:
                assert misses.max() >= 10.0, (gid, nb, misses.max())


def test_sharpen_inside_a_grad_pair_is_the_checker_the_cases_build():
    """the hook the families' _grad_pair take and sharp_cases.build make the same checker and the same buffer"""
    g = SC.GRAD_BY_ID["ppo-liar-m0"]
    a, b = SC.build(g, 30, 77), SC.build(g, 30, 77)
    assert np.array_equal(a["orac"].flat_params(), b["orac"].flat_params())
    for k in ("observations", "actions", "log_probs", "advantages", "returns", "values"):
        assert np.array_equal(getattr(a["ob"], k), getattr(b["ob"], k)), k
    plain = OC.checker(g.oc(77), OC.SEED)
    assert np.array_equal(SC.preparer(30)(plain).flat_params(), a["orac"].flat_params())
