"""The off-policy cases of the gradient tests: every caller of the row loss (ph_ppo_loss.h) on a STALE buffer.

In the older single-minibatch gradient tests the policy under differentiation is the policy that filled the buffer, so ratio == 1 and
v == old_v on every row: only the tie arm of the policy gate and only `pass = 1` of the value clip ever run.  Here a drifted copy of
the checker fills the buffer (helpers.stale_oracle_buffer) and the checker itself is differentiated, so each minibatch holds rows of
all eight classes (helpers.offpolicy_rows):

    P1 ratio > 1+c, adv > 0   clipped, zero policy gradient        V1 v - old_v >  c_vf   clipped, zero value gradient
    P2 ratio > 1+c, adv < 0   outside the range but live           V2 v - old_v < -c_vf   clipped
    P3 ratio < 1-c, adv > 0   live                                 V3 inside              live
    P4 ratio < 1-c, adv < 0   clipped
    P5 inside the range       live

Edge rule: a row with |ratio - (1 +- c)| < 1e-4 s ratio or ||v - old_v| - c_vf| < 1e-4 s (s = max(1, w_last / 64), five times the
forward tolerance 2e-5 s) may legitimately fall on the other side of a clip on the device; such rows are taken out of `idx` BEFORE
either side sees the minibatch (a flipped row changes its whole contribution, it cannot be masked afterwards).  At most 2 % of the
candidate rows may go that way (tests/test_offpolicy_checks.py asserts the cap).

`drift` and `clip_range_vf` are inputs, chosen per case on the checker alone so that every class holds >= 5 % of the minibatch and
>= 3 rows and ratios stay within [0.05, 20] (test_offpolicy_checks.py asserts it); clip_range_vf never equals clip_range, so that
counting clip_fraction with the wrong range changes the count.  Half the cases run normalize_advantage=False with clip_range=0.1,
the rest the defaults (Modular's loss always normalises); every case sets clip_range_vf; every second one has a minibatch that is no
multiple of the 64-row tile.

Which kernel (which caller of the row loss) each case lands on -- read off launch_ppo_grad / grad_fast_eligible / select_gemm
(ph_ppo.hip, ph_ppo_fast.hip, ph_abi.hip), ph_arch.hip, ph_modular.hip, ph_adap.hip, ph_adapmult.hip -- is the `kernel` field."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import arch_oracle as A
from tests import helpers as H
from tests import adapmult_cases as AM
from tests import modular_cases as M

SEED = 11


@dataclass(frozen=True)
class Case:
    family: str                 # ppo | arch | modular | adap | adapmult   (the ph_*_minibatch_grad entry point)
    config: str
    gemm_mode: int
    T: int
    E: int
    nb: int                     # candidate rows; edge rows are removed from these
    drift: float
    clip_range: float
    clip_range_vf: Optional[float]
    normalize_advantage: bool
    ent_coef: float
    kernel: str
    arch: Optional[Tuple[int, ...]] = None      # arch
    K: int = 0                                  # modular: partners
    partner: int = 0
    coef: Optional[float] = None                # modular: marginal_reg_coef; adap / adapmult: context_loss_coeff (None: no term)

    @property
    def id(self) -> str:
        extra = "x".join(map(str, self.arch)) if self.arch else ("K%dp%d" % (self.K, self.partner) if self.K else "")
        return "-".join(x for x in (self.family, self.config, extra, "m%d" % self.gemm_mode, "nb%d" % self.nb) if x)

    @property
    def scale(self) -> float:
        return max(1.0, self.arch[-1] / 64.0) if self.arch else 1.0


def _raw(family, config, mode, T, E, nb, drift, cvf, kernel, **kw):
    """normalize_advantage=False, clip_range=0.1"""
    return Case(family, config, mode, T, E, nb, drift, 0.1, cvf, False, 0.01, kernel, **kw)


def _dflt(family, config, mode, T, E, nb, drift, cvf, kernel, **kw):
    """the defaults (clip_range 0.2, normalised advantages) with clip_range_vf set"""
    return Case(family, config, mode, T, E, nb, drift, 0.2, cvf, True, 0.0, kernel, **kw)


FAST = "ppo_grad_fast_kernel (ph_ppo_fast.hip: one chunk, Discrete <= 8)"
SPLIT = "ppo_grad_split_kernel (ph_ppo_split.hip), "
SPLIT_OH = "ppo_grad_split_oh_kernel (ph_ppo_split_oh.hip), "
GEN = "ppo_grad_kernel (ph_ppo.hip), "
ARCH = "arch_grad kernels (ph_arch.hip: policy tail and value tail), "

CASES = [
    # ---- ph_ppo_minibatch_grad -----------------------------------------------------------------------------------------------------
    _raw("ppo", "overcooked", 0, 16, 8, 100, 0.03, 0.15, FAST + ", MFMA tiles"),
    _dflt("ppo", "overcooked", 1, 16, 8, 77, 0.03, 0.15, FAST + ", fmaf restatement (bits of mode 0)"),
    _raw("ppo", "overcooked", 2, 16, 8, 100, 0.03, 0.15, SPLIT + "NK 8, folded bias"),
    _dflt("ppo", "box64", 2, 16, 8, 77, 0.03, 0.15, SPLIT + "NK 8, no free column"),
    _raw("ppo", "box1", 2, 16, 8, 100, 0.1, 0.05, SPLIT + "NK 2, one feature"),
    _dflt("ppo", "liar", 0, 16, 8, 77, 0.03, 0.15, GEN + "one-hot, H16 per-component tail, Lp 32"),
    _raw("ppo", "quad16", 0, 16, 8, 100, 0.03, 0.05, GEN + "Box, H16 per-component tail, Lp 64"),
    _dflt("ppo", "wide", 0, 16, 8, 77, 0.03, 0.15, GEN + "Box, three chunks, two-pass MultiDiscrete tail (a 30-way component)"),
    _raw("ppo", "onehot17", 0, 16, 8, 100, 0.03, 0.15, GEN + "one-hot, two-pass MultiDiscrete tail (a 17-way component)"),
    # no single-chunk config reaches the `nd.A == 1 && L <= 8` tail of ppo_grad_kernel (grad_fast_eligible takes them all); a Discrete(6)
    # head behind TWO feature chunks does
    _dflt("ppo", "adap_oc", 0, 16, 8, 77, 0.03, 0.15, GEN + "Box, two chunks, the `A == 1 && L <= 8` register tail"),
    _raw("ppo", "liar", 2, 16, 8, 100, 0.03, 0.15, SPLIT_OH + "one-hot form, five chunks"),
    _dflt("ppo", "onehot32", 2, 16, 8, 77, 0.03, 0.05, SPLIT_OH + "one-hot form, 32 logits in three components"),
    _raw("ppo", "discrete20", 2, 16, 8, 100, 0.1, 0.05, SPLIT_OH + "one-hot form, one 20-way head"),
    _dflt("ppo", "box130", 2, 16, 8, 77, 0.03, 0.15, SPLIT_OH + "Box form, three chunks"),
    _raw("ppo", "gauss5", 0, 16, 8, 100, 0.015, 0.07, GEN + "Gaussian tail (ratio from a squared residual), A 5"),
    _dflt("ppo", "gauss16", 0, 16, 8, 77, 0.015, 0.07, GEN + "Gaussian tail, A 16"),
    _dflt("ppo", "gauss5", 1, 16, 8, 77, 0.015, 0.07, GEN + "Gaussian tail, fmaf restatement (bits of mode 0)"),
    # ---- ph_arch_minibatch_grad ----------------------------------------------------------------------------------------------------
    _raw("arch", "overcooked", 0, 16, 8, 100, 0.04, 0.15, ARCH + "one 32-wide layer", arch=(32,)),
    _dflt("arch", "overcooked", 1, 16, 8, 77, 0.03, 0.15, ARCH + "128-128 (bits of mode 0)", arch=(128, 128)),
    _raw("arch", "overcooked", 0, 16, 8, 100, 0.03, 0.15, ARCH + "96-160-32", arch=(96, 160, 32)),
    _dflt("arch", "liar", 0, 16, 8, 77, 0.03, 0.15, ARCH + "one 32-wide layer, MultiDiscrete", arch=(32,)),
    _raw("arch", "liar", 0, 16, 8, 100, 0.03, 0.15, ARCH + "128-128, MultiDiscrete", arch=(128, 128)),
    _dflt("arch", "liar", 2, 16, 8, 77, 0.03, 0.15, ARCH + "96-160-32, MultiDiscrete (bits of mode 0)", arch=(96, 160, 32)),
    # ---- ph_modular_minibatch_grad: K = 2, both partners, coef > 0 -----------------------------------------------------------------------
    _dflt("modular", "mod_oc", 0, 16, 16, 100, 0.03, 0.15, "modular_grad kernels (ph_modular.hip: policy tail and value tail)", K=2, partner=0,
          coef=0.5),
    _dflt("modular", "mod_oc", 1, 16, 16, 77, 0.03, 0.15, "modular_grad kernels, fmaf restatement (bits of mode 0)", K=2, partner=1, coef=0.5),
    # ---- ph_adap_minibatch_grad ----------------------------------------------------------------------------------------------------------
    _raw("adap", "adap_oc", 0, 16, 8, 100, 0.03, 0.15, GEN + "the `A == 1 && L <= 8` register tail, plus the context term", coef=1.0),
    _dflt("adap", "adap_small", 0, 16, 8, 77, 0.03, 0.15, FAST + ", plus the context term", coef=1.0),
    # ---- ph_adapmult_minibatch_grad --------------------------------------------------------------------------------------------------------
    _raw("adapmult", "adap_oc", 0, 16, 8, 100, 0.03, 0.15, "am_loss_pi_kernel + am_loss_vf_kernel (ph_adapmult.hip), with the context term",
         coef=1.0),
    _dflt("adapmult", "adap_small", 0, 16, 8, 77, 0.03, 0.15, "am_loss_pi_kernel + am_loss_vf_kernel, PPO terms alone"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- the checker side of a case ------------------------------------------------------------------------------------------------
def hyper(c: Case) -> orc.PPOHyper:
    return orc.PPOHyper(clip_range=c.clip_range, clip_range_vf=c.clip_range_vf, normalize_advantage=c.normalize_advantage,
                        ent_coef=c.ent_coef)


def checker(c: Case, seed: int = SEED):
    """the policy under test, as the family's _grad_pair builds it for `seed`"""
    if c.family == "arch":
        return A.oracle_policy(c.config, c.arch, seed=seed)
    if c.family == "modular":
        return M._oracle(c.config, c.K, seed=seed)
    if c.family == "adapmult":
        return AM._oracle(c.config, seed=seed)
    return H.oracle_policy(c.config, seed=seed)


def flat_fn(c: Case):
    return M._flat if c.family == "modular" else None


def eval_kw(c: Case) -> dict:
    return dict(partner_idx=c.partner) if c.family == "modular" else {}


def fill(c: Case):
    """the buffer builder the family's _grad_pair takes in place of its own: (name, checker, T, E, seed=) -> a STALE buffer"""
    inner = None
    if c.family == "modular":
        def inner(name, beh, T, E, seed=0):
            return M._filled(beh, name, c.partner, T, E, seed=seed)

    def stale(name, orac, T, E, seed=0, **kw):
        return H.stale_oracle_buffer(name, orac, T, E, seed=seed, drift=c.drift, fill=inner)
    return stale


def minibatch(ob, idx) -> dict:
    return {k: th.as_tensor(v[idx]) for k, v in ob.flat().items()}


def rows(c: Case, o64, ob, idx) -> dict:
    return H.offpolicy_rows(o64, minibatch(ob, idx), hyper(c), s=c.scale, always_normalize=c.family == "modular", **eval_kw(c))


def pick_idx(c: Case, record: Optional[dict] = None):
    """the `idx` the family's _grad_pair takes: (checker, buffer) -> the case's candidate rows without the edge rows"""
    def pick(orac, ob):
        cand = np.random.default_rng(c.nb).permutation(c.T * c.E)[:c.nb]
        edge = rows(c, H.double_copy(orac)[0], ob, cand)["edge"]
        if record is not None:
            record.update(candidates=cand, edge=edge)
        return cand[~edge]
    return pick


def context_samples(c: Case, nb: int, seed: int = SEED):
    """ADAP's teacher-forced samples (state positions, contexts) for a minibatch of nb rows, or None"""
    if c.coef is None or c.family not in ("adap", "adapmult"):
        return None
    from tests.adap_cases import CTX, _context_samples
    return _context_samples(CTX[c.config], nb, 5, 32, seed)


def checker_loss(c: Case, orac, mb, samples=None):
    """(loss, stats) of the family's own minibatch loss on checker `orac` (float32, or a float64 copy inside float64_checker)"""
    hp = hyper(c)
    if c.family == "modular":
        return orc.modular_minibatch_loss(orac, mb, hp, c.partner, c.coef)
    loss, stats = orc.ppo_minibatch_loss(orac, mb, hp)
    if samples is not None:
        from tests.adap_cases import CTX
        sidx, ctxs = samples
        cl = orc.adap_context_loss(orac, mb["observations"], CTX[c.config], sidx[sidx >= 0], ctxs)
        loss = loss + c.coef * cl
        stats["context_loss"], stats["loss"] = cl.item(), loss.item()
    return loss, stats


def checker_gradients(c: Case, orac, ob, idx):
    """-> (g32, g64, stats32): the family's loss differentiated on the float32 checker and on its float64 copy, in flat order"""
    mb = minibatch(ob, idx)
    samples = context_samples(c, len(idx))
    o64 = H.double_copy(orac)[0]
    for p in orac.parameters():
        p.grad = None
    loss, stats = checker_loss(c, orac, mb, samples)
    loss.backward()
    g32 = H.flat_grads_exact(orac, flat_fn(c))
    with H.float64_checker():
        mb64 = {k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
        loss64, _ = checker_loss(c, o64, mb64, samples)
        loss64.backward()
    return g32, H.flat_grads_exact(o64, flat_fn(c)), stats


def build(c: Case, seed: int = SEED):
    """the whole checker side: -> dict(orac, ob, idx, candidates, edge)"""
    orac = checker(c, seed)
    ob = fill(c)(c.config, orac, c.T, c.E, seed=seed)
    rec: dict = {}
    idx = pick_idx(c, rec)(orac, ob)
    return dict(orac=orac, ob=ob, idx=idx, **rec)


def sibling_mode0(c: Case) -> Case:
    return dataclasses.replace(c, gemm_mode=0)


# ---- train level: one epoch of two minibatches on a stale buffer, from a zero Adam state ---------------------------------------
@dataclass(frozen=True)
class TrainCase:
    family: str                 # ppo | arch | modular | adap | adapmult
    config: str
    drift: float
    clip_range_vf: float
    kernel: str
    exclusive: Optional[bool] = None            # ppo: set_exclusive_device (one launch for reduce + clip + Adam)
    arch: Optional[Tuple[int, ...]] = None
    K: int = 0
    coef: Optional[float] = None
    ent_coef: float = 0.0
    seed: int = 21
    T: int = 16
    E: int = 8
    batch: int = 64

    @property
    def id(self) -> str:
        extra = "x".join(map(str, self.arch)) if self.arch else ("K%d" % self.K if self.K else "")
        launch = {None: "", False: "two-launch", True: "one-launch"}[self.exclusive]
        return "-".join(x for x in (self.family, self.config, extra, launch) if x)

    @property
    def scale(self) -> float:
        return max(1.0, self.arch[-1] / 64.0) if self.arch else 1.0


TRAIN_CASES = [
    TrainCase("ppo", "overcooked", 0.03, 0.15, "train(): split kernel, ppo_adam_kernel after the reduce", exclusive=False, seed=22),
    TrainCase("ppo", "overcooked", 0.03, 0.15, "train(): split kernel, ppo_step_kernel (one launch)", exclusive=True, seed=22),
    TrainCase("arch", "overcooked", 0.03, 0.15, "train(): arch kernels", arch=(128, 128)),
    TrainCase("ppo", "gauss5", 0.015, 0.07, "train(): general kernel, Gaussian tail", ent_coef=0.01),
    TrainCase("modular", "mod_oc", 0.03, 0.15, "ph_modular_train", K=2, coef=0.5, ent_coef=0.01, seed=25),
    TrainCase("adap", "adap_oc", 0.03, 0.15, "ph_adap_train: general kernel + context term", coef=0.5, seed=26),
    TrainCase("adapmult", "adap_small", 0.03, 0.15, "ph_adapmult train: am_loss kernels + context term", coef=0.5),
]
TRAIN_BY_ID = {t.id: t for t in TRAIN_CASES}
assert len(TRAIN_BY_ID) == len(TRAIN_CASES)
N_CTX, N_STATES = 5, 32


def train_hyper(t: TrainCase, **kw) -> orc.PPOHyper:
    return orc.PPOHyper(batch_size=t.batch, n_epochs=1, clip_range_vf=t.clip_range_vf, ent_coef=t.ent_coef, **kw)


def _as_case(t: TrainCase, partner: int = 0) -> Case:
    """the minibatch-level view of a train case (checker, buffer builder, evaluate_actions keywords are the same functions)"""
    return Case(t.family, t.config, 0, t.T, t.E, t.batch, t.drift, 0.2, t.clip_range_vf, True, t.ent_coef, t.kernel, arch=t.arch, K=t.K,
                partner=partner, coef=t.coef)


def train_perms(t: TrainCase, n_epochs: int = 1, N: Optional[int] = None):
    """the families' _train_pair convention: epoch ep is default_rng(seed + ep).permutation(N)"""
    return np.stack([np.random.default_rng(t.seed + ep).permutation(N or t.T * t.E) for ep in range(n_epochs)])


def train_samples(t: TrainCase, n_mb: int, nb: int):
    """ADAP's teacher-forced samples per minibatch -> (state_idx (n_mb, N_STATES) int32, contexts (n_mb, N_CTX, cs), AdapTerm) or None"""
    if t.family not in ("adap", "adapmult"):
        return None
    from tests.adap_cases import CTX
    cs = CTX[t.config]
    rng = np.random.default_rng(t.seed)
    sidx = np.stack([rng.permutation(nb)[:N_STATES] for _ in range(n_mb)]).astype(np.int32)
    ctxs = np.stack([orc.adap_sample_contexts("l2", cs, N_CTX, rng.random((N_CTX, cs))) for _ in range(n_mb)])
    return sidx, ctxs, orc.AdapTerm(cs, t.coef, list(sidx), ctxs)


def train_buffers(t: TrainCase, orac):
    """the stale buffer(s) of a train case: one, or one per partner for Modular (built in partner order right after the checker)"""
    if t.family == "modular":
        return [fill(_as_case(t, k))(t.config, orac, t.T, t.E, seed=t.seed + k) for k in range(t.K)]
    return [fill(_as_case(t))(t.config, orac, t.T, t.E, seed=t.seed)]


def checker_train(t: TrainCase, orac, bufs, hp, perms, samples=None):
    """the family's train() on the checker -> its statistics rows"""
    if t.family == "modular":
        return orc.modular_train(orac, bufs, hp, t.coef, perms=[list(perms)] * t.K)
    return orc.ppo_train(orac, bufs[0], hp, perms, adap=samples[2] if samples else None)


class recorded_rows:
    """context: every minibatch loss the checker evaluates also leaves its helpers.offpolicy_rows in .rows (the float64 copy of the
    checker walks the chain, so the rows of the second minibatch are those of the parameters after the first step)"""

    def __init__(self, t: TrainCase):
        self.t, self.rows = t, []

    def __enter__(self):
        self._ppo, self._mod = orc.ppo_minibatch_loss, orc.modular_minibatch_loss
        ppo, mod, t, rows = self._ppo, self._mod, self.t, self.rows

        def ppo_rec(policy, mb, hp):
            rows.append(H.offpolicy_rows(policy, mb, hp, s=t.scale))
            return ppo(policy, mb, hp)

        def mod_rec(policy, mb, hp, partner_idx, coef):
            rows.append(H.offpolicy_rows(policy, mb, hp, s=t.scale, always_normalize=True, partner_idx=partner_idx))
            return mod(policy, mb, hp, partner_idx, coef)
        orc.ppo_minibatch_loss, orc.modular_minibatch_loss = ppo_rec, mod_rec
        return self

    def __exit__(self, *exc):
        orc.ppo_minibatch_loss, orc.modular_minibatch_loss = self._ppo, self._mod
        return False


def train_reference(t: TrainCase, hp=None, n_epochs: int = 1):
    """the checker side of a train case -> dict(orac0 (untouched), orac (trained), bufs, hp, perms, samples, stats, rows)"""
    import copy
    orac0 = checker(_as_case(t), t.seed)
    bufs = train_buffers(t, orac0)
    hp = hp or train_hyper(t)
    N = t.T * t.E
    perms = train_perms(t, n_epochs)
    samples = train_samples(t, n_epochs * (-(-N // t.batch)), t.batch)
    orac = copy.deepcopy(orac0)
    stats = checker_train(t, orac, bufs, hp, perms, samples)
    o64 = H.double_copy(orac0)[0]
    with recorded_rows(t) as rec, H.float64_checker():
        checker_train(t, o64, bufs, hp, perms, samples)
    return dict(orac0=orac0, orac=orac, bufs=bufs, hp=hp, perms=perms, samples=samples, stats=stats, rows=rec.rows)


def first_minibatch_buffer(ob, rows):
    """a (len(rows), 1) buffer holding exactly `rows` (env-major positions) of ob, in that order: one train() step on it IS the first
    step of a train() whose first minibatch is `rows` (advantages and returns are stored, not recomputed)"""
    n = len(rows)
    sub = orc.RolloutBufferOracle(n, 1, ob.D, ob.A, ob.gamma, ob.gae_lambda)
    f = ob.flat()
    sub.observations[:, 0] = f["observations"][rows]
    sub.actions[:, 0] = f["actions"][rows]
    sub.values[:, 0], sub.log_probs[:, 0] = f["old_values"][rows], f["old_log_prob"][rows]
    sub.advantages[:, 0], sub.returns[:, 0] = f["advantages"][rows], f["returns"][rows]
    sub.pos, sub.full = n, True
    return sub


def first_step_reference(t: TrainCase, ref):
    """the first optimizer step of train_reference's chain as a unit of its own: -> dict(sub (buffer of the first minibatch), hp, perms,
    samples, g_ref, n_ref (its unclipped gradient and norm), m_ref (the checker's adam_m after it), p0)"""
    import copy
    sub = first_minibatch_buffer(ref["bufs"][0], ref["perms"][0][:t.batch])
    hp1 = dataclasses.replace(ref["hp"], batch_size=t.batch, n_epochs=1)
    # (the families' _train_pair draws its own permutation; ADAP's state positions refer to the minibatch order, which is kept)
    perms1 = train_perms(t, 1, N=t.batch) if t.family in ("ppo", "arch") else np.arange(t.batch)[None]
    s = ref["samples"]
    samples1 = None if s is None else (s[0][:1], s[1][:1], orc.AdapTerm(s[2].context_size, t.coef, [s[0][0]], s[1][:1]))
    t1 = dataclasses.replace(t, K=1) if t.family == "modular" else t

    def run(c, max_grad_norm):
        return checker_train(t1, c, [sub], dataclasses.replace(hp1, max_grad_norm=max_grad_norm), perms1, samples1)
    orac0 = ref["orac0"]
    if t.family == "modular":          # a ONE-partner model holding the main network and partner 0's module: train() is that step alone
        orac0 = checker(_as_case(t1), t.seed)
        full = ref["orac0"].state_dict()
        orac0.load_state_dict({k: full[k] for k in orac0.state_dict()})
    c = copy.deepcopy(orac0)
    stats = run(c, 1e9)
    g_ref = H.flat_grads_exact(c, flat_fn(_as_case(t)))
    stepped = copy.deepcopy(orac0)
    run(stepped, hp1.max_grad_norm)
    m_ref = H.flat_adam_state(stepped, flat_fn=flat_fn(_as_case(t)))[0]
    return dict(sub=sub, hp=hp1, perms=perms1, samples=samples1, g_ref=g_ref, n_ref=float(stats[0]["grad_norm"]), m_ref=m_ref,
                orac0=orac0, t1=t1)


# ---- the target_kl stop on a stale buffer ---------------------------------------------------------------------------------------------
# The checker's approx_kl on this buffer is 0.0016 and 0.0048 on the first two minibatches and 0.0226 on the third; the test is
# approx_kl > 1.5 * target_kl = 0.0105: the stop is a factor 2 away from a tie on both sides (test_offpolicy_checks.py asserts it)
KL_STOP = dict(case=TrainCase("ppo", "overcooked", 0.005, 0.15, "train(): the KL test before the step", seed=21, T=32, E=8, batch=64),
               n_epochs=4, learning_rate=3e-3, target_kl=0.007)


def kl_stop_reference():
    t = KL_STOP["case"]
    hp = dataclasses.replace(train_hyper(t, learning_rate=KL_STOP["learning_rate"], target_kl=KL_STOP["target_kl"]),
                             n_epochs=KL_STOP["n_epochs"])
    return t, hp, train_reference(t, hp=hp, n_epochs=KL_STOP["n_epochs"])
