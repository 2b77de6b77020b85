"""The checker side of tests/test_gpu_sharp.py: every policy head and its gradient on SHARP and SATURATED policies.

Every checker the rest of the suite builds is close to its initial weights (helpers.oracle_policy adds 0.3 N(0, 1) to the 0.01-gain
action head): no probability below ~1e-5, no row of entropy below 0.3.  Here the weight and bias of every categorical action head
are multiplied by 8 ("sharp": probabilities of 1e-13 .. 1e-40, tiny but representable) or by 30 ("saturated": probabilities below
float32's smallest denormal, rows of entropy < 1e-6 beside soft rows in the same launch).  Nothing else of the checker moves, so
values are unchanged.  What goes wrong in a hand-written head only there: the max subtraction before fast_exp, lse = m + log(1 +
tiny), p * lp with p underflowed, hit - p one ulp from 1, the inverse CDF against a cumulative sum that reaches 0.99999994 before the
last slot, the -30 mask offset under an unmasked logit more than 30 below a masked one, exp(-kl) of ADAP's context term at a KL in
the hundreds.

Everything here runs on the CPU and nothing of the device is imported; tests/test_sharp_checks.py proves on it what a case claims
about itself (populations, the reach of every allowance against wrong heads), so that the GPU run only compares.

Forward cases: sampler_cases.CASES without overcooked-16384, inputs from sampler_cases.inputs, the checker a sharpened deep copy of
sampler_cases.checker.  Every family hands out an entropy (`entropy` below is True for all of them; Modular hands out its logits as
the pair (main, partner), compared as their sum).  Gradient cases: on-policy, one minibatch, T = 16, E = 8, nb in {77, 100}, ent_coef
0.01, normalised advantages, through the families' own _grad_pair(prepare=, fill=).

Allowances (derived; s = max(1, w_last / 64), c32 / c64 the float32 checker and its float64 copy, d_x = max |c32 - c64| of output x
over the rows of the case, 4 = helpers.CHAIN_FACTOR, 2e-7 = the absolute error ph_device.h states for fast_tanh, carried through
the head's weights -- the part the sharpening multiplies):
    logit k      A_z[k] = 2e-5 s + 4 d_z + 2e-7 sum_j |W_head[j, k]|
    log-prob     A_lp   = 2 max_k A_z[k] + 4 d_lp              (the chosen logit and the log-sum-exp each move by at most max A_z)
    entropy      A_H    = 2e-5 s + 4 d_H + max_k A_z[k] * sum_k p_k |lp_k + H|      (the sum is |dH/dz| in float64, per component, added)
    value        2e-5 s
    gradients    helpers.assert_block_gradients unchanged (BC: with bc_cases.assert_stats, as tests/test_gpu_bc_shapes.py)
    statistics   1e-5 + 1e-4 |x| + 4 d_x; clip_fraction exactly 0"""
from __future__ import annotations

import contextlib
import copy
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from tests import bc_cases as B
from tests import helpers as H
from tests import offpolicy_cases as OC
from tests import sampler_cases as S

SCALES = (8, 30)
TANH_ERR = 2e-7                 # ph_device.h: fast_tanh's absolute error
BASE_TOL = S.FORWARD_TOL        # 2e-5, times s
F32 = np.float32


# ---- sharpening --------------------------------------------------------------------------------------------------------------------
def heads(checker) -> list:
    """the categorical action heads: action_net of the MLP, net_arch, ADAP and ADAP-MULT checkers, every DISTINCT partner head of the
    Modular checker, the last layer of the BC checker"""
    if isinstance(checker, orc.ModularPolicyOracle):
        from tests.modular_cases import _unique
        return [pm["act"] for pm in _unique(checker)]
    return [checker.action_net]


def sharpen(checker, scale):
    """multiply weight and bias of every categorical action head by `scale`, in place; -> checker"""
    with th.no_grad():
        for h in heads(checker):
            h.weight.mul_(float(scale))
            h.bias.mul_(float(scale))
    return checker


def preparer(scale):
    return lambda checker: sharpen(checker, scale)


# ---- forward cases -----------------------------------------------------------------------------------------------------------------
def _rows(case: S.Case) -> tuple:
    if case.family in ("adapmult", "modular"):
        return case.rows                                   # (7, 64) / (70,), as they are
    if case.kernel.startswith("policy_fwd16_kernel"):
        return (1, 64, 65)
    return (65, 257)


@dataclass(frozen=True)
class ForwardCase:
    case: S.Case
    rows: tuple
    entropy: bool = True        # every family's forward hands out an entropy
    logits: bool = True         # ... and its logits (Modular: main and partner logits, compared as their sum)

    @property
    def id(self) -> str:
        return self.case.id


FORWARD = [ForwardCase(c, _rows(c)) for c in S.CASES if c.id != "overcooked-16384"]
FORWARD_BY_ID = {f.id: f for f in FORWARD}
MASKED = [f.id for f in FORWARD if f.case.mask]
POPULATION_ROWS = 63            # the population asserts hold at n >= 63


@functools.lru_cache(maxsize=None)
def checker(case_id: str, scale: int):
    """a sharpened DEEP COPY of the sampler case's checker; the cached original is left as it is"""
    return sharpen(copy.deepcopy(S.checker(case_id)), scale)


def _torch_forward(case: S.Case, orac, obs):
    x = th.as_tensor(obs)
    if case.family == "modular":
        lat_pi, lat_vf, p_pi, p_vf, pm = orac._towers(x, case.extra["partner"])
        return orac._mean_actions(lat_pi, p_pi, pm, None), (orac.value_net(lat_vf) + pm["val"](p_vf)).reshape(-1)
    if case.family == "bc":
        lat = orac._latent(x)
        return orac.action_net(lat), orac.value_net(lat).reshape(-1)
    return orac.logits(x), orac.predict_values(x).reshape(-1)


def logits_values(case: S.Case, orac, obs, double: bool = False):
    """-> (unmasked logits (n, L), values (n,)) of the float32 checker, or of its float64 copy"""
    with th.no_grad():
        if double:
            o64 = copy.deepcopy(orac).double()
            with H.float64_checker():
                z, v = _torch_forward(case, o64, obs)
            assert z.dtype == th.float64 and v.dtype == th.float64
        else:
            z, v = _torch_forward(case, orac, obs)
    return z.numpy(), v.numpy()


def apply_mask(z: np.ndarray, mask) -> np.ndarray:
    """modular/policies.py:330-333: logits - 30 on masked entries, in z's dtype"""
    if mask is None:
        return z
    return (z - z.dtype.type(30.0) * (z.dtype.type(1.0) - mask.astype(z.dtype))).astype(z.dtype)


def split(z: np.ndarray, nvec) -> list:
    out, lo = [], 0
    for k in nvec:
        out.append(z[:, lo:lo + k])
        lo += k
    return out


def head_weight_sums(case: S.Case, orac) -> np.ndarray:
    """sum_j |W_head[j, k]| per logit k: what an absolute error of the last activations is multiplied by"""
    if case.family == "modular":
        w = orac.partners[case.extra["partner"]]["act"].weight.detach().abs().sum(dim=1)
        if not orac.nomain:
            w = w + orac.action_net.weight.detach().abs().sum(dim=1)
        return w.double().numpy()
    return orac.action_net.weight.detach().abs().sum(dim=1).double().numpy()


def width_scale(orac) -> float:
    return max(1.0, orac.action_net.in_features / 64.0)


def softmax64(z64: np.ndarray, nvec):
    """float64 per component -> (log-softmax list, probability list)"""
    ls = []
    for zc in split(z64, nvec):
        m = zc.max(axis=1, keepdims=True)
        ls.append(zc - m - np.log(np.exp(zc - m).sum(axis=1, keepdims=True)))
    return ls, [np.exp(x) for x in ls]


def entropy64(ls: list, ps: list):
    """-> (H (n,), |dH/dz| summed: sum_c sum_k p_k |lp_k + H_c| (n,), H per component list)"""
    Hs = [-(p * l).sum(axis=1) for l, p in zip(ls, ps)]
    dH = sum((p * np.abs(l + h[:, None])).sum(axis=1) for l, p, h in zip(ls, ps, Hs))
    return sum(Hs), dH, Hs


def torch_head32(z32: np.ndarray, nvec):
    """the float32 checker's own head (torch's Categorical: log_softmax, entropy = -sum p * logp) -> (log-softmax list, H (n,))"""
    ls = [th.log_softmax(th.as_tensor(zc.copy()), dim=1) for zc in split(z32, nvec)]
    ent = sum(-(l.exp() * l).sum(dim=1) for l in ls)
    return [l.numpy() for l in ls], ent.numpy()


def gather(ls: list, acts: np.ndarray) -> np.ndarray:
    r = np.arange(len(acts))
    return sum(l[r, acts[:, c]] for c, l in enumerate(ls))


class Reference:
    """one (forward case, scale, n): inputs, the checker's logits and values in both precisions, the allowances"""

    def __init__(self, fc: ForwardCase, scale: int, n: int):
        case = fc.case
        self.fc, self.case, self.scale, self.n = fc, case, scale, n
        self.orac = checker(case.id, scale)
        self.nvec = tuple(S.spaces(case)[1].nvec)
        self.obs, self.mask = S.inputs(case, n)
        self.raw32, self.v32 = logits_values(case, self.orac, self.obs)
        raw64, self.v64 = logits_values(case, self.orac, self.obs, double=True)
        self.z32, self.z64 = apply_mask(self.raw32, self.mask), apply_mask(raw64, self.mask)
        assert self.z32.dtype == np.float32 and self.z64.dtype == np.float64
        self.s = width_scale(self.orac)
        self.d_z = float(np.abs(self.z32 - self.z64).max())
        self.A_z = BASE_TOL * self.s + H.CHAIN_FACTOR * self.d_z + TANH_ERR * head_weight_sums(case, self.orac)      # (L,)
        self.Az = float(self.A_z.max())
        self.A_v = BASE_TOL * self.s
        self.ls64, self.p64 = softmax64(self.z64, self.nvec)
        self.H64, self.dH, self.H64_c = entropy64(self.ls64, self.p64)
        self.ls32, self.H32 = torch_head32(self.z32, self.nvec)
        self.d_H = float(np.abs(self.H32 - self.H64).max())
        self.A_H = BASE_TOL * self.s + H.CHAIN_FACTOR * self.d_H + self.Az * self.dH                                  # (n,)

    # -- action sets ----------------------------------------------------------------------------------------------------------------
    def action_sets(self) -> dict:
        """the float64 checker's most likely action per component (first index), its least likely one, one seeded uniform draw"""
        rng = np.random.default_rng([sum(self.case.id.encode()), self.scale, self.n, 17])
        return {"most": np.stack([p.argmax(axis=1) for p in self.p64], axis=1),
                "least": np.stack([p.argmin(axis=1) for p in self.p64], axis=1),
                "random": np.stack([rng.integers(0, k, size=self.n) for k in self.nvec], axis=1)}

    def log_probs(self, acts: np.ndarray):
        """-> (c32's log-prob of acts, c64's, the allowance A_lp, d_lp)"""
        lp32, lp64 = gather(self.ls32, acts).astype(np.float64), gather(self.ls64, acts)
        d = float(np.abs(lp32 - lp64).max())
        return lp32, lp64, 2.0 * self.Az + H.CHAIN_FACTOR * d, d

    def decided_argmax(self):
        """-> (first-index argmax per component of c64 (n, A), rows whose top two logits differ by more than 2 max A_z in EVERY component)"""
        arg = np.stack([zc.argmax(axis=1) for zc in split(self.z64, self.nvec)], axis=1)
        ok = np.ones(self.n, bool)
        for zc in split(self.z64, self.nvec):
            if zc.shape[1] > 1:
                top = np.sort(zc, axis=1)[:, -2:]
                ok &= (top[:, 1] - top[:, 0]) > 2.0 * self.Az
        return arg, ok

    def prediction(self, counter: int):
        """-> (uniforms (n, A), the float64 inverse CDF's actions, near rows) at (sampler_cases.KEY, counter)"""
        u = S.uniforms(self.n, len(self.nvec), S.KEY, counter)
        want, near = S.predict(self.p64, u)
        return u, want, near


@functools.lru_cache(maxsize=None)
def reference(case_id: str, scale: int, n: int) -> Reference:
    return Reference(FORWARD_BY_ID[case_id], scale, n)


# ---- the head in numpy float32, as ph_rowtail.h writes it, and wrong heads ("mutants") -----------------------------------------------
MUTANTS = {"M1": "softmax without the max subtraction", "M2": "log-prob as log(softmax(z)[a]) instead of z[a] - lse",
           "M3": "entropy as -sum p log(p) from the probabilities", "M4": "the mask as -inf instead of -30",
           "M5": "the inverse CDF against unnormalised prefix sums of exp(z - m)",
           "G1": "gradient with rows of entropy below 1e-6 contributing nothing"}


def tail32(z: np.ndarray, nvec, acts=None, u=None, variant: str = "real") -> dict:
    """float32 numpy of the row tail (np.exp / np.log for fast_exp / fast_log): per component m = max z, se = sum exp(z - m),
    lse = m + log(se), log-prob z[a] - lse, entropy -sum p (z - lse) with p = exp(z - m) / se in the register tail of a Discrete head
    of <= 8 logits (discrete8_row_tail) and p = exp(z - lse) elsewhere (general_row_tail), inverse CDF = the count of prefix sums of p
    that are <= u over the first nk - 1 entries, argmax = first index of the largest logit.  acts given: their log-prob; u given: the
    sampled actions and theirs; neither: the argmax and its log-prob.  variant: "real" or one of M1, M2, M3, M5 (M4 is an input:
    logits holding -inf)."""
    z = np.asarray(z, F32)
    n = len(z)
    r = np.arange(n)
    small = len(nvec) == 1 and nvec[0] <= 8
    logp, ent, out = np.zeros(n, F32), np.zeros(n, F32), []
    with np.errstate(all="ignore"):
        for c, zc in enumerate(split(z, nvec)):
            m = zc.max(axis=1, keepdims=True) if variant != "M1" else np.zeros((n, 1), F32)
            e = np.exp(zc - m)
            se = e.sum(axis=1, keepdims=True, dtype=F32)
            lse = m + np.log(se)
            lpk = zc - lse
            p = e * (F32(1.0) / se) if small else np.exp(lpk)
            ent += (-(p * np.log(p)).sum(axis=1) if variant == "M3" else -(p * lpk).sum(axis=1)).astype(F32)
            if acts is not None:
                a = np.asarray(acts)[:, c]
            elif u is not None:
                steps = e if variant == "M5" else p
                a = (np.asarray(u, F32)[:, c:c + 1] >= np.cumsum(steps[:, :-1], axis=1, dtype=F32)).sum(axis=1)
            else:
                a = zc.argmax(axis=1)
            out.append(a)
            logp += (np.log((e / se)[r, a]) if variant == "M2" else lpk[r, a]).astype(F32)
    return dict(actions=np.stack(out, axis=1), logp=logp, entropy=ent)


def miss(err, allowed) -> float:
    """by which factor `err` misses `allowed` at its worst entry; inf where anything is not finite"""
    err = np.asarray(err, np.float64)
    if not np.isfinite(err).all():
        return float("inf")
    return float((err / np.broadcast_to(np.asarray(allowed, np.float64), err.shape)).max())


# ---- gradient cases ------------------------------------------------------------------------------------------------------------------
T, E, NBS, ENT_COEF = 16, 8, (77, 100), 0.01
LOGP_UNLIKELY, UNLIKELY_SHARE = -40.0, 0.10
BC_WEIGHTS = ((1e-3, 0.0), (0.5, 0.0))        # bc_cases.WEIGHTS without the L2 row: the defaults; the entropy term visible


@dataclass(frozen=True)
class GradCase:
    family: str                 # ppo | arch | modular | adap | adapmult | bc
    config: str                 # helpers.CONFIGS / modular_cases.SHAPES name, or a bc_cases id
    gemm_mode: int
    kernel: str
    arch: Optional[Tuple[int, ...]] = None
    K: int = 0
    partner: int = 0
    coef: Optional[float] = None

    @property
    def id(self) -> str:
        extra = "x".join(map(str, self.arch)) if self.arch else ("K%dp%d" % (self.K, self.partner) if self.K else "")
        return "-".join(x for x in (self.family, self.config, extra, "m%d" % self.gemm_mode) if x)

    def oc(self, nb: int) -> OC.Case:
        """the offpolicy_cases view (checker, loss, flat order are the same functions); drift 0: the buffer is the checker's own"""
        return OC.Case(self.family, self.config, self.gemm_mode, T, E, nb, 0.0, 0.2, None, True, ENT_COEF, self.kernel, arch=self.arch,
                       K=self.K, partner=self.partner, coef=self.coef)


def _kernel(family, config, mode, arch=None) -> str:
    """the `kernel` string of the off-policy case of the same family, config, gemm_mode and widths"""
    found = [c.kernel for c in OC.CASES if (c.family, c.config, c.gemm_mode, c.arch) == (family, config, mode, arch)]
    assert found, (family, config, mode, arch)
    return found[0]


GRAD_CASES = (
    [GradCase("ppo", cfg, mode, _kernel("ppo", cfg, mode)) for cfg, mode in
     (("overcooked", 0), ("overcooked", 2), ("liar", 2), ("discrete20", 2), ("liar", 0), ("wide", 0), ("onehot17", 0), ("adap_oc", 0))]
    + [GradCase("arch", "overcooked", 0, _kernel("arch", "overcooked", 0, (32,)), arch=(32,)),
       GradCase("arch", "liar", 0, _kernel("arch", "liar", 0, (128, 128)), arch=(128, 128)),
       GradCase("modular", "mod_oc", 0, _kernel("modular", "mod_oc", 0), K=2, partner=1, coef=0.5),
       GradCase("adap", "adap_small", 0, _kernel("adap", "adap_small", 0), coef=1.0),
       GradCase("adapmult", "adap_oc", 0, _kernel("adapmult", "adap_oc", 0), coef=1.0),
       # bc_cases: path 1 = bc_train_kernel (VALU loops), path 3 = bc_train_mfma_kernel; both hold a wide component
       GradCase("bc", "box130-16x4", 0, "bc_train_kernel (ph_bc.hip, VALU loops)"),
       GradCase("bc", "box33-3x30x7", 0, "bc_train_mfma_kernel (ph_bc.hip, MFMA tiles, two logit tiles)")]
)
GRAD_BY_ID = {g.id: g for g in GRAD_CASES}
assert len(GRAD_BY_ID) == len(GRAD_CASES)
assert B.BY_ID["box130-16x4"].path == 1 and B.BY_ID["box33-3x30x7"].path == 3


def hyper() -> orc.PPOHyper:
    return orc.PPOHyper(ent_coef=ENT_COEF)


def minibatch_rows(nb: int) -> np.ndarray:
    return np.random.default_rng(nb).permutation(T * E)[:nb]


def replace_actions(g: GradCase, orac, ob, seed: int):
    """every second row (time-major order) gets one seeded uniform draw per action component, and the float32 checker's log-prob of
    it as old_log_prob: ratios stay at 1, and unlikely actions (log-prob -50 and below) sit beside saturated likely ones"""
    n, A = ob.T * ob.E, ob.A
    nvec = orac.act_space.nvec
    rows = np.arange(1, n, 2)
    rng = np.random.default_rng([seed, 4099])
    draw = np.stack([rng.integers(0, k, size=len(rows)) for k in nvec], axis=1).astype(np.float32)
    acts, logp, obs = ob.actions.reshape(n, A), ob.log_probs.reshape(n), ob.observations.reshape(n, -1)
    assert np.shares_memory(acts, ob.actions) and np.shares_memory(logp, ob.log_probs)
    acts[rows] = draw
    a = th.as_tensor(draw)
    if orac.act_space.kind == "discrete":
        a = a.long().flatten()
    with th.no_grad():
        _, lp, _ = orac.evaluate_actions(th.as_tensor(obs[rows]), a, **(dict(partner_idx=g.partner) if g.family == "modular" else {}))
    logp[rows] = lp.numpy()
    ob.replaced_rows = rows
    return ob


def fill(g: GradCase):
    """the buffer builder the family's _grad_pair takes: the family's usual filled buffer, made by the (already sharpened) checker
    it is handed, then replace_actions.  The checker samples from torch's global stream: seeded here, the same buffer on every call"""
    def build(name, orac, T_, E_, seed=0, **kw):
        with th.random.fork_rng(devices=[]):
            th.manual_seed(seed)
            if g.family == "modular":
                from tests.modular_cases import _filled
                ob = _filled(orac, name, g.partner, T_, E_, seed=seed)
            else:
                ob = H.filled_oracle_buffer(name, orac, T_, E_, seed=seed)
        return replace_actions(g, orac, ob, seed)
    return build


def build(g: GradCase, scale: int, nb: int, seed: int = OC.SEED) -> dict:
    """the checker side of a PPO-family gradient case -> dict(c (the offpolicy_cases view), orac, ob, idx)"""
    c = g.oc(nb)
    orac = sharpen(OC.checker(c, seed), scale)
    ob = fill(g)(g.config, orac, T, E, seed=seed)
    return dict(c=c, orac=orac, ob=ob, idx=minibatch_rows(nb))


def checker_gradients(c: OC.Case, orac, ob, idx):
    """offpolicy_cases.checker_gradients, with the float64 statistics too -> (g32, g64, stats32, stats64)"""
    mb = OC.minibatch(ob, idx)
    samples = OC.context_samples(c, len(idx))
    o64 = H.double_copy(orac)[0]
    for p in orac.parameters():
        p.grad = None
    loss, st32 = OC.checker_loss(c, orac, mb, samples)
    loss.backward()
    g32 = H.flat_grads_exact(orac, OC.flat_fn(c))
    with H.float64_checker():
        mb64 = {k: (v.double() if v.is_floating_point() else v) for k, v in mb.items()}
        loss64, st64 = OC.checker_loss(c, o64, mb64, samples)
        loss64.backward()
    return g32, H.flat_grads_exact(o64, OC.flat_fn(c)), st32, st64


def minibatch_log_probs(c: OC.Case, orac, ob, idx):
    """float64: -> (log-prob of the stored action, entropy) per row of the minibatch"""
    mb = OC.minibatch(ob, idx)
    o64 = H.double_copy(orac)[0]
    a = mb["actions"]
    if o64.act_space.kind == "discrete":
        a = a.long().flatten()
    with H.float64_checker(), th.no_grad():
        _, lp, ent = o64.evaluate_actions(mb["observations"].double(), a, **OC.eval_kw(c))
    return lp.numpy(), ent.numpy()


CONTEXT_GAP = 1e-3      # relative: ten times the relative part of the statistics rule -- beyond it the gap is no rounding


def context_term_degenerate(st32: dict, st64: dict) -> bool:
    """ADAP's context term on a saturated policy: torch's kl_divergence(Categorical, Categorical) returns inf wherever q's probability
    is exactly 0 and p's is not, and in float32 a probability below 1e-45 IS 0 -- so the float32 checker drops exp(-kl) of every
    such (state, context pair) to 0 where the float64 checker (and the arithmetic: kl = sum p (lp - lq) with lq ~ -150) keeps a
    finite KL that may be small.  Measured at x30: context loss 0.67 in float32 against 0.80 in float64 (adap_small, nb 100), 0.31
    against 0.48 (ADAP-MULT adap_oc, nb 77).  Where the two context losses differ by more than CONTEXT_GAP the float32 checker is
    no yardstick for the term: the float64 checker takes its place (gradient_reference), at the rule WITHOUT the d terms."""
    if "context_loss" not in st64:
        return False
    return abs(st32["context_loss"] - st64["context_loss"]) > CONTEXT_GAP * abs(st64["context_loss"])


def gradient_reference(g32, g64, st32: dict, st64: dict):
    """-> (gradient to compare with, statistics to compare with, whether the float64 checker replaced the float32 one)"""
    if context_term_degenerate(st32, st64):
        return g64, st64, True
    return g32, st32, False


def mode2_allowances(g0, g32, g64, block, names) -> np.ndarray:
    """per parameter block, what gemm_mode 2 may differ from gemm_mode 0 by: the off-policy test's 2e-6 of the largest entry of mode
    0, or 8 d_b where that is more (d_b = the float32 checker's distance from its float64 copy in the block; assert_block_gradients
    grants EACH float32 evaluation CHAIN_FACTOR d_b = 4 d_b from the float32 checker, so two of them lie at most 8 d_b apart: the
    triangle inequality on the rule both kernels are already held to -- where 2e-4 M_b leads that rule, this one is still ten to
    a hundred times narrower than what the two block checks imply).  Why the 2e-6 rule cannot hold here: ratio = exp(lp - old_lp) inherits the absolute
    rounding of lp as a relative error of the row's whole contribution; float32's spacing is 7.6e-6 at |lp| >= 64 and 3e-5 at
    |lp| >= 256 (this buffer holds log-probs down to -460), so two faithful float32 evaluations of these minibatches differ by
    more than 2e-6 of the largest entry -- torch's float32 autograd itself lies 2.2e-6 (x8) to 4.6e-5 (x30) from float64 where the
    rule would allow 2.2e-6 to 9.6e-6.  Measured on an MI355X, mode 2 against mode 0 / largest d_b: 3.8e-6 / 2.2e-6 and 4.8e-5 /
    2.6e-5 (overcooked x8, x30), 4.7e-6 / 3.8e-6 and 4.3e-5 / 4.6e-5 (liar), 1.8e-6 / 8.7e-7 and 2.0e-5 / 1.35e-5 (discrete20)."""
    g0, g32, g64 = (np.asarray(x, np.float64) for x in (g0, g32, g64))
    base = 2e-6 * max(np.abs(g0).max(), 1e-3)
    return np.array([max(base, 2.0 * H.CHAIN_FACTOR * np.abs(g32[block == b] - g64[block == b]).max()) for b in range(len(names))])


STAT_KEYS = ("policy_loss", "value_loss", "entropy_loss", "loss")
STAT_SLOT = {"policy_loss": 0, "value_loss": 1, "entropy_loss": 2, "clip_fraction": 3, "loss": 5}


def stat_allowance(x32: float, x64: float) -> float:
    return 1e-5 + 1e-4 * abs(x32) + H.CHAIN_FACTOR * abs(x32 - x64)


def reached_blocks(g: GradCase, orac, names) -> np.ndarray:
    """which parameter blocks the loss reaches: all of them, except the value side of the Modular modules that are not trained
    (tests/test_gpu_modular.py asserts their gradient is exactly zero) and the value head of the BC network (no L2 term here:
    tests/test_gpu_bc_shapes._assert_value_head asserts exactly zero)"""
    ok = np.ones(len(names), bool)
    for b, name in enumerate(names):
        if g.family == "bc" and name.startswith("value_net"):
            ok[b] = False
        if g.family == "modular" and name.startswith("partners.") and (".vf." in name or ".val." in name) \
                and not name.startswith("partners.%d." % g.partner):
            ok[b] = False
    return ok


@contextlib.contextmanager
def dead_saturated_rows(orac, threshold: float = 1e-6):
    """mutant G1: inside, rows of entropy below `threshold` hand out a log-prob and an entropy that carry no gradient -- a gradient
    kernel that skips the head of a row whose probabilities have underflowed"""
    cls = type(orac)
    own = cls.__dict__.get("evaluate_actions")
    orig = cls.evaluate_actions

    def mutated(self, *a, **kw):
        v, lp, ent = orig(self, *a, **kw)
        dead = ent.detach() < threshold
        return v, th.where(dead, lp.detach(), lp), th.where(dead, ent.detach(), ent)
    cls.evaluate_actions = mutated
    try:
        yield
    finally:
        if own is None:
            del cls.evaluate_actions
        else:
            cls.evaluate_actions = own


def block_misses(g, g32, g64, block, names) -> np.ndarray:
    """per block, by which factor `g` misses helpers.assert_block_gradients' allowance against g32"""
    g, g32, g64 = (np.asarray(x, np.float64) for x in (g, g32, g64))
    out = np.zeros(len(names))
    for b in range(len(names)):
        sel = block == b
        allowed = 1e-6 + max(2e-4 * np.abs(g64[sel]).max(), H.CHAIN_FACTOR * np.abs(g32[sel] - g64[sel]).max())
        out[b] = miss(np.abs(g[sel] - g32[sel]), allowed)
    return out


# ---- behavioural cloning ---------------------------------------------------------------------------------------------------------------
def bc_build(g: GradCase, scale: int, nb: int) -> dict:
    """bc_cases.checker with the last layer sharpened, nb rows.  The expert table is not the checker's own: every second row keeps
    bc_cases' uniform draw, the others take the float32 checker's most likely action per component"""
    case = B.BY_ID[g.config]
    orac, obs, acts = B.checker(case, nb, prepare=preparer(scale))
    with th.no_grad():
        z = orac.logits(th.as_tensor(obs)).numpy()
    likely = np.stack([zc.argmax(axis=1) for zc in split(z, case.act.nvec)], axis=1).astype(np.float32)
    acts = acts.copy()
    acts[0::2] = likely[0::2]
    return dict(case=case, orac=orac, obs=obs, acts=acts, replaced_rows=np.arange(1, nb, 2))


def bc_log_probs(b: dict):
    o64 = copy.deepcopy(b["orac"]).double()
    with H.float64_checker(), th.no_grad():
        _, lp, ent = o64.evaluate_actions(th.as_tensor(b["obs"]), th.as_tensor(b["acts"]))
    return lp.numpy(), ent.numpy()
