"""The shape classes of behavioural cloning's kernels (csrc/ph_bc.hip) and the checker side of tests/test_gpu_bc_shapes.py.

ph_bc_train runs one of three kernels, chosen by shape (bc_train_path in ph_bc.hip, asked through ph_bc_train_path):

    3  bc_train_mfma_kernel<true>    MFMA tiles, Adam moments in LDS     32 D <= 4096, 32 A <= 256, L <= 64 and 4 P + tiles fit 160 KiB
    2  bc_train_mfma_kernel<false>   MFMA tiles, moments through L2      the same, with 2 P + tiles fitting
    1  bc_train_kernel               VALU loops                          every other shape whose 2 P + tiles fit
    0  refused                       "working set exceeds"

`path` below is what the library answers under the default environment (PH_BC_MFMA=0 turns every 2 and 3 into 1);
tests/test_bc_checks.py compares the column with the library on the host, the GPU module asserts it before each launch.  Cases are
observation -> action; Fpad, Lk and the logit tiles are the MFMA kernel's K and N paddings (multiples of 32, 8 and 32).

Everything here runs on the CPU: the checker is oracle.sb3_oracle's FeedForward32Oracle / bc_loss, in float32 and in a float64 copy,
and the project's per-block gradient rule (helpers.assert_block_gradients) does the comparing.  Nothing GPU-side is imported."""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np
import torch as th

from oracle import sb3_oracle as orc
from oracle.sb3_oracle import SpaceSpec
from tests import helpers as H


def box(n):
    return SpaceSpec("box", dim=n)


def disc(n):
    return SpaceSpec("discrete", nvec=(n,))


def multi(*nvec):
    return SpaceSpec("multidiscrete", nvec=tuple(nvec))


@dataclass(frozen=True)
class Case:
    id: str
    obs: SpaceSpec
    act: SpaceSpec
    path: int            # ph_bc_train_path under the default environment
    pins: str

    @property
    def onehot(self) -> bool:
        return self.obs.kind != "box"

    @property
    def F(self) -> int:
        return self.obs.flat_len

    @property
    def L(self) -> int:
        return self.act.flat_len

    @property
    def A(self) -> int:
        return self.act.stored_len


CASES = [
    Case("box1-d2", box(1), disc(2), 3, "Fpad 32 from F = 1; Lk 8 from L = 2"),
    Case("box32-d8", box(32), disc(8), 3, "F == Fpad, L == Lk"),
    Case("box33-3x30x7", box(33), multi(3, 30, 7), 3, "31 zero K columns; L = 40: two logit tiles, the 30-way component crosses column 32"),
    Case("box16-2x8", box(16), multi(*[2] * 8), 3, "32 A = 256, at the limit of one action per thread"),
    Case("box16-2x9", box(16), multi(*[2] * 9), 1, "A over that limit"),
    Case("onehot20-5x16x11", multi(3, 4, 5, 2, 6), multi(5, 16, 11), 3, "small one-hot observations; L = 32 is one full logit tile"),
    Case("box128-16x4", box(128), multi(16, 16, 16, 16), 2, "32 D = 4096, the prefetch limit; L = 64"),
    Case("onehot256-d20", multi(*[2] * 128), disc(20), 2, "one-hot at D = 128, F = 256"),
    Case("onehot320-d3", multi(*[5] * 64), disc(3), 1, "F = 320: the MFMA layout no longer fits, the VALU layout does, with D <= 128"),
    Case("box130-d20", box(130), disc(20), 1, "D > 128"),
    Case("box200-5x16x11", box(200), multi(5, 16, 11), 1, "D > 128"),
    Case("box130-16x4", box(130), multi(16, 16, 16, 16), 1, "the VALU kernel at L = 64"),
    Case("overcooked", *H.CONFIGS["overcooked"], 3, "anchor: Box 62 -> Discrete 6"),
    Case("liar", *H.CONFIGS["liar"], 2, "anchor: one-hot F = 270 -> (7, 12)"),
    Case("onehot360-d3", multi(*[5] * 72), disc(3), 0, 'F = 360: refused with "working set exceeds"'),
]
BY_ID = {c.id: c for c in CASES}
TRAINABLE = [c for c in CASES if c.path != 0]
REFUSED = [c for c in CASES if c.path == 0]
# one case per path, plus the two-logit-tile Box case
LEAK_CASES = ["box33-3x30x7", "onehot20-5x16x11", "box128-16x4", "onehot320-d3"]
# one Box and one one-hot case per kernel family (MFMA tiles, VALU loops)
CLAMP_CASES = ["box33-3x30x7", "onehot20-5x16x11", "box130-16x4", "onehot320-d3"]

N_ROWS = (1, 31, 33, 77)                                   # 31 padding rows; a second tile of one row; a third tile
WEIGHTS = ((1e-3, 0.0), (0.5, 0.0), (1e-3, 0.25))          # (ent_weight, l2_weight): the defaults; entropy visible; L2 visible
STAT_KEYS = ("neglogp", "entropy", "ent_loss", "prob_true_act", "l2_norm", "l2_loss", "loss")
FORWARD_ROWS = (1, 63, 64, 65, 300)                        # bc_forward_kernel: one lane per row, 64 rows per workgroup
FORWARD_TOL = 2e-5                                         # tests/test_gpu_bc.py's forward figure
EDGE = 1e-5                                                # a uniform this close to a float64 CDF edge decides nothing
SAMPLING_SEED = 8                                          # chosen on the checker: no case has a uniform on an edge at 1..65 rows (test_bc_checks.py)
PHILOX_ROWS = 65536


def native_spec(case: Case):
    """the ph_spec of a case (host structure; loads the library, needs no GPU)"""
    from pantheonrl_amd import spaces as sp
    return sp.make_spec(H.to_space(case.obs), H.to_space(case.act))


def checker(case: Case, N: int, seed: int = 3, prepare=None):
    """-> (FeedForward32Oracle perturbed as tests/test_gpu_bc._pair does, obs (N, D), acts (N, A)), all seeded.
    prepare(checker): called on the checker right after it is built (tests/sharp_cases.py sharpens its last layer there)"""
    rng = np.random.default_rng(seed)
    obs = H.sample_obs(case.obs, N, rng)
    acts = np.stack([rng.integers(0, k, size=N) for k in case.act.nvec], axis=1).astype(np.float32)
    th.manual_seed(seed)
    orac = orc.FeedForward32Oracle(case.obs, case.act)
    with th.no_grad():          # biases and the 0.01-gain head perturbed so that the logits are not ~uniform
        g = th.Generator().manual_seed(seed + 1)
        for p in orac.parameters():
            p.add_(0.2 * th.randn(p.shape, generator=g) * (1.0 if p.ndim == 1 else 0.3))
    if prepare is not None:
        prepare(orac)
    return orac, obs, acts


def permutation(N: int, seed: int = 0) -> np.ndarray:
    """a visiting order that is not the identity (N = 1 has no other)"""
    rng = np.random.default_rng(100 + seed)
    while True:
        p = rng.permutation(N)
        if N == 1 or not np.array_equal(p, np.arange(N)):
            return p.astype(np.int32)


def gradient(orac, obs, acts, ent_weight, l2_weight, double=False):
    """-> (gradient of bc_loss on the rows as ONE minibatch, flat in ph_bc_layout order, float64 array; the loss's statistics).
    double: on a float64 copy of the checker.  The value head, which the BC loss reaches only through the L2 term, counts as zero
    where autograd leaves it without a gradient."""
    c = copy.deepcopy(orac)
    if double:
        c = c.double()
        with H.float64_checker():
            loss, stats = orc.bc_loss(c, th.as_tensor(obs), th.as_tensor(acts), ent_weight, l2_weight)
    else:
        loss, stats = orc.bc_loss(c, th.as_tensor(obs), th.as_tensor(acts), ent_weight, l2_weight)
    loss.backward()
    return H.flat_grads_exact(c), stats


def reference(orac, obs, acts, ent_weight, l2_weight):
    """-> dict(g32, g64, stats): what one minibatch's adam_m (beta1 = 0, zero moments) and statistics row are compared with"""
    g32, stats = gradient(orac, obs, acts, ent_weight, l2_weight)
    g64, _ = gradient(orac, obs, acts, ent_weight, l2_weight, double=True)
    return dict(g32=g32, g64=g64, stats=stats)


def offsets(case: Case):
    """ph_bc_layout's offsets, restated: W1[F][32] b1 W2[32][32] b2 act_W[32][L] act_b val_W[32] val_b"""
    Hd, o, out = orc.BC_HIDDEN, 0, {}
    for name, n in (("W1", case.F * Hd), ("b1", Hd), ("W2", Hd * Hd), ("b2", Hd), ("act_W", Hd * case.L), ("act_b", case.L),
                    ("val_W", Hd), ("val_b", 1)):
        out[name] = o
        o += n
    out["P"] = o
    return out


def assert_stats(row, stats, n_rows, where=()):
    """a PH_BC_NSTAT row against bc_loss's dict at tests/test_gpu_bc.py's bound, and the row count"""
    for j, k in enumerate(STAT_KEYS):
        assert abs(row[j] - stats[k]) <= 2e-5 + 2e-4 * abs(stats[k]), (where, k, row[j], stats[k])
    assert int(row[7]) == n_rows, (where, row[7], n_rows)


# ---- out-of-range entries: the kernels clamp expert actions and one-hot observation components into their range ----------------------
def poison(case: Case, obs, acts, seed: int = 0):
    """-> (obs, acts, rows): copies with a few rows out of range -- per action component -1, n and n + 5 in turn; one-hot
    observations: -1 and n"""
    obs, acts = obs.copy(), acts.copy()
    N = len(obs)
    rows = np.random.default_rng(200 + seed).permutation(N)[:max(3, N // 6)]
    for i, r in enumerate(rows):
        for c, n in enumerate(case.act.nvec):
            acts[r, c] = (-1, n, n + 5)[(i + c) % 3]
        if case.onehot:
            for c, n in enumerate(case.obs.nvec):
                if (i + c) % 2 == 0:
                    obs[r, c] = (-1, n)[(i // 2 + c) % 2]
    return obs, acts, rows


def clamp(case: Case, obs, acts):
    """what the kernels make of out-of-range entries"""
    acts = np.clip(acts, 0, np.asarray(case.act.nvec, np.float32) - 1)
    if case.onehot:
        obs = np.clip(obs, 0, np.asarray(case.obs.nvec, np.float32) - 1)
    return obs.astype(np.float32), acts.astype(np.float32)


# ---- forward: action mask, teacher-forced inverse-CDF sampling, given actions -------------------------------------------------------------
def forward_inputs(case: Case, n: int, seed: int = SAMPLING_SEED):
    """-> dict(obs (n, D), mask (n, L) uint8 with at least one allowed entry per component, given (n, A) allowed actions,
    uniforms (n, A) float32 in [0, 1))"""
    rng = np.random.default_rng(1000 * seed + n)
    obs = H.sample_obs(case.obs, n, rng)
    mask = (rng.random((n, case.L)) < 0.6).astype(np.uint8)
    lo = 0
    for k in case.act.nvec:
        keep = rng.integers(0, k, size=n)
        mask[np.arange(n), lo + keep] = 1
        lo += k
    # given actions are drawn among the allowed entries: a masked one has log-prob ~ -30 per component, and float32's spacing at
    # |log_prob| ~ 30 A (A up to 9) is already past the 2e-5 the log-prob is held to -- on the checker as on the device
    given, lo = [], 0
    for k in case.act.nvec:
        given.append(((rng.random((n, k)) + 1e-3) * mask[:, lo:lo + k]).argmax(axis=1))
        lo += k
    given = np.stack(given, axis=1).astype(np.float32)
    uniforms = rng.random((n, case.A), dtype=np.float32)
    return dict(obs=obs, mask=mask, given=given, uniforms=uniforms)


def masked_logits(orac, obs, mask):
    """the checker's logits minus 30 on every masked entry (reference modular/policies.py:330-333), in the checker's dtype"""
    double = next(orac.parameters()).dtype == th.float64
    with th.no_grad():
        if double:
            with H.float64_checker():
                z = orac.logits(th.as_tensor(obs))
        else:
            z = orac.logits(th.as_tensor(obs))
    return z - 30.0 * (1.0 - th.as_tensor(mask).to(z.dtype))


def masked_evaluate(orac, obs, mask, acts):
    """-> (logits, values (n,), log_prob (n,), entropy (n,)) of `acts` under the mask, numpy, in the checker's dtype"""
    z = masked_logits(orac, obs, mask)
    double = z.dtype == th.float64
    with th.no_grad():
        if double:
            with H.float64_checker():
                v = orac.value_net(orac._latent(th.as_tensor(obs)))
        else:
            v = orac.value_net(orac._latent(th.as_tensor(obs)))
        a = th.as_tensor(np.asarray(acts)).long().reshape(len(obs), -1)
        logp, ent = 0.0, 0.0
        for c, zc in enumerate(th.split(z, list(orac.act_space.nvec), dim=1)):
            dist = th.distributions.Categorical(logits=zc)
            logp = logp + dist.log_prob(a[:, c])
            ent = ent + dist.entropy()
    return z.numpy(), v.reshape(-1).numpy(), logp.numpy(), ent.numpy()


def sampling_reference(orac, obs, mask, uniforms):
    """teacher-forced sampling on the masked softmax -> (actions (n, A) by orc.inverse_cdf_sample on the float32 checker, decided
    (n,) bool: no component's uniform lies within EDGE of an edge of the float64 CDF)"""
    o64 = copy.deepcopy(orac).double()
    z32, z64 = masked_logits(orac, obs, mask), masked_logits(o64, obs, mask)
    u = th.as_tensor(uniforms)
    acts, decided = [], np.ones(len(obs), bool)
    nvec = list(orac.act_space.nvec)
    for c, (zc32, zc64) in enumerate(zip(th.split(z32, nvec, dim=1), th.split(z64, nvec, dim=1))):
        acts.append(orc.inverse_cdf_sample(th.softmax(zc32, dim=1), u[:, c]).numpy())
        edges = th.cumsum(th.softmax(zc64, dim=1), dim=1).numpy()
        decided &= (np.abs(edges - uniforms[:, c:c + 1].astype(np.float64)) >= EDGE).all(axis=1)
    return np.stack(acts, axis=1), decided


def component_probabilities(orac, obs_row, mask_row):
    """float64 probabilities of every category of every action component for ONE observation row -> list of arrays"""
    o64 = copy.deepcopy(orac).double()
    z = masked_logits(o64, obs_row[None], mask_row[None])
    return [th.softmax(zc, dim=1)[0].numpy() for zc in th.split(z, list(orac.act_space.nvec), dim=1)]
