"""The checker side of tests/test_gpu_sampler_streams.py: the cases of the categorical own-draw test, their inputs, the host
prediction of every drawn action from tests/philox_ref.py and the checker's float64 softmax, the rows that decide nothing
("near": a uniform within helpers.EDGE_MARGIN of a CDF edge of the CHECKER, never of the device) and the shifted-coordinate
negative control.  Everything here runs on the CPU; tests/test_philox_host.py checks on it that the caps on near rows and the
control hold for the chosen key, counters and observation seeds.

`kernel` names what the case reaches, read off the dispatch (csrc/ph_policy.hip launch_policy_fwd: fwd16_eligible = one feature
chunk, Discrete head of <= 8 logits, n < 16384 -> policy_fwd16_kernel, whose row tail is discrete8_row_tail; fwd16h_eligible =
one-hot observations of <= 64 components, Lp == 32, n < 16384 -> policy_fwd16h_kernel, head_draw32 / head_tail32; everything else
-> policy_fwd_kernel, general_row_tail -- which hands a small Discrete head on to discrete8_row_tail)."""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np
import torch as th

from tests import helpers as H
from tests import philox_ref as R

KEY = 0x5EED00070000BEEF                      # a Philox key with a non-zero high word (below 2**63: the ABI's signed range is not at issue)
COUNTERS = (7, 2 ** 32 + 5)                   # the second fails a kernel that drops the counter's high word
# observation seed per case, chosen on the checker alone (no device involved): the smallest seed at which no row of the case's
# n <= 65 inputs is near under either counter, at most 3 % are at n >= 257, and the control holds (tests/test_philox_host.py asserts it)
OBS_SEEDS = {'overcooked': 1, 'liar': 3, 'onehot32': 1, 'arch32-wide': 2, 'adapmult-small': 1, 'bc-liar': 1}      # every other case: 0
NEAR_CAP_LARGE, CONTROL_MIN = 0.03, 0.20
FORWARD_TOL = 2e-5


@dataclass(frozen=True)
class Case:
    id: str
    family: str                # mlp | arch | adapmult | modular | bc
    name: str                  # helpers.CONFIGS name, modular_cases.SHAPES name or a bc_cases id
    rows: tuple
    kernel: str
    gemm_modes: tuple = (None,)
    mask: bool = False
    extra: dict = field(default_factory=dict, hash=False, compare=False)


SMALL_ROWS = (1, 63, 64, 65, 257)
CASES = (
    [Case(f"{name}", "mlp", name, SMALL_ROWS, "policy_fwd16_kernel<MFMA | VALU> -> discrete8_row_tail", gemm_modes=(0, 1))
     for name in ("overcooked", "rps", "mpe8")]
    + [Case("overcooked-16384", "mlp", "overcooked", (16384,), "policy_fwd_kernel<64 rows> -> general_row_tail -> discrete8_row_tail",
            gemm_modes=(0,))]
    + [Case(name, "mlp", name, (65, 257), "policy_fwd16h_kernel -> head_draw32 / head_tail32", gemm_modes=(0, 1))
       for name in ("liar", "onehot32", "discrete20")]
    + [Case(name, "mlp", name, (65, 257), "policy_fwd_kernel -> general_row_tail, per-component loop", gemm_modes=(0,))
       for name in ("wide", "quad16", "onehot17")]
    + [Case("arch32-wide", "arch", "wide", (65, 257), "ph_arch.hip tower kernel -> general_row_tail", extra=dict(arch=(32,))),
       Case("mpe8-masked", "mlp", "mpe8", (65, 257), "policy_fwd16_kernel -> discrete8_row_tail under an action mask", gemm_modes=(0,),
            mask=True),
       Case("discrete20-masked", "mlp", "discrete20", (257,), "policy_fwd16h_kernel -> head_tail32 under an action mask",
            gemm_modes=(0,), mask=True),
       Case("adapmult-small", "adapmult", "adap_small", (7, 64), "ph_adapmult.hip am_act_kernel -> discrete8_row_tail"),
       Case("modular-small", "modular", "mod_small", (70,), "ph_modular.hip modular_act_kernel -> discrete8_row_tail",
            extra=dict(K=2, partner=1, kw={"nomain": True})),
       Case("modular-rps", "modular", "mod_rps", (70,), "ph_modular.hip modular_act_kernel -> discrete8_row_tail",
            extra=dict(K=2, partner=1, kw={})),
       Case("bc-liar", "bc", "liar", (65, 300), "ph_bc.hip bc_forward_kernel"),
       Case("bc-box33-3x30x7", "bc", "box33-3x30x7", (65, 300), "ph_bc.hip bc_forward_kernel", mask=True)]
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- checker, inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def checker(case_id: str):
    """the case's float32 checker (perturb = 0.3: logits far from uniform, 1 - sum p^2 far above the control's 20 %)"""
    case = BY_ID[case_id]
    if case.family == "mlp":
        return H.oracle_policy(case.name, seed=3)
    if case.family == "arch":
        from tests import arch_oracle as A
        return A.oracle_policy(case.name, case.extra["arch"], seed=3)
    if case.family == "adapmult":
        from tests.adapmult_cases import _oracle
        return _oracle(case.name, seed=3)
    if case.family == "modular":
        from tests.modular_cases import _oracle
        return _oracle(case.name, case.extra["K"], **case.extra["kw"])
    from tests import bc_cases as B
    return B.checker(B.BY_ID[case.name], 1)[0]


def spaces(case: Case):
    """(observation SpaceSpec, action SpaceSpec)"""
    if case.family == "modular":
        from tests.modular_cases import SHAPES
        return SHAPES[case.name]
    if case.family == "bc":
        from tests import bc_cases as B
        return B.BY_ID[case.name].obs, B.BY_ID[case.name].act
    return H.CONFIGS[case.name]


def inputs(case: Case, n: int):
    """-> (obs (n, D) float32 with DISTINCT rows, mask (n, L) uint8 or None): seeded by the case and n"""
    obs_s, act_s = spaces(case)
    rng = np.random.default_rng([OBS_SEEDS.get(case.id, 0), sum(case.id.encode()), n])
    obs = H.sample_obs(obs_s, n, rng)
    mask = None
    if case.mask:
        L = act_s.flat_len
        mask = (rng.random((n, L)) < 0.6).astype(np.uint8)
        lo = 0
        for k in act_s.nvec:                                     # at least one allowed entry per component
            mask[np.arange(n), lo + rng.integers(0, k, size=n)] = 1
            lo += k
    return obs, mask


def probabilities64(case: Case, obs: np.ndarray, mask) -> list:
    """the checker's float64 softmax per action component: list of (n, K_c) arrays"""
    o64 = copy.deepcopy(checker(case.id)).double()
    with H.float64_checker(), th.no_grad():
        x = th.as_tensor(obs)
        if case.family == "modular":
            lp, _, p_pi, _, pm = o64._towers(x, case.extra["partner"])
            z = o64._mean_actions(lp, p_pi, pm, None)
        else:
            z = o64.logits(x)
        if mask is not None:                                     # modular/policies.py:330-333: logits - 30 on masked entries
            z = z - 30.0 * (1.0 - th.as_tensor(mask).double())
    assert z.dtype == th.float64
    _, act_s = spaces(case)
    return [th.softmax(zc, dim=1).numpy() for zc in th.split(z, list(act_s.nvec), dim=1)]


# ---- the host prediction ---------------------------------------------------------------------------------------------------------------
def uniforms(n: int, A: int, key: int, counter: int, row_shift: int = 0, comp_shift: int = 0, row0: int = 0) -> np.ndarray:
    """(n, A) float32: component c of row g draws philox_uniform(key, counter, g, c)"""
    rows = (np.arange(n, dtype=np.int64) + row0 + row_shift)[:, None]
    comps = (np.arange(A, dtype=np.int64) + comp_shift)[None, :]
    return R.uniform(key, counter, rows, comps)


def predict(probs: list, u: np.ndarray):
    """-> (actions (n, A) int64, near (n,) bool)"""
    acts = np.stack([R.inverse_cdf(p, u[:, c]) for c, p in enumerate(probs)], axis=1)
    near = np.zeros(len(u), bool)
    for c, p in enumerate(probs):
        near |= R.near_edge(p, u[:, c], H.EDGE_MARGIN)
    return acts, near


def log_prob64(probs: list, acts: np.ndarray) -> np.ndarray:
    return sum(np.log(p[np.arange(len(acts)), acts[:, c]]) for c, p in enumerate(probs))


SHIFTS = {"row + 1": dict(row_shift=1), "component + 1": dict(comp_shift=1), "counter + 1": dict(dc=1),
          "counter + 2**32": dict(dc=2 ** 32), "key high word cleared": dict(key_mask=0xFFFFFFFF)}


def shifted_uniforms(n: int, A: int, key: int, counter: int, shift: str, row0: int = 0) -> np.ndarray:
    s = dict(SHIFTS[shift])
    k = key & s.pop("key_mask", R.MASK64)
    assert shift != "key high word cleared" or k != key
    return uniforms(n, A, k, counter + s.pop("dc", 0), row0=row0, **s)


def control(probs: list, n: int, key: int, counter: int, row0: int = 0) -> dict:
    """the negative control: per shifted coordinate, the share of rows whose host prediction changes"""
    A = len(probs)
    base, _ = predict(probs, uniforms(n, A, key, counter, row0=row0))
    return {name: float((predict(probs, shifted_uniforms(n, A, key, counter, name, row0))[0] != base).any(axis=1).mean())
            for name in SHIFTS}


def assert_caps_and_control(case_id: str, n: int, near: np.ndarray, ctl: dict, counter: int) -> None:
    """no near row at n <= 65, at most 3 % at n >= 257 (in between: 3 %); every shifted coordinate moves >= 20 % of the rows.  One
    row alone decides no share: the control starts at n >= 5 rows (20 % of 5 is one row)."""
    where = (case_id, n, counter)
    if n <= 65:
        assert not near.any(), (where, np.nonzero(near)[0])
    else:
        assert near.mean() <= NEAR_CAP_LARGE, (where, near.mean())
    if n >= 5:
        low = {k: v for k, v in ctl.items() if v < CONTROL_MIN}
        assert not low, (where, low)


# ---- the one-launch rollouts (ph_scripted_rollout) --------------------------------------------------------------------------------------
ROLLOUT_NAME = "overcooked"                   # Box 62 -> Discrete 6: the shape class of policy_fwd16_rollout_kernel
ROLLOUT_SHAPES = ((17, 2), (40, 7), (16, 1), (17, 3))      # (E, T): two shapes of the bitwise test; the tail wave's smallest: one step, one overlapped tail
ROLLOUT_RUNS = ((COUNTERS[1], 0), (COUNTERS[0], 1))        # (Philox counter of step 0, RNG epoch word): the word rides in the counter's high half
ROLLOUT_SEEDS = {}                            # seed of SyntheticRollouts per shape, chosen like OBS_SEEDS


def rollout_data(E: int, T: int, device="cpu"):
    from pantheonrl_amd.vec import SyntheticRollouts
    obs_s, _ = H.CONFIGS[ROLLOUT_NAME]
    return SyntheticRollouts(H.to_space(obs_s), E, T, horizon=5, seed=ROLLOUT_SEEDS.get((E, T), 0), device=device)


def rollout_prediction(obs: np.ndarray, key: int, counter0: int, epoch: int):
    """obs (T, E, D) as the rollout buffer stores it -> (actions (T, E), near (T, E), control: share of moved rows per shift):
    row t holds the draw of counter0 + t + (epoch << 32) at row = environment, component 0"""
    T, E = obs.shape[:2]
    case = BY_ID[ROLLOUT_NAME]
    acts, near, ctl = [], [], {k: 0.0 for k in SHIFTS}
    for t in range(T):
        probs = probabilities64(case, obs[t], None)
        c = counter0 + t + (epoch << 32)
        a, nr = predict(probs, uniforms(E, 1, key, c))
        acts.append(a[:, 0]), near.append(nr)
        for k, v in control(probs, E, key, c).items():
            ctl[k] += v / T
    return np.stack(acts), np.stack(near), ctl


def assert_rollout_caps(where, near: np.ndarray, ctl: dict) -> None:
    if near.size <= 65:
        assert not near.any(), (where, np.argwhere(near))
    else:
        assert near.mean() <= NEAR_CAP_LARGE, (where, near.mean())
    low = {k: v for k, v in ctl.items() if v < CONTROL_MIN}
    assert not low, (where, low)


# ---- the grouped forward of the Liar's Dice pool (ph_pool_forward): clone tiles beside 64-64 tiles -----------------------------------
POOL_N = 50
POOL_KINDS = ("clone", "frozen")              # member 0: a behavioural clone (bc_clone_tile, ph_bc_row.h); member 1: a frozen 64-64 policy
POOL_KEYS = (KEY, KEY + (1 << 33) + 1)        # every member samples under its own key
POOL_CHECKERS = ("bc-liar", "liar")
POOL_SEED = 0                                 # chosen like OBS_SEEDS


def pool_inputs():
    """-> (obs (n, 30), member of every table (n,), active (n,) uint8): tables alternate between the members, four sit out"""
    rng = np.random.default_rng([POOL_SEED, 77])
    obs = H.sample_obs(H.CONFIGS["liar"][0], POOL_N, rng)
    pid = (np.arange(POOL_N) % 2).astype(np.int32)
    active = np.ones(POOL_N, np.uint8)
    active[[3, 17, 30, 41]] = 0
    return obs, pid, active


def pool_prediction(obs, pid, counter: int):
    """-> (actions (n, 2), near (n,), control per shift): table e of member k draws (POOL_KEYS[k], counter, row = e, component)"""
    n = len(obs)
    acts, near, ctl = np.zeros((n, 2), np.int64), np.zeros(n, bool), {k: 0.0 for k in SHIFTS}
    for k, cid in enumerate(POOL_CHECKERS):
        probs = probabilities64(BY_ID[cid], obs, None)
        a, nr = predict(probs, uniforms(n, 2, POOL_KEYS[k], counter))
        mine = pid == k
        acts[mine], near[mine] = a[mine], nr[mine]
        for name in SHIFTS:
            moved = (predict(probs, shifted_uniforms(n, 2, POOL_KEYS[k], counter, name))[0] != a).any(axis=1)
            ctl[name] += float(moved[mine].sum()) / n
    return acts, near, ctl


def device(case, orac=None):
    """the case's device object holding the parameters of `orac` (default: the case's cached checker) -- the one function here
    that needs a GPU"""
    orac = checker(case.id) if orac is None else orac
    if case.family == "mlp":
        return H.device_policy(case.name, orac)
    if case.family == "arch":
        from tests import arch_oracle as A
        return A.device_policy(case.name, orac)
    if case.family == "adapmult":
        from tests.adapmult_cases import _device as dev
        return dev(case.name, orac)
    if case.family == "modular":
        from tests.modular_cases import _device as dev
        return dev(case.name, orac, case.extra["K"], **case.extra["kw"])
    from pantheonrl_amd.bc import FeedForward32Policy
    obs_s, act_s = spaces(case)
    pol = FeedForward32Policy(H.to_space(obs_s), H.to_space(act_s), device="cuda:0", seed=7)
    pol.set_flat_params(orac.flat_params())
    return pol
