"""One clip + Adam step in float64 numpy, and the error a float32 implementation of it may show when what feeds the step is
within the tolerances the suite already enforces.  Plain numpy: no torch, no device.

The formulas are torch.nn.utils.clip_grad_norm_'s (coef = min(1, max_norm / (norm + 1e-6))) and torch.optim.Adam's single-tensor
update with t = t0 + 1 per entry:
    g' = coef * g (+ l2 * p0 for BC's L2 term, which has no clip)
    m = m0 + (1 - beta1) (g' - m0),   v = beta2 v0 + (1 - beta2) g'^2
    p = p0 - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
"""
from __future__ import annotations

import numpy as np

# the two tolerances on what feeds the step: gradient entries (_assert_grads), gradient norm (_assert_train_stats)
E_G_ABS, E_G_REL = 1e-6, 2e-4
E_N_ABS, E_N_REL = 1e-5, 2e-4


def _f64(x):
    return np.asarray(x, np.float64)


def _ulp32(x):
    """one float32 unit in the last place at |x|"""
    return np.spacing(np.abs(_f64(x)).astype(np.float32)).astype(np.float64)


def _update(m, v, t, lr, beta1, beta2, eps):
    t = _f64(t)
    return lr / (1.0 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)


def adam_step_f64(p0, m0, v0, t0, g, max_norm, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, clip=True, l2=0.0, live=None,
                  norm=None, coef_scale=1.0, clamp=True, stale_step=False, raw_into_m=False, raw_into_v=False):
    """-> (p, m, v, norm, coef).  `t0`: steps taken so far, a scalar or one per entry.  `live` (bool per entry): entries that
    take part (the others keep p, m, v; the caller keeps their step count) -- ModularAlgorithm's value sides.
    The remaining keywords build WRONG optimizers for tests/test_optimizer_checks.py: coef_scale multiplies the clip coefficient,
    clamp=False drops the min(1, .), stale_step uses t0 for t0 + 1 in the bias corrections, raw_into_m / raw_into_v feed the
    unclipped gradient into that moment."""
    p0, m0, v0, g = _f64(p0), _f64(m0), _f64(v0), _f64(g)
    t = np.broadcast_to(_f64(t0), p0.shape) + (0.0 if stale_step else 1.0)
    norm = float(np.sqrt(np.sum(g * g))) if norm is None else float(norm)    # norm=: the norm as someone else computed it
    coef = 1.0
    if clip:
        coef = max_norm / (norm + 1e-6)
        if clamp:
            coef = min(1.0, coef)
        coef *= coef_scale
    reg = l2 * p0
    cg = coef * g + reg
    gm = g + reg if raw_into_m else cg
    gv = g + reg if raw_into_v else cg
    m = m0 + (1.0 - beta1) * (gm - m0)
    v = beta2 * v0 + (1.0 - beta2) * gv * gv
    with np.errstate(divide="ignore", invalid="ignore"):
        p = p0 - _update(m, v, np.maximum(t, 1e-300), lr, beta1, beta2, eps)
    if live is not None:
        live = np.asarray(live, bool)
        p, m, v = np.where(live, p, p0), np.where(live, m, m0), np.where(live, v, v0)
    return p, m, v, norm, coef


def one_step_bounds(p0, m0, v0, t0, g_ref, max_norm, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, clip=True, l2=0.0,
                    e_g_abs=E_G_ABS, e_g_rel=E_G_REL, e_n_abs=E_N_ABS, e_n_rel=E_N_REL, norm=None):
    """Per-entry bounds on |device - reference| for m, v and p after ONE step from the shared state (p0, m0, v0, t0), derived from
    the tolerances on the gradient (e_g) and on its norm (e_n); e_*_abs = e_*_rel = 0 leaves the rounding terms alone.

      e_g  = e_g_abs + e_g_rel * max|g_ref|                     every gradient entry
      e_n  = e_n_abs + e_n_rel * n_ref                          the norm
      e_c  = 0 where neither side can clip (max_norm / (n_ref + e_n + 1e-6) >= 1), else coef_ref * e_n / n_ref
             (d/dn of max_norm / (n + 1e-6) is coef / (n + 1e-6)) + 2 ulps of coef_ref: the sum and the division that make the
             coefficient are float32 operations on both sides
      e_cg = coef_ref * e_g + |g_ref| * e_c + 1 ulp of |coef g|  the clipped gradient (the product is rounded on both sides)
      e_m  = (1 - beta1) * e_cg                                 + rounding
      e_v  = (1 - beta2) * (2 |coef g| e_cg + e_cg^2)           + rounding
      e_p  : the update u(m, v) is monotone in m and in v, so its largest deviation over the box (m +- e_m, max(v +- e_v, 0)) is
             at one of the four corners; evaluated there in float64                          + rounding
    Rounding terms (float32, both sides):
      m: 4 ulps at max(|m_ref|, |m0|).  The issue's sketch took them at |m_ref|; m = m0 + 0.1 (g' - m0) is a difference, and where
         it cancels (|m| << |m0|) the rounding of the operands, half an ulp of |m0| each, is what remains.
      v: 4 ulps of v_ref (a sum of two non-negative terms: no cancellation).
      p: 2 ulps at max(|p_ref|, |p0|) for the final subtraction (the same cancellation argument), and 4 ulps of the update
         itself: sqrt, two divisions, an addition and a product, each correctly rounded or within one ulp.
    -> dict(e_m, e_v, e_p, e_n, and the float64 reference p, m, v, norm, coef, update)."""
    p0, m0, v0, g = _f64(p0), _f64(m0), _f64(v0), _f64(g_ref)
    p, m, v, norm, coef = adam_step_f64(p0, m0, v0, t0, g, max_norm, lr, beta1, beta2, eps, clip=clip, l2=l2, norm=norm)
    t = np.broadcast_to(_f64(t0), p0.shape) + 1.0
    e_g = e_g_abs + e_g_rel * np.abs(g).max()
    e_n = e_n_abs + e_n_rel * norm
    if not clip or max_norm / (norm + e_n + 1e-6) >= 1.0:
        e_c = 0.0
    else:
        e_c = coef * e_n / norm + 2.0 * float(_ulp32(coef))
    cg = coef * g + l2 * p0
    e_cg = coef * e_g + np.abs(g) * e_c + _ulp32(cg)
    e_m = (1.0 - beta1) * e_cg + 4.0 * _ulp32(np.maximum(np.abs(m), np.abs(m0)))
    e_v = (1.0 - beta2) * (2.0 * np.abs(cg) * e_cg + e_cg ** 2) + 4.0 * _ulp32(v)
    u = _update(m, v, t, lr, beta1, beta2, eps)
    dev = np.zeros_like(u)
    for sm in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            uc = _update(m + sm * e_m, np.maximum(v + sv * e_v, 0.0), t, lr, beta1, beta2, eps)
            dev = np.maximum(dev, np.abs(uc - u))
    e_p = dev + 2.0 * _ulp32(np.maximum(np.abs(p), np.abs(p0))) + 4.0 * _ulp32(u)
    return dict(e_m=e_m, e_v=e_v, e_p=e_p, e_n=e_n, p=p, m=m, v=v, norm=norm, coef=coef, update=u)


# ---- the scenarios of tests/test_gpu_optimizer.py (DESIGN.md has the table) ----------------------------------------------------
SCENARIOS = ("fresh", "resumed-clipped", "resumed-unclipped", "just-clipped", "never", "late", "eps", "lr")
LOADED = tuple(s for s in SCENARIOS if s != "fresh")


def scenario_state(scenario: str, P: int, n_ref: float, seed: int = 0, state_scale: float = 1e-3):
    """-> (m0, v0, t0, max_grad_norm, lr) of a scenario for a P-entry parameter vector whose gradient has norm n_ref.
    Random state: m0 = state_scale N(0, 1), v0 = (state_scale N(0, 1))^2 from a seeded generator ("eps": 1e-5 for state_scale)."""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(P), rng.standard_normal(P)
    lr = 3e-4
    if scenario == "fresh":
        return np.zeros(P, np.float32), np.zeros(P, np.float32), 0, 0.5, lr
    if scenario == "eps":
        return (1e-5 * a).astype(np.float32), ((1e-5 * b) ** 2).astype(np.float32), 100000, float(np.float32(1e-4)), lr
    m0, v0 = (state_scale * a).astype(np.float32), ((state_scale * b) ** 2).astype(np.float32)
    t0, max_norm = {"resumed-clipped": (7, 0.5), "resumed-unclipped": (7, 1.25 * n_ref), "just-clipped": (7, 0.8 * n_ref),
                    "never": (7, 1e9), "late": (100000, 0.8 * n_ref), "lr": (7, 0.5)}[scenario]
    if scenario == "lr":
        lr = 1e-3 * 0.25            # learning_rate = lambda p: 1e-3 * p at _current_progress_remaining = 0.25
    return m0, v0, t0, float(np.float32(max_norm)), lr       # (a value float32 holds: both sides get the same number)


def check_one_step(got, ref, bounds, where=()):
    """got, ref: dicts with m, v, p (device values, float32 checker values); every entry of each under `bounds`.  Prints the
    largest error beside the bound at that entry and the largest error / bound ratio; -> list of the names that FAIL."""
    failed = []
    for k in ("m", "v", "p"):
        err = np.abs(_f64(got[k]) - _f64(ref[k]))
        b = bounds["e_" + k]
        ratio = err / b
        i = int(np.argmax(ratio))
        print(where, k, "largest error %.3g (bound there %.3g); largest error / bound %.3g at entry %d (error %.3g, bound %.3g)"
              % (err.max(), b[int(np.argmax(err))], ratio[i], i, err[i], b[i]))
        if not (err <= b).all():
            failed.append(k)
    return failed
