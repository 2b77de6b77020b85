// The PPO loss of one minibatch row (SB3 PPO.train): the definition the gradient kernels call.  (ppo_grad_split_oh_kernel's policy tail
// alone keeps a written-out copy of ppo_policy_row, see there.)  Scalars in, small structs out; a kernel keeps its own softmax /
// log-sum-exp, LDS layout, lane mapping, row masking and the choice of the lane that accumulates.
// The expression trees (operand order, association) are what the results are bit-compared on: do not tidy them.
#pragma once
#include "ph_device.h"

namespace ph {

// The statistics and dv are member functions, not fields filled in by the helper, and the structs carry what those need (ratio,
// pl1, pl2, clip; pass, vf_coef, inv_nb).  Plain fields were tried: a kernel uses the statistics only behind its `valid` branch, LLVM
// then sinks the helper's arithmetic into that block -- in another order than the kernel had it, and in ppo_grad_split_oh_kernel's
// value tail it turned two selects into a branch -- and registers and instruction order of the compiled kernels moved.  As member
// functions the arithmetic is emitted where the kernel evaluates it, as when each kernel wrote the loss out itself.
struct PolicyRow {
  float g_lp;   // dL/dlogp
  float g_en;   // dL/dH (entropy)
  float lr;     // logp - old_logp
  float ratio, pl1, pl2, clip;
  __device__ __forceinline__ float loss() const { return -fminf(pl1, pl2); }                               // policy-loss partial
  __device__ __forceinline__ float clipped() const { return (fabsf(ratio - 1.0f) > clip) ? 1.f : 0.f; }   // clip-fraction partial
  __device__ __forceinline__ float kl() const { return (ratio - 1.0f) - lr; }                              // approximate-KL partial
};

// Clipped surrogate of one row.  torch.min backward: the smaller branch gets the gradient, ties split 1/2 + 1/2; clamp passes
// the gradient iff lo <= ratio <= hi.
__device__ __forceinline__ PolicyRow ppo_policy_row(float logp, float old_logp, float adv, float clip, float ent_coef, float inv_nb) {
  PolicyRow o;
  o.lr = logp - old_logp;
  o.ratio = fast_exp(o.lr);
  o.clip = clip;
  const float lo_c = 1.0f - clip, hi_c = 1.0f + clip;
  const float rc = fminf(fmaxf(o.ratio, lo_c), hi_c);
  o.pl1 = adv * o.ratio, o.pl2 = adv * rc;
  const float inr = (o.ratio >= lo_c && o.ratio <= hi_c) ? 1.f : 0.f;
  const float gate = (o.pl1 < o.pl2) ? 1.f : ((o.pl1 > o.pl2) ? inr : 0.5f + 0.5f * inr);
  o.g_lp = -inv_nb * adv * o.ratio * gate;
  o.g_en = -ent_coef * inv_nb;
  return o;
}

// the row's partial statistics {policy loss, -, entropy loss, clip fraction, approximate KL} into a lane's record
__device__ __forceinline__ void ppo_policy_stats(float (&st)[NSTATP], const PolicyRow& p, float ent) {
  st[0] += p.loss();
  st[2] += -ent;
  st[3] += p.clipped();
  st[4] += p.kl();
}

// dL/dlogit of one slot of a categorical head: probability p, log-probability lp, entropy ent of its component, hit = (k == act)
__device__ __forceinline__ float ppo_logit_grad(float g_lp, float g_en, float hit, float p, float lp, float ent) {
  return g_lp * (hit - p) + g_en * (-p * (lp + ent));
}

struct ValueRow {
  float err;   // clipped prediction - return; the row's value loss is err * err
  float pass, vf_coef, inv_nb;
  __device__ __forceinline__ float dv() const { return vf_coef * 2.0f * err * inv_nb * pass; }   // dL/dv
};

struct ValueClip {
  float vp;     // prediction after the clip_range_vf clamp
  float pass;   // 1 if the clamp passes the gradient: |v - old_v| <= clip_vf
};

// clip_vf < 0: no clipping
__device__ __forceinline__ ValueClip ppo_value_clip(float v, float old_v, float clip_vf) {
  float vp = v, pass = 1.f;
  if (clip_vf >= 0.f) {
    const float dlt = v - old_v;
    pass = (dlt >= -clip_vf && dlt <= clip_vf) ? 1.f : 0.f;
    vp = old_v + fminf(fmaxf(dlt, -clip_vf), clip_vf);
  }
  return {vp, pass};
}

// Value loss of one row.  The two-step form is for the one kernel that fetches the return only after the clamp (am_loss_vf_kernel):
// as a by-value argument of the one-call form the load moves in front of the clamp's branch and costs that kernel a VGPR.
__device__ __forceinline__ ValueRow ppo_value_row(const ValueClip& c, float ret, float vf_coef, float inv_nb) {
  return {c.vp - ret, c.pass, vf_coef, inv_nb};
}
__device__ __forceinline__ ValueRow ppo_value_row(float v, float old_v, float ret, float clip_vf, float vf_coef, float inv_nb) {
  return ppo_value_row(ppo_value_clip(v, old_v, clip_vf), ret, vf_coef, inv_nb);
}

// One lane per row, logits in LDS, any Discrete / MultiDiscrete head: pass 1 sums log-prob and entropy over the components, pass 2
// overwrites z[0..L) with dL/dlogits; the padding up to Lp is zeroed.  Lp (= nd.Lp) is a parameter because ppo_grad_kernel has it
// as a template constant: with nd.Lp read at run time here, two of that kernel's instantiations changed registers.
__device__ __forceinline__ void ppo_two_pass_row(const NetDims& nd, float* z, const float* rb_act, int phys, float adv, float old_logp,
                                                 float clip, float ent_coef, float inv_nb, float (&st)[NSTATP], int Lp) {
  float logp = 0.f, ent = 0.f;
  for (int c = 0; c < nd.A; ++c) {
    const int lo = nd.act_off[c], nk = nd.act_off[c + 1] - lo;
    float m = z[lo];
    for (int k = 1; k < nk; ++k) m = fmaxf(m, z[lo + k]);
    float se = 0.f;
    for (int k = 0; k < nk; ++k) se += fast_exp(z[lo + k] - m);
    const float lse = m + fast_log(se);
    int act = (int)rb_act[(size_t)phys * nd.A + c];
    act = act < 0 ? 0 : (act >= nk ? nk - 1 : act);
    float e = 0.f;
    for (int k = 0; k < nk; ++k) {
      const float lp = z[lo + k] - lse;
      e -= fast_exp(lp) * lp;
    }
    logp += z[lo + act] - lse;
    ent += e;
  }
  const PolicyRow p = ppo_policy_row(logp, old_logp, adv, clip, ent_coef, inv_nb);
  ppo_policy_stats(st, p, ent);
  for (int c = 0; c < nd.A; ++c) {
    const int lo = nd.act_off[c], nk = nd.act_off[c + 1] - lo;
    float m = z[lo];
    for (int k = 1; k < nk; ++k) m = fmaxf(m, z[lo + k]);
    float se = 0.f;
    for (int k = 0; k < nk; ++k) se += fast_exp(z[lo + k] - m);
    const float lse = m + fast_log(se);
    int act = (int)rb_act[(size_t)phys * nd.A + c];
    act = act < 0 ? 0 : (act >= nk ? nk - 1 : act);
    float hc = 0.f;
    for (int k = 0; k < nk; ++k) {
      const float lp = z[lo + k] - lse;
      hc -= fast_exp(lp) * lp;
    }
    for (int k = 0; k < nk; ++k) {
      const float lp = z[lo + k] - lse;
      z[lo + k] = ppo_logit_grad(p.g_lp, p.g_en, (k == act) ? 1.f : 0.f, fast_exp(lp), lp, hc);
    }
  }
  for (int k = nd.L; k < Lp; ++k) z[k] = 0.f;
}

}  // namespace ph
