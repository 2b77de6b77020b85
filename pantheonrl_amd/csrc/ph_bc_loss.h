// One minibatch step of behavioural cloning (reference bc.py:291-303 under torch.optim.Adam), everything in it that is not a matrix
// product: the definition bc_train_kernel (VALU loops) and bc_train_mfma_kernel (MFMA tiles) of ph_bc.hip both call -- the role
// ph_ppo_loss.h has for the PPO gradient kernels.  A kernel keeps its products, its LDS layout, how the dataset rows reach LDS
// (a gather per tile; a prefetch pipeline), its block reduction and where Adam's moments live.
// Scalars in, by value (BcCloneArgs in ph_bc_row.h says why nothing takes a reference into a kernel's argument record).  The
// expression trees (operand order, association) are what the results are bit-compared on: do not tidy them.
#pragma once
#include "ph_bc_row.h"

namespace ph {

// ---- the minibatch schedule: which rows of the visiting order a 32-row tile covers ---------------------------------------------------
struct BcTile {
  int ep, start, t0, nb;   // epoch, first position of the minibatch in the epoch's order, first row of the tile in it, its rows
};

struct BcSchedule {
  int N, batch, per_epoch, total;   // dataset rows, rows per minibatch, minibatches per epoch, minibatches of the run
  __device__ __forceinline__ BcTile tile(int mb, int t0) const {
    BcTile t;
    t.ep = mb / per_epoch;
    const int b = mb - t.ep * per_epoch;
    t.start = b * batch;
    t.nb = (N - t.start < batch) ? N - t.start : batch;   // the last minibatch of an epoch is the short one
    t.t0 = t0;
    return t;
  }
  // dataset row of the tile's row r (order: (n_epochs, N), one permutation per epoch), -1 = padding
  __device__ __forceinline__ int row(const int* order, const BcTile t, int r) const {
    return (t.t0 + r < t.nb) ? order[(size_t)t.ep * N + t.start + t.t0 + r] : -1;
  }
};
__device__ __forceinline__ BcSchedule bc_schedule(int N, int batch, int n_epochs, int max_batches) {
  BcSchedule s;
  s.N = N;
  s.batch = batch;
  s.per_epoch = (N + batch - 1) / batch;
  s.total = n_epochs * s.per_epoch;
  if (max_batches > 0 && max_batches < s.total) s.total = max_batches;
  return s;
}

// ---- per row: log-prob of the expert action, entropy, dL/dlogits (one lane per row; sums over the action components) ------------------
// z: the row's L logits in LDS, overwritten with dL/dlogits -- zeros for a padding row (!valid); act_row: its A expert actions, clamped into
// their components here; the row's log-prob, entropy and probability of the expert action are added to s_lp, s_h, s_pt.
__device__ __forceinline__ void bc_loss_row(float* z, const int* act_row, bool valid, const int* act_off, int A, int L, float inv_nb,
                                            float ent_weight, float& s_lp, float& s_h, float& s_pt) {
  if (valid) {
    float lp = 0.f, ent = 0.f;
    for (int comp = 0; comp < A; ++comp) {
      const int lo = act_off[comp], n = act_off[comp + 1] - lo;
      auto zc = [&](int c) { return z[lo + c]; };
      float mx = BC_MAX_INIT;
      for (int c = 0; c < n; ++c) mx = fmaxf(mx, zc(c));
      const float lse = bc_lse(zc, n, mx);
      int act = act_row[comp];
      act = act < 0 ? 0 : (act >= n ? n - 1 : act);
      const float h = bc_entropy(zc, n, lse);
      lp += zc(act) - lse;
      ent += h;
      // d/dz_c [ -(1/nb) log p_a - (w/nb) H ] = -(1/nb)([c = a] - p_c) + (w/nb) p_c ((z_c - lse) + H)
      for (int c = 0; c < n; ++c) {
        const float lq = zc(c) - lse, pc = __expf(lq);
        z[lo + c] = -inv_nb * (((c == act) ? 1.f : 0.f) - pc) + ent_weight * inv_nb * pc * (lq + h);
      }
    }
    s_lp += lp;
    s_h += ent;
    s_pt += __expf(lp);
  } else {
    for (int c = 0; c < L; ++c) z[c] = 0.f;
  }
}

// ---- the statistics row of a minibatch (before the update, like the reference's stats_dict): st[0 .. PH_BC_NSTAT) ---------------------
// sum_sq: sum of the squared parameters; sum_lp, sum_h, sum_pt: the rows' s_lp, s_h, s_pt, each summed over the block.
// (bc_train_kernel alone keeps a written-out copy of this row, see there.)
__device__ __forceinline__ void bc_write_stats(float* st, float sum_sq, float sum_lp, float sum_h, float sum_pt, float inv_nb, int nb,
                                               float ent_weight, float l2_weight) {
  const float l2_norm = 0.5f * sum_sq, mean_lp = sum_lp * inv_nb, mean_h = sum_h * inv_nb;
  const float neglogp = -mean_lp, ent_loss = -ent_weight * mean_h, l2_loss = l2_weight * l2_norm;
  st[0] = neglogp;
  st[1] = mean_h;
  st[2] = ent_loss;
  st[3] = sum_pt * inv_nb;
  st[4] = l2_norm;
  st[5] = l2_loss;
  st[6] = neglogp + ent_loss + l2_loss;
  st[7] = (float)nb;
}

// ---- Adam ----------------------------------------------------------------------------------------------------------------------------
// beta^t of the bias corrections as running products in fp64 (one lane; one pow at the start of a launch instead of two per step):
// advances them by one step and writes bcorr[0] = lr / (1 - beta1^t), bcorr[1] = sqrt(1 - beta2^t)
__device__ __forceinline__ void bc_bias_corrections(double& b1t, double& b2t, float beta1, float beta2, float lr, float* bcorr) {
  b1t *= (double)beta1;
  b2t *= (double)beta2;
  bcorr[0] = (float)((double)lr / (1.0 - b1t));
  bcorr[1] = (float)sqrt(1.0 - b2t);
}

struct BcMoments {
  float m, v;
};
// g: the loss's gradient entry, w its parameter (the L2 term's gradient is added here), m0 / v0 the moments before the step
__device__ __forceinline__ BcMoments bc_adam_moments(float g, float w, float m0, float v0, float l2_weight, float beta1, float beta2) {
  const float gr = g + l2_weight * w;
  BcMoments o;
  o.m = m0 + (gr - m0) * (1.0f - beta1);           // exp_avg.lerp_(grad, 1 - beta1)
  o.v = v0 * beta2 + (1.0f - beta2) * gr * gr;     // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
  return o;
}

// param.addcdiv_(exp_avg, denom, -step_size), denom = sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps, step_size = bcorr[0].  There are two
// on purpose.  bc_train_kernel takes torch's update as written, IEEE divisions and square root.  In bc_train_mfma_kernel the products
// are short enough that the Adam loop was the longest phase of a step, and the IEEE sequences cost ~60 instructions per parameter
// there: it takes the two divisions and the square root on the hardware's 1-ulp v_rcp_f32 / v_sqrt_f32, with 1 / sqrt(1 - beta2^t)
// computed once per step (inv_bc2s = __builtin_amdgcn_rcpf(bcorr[1])).  The resulting last-bit differences are far inside what
// 1e-3-sized Adam steps do to a near-zero gradient entry anyway; both forms are held to the checker by the same tests.
__device__ __forceinline__ float bc_adam_param_ieee(float w, float m, float v, float step_size, float bc2s, float eps) {
  return w - step_size * (m / (sqrtf(v) / bc2s + eps));
}
__device__ __forceinline__ float bc_adam_param_fast(float w, float m, float v, float step_size, float inv_bc2s, float eps) {
  return w - step_size * m * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) * inv_bc2s + eps);
}

}  // namespace ph
