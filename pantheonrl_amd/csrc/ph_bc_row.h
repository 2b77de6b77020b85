// The row arithmetic of the shared-trunk FeedForward32Policy forward, written once: bc_forward_kernel (ph_bc.hip: one lane per
// row, the parameters in LDS) and the clone tile of the pool's grouped forward (bc_clone_tile below, run by pool_clone16_kernel in
// ph_policy.hip: 16 rows spread over 256 lanes) are built from the functions of this file, so a row's logits and its sampled action
// are the same bits in both -- the pattern of ph_ppo_loss.h and ph_liar_step.h.  What fixes the bits of an output is its own
// summation order, not the lane that computes it:
//   h1[j]     starts at b1[j] and adds W1[lo + x][j] for the observation components in ascending order, x clamped into the
//             component (bc_hot_feature, bc_h1_add);
//   h2[j], logit c, value   one fmaf per k in ascending k on top of the bias (bc_chain);
//   the tail  max and first arg-max over the component's logits, lse = max + log(sum exp(z - max)), then the running CDF of
//             exp(z - lse) against u with `u < cdf` and the fall-through to the last class (bc_max_step, bc_lse, bc_sample_cdf);
//   u         philox_uniform(seed, counter, row, component), row = the row's index in the call (bc_forward_kernel) = the table
//             (clone tile).
#pragma once
#include "ph_device.h"

namespace ph {

constexpr int BH = PH_BC_HIDDEN;       // hidden width of the shared trunk

__device__ __forceinline__ float bc_tanh(float x) { return fast_tanh(x); }

// the row of W1 that component `comp` of a one-hot observation row selects: lo + x, x clamped into the component's range
__device__ __forceinline__ int bc_hot_feature(int lo, int n, float value) {
  int x = (int)value;
  x = x < 0 ? 0 : (x >= n ? n - 1 : x);
  return lo + x;
}
__device__ __forceinline__ int bc_hot_feature(const int* obs_off, const float* obs_row, int comp) {
  const int lo = obs_off[comp];
  return bc_hot_feature(lo, obs_off[comp + 1] - lo, obs_row[comp]);
}
// one term of a one-hot row's layer 1 (the dense layer's k-ordered sum with the zero terms left out): callers add in component order
__device__ __forceinline__ float bc_h1_add(float acc, float w) { return acc + w; }

// bias + sum_k h(k) w(k): one fmaf per k, ascending -- a hidden unit of layer 2, a logit, the value
template <class H, class W>
__device__ __forceinline__ float bc_chain(float bias, H h, W w) {
  float s = bias;
#pragma unroll
  for (int k = 0; k < BH; ++k) s = __builtin_fmaf(h(k), w(k), s);
  return s;
}

// the running max of a component's logits and the first class that reaches it
__device__ __forceinline__ void bc_max_step(float s, int c, float& mx, int& arg) {
  if (s > mx) {
    mx = s;
    arg = c;
  }
}
constexpr float BC_MAX_INIT = -3.0e38f;

// log-sum-exp of the n logits z(0 .. n) under their max
template <class Z>
__device__ __forceinline__ float bc_lse(Z z, int n, float mx) {
  float se = 0.f;
  for (int c = 0; c < n; ++c) se += __expf(z(c) - mx);
  return mx + __logf(se);
}

// entropy of the component: -sum_c p_c log p_c, log p_c = z(c) - lse
template <class Z>
__device__ __forceinline__ float bc_entropy(Z z, int n, float lse) {
  float h = 0.f;
  for (int c = 0; c < n; ++c) {
    const float lq = z(c) - lse;
    h -= __expf(lq) * lq;
  }
  return h;
}

// the class a uniform u selects: the first c with u < cdf(c), cdf the running sum of exp(z - lse); the last class otherwise
template <class Z>
__device__ __forceinline__ int bc_sample_cdf(Z z, int n, float lse, float u) {
  float cdf = 0.f;
  for (int c = 0; c < n; ++c) {
    cdf += __expf(z(c) - lse);
    if (u < cdf) return c;
  }
  return n - 1;
}

// ---- the clone tile of the pool's grouped forward (ph_pool.h: PH_POOL_CLONE) -----------------------------------------------------
// One workgroup of 256 lanes runs the rows g = map[0 .. rows), rows <= 16, of one member whose `params` is a ph_bc_layout vector of
// the Liar's Dice spec, and stores each row's sampled action as one int2 at act_i32 + 2 g.  Nothing else is written; lanes that own
// no row read neither `map` nor `obs`.  The parameter vector is not staged (41.5 KB for 16 rows): W2, the biases and the head
// (P - F * 32 floats, about 1.7 k) go to LDS, and a row's D hot rows of W1 are gathered from global memory by the lanes that sum them.
//   phase 0   every lane: the small parameters, loaded first and all at once; lane (row r = tid / 32 and r + 8, component tid % 32):
//             table -> observation -> the hot feature of (row, component) -> LDS; then the small parameters -> LDS
//   phase 1   lane (unit j = tid % 32, rows r and r + 8): the D loads W1[feature][j] of both rows issued back to back, then the
//             in-order adds; tanh -> h1 in LDS
//   phase 2   the same lanes: h2[r][j] by bc_chain over h1[r][.] (an LDS broadcast) and W2[.][j]; tanh -> h2 in LDS
//   phase 3   lane (logit c = tid % 32 < L, rows r and r + 8): bc_chain -> logits in LDS
//   phase 4   lane r < rows: the serial tail of the row's action components (its two uniforms drawn in phase 1, under the gathers)
// smem: bc_clone_lds_floats(P - b1) floats of dynamic LDS, 15.4 KB for Liar's Dice (it also fits inside the grouped launch's fwd16h_lds_bytes()).
constexpr int BC_CLONE_ROWS = 16, BC_CLONE_LDZ = 33, BC_CLONE_MAXD = 32, BC_CLONE_MAXL = 32;
// passes of 256 lanes over the parameters behind W1: b1, W2, b2, act_W (32 x L, L <= 32), act_b, val_W, val_b
constexpr int BC_CLONE_SMALL_MAX = BH + BH * BH + BH + BH * BC_CLONE_MAXL + BC_CLONE_MAXL + BH + 1;
constexpr int BC_CLONE_SMALL_PASSES = (BC_CLONE_SMALL_MAX + 255) / 256;
__host__ __device__ constexpr int bc_clone_lds_floats(int small) {
  return BC_CLONE_ROWS * (BC_CLONE_MAXD + 3 * BC_CLONE_LDZ) + small;
}
// the shapes the tile is written for (checked on the host before the launch): one-hot, D <= 32 components, L <= 32 logits
__host__ __device__ inline bool bc_clone_eligible(int obs_kind, int D, int L) {
  return obs_kind != PH_SPACE_BOX && D >= 1 && D <= BC_CLONE_MAXD && L >= 1 && L <= BC_CLONE_MAXL;   // (so P - b1 <= BC_CLONE_SMALL_MAX)
}

// the tile's arguments as scalars, by value (26 dwords: registers, should a caller not inline the tile -- a reference to a kernel's
// argument record would put the record into scratch memory then)
struct BcCloneArgs {
  const int *obs_off, *act_off;   // device: prefix sums of the observation / action nvec
  const float* W1;                // params + lay.W1
  const float* small;             // params + lay.b1: b1, W2, b2, act_W, act_b, val_W, val_b, contiguous behind W1
  const float* obs;               // (n, D)
  const int* map;                 // the tile's tables
  int* act_i32;                   // (n, 2)
  uint64_t seed, counter;
  int D, L, rows, nsmall;         // nsmall = lay.P - lay.b1
  int W2, b2, act_W, act_b;       // offsets from `small`
};
__device__ __forceinline__ BcCloneArgs bc_clone_args(const NetDims& nd, const ph_bc_layout& lay, const float* params, const float* obs,
                                                     const int* map, int rows, uint64_t seed, uint64_t counter, int* act_i32) {
  return BcCloneArgs{nd.obs_off, nd.act_off, params + lay.W1, params + lay.b1, obs, map, act_i32, seed, counter, nd.D, nd.L, rows,
                     lay.P - lay.b1, lay.W2 - lay.b1, lay.b2 - lay.b1, lay.act_W - lay.b1, lay.act_b - lay.b1};
}

__device__ __forceinline__ void bc_clone_tile(const BcCloneArgs a, float* smem) {
  constexpr int R = BC_CLONE_ROWS, LDZ = BC_CLONE_LDZ, MD = BC_CLONE_MAXD;
  const int tid = threadIdx.x, j = tid & 31, r0 = tid >> 5;   // rows r0 and r0 + 8
  const int D = a.D, L = a.L, small = a.nsmall, rows = a.rows;
  const int* __restrict__ map = a.map;
  const float* __restrict__ obs = a.obs;
  int* feat = (int*)smem;                  // [16][32] hot feature per (row, component)
  float* h1s = smem + R * MD;              // [16][33]
  float* h2s = h1s + R * LDZ;              // [16][33]
  float* zs = h2s + R * LDZ;               // [16][33] logits
  float* ps = zs + R * LDZ;                // the parameters behind W1; ps[i] = a.small[i]
  auto par = [&](int off) -> const float* { return ps + off; };

  // ---- phase 0 ----
  // A kernel starts with cold caches and every dependent round trip costs about a microsecond at this occupancy, so the loads that
  // depend on nothing go out first and back to back: the small parameters (all BC_CLONE_SMALL_PASSES passes into registers,
  // unconditional loads at clamped positions -- a load -> LDS store loop would be one round trip per pass) and the component's
  // bounds.  Then the chain tables -> observations, both rows of a lane inside ONE block (a lane whose second row does not exist
  // reads its first row again; a lane with no row reads neither `map` nor `obs`).
  float sp[BC_CLONE_SMALL_PASSES];
#pragma unroll
  for (int i = 0; i < BC_CLONE_SMALL_PASSES; ++i) {
    const int p = tid + 256 * i;
    sp[i] = a.small[p < small ? p : small - 1];
  }
  const int jc = j < D ? j : D - 1;
  const int lo = a.obs_off[jc], hi = a.obs_off[jc + 1];
  int g_own = 0;                                 // the table of the row this lane finishes in phase 4
  if (tid < rows) g_own = map[tid];
  int fa = 0, fb = 0;   // feature 0 where there is no row or no such component: phase 1 gathers every position without a test
  if (r0 < rows && j < D) {
    const bool two = r0 + 8 < rows;
    const int ga = map[r0], gb = map[two ? r0 + 8 : r0];
    const float xa = obs[(size_t)ga * D + j], xb = obs[(size_t)gb * D + j];
    fa = bc_hot_feature(lo, hi - lo, xa);
    fb = two ? bc_hot_feature(lo, hi - lo, xb) : 0;
  }
  feat[r0 * MD + j] = fa;
  feat[(r0 + 8) * MD + j] = fb;
#pragma unroll
  for (int i = 0; i < BC_CLONE_SMALL_PASSES; ++i) {
    const int p = tid + 256 * i;
    if (p < small) ps[p] = sp[i];
  }
  __syncthreads();

  // ---- phase 1: layer 1, unit j of rows r0 and r0 + 8 ----
  float u_tail[2] = {0.f, 0.f};
  {
    const float* __restrict__ W1 = a.W1;   // workgroup-uniform base + one 32-bit offset per load (a 64-bit address each would double the registers)
    float w[2][MD];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r = r0 + 8 * t;
      // unconditional loads (feature 0 where the lane has no row or the observation no such component, written so in phase 0): a
      // load under `if` is a basic block of its own, and the loads of a lane would then go out one behind the other's wait
#pragma unroll
      for (int c = 0; c < MD; ++c) w[t][c] = W1[(unsigned)(feat[r * MD + c] * BH + j)];
    }
    if (tid < rows) {   // the tail's uniforms, under the gathers' latency
      u_tail[0] = philox_uniform(a.seed, a.counter, (uint32_t)g_own, 0u);
      u_tail[1] = philox_uniform(a.seed, a.counter, (uint32_t)g_own, 1u);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r = r0 + 8 * t;
      if (r < rows) {
        float acc = par(0)[j];
#pragma unroll
        for (int c = 0; c < MD; ++c) acc = c < D ? bc_h1_add(acc, w[t][c]) : acc;
        h1s[r * LDZ + j] = bc_tanh(acc);
      }
    }
  }
  __syncthreads();

  // ---- phase 2: layer 2 ----
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = r0 + 8 * t;
    if (r < rows) {
      const float* h = h1s + r * LDZ;
      const float* w = par(a.W2) + j;
      h2s[r * LDZ + j] = bc_tanh(bc_chain(par(a.b2)[j], [&](int k) { return h[k]; }, [&](int k) { return w[k * BH]; }));
    }
  }
  __syncthreads();

  // ---- phase 3: logits ----
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = r0 + 8 * t;
    if (r < rows && j < L) {
      const float* h = h2s + r * LDZ;
      const float* w = par(a.act_W) + j;
      zs[r * LDZ + j] = bc_chain(par(a.act_b)[j], [&](int k) { return h[k]; }, [&](int k) { return w[k * L]; });
    }
  }
  __syncthreads();

  // ---- phase 4: one lane per row ----
  if (tid < rows) {
    int act[2] = {0, 0};
    for (int comp = 0; comp < 2; ++comp) {   // the pool's spec has two action components (pool_fwd_eligible)
      const int lo = a.act_off[comp], n = a.act_off[comp + 1] - lo;
      const float* zr = zs + tid * LDZ + lo;
      auto z = [&](int c) { return zr[c]; };
      float mx = BC_MAX_INIT;
      int arg = 0;
      for (int c = 0; c < n; ++c) bc_max_step(z(c), c, mx, arg);
      const float lse = bc_lse(z, n, mx);
      const int pick = bc_sample_cdf(z, n, lse, comp == 0 ? u_tail[0] : u_tail[1]);
      if (comp == 0) act[0] = pick;
      else act[1] = pick;
    }
    *reinterpret_cast<int2*>(a.act_i32 + 2 * (size_t)g_own) = make_int2(act[0], act[1]);
  }
}

}  // namespace ph
