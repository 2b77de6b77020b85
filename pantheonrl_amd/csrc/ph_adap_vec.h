// ADAP in the device-resident games: the two rules an AdapPolicy seat adds to a vectorised step, as __host__ __device__ functions of
// one table -- what the kernels run with one lane per row element / per table (ph_adap_vec.hip) and what ph_adap_vec_host runs on
// the CPU (ph_abi.hip): one text, so the rules are pinned to a numpy statement where there is no GPU.
//
//   row build     a raw observation of D components -> F + C floats: SB3's one-hot features in component order (preprocess_obs +
//                 FlattenExtractor; a component outside [0, nvec_i) is clamped, as AdapPolicy.features clamps it) or a Box's values
//                 unchanged, then the table's context (adap/policies.py:104-119).
//   context draw  the five samplers of adap/util.py:42-89 over philox_uniform(key, counter, table, component), in the arithmetic of
//                 the loss term's in-kernel sampler (ph_adap.hip): u * 2 - 1 onto [-1, 1), sqrtf then divide for "l2", the >= cs clamp
//                 of the integer draws.  key = the learner's policy seed ^ ADAP_VEC_SALT: another key than the policy's own (its action
//                 components), than the loss term's (seed ^ 0xADA9C0DE, then epoch_key) and than the pool's (dice seed ^ its salt), so
//                 no draw shares (key, block, counter) with another stream.  counter = the step counter + (RNG epoch word << 32), as
//                 the dice combine them (liar_after_reply_lane).  The sum of squares is formed without contraction so that the host,
//                 the device and a numpy statement round alike.
#pragma once
#include "ph_launch.h"

namespace ph {

constexpr uint64_t ADAP_VEC_SALT = 0xC0A7E87D5A17ADA9ull;
constexpr int ADAP_VEC_MAX_CONTEXT = 64;   // a context is part of a Box row; the stream map reserves this many components

// the row's shape, by value in the launch: prefix sums of the environment space's nvec (one-hot) or nothing (Box)
struct AdapRowShape {
  int D, F, C;   // stored observation length, features, context size; a row is F + C floats
  int box;       // 1: the observation is a Box, features = its D values
  int off[PH_MAX_COMP + 1];
};

// element f of the row of one table; off = the shape's prefix sums (wherever the caller keeps them)
__host__ __device__ inline float adap_row_value(const AdapRowShape& s, const int* off, const float* obs_row, const float* ctx_row, int f) {
  if (f >= s.F) return ctx_row[f - s.F];
  if (s.box) return obs_row[f];
  int lo = 0, hi = s.D - 1;   // the component whose features hold f: the last one with off[comp] <= f
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= f) lo = mid;
    else hi = mid - 1;
  }
  const int base = off[lo], nv = off[lo + 1] - base;
  int v = (int)obs_row[lo];
  v = v < 0 ? 0 : (v >= nv ? nv - 1 : v);
  return f - base == v ? 1.f : 0.f;
}

__host__ __device__ inline uint64_t adap_vec_counter(uint64_t counter, const unsigned long long* epoch) {
  return counter + (epoch ? (uint64_t)(*epoch) << 32 : 0ull);
}

// one table's context; c holds cs floats
__host__ __device__ inline void adap_draw_context(int sampler, int cs, uint64_t seed, uint64_t counter, uint32_t table, float* c) {
  const uint64_t key = seed ^ ADAP_VEC_SALT;
  if (sampler == PH_CTX_NATURAL_NUMBERS || sampler == PH_CTX_CATEGORICAL) {
    int v = (int)(philox_uniform(key, counter, table, 0u) * (float)cs);
    v = v >= cs ? cs - 1 : v;
    for (int k = 0; k < cs; ++k)
      c[k] = sampler == PH_CTX_CATEGORICAL ? (k == v ? 1.f : 0.f) : (k == 0 ? (float)v : 0.f);
    return;
  }
  float ss = 0.f;
  for (int k = 0; k < cs; ++k) {
    const float u = philox_uniform(key, counter, table, (uint32_t)k);
    const float v = sampler == PH_CTX_POSITIVE_SQUARE ? u : u * 2.f - 1.f;
    c[k] = v;
    {
#pragma clang fp contract(off)
      const float sq = v * v;
      ss = ss + sq;
    }
  }
  if (sampler == PH_CTX_L2) {
    const float nrm = sqrtf(ss);
    for (int k = 0; k < cs; ++k) {   // the draw again, not the store read back
      const float u = philox_uniform(key, counter, table, (uint32_t)k);
      c[k] = (u * 2.f - 1.f) / nrm;
    }
  }
}

// rows (n, F + C) <- obs (n, D) ++ contexts (n, C) where active (null: everywhere); one lane per row element
hipError_t launch_adap_rows(const AdapRowShape& shape, const float* obs, const float* contexts, const unsigned char* active, float* rows,
                            int n, hipStream_t st);
// contexts (n, C) <- a draw at `counter` (+ the epoch word's high half) where redraw or redraw2 (both null: everywhere); one lane
// per table
hipError_t launch_adap_context_draw(int sampler, int cs, unsigned long long seed, unsigned long long counter,
                                    const unsigned long long* epoch, const unsigned char* redraw, float* contexts, int n, hipStream_t st,
                                    const unsigned char* redraw2 = nullptr);

}  // namespace ph
