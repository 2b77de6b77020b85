// Liar's Dice against a pool of partners: the device-side member table, the bucket pass and the grouped forward's launch record,
// and the per-table book-keeping of the pool step (ph_liar.h's after_ego / after_reply / after_opening with the member index).
// Kernels: ph_pool.hip (bucket pass, scripted rule, book-keeping) and ph_policy.hip (pool_fwd16h_kernel: the grouped forward is the
// 16-row one-hot forward with its rows gathered through `order`, so it lives beside policy_fwd16h_body).
#pragma once
#include "ph_liar.h"

namespace ph {

// a member as the kernels read it -- from DEVICE memory (the context keeps the table): a by-value array inside the kernel
// arguments, indexed by the tile's member, would put the whole argument block into scratch memory (see ph_arch.h, ph_launch.h)
struct PoolMemberDev {
  int kind, rb_T;
  const float* params;
  float *rb_obs, *rb_act, *rb_rew, *rb_es, *rb_val, *rb_logp;   // array bases of the ragged buffer (learner), else null
  int* pos;
  unsigned char *boundary, *term, *open;
  float *values, *log_probs;
  unsigned long long seed;
};

constexpr int POOL_TILE = 16;            // rows of one tile = rows of the 16-row forward
constexpr int POOL_BUCKET_THREADS = 256;
// tiles a launch must provide workgroups for: sum over members of ceil(count_k / 16) <= n / 16 + K
inline int pool_max_tiles(int n, int K) { return n / POOL_TILE + K; }

// the bucket pass's outputs: order[i] = table of sorted position i (tables of member 0 first, each member's in table order);
// tiles[3 t ..] = (member, first position, rows) of tile t; ntiles[0] = tiles in use
struct PoolBuckets {
  int* order;
  int* tiles;
  int* ntiles;
};
struct PoolFwd {
  FwdArgs a;                        // the shared part: spec, obs, n, counter, epoch, act_i32, es_in, rec_mask; the member's part is patched in
  const PoolMemberDev* members;     // device
  PoolBuckets b;
};

// the pool step's description as the book-keeping kernels take it
struct PoolStep {
  int n, K, resample;
  int *hands, *history, *nmoves;
  unsigned char* ego_first;
  unsigned long long dice_seed, pool_seed;
  float probegostart;
  const int* ego_actions;
  float* ego_episode_start;
  const PoolMemberDev* members;     // device
  int* partnerid;
  const int* alt_actions;
  unsigned char* alt_acted;
  float *obs_ego, *obs_alt;
  unsigned long long* episodes;
  float *obs_next, *rew1, *rew2, *es_alt;
  unsigned char *done1, *done2, *running, *can, *alt_opens, *ego_opens, *done;
};

// LiarDefaultAgent.get_action (envs/liar.py): bid the most frequent face (the first of equals) at its own count; call as soon as
// the standing bid exceeds that count.  o = the row's 30 observation components.
__device__ __forceinline__ int2 liar_default_move(const float* o) {
  int best = (int)o[0], side = 0;
#pragma unroll
  for (int k = 1; k < LD_SIDES; ++k) {
    const int h = (int)o[k];
    if (h > best) { best = h; side = k; }
  }
  const int last_side = (int)o[LD_SIDES], last_count = (int)o[LD_SIDES + 1];
  if (last_side != LD_SIDES && last_count > best) return make_int2(LD_SIDES, 2 * LD_DICE - 1);
  return make_int2(side, best);
}

// the resample rule at a deal of table e (the caller stores the result)
__device__ __forceinline__ int pool_resample(int prev, int K, int rule, unsigned long long seed, uint64_t counter, int e) {
  if (rule == PH_POOL_RANDOM) {
    uint32_t c[4] = {(uint32_t)e, 101u, (uint32_t)counter, (uint32_t)(counter >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (int)(((uint64_t)c[0] * (uint64_t)K) >> 32);
  }
  return (prev + 1) % K;
}

hipError_t launch_pool_bucket(const int* partnerid, const unsigned char* active, int n, int K, const PoolBuckets& b, hipStream_t s);
hipError_t launch_pool_fwd(const PoolFwd& p, int K, hipStream_t s);   // ph_policy.hip
bool pool_fwd_eligible(const NetDims& nd, int n);                     // ph_policy.hip
hipError_t launch_liar_default_actions(const float* obs, const unsigned char* active, int* actions, int n, hipStream_t s);
hipError_t launch_pool_after_ego(const PoolStep& s, hipStream_t st);
hipError_t launch_pool_after_reply(const PoolStep& s, float* ego_rew_row, unsigned long long counter, const unsigned long long* epoch,
                                   int deal_only, hipStream_t st);
hipError_t launch_pool_after_opening(const PoolStep& s, hipStream_t st);

}  // namespace ph
