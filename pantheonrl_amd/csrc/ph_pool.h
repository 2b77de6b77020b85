// Liar's Dice against a pool of partners: the device-side member table, the bucket pass and the grouped forward's launch record,
// and seat 1's book of the pool step (ph_liar_step.h's after_ego / after_reply / after_opening with the member index).
// Kernels: ph_pool.hip (bucket pass, scripted rule), ph_envs.hip (the step's book-keeping) and ph_policy.hip (pool_fwd16h_kernel: the grouped forward is the
// 16-row one-hot forward with its rows gathered through `order`, so it lives beside policy_fwd16h_body).  A PH_POOL_CLONE member
// (the shared-trunk FeedForward32Policy, params in ph_bc_layout) is a non-learner like a frozen one -- PoolBook below asks for
// `kind == PH_POOL_LEARNER` only -- and its tile of the grouped forward is ph_bc_row.h's bc_clone_tile.  A learner or frozen member
// whose `tower` flag is set plays an MLP tower of that run-time shape (ph_arch.h): its tiles are pool_tower_kernel's (ph_arch.hip).
// A frozen member whose `adap_C` is set plays an AdapPolicy checkpoint (adap/policies.py:21-146; seated by the reference as
// FIXED '{"type":"ADAP",...,"latent_val":[...]}', trainer.py:140-147, set_context): the 64-64 MLP over one_hot(observation) ++ the
// table's context, its tiles pool_adap_kernel's (ph_policy.hip).
#pragma once
#include "ph_liar_step.h"
#include "ph_arch.h"

namespace ph {

// a member as the kernels read it -- from DEVICE memory (the context keeps the table): a by-value array inside the kernel
// arguments, indexed by the tile's member, would put the whole argument block into scratch memory (see ph_arch.h, ph_launch.h)
struct PoolMemberDev {
  int fwd;           // what pool_fwd16h_kernel asks, in ONE word: the member's kind, but PH_POOL_CLONE ("another kernel's tile") for a tower
  int kind;          // PH_POOL_*: what the step's book asks (PoolBook), and the other tile kernels
  int rb_T;
  int tower;         // != 0: `ad` below describes the member's towers; its tiles are pool_tower_kernel's
  const float* params;
  float *rb_obs, *rb_act, *rb_rew, *rb_es, *rb_val, *rb_logp;   // array bases of the ragged buffer (learner), else null
  int* pos;
  unsigned char *boundary, *term, *open;
  float *values, *log_probs;
  unsigned long long seed;
  ArchDims ad;   // a tower member's (learner or frozen); read from this table on the device, never from a kernel argument
  // an ADAP member's (frozen): context size (0: no ADAP member), its (n, C) contexts and the layout of its Box(F + C) parameters;
  // read from this table on the device like `ad`.  `fwd` states it as PH_POOL_CLONE too.
  int adap_C;
  const float* adap_ctx;
  ph_layout adap_lay;
};
// (pool_fwd16h_kernel is held to the text it had without towers: a tower flag that it reads beside `kind` is a second load behind the
// branch on `kind`, a dependent round trip to L2 in front of every tile -- 1.1 us per cross-play step of a population without a tower,
// measured -- and a flag folded into the kind's word with a compare of its own still measured 0.4 us per step)

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
  ph_bc_layout bc;                  // the spec's shared-trunk layout: what a PH_POOL_CLONE member's params are (P = 0: no clone in the table)
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

// Seat 1's book of the pool step (ph_liar_step.h): table e's lane binds the member that holds (or, behind a deal, is about to hold)
// seat 1 of table e, so a member's flags of table e are touched by that lane only.  A learner keeps LearnerBook's cursor; members
// without a buffer record nothing (can = 0) and only mark the seat as having acted.  The index is device data: clamped.
struct PoolBook {
  int n, K, resample;
  unsigned long long pool_seed;
  const PoolMemberDev* members;     // device
  int* partnerid;
  unsigned char *alt_acted, *can;
  float* es_alt;
  struct Lane {
    int k;
    bool learner;
    LearnerBook m;
    LearnerBook::Lane s;
  };
  // the member at b.k: a learner's cursor addresses (members[] is device memory: a dependent load behind partnerid)
  __device__ __forceinline__ void bind(Lane& b) const {
    const PoolMemberDev m = members[b.k];
    b.learner = m.kind == PH_POOL_LEARNER;
    b.m = LearnerBook{SeatFields{n, m.pos, m.boundary, m.term, m.open, alt_acted, can, es_alt}, m.rb_rew, m.rb_T};
    b.s.q = LiarSeat{0, false, false, false};
  }
  __device__ __forceinline__ Lane seat(int e) const {
    Lane b;
    const int k = partnerid[e];
    b.k = k < 0 ? 0 : (k >= K ? K - 1 : k);
    b.s.can = can[e] != 0;
    bind(b);
    return b;
  }
  __device__ __forceinline__ void cursor(Lane& b, int e) const {   // a third dependent load
    if (b.learner) b.s.q = liar_seat_load(b.m.v, e);
  }
  __device__ __forceinline__ Lane load(int e) const {
    Lane b = seat(e);
    cursor(b, e);
    return b;
  }
  __device__ __forceinline__ bool acted(const Lane& b) const { return b.s.q.acted; }
  __device__ __forceinline__ void credit(Lane& b, int e, float r, bool done, bool credited) const {
    if (b.learner) b.m.credit(b.s, e, r, done, credited);
  }
  __device__ __forceinline__ void commit(Lane& b, int e) const {
    if (b.learner) b.m.commit(b.s, e);
    else alt_acted[e] = 1;
  }
  __device__ __forceinline__ void prepare(const Lane& b, int e, bool requested) const {
    if (b.learner) {
      b.m.prepare(b.s, e, requested);
    } else {
      can[e] = 0;
      es_alt[e] = 0.f;
    }
  }
  // the member that sits at the new game: its cursor of this table is what the opening forward records at
  __device__ __forceinline__ void on_deal(Lane& b, int e, uint64_t c) const {
    alt_acted[e] = 0;
    b.k = pool_resample(b.k, K, resample, pool_seed, c, e);
    partnerid[e] = b.k;
    bind(b);
    cursor(b, e);
  }
};

hipError_t launch_pool_bucket(const int* partnerid, const unsigned char* active, int n, int K, const PoolBuckets& b, hipStream_t s);
// ph_policy.hip; p.bc.P != 0: the member table holds a clone (its tiles' kernel follows); tower_lds != 0: it holds a tower (the
// largest arch_fwd_lds_bytes over its tower members; pool_tower_kernel follows); no_wide: it holds neither a 64-wide nor a scripted
// member (no 64-64 launch); adap: it holds an ADAP member (pool_adap_kernel follows, last)
hipError_t launch_pool_fwd(const PoolFwd& p, int K, hipStream_t s, bool no_wide = false, size_t tower_lds = 0, bool adap = false);
// ph_arch.hip: the tower tiles of the bucket pass (lds: the launch's dynamic LDS, at least every tower member's carve)
hipError_t launch_pool_tower(const PoolFwd& p, int K, size_t lds, hipStream_t s);
bool pool_fwd_eligible(const NetDims& nd, int n);                     // ph_policy.hip
bool pool_clone_eligible(const NetDims& nd, const ph_bc_layout& lay); // ph_policy.hip: the clone tile's shapes and LDS inside the grouped launch
// ph_policy.hip: the grouped forward for any categorical spec of 32 padded logits (the block worlds' cross-play): the frozen members'
// tiles, on the body launch_policy_fwd picks for the spec.  p.bc is not read; a scripted member's `rb_T` word holds its rule, for
// launch_block_group_scripted (ph_block.h).
bool group_fwd_eligible(const NetDims& nd, int n);
hipError_t launch_group_fwd(const PoolFwd& p, int K, hipStream_t s);
// ph_policy.hip: the same launch for a constructor table that holds a learner (the block worlds' partner pool): grid (tiles, 2), the
// learners' tiles recorded through p.a.rec_mask / p.a.es_in into their ragged buffers, the frozen members' tiles as above.  On the
// 16-row one-hot body only.
bool group_learn_eligible(const NetDims& nd, int n);
hipError_t launch_group_learn(const PoolFwd& p, int K, hipStream_t s);
hipError_t launch_liar_default_actions(const float* obs, const unsigned char* active, int* actions, int n, hipStream_t s);

}  // namespace ph
