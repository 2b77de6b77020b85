// Liar's Dice against a pool of partners (ph_pool.h): the bucket pass in front of the grouped forward, the scripted member's rule
// and the three book-keeping launches of the pool step.  The grouped forward itself is pool_fwd16h_kernel in ph_policy.hip.
#include "ph_pool.h"

namespace ph {

// ---- bucket pass: a stable counting sort of the active tables by member, integer prefix sums only -----------------------------
// ONE workgroup.  Lane t owns the contiguous tables [t * seg, (t + 1) * seg): it counts them per member, lanes 0..K-1 turn the
// counts of their member into exclusive prefixes over the lanes, and every lane writes its tables behind its prefix -- tables of
// one member keep their order.  The tile table is cut from the member totals by lane 0.
__global__ __launch_bounds__(POOL_BUCKET_THREADS) void pool_bucket_kernel(const int* __restrict__ partnerid,
                                                                          const unsigned char* __restrict__ active, int n, int K,
                                                                          PoolBuckets b) {
  __shared__ int cnt[POOL_BUCKET_THREADS][PH_MAX_POOL + 1];   // (+1: lanes of a wave on different banks)
  __shared__ int base[PH_MAX_POOL + 1];
  const int t = threadIdx.x;
  const int seg = (n + POOL_BUCKET_THREADS - 1) / POOL_BUCKET_THREADS;
  const int lo = t * seg < n ? t * seg : n, hi = lo + seg < n ? lo + seg : n;
#pragma unroll
  for (int k = 0; k < PH_MAX_POOL; ++k) cnt[t][k] = 0;
  for (int e = lo; e < hi; ++e) {
    const int k = partnerid[e];
    if (active[e] && k >= 0 && k < K) cnt[t][k] += 1;
  }
  __syncthreads();
  if (t < K) {
    int run = 0;
    for (int i = 0; i < POOL_BUCKET_THREADS; ++i) {
      const int c = cnt[i][t];
      cnt[i][t] = run;
      run += c;
    }
    base[t] = run;   // member total, turned into the member's first position below
  }
  __syncthreads();
  if (t == 0) {
    int first = 0, nt = 0;
    for (int k = 0; k < K; ++k) {
      const int c = base[k];
      base[k] = first;
      for (int r = 0; r < c; r += POOL_TILE) {
        b.tiles[3 * nt] = k;
        b.tiles[3 * nt + 1] = first + r;
        b.tiles[3 * nt + 2] = c - r < POOL_TILE ? c - r : POOL_TILE;
        ++nt;
      }
      first += c;
    }
    b.ntiles[0] = nt;
  }
  __syncthreads();
  for (int e = lo; e < hi; ++e) {
    const int k = partnerid[e];
    if (active[e] && k >= 0 && k < K) {
      b.order[base[k] + cnt[t][k]] = e;
      cnt[t][k] += 1;
    }
  }
}
hipError_t launch_pool_bucket(const int* partnerid, const unsigned char* active, int n, int K, const PoolBuckets& b, hipStream_t s) {
  hipLaunchKernelGGL(pool_bucket_kernel, dim3(1), dim3(POOL_BUCKET_THREADS), 0, s, partnerid, active, n, K, b);
  return hipGetLastError();
}

// ---- the scripted member on its own -----------------------------------------------------------------------------------------
__global__ void liar_default_actions_kernel(const float* __restrict__ obs, const unsigned char* __restrict__ active,
                                            int* __restrict__ actions, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n || (active && !active[e])) return;
  *reinterpret_cast<int2*>(actions + 2 * (size_t)e) = liar_default_move(obs + (size_t)e * 30);
}
hipError_t launch_liar_default_actions(const float* obs, const unsigned char* active, int* actions, int n, hipStream_t s) {
  hipLaunchKernelGGL(liar_default_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, s, obs, active, actions, n);
  return hipGetLastError();
}

// ---- book-keeping of the pool step, one lane per table ------------------------------------------------------------------------
// The partner-seat fields ph_liar.h's helpers work on, bound to ONE member: table e's lane binds the member that holds (or is about
// to hold) seat 1 of table e, so a member's flags of table e are touched by that lane only.
struct PoolSeat {
  int n;
  int* alt_pos;
  unsigned char *alt_boundary, *alt_term, *alt_open, *alt_acted, *can;
  float* es_alt;
};
__device__ __forceinline__ PoolSeat pool_seat(const PoolStep& s, const PoolMemberDev& m) {
  return PoolSeat{s.n, m.pos, m.boundary, m.term, m.open, s.alt_acted, s.can, s.es_alt};
}
// the member of table e (clamped: the index is device data)
__device__ __forceinline__ int pool_member_of(const PoolStep& s, int e) {
  const int k = s.partnerid[e];
  return k < 0 ? 0 : (k >= s.K ? s.K - 1 : k);
}
// what the member's next forward records in table e; members without a buffer record nothing
__device__ __forceinline__ void pool_prepare(const PoolStep& s, const PoolMemberDev& m, int e, bool requested) {
  if (m.kind == PH_POOL_LEARNER) {
    const PoolSeat v = pool_seat(s, m);
    const LiarSeat q = liar_seat_load(v, e);
    liar_sp_prepare(v, q, m.rb_T, e, requested);
  } else {
    s.can[e] = 0;
    s.es_alt[e] = 0.f;
  }
}

__global__ void pool_after_ego_kernel(PoolStep s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  const PoolMemberDev m = s.members[pool_member_of(s, e)];
  LiarTable t;
  liar_load(t, e, s.hands, s.history, s.nmoves);
  const LiarOutcome o1 = liar_move(t, e, s.history, s.nmoves, s.ego_actions, true, s.obs_next, s.rew1, s.done1);
  s.running[e] = o1.done ? 0 : 1;
  if (m.kind == PH_POOL_LEARNER) {
    const PoolSeat v = pool_seat(s, m);
    LiarSeat q = liar_seat_load(v, e);
    liar_sp_credit(v, q, m.rb_rew, m.rb_T, e, o1.r_alt, o1.done, q.acted);
    liar_sp_prepare(v, q, m.rb_T, e, !o1.done);
  } else {
    s.can[e] = 0;
    s.es_alt[e] = 0.f;
  }
}

__global__ void pool_after_reply_kernel(PoolStep s, float* ego_rew_row, uint64_t counter, const unsigned long long* __restrict__ epoch,
                                        int deal_only) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  int k = pool_member_of(s, e);
  LiarTable t;
  liar_load(t, e, s.hands, s.history, s.nmoves);
  bool ego_first = s.ego_first[e] != 0;
  bool fresh = s.done[e] != 0;
  if (!deal_only) {
    const PoolMemberDev m = s.members[k];
    const bool learner = m.kind == PH_POOL_LEARNER;
    const PoolSeat v = pool_seat(s, m);
    LiarSeat q{0, false, false, false};
    if (learner) q = liar_seat_load(v, e);
    const bool run = s.running[e] != 0, can = s.can[e] != 0, d1 = s.done1[e] != 0;
    const float r1_ego = s.rew1[2 * e];
    LiarOutcome o2{0.f, 0.f, false};
    if (run) {
      if (learner) liar_sp_commit(v, q, e, can);
      else s.alt_acted[e] = 1;
      o2 = liar_move(t, e, s.history, s.nmoves, s.alt_actions, false, s.obs_next, s.rew2, s.done2);
    }
    const bool d2 = run && o2.done;
    if (learner) liar_sp_credit(v, q, m.rb_rew, m.rb_T, e, o2.r_alt, d2, run);
    const bool done = d1 || d2;
    liar_add_f32(ego_rew_row + e, r1_ego + (run ? o2.r_ego : 0.f));
    s.ego_episode_start[e] = done ? 1.f : 0.f;
    if (run && !d2) liar_write_obs(t, true, s.obs_ego + (size_t)e * 30);
    s.done[e] = done ? 1 : 0;
    if (done) atomicAdd(s.episodes, 1ull);
    fresh = done;
  }
  if (fresh) {
    const uint64_t c = counter + (epoch ? (uint64_t)(*epoch) << 32 : 0ull);
    ego_first = liar_deal(t, e, s.hands, s.history, s.nmoves, s.ego_first, s.dice_seed, c, s.probegostart);
    s.alt_acted[e] = 0;
    k = pool_resample(k, s.K, s.resample, s.pool_seed, c, e);   // the member that sits at the new game
    s.partnerid[e] = k;
  }
  s.alt_opens[e] = (fresh && !ego_first) ? 1 : 0;
  s.ego_opens[e] = (fresh && ego_first) ? 1 : 0;
  pool_prepare(s, s.members[k], e, fresh && !ego_first);
  if (fresh && !ego_first) liar_write_obs(t, false, s.obs_alt + (size_t)e * 30);
}

__global__ void pool_after_opening_kernel(PoolStep s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  const bool alt_opens = s.alt_opens[e] != 0, ego_opens = s.ego_opens[e] != 0;
  if (!alt_opens && !ego_opens) return;
  LiarTable t;
  liar_load(t, e, s.hands, s.history, s.nmoves);
  if (alt_opens) {
    const PoolMemberDev m = s.members[pool_member_of(s, e)];
    if (m.kind == PH_POOL_LEARNER) {
      const PoolSeat v = pool_seat(s, m);
      LiarSeat q = liar_seat_load(v, e);
      liar_sp_commit(v, q, e, s.can[e] != 0);
    } else {
      s.alt_acted[e] = 1;
    }
    (void)liar_move(t, e, s.history, s.nmoves, s.alt_actions, false, s.obs_next, s.rew2, s.done2);
  }
  liar_write_obs(t, true, s.obs_ego + (size_t)e * 30);
}

#define PH_POOL_GRID(s) dim3(((s).n + 255) / 256), dim3(256)
hipError_t launch_pool_after_ego(const PoolStep& s, hipStream_t st) {
  hipLaunchKernelGGL(pool_after_ego_kernel, PH_POOL_GRID(s), 0, st, s);
  return hipGetLastError();
}
hipError_t launch_pool_after_reply(const PoolStep& s, float* ego_rew_row, unsigned long long counter, const unsigned long long* epoch,
                                   int deal_only, hipStream_t st) {
  hipLaunchKernelGGL(pool_after_reply_kernel, PH_POOL_GRID(s), 0, st, s, ego_rew_row, (uint64_t)counter, epoch, deal_only);
  return hipGetLastError();
}
hipError_t launch_pool_after_opening(const PoolStep& s, hipStream_t st) {
  hipLaunchKernelGGL(pool_after_opening_kernel, PH_POOL_GRID(s), 0, st, s);
  return hipGetLastError();
}

}  // namespace ph
