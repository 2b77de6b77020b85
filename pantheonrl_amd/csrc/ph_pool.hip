// Liar's Dice against a pool of partners (ph_pool.h): the bucket pass in front of the grouped forward and the scripted member's rule.
// The grouped forward itself is pool_fwd16h_kernel in ph_policy.hip; the step's book-keeping is ph_liar_step.h with PoolBook.
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

}  // namespace ph
