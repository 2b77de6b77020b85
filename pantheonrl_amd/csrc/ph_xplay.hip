// Cross-play evaluation of Liar's Dice (ph_xplay.h): the statistics reduction.  What runs between the seat forwards is
// ph_liar_step.h with EvalEnd; the forwards are the pool's (ph_pool.hip, ph_policy.hip).
#include "ph_xplay.h"

namespace ph {

// ---- per-pair statistics: count, sum, sum of squares, sum of lengths in float64 ------------------------------------------------------
// One lane per pair walks that pair's tables (p, p + P, ...) in ascending order and each table's logged games in ascending order:
// a fixed summation order and no atomics, so two runs give the same bits.  It runs once per evaluation.
__global__ void xplay_stats_kernel(const float* __restrict__ returns, const int* __restrict__ lengths, const int* __restrict__ games,
                                   int n, int G, int P, double* __restrict__ stats) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double cnt = 0.0, sum = 0.0, sq = 0.0, len = 0.0;
  for (int e = p; e < n; e += P) {
    int g = games[e];
    g = g < 0 ? 0 : (g > G ? G : g);
    const float* r = returns + (size_t)e * G;
    const int* l = lengths + (size_t)e * G;
    for (int i = 0; i < g; ++i) {
      const double x = (double)r[i];
      cnt += 1.0;
      sum += x;
      sq += x * x;
      len += (double)l[i];
    }
  }
  double2* out = reinterpret_cast<double2*>(stats + (size_t)XPLAY_NSTAT * p);
  out[0] = make_double2(cnt, sum);
  out[1] = make_double2(sq, len);
}

hipError_t launch_xplay_stats(const float* returns, const int* lengths, const int* games, int n, int G, int n_pairs, double* stats,
                              hipStream_t st) {
  hipLaunchKernelGGL(xplay_stats_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, returns, lengths, games, n, G, n_pairs, stats);
  return hipGetLastError();
}

}  // namespace ph
