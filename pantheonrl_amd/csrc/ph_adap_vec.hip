// ADAP seats of the device-resident games: the row build and the context redraw (rules: ph_adap_vec.h).
//
// Both are small and memory-shaped.  The row build runs one lane per row ELEMENT, so a wave stores 64 consecutive floats whatever the
// row length (F + C = 273 for Liar's Dice: odd, so no row but the first is 16-byte aligned and nothing here is wider than a float);
// the prefix sums of the one-hot layout come by value in the launch and are staged in LDS once per workgroup.  The redraw runs one
// lane per table: C Philox calls and C stores.
#include "ph_adap_vec.h"

namespace ph {

namespace {
constexpr int AV_THREADS = 256;

__global__ __launch_bounds__(AV_THREADS) void adap_rows_kernel(const AdapRowShape s, const float* __restrict__ obs,
                                                               const float* __restrict__ contexts,
                                                               const unsigned char* __restrict__ active, float* __restrict__ rows, int n) {
  __shared__ int off_s[PH_MAX_COMP + 1];
  if (!s.box)
    for (int i = threadIdx.x; i <= s.D; i += AV_THREADS) off_s[i] = s.off[i];
  __syncthreads();
  const int W = s.F + s.C;
  const long long g = (long long)blockIdx.x * AV_THREADS + threadIdx.x;
  if (g >= (long long)n * W) return;
  const int e = (int)(g / W), f = (int)(g - (long long)e * W);
  if (active && !active[e]) return;
  rows[g] = adap_row_value(s, off_s, obs + (size_t)e * s.D, contexts + (size_t)e * s.C, f);
}

__global__ __launch_bounds__(AV_THREADS) void adap_context_draw_kernel(int sampler, int cs, unsigned long long seed,
                                                                       unsigned long long counter, const unsigned long long* epoch,
                                                                       const unsigned char* __restrict__ redraw,
                                                                       const unsigned char* __restrict__ redraw2,
                                                                       float* __restrict__ contexts, int n) {
  const int e = blockIdx.x * AV_THREADS + threadIdx.x;
  if (e >= n) return;
  if ((redraw || redraw2) && !(redraw && redraw[e]) && !(redraw2 && redraw2[e])) return;
  adap_draw_context(sampler, cs, seed, adap_vec_counter(counter, epoch), (uint32_t)e, contexts + (size_t)e * cs);
}
}  // namespace

hipError_t launch_adap_rows(const AdapRowShape& shape, const float* obs, const float* contexts, const unsigned char* active, float* rows,
                            int n, hipStream_t st) {
  const long long total = (long long)n * (shape.F + shape.C);
  const unsigned blocks = (unsigned)((total + AV_THREADS - 1) / AV_THREADS);
  hipLaunchKernelGGL(adap_rows_kernel, dim3(blocks), dim3(AV_THREADS), 0, st, shape, obs, contexts, active, rows, n);
  return hipGetLastError();
}

hipError_t launch_adap_context_draw(int sampler, int cs, unsigned long long seed, unsigned long long counter,
                                    const unsigned long long* epoch, const unsigned char* redraw, float* contexts, int n, hipStream_t st,
                                    const unsigned char* redraw2) {
  hipLaunchKernelGGL(adap_context_draw_kernel, dim3((n + AV_THREADS - 1) / AV_THREADS), dim3(AV_THREADS), 0, st, sampler, cs, seed,
                     counter, epoch, redraw, redraw2, contexts, n);
  return hipGetLastError();
}

}  // namespace ph
