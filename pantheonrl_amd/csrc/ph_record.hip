// The device-resident move log of the vectorised Liar's Dice step (ph_record.h): the two record launches of a step and the export.
// The recorder reads what the step's forwards and passes left in the step's arrays and writes its own log only.
#include "ph_record.h"

namespace ph {

namespace {

// append one row to table e's log: cnt = the table's cursor in registers.  -> the row's index, -1: the table is full (dropped)
__device__ __forceinline__ int rec_put(const RecordLog& L, int e, int& cnt, const float* obs, const int* actions, int flag, int who) {
  if ((unsigned)cnt >= (unsigned)L.cap) return -1;
  const size_t slot = (size_t)e * L.cap + cnt;
  float* r = L.rows + slot * REC_ROW;
  const float2* o2 = reinterpret_cast<const float2*>(obs + (size_t)e * REC_OBS);
#pragma unroll
  for (int k = 0; k < REC_OBS / 2; ++k) {
    const float2 v = o2[k];
    r[2 * k] = v.x;
    r[2 * k + 1] = v.y;
  }
  const int2 a = *reinterpret_cast<const int2*>(actions + 2 * (size_t)e);   // the raw move, as the recorder logs it
  r[REC_OBS] = (float)a.x;
  r[REC_OBS + 1] = (float)a.y;
  r[REC_OBS + REC_ACT] = (float)flag;
  if (L.member) L.member[slot] = who;
  return cnt++;
}

// A: behind the reply forward, in front of after_reply
__global__ __launch_bounds__(256) void record_moves_kernel(RecordLog L, RecordStep s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L.n) return;
  if (s.playing && !s.playing[e]) return;   // an idle cross-play table logs nothing
  const bool d1 = s.done1[e] != 0, run = s.running[e] != 0;
  int cnt = L.count[e], lost = 0, alt_rows = 0, pend = -1;
  if (rec_put(L, e, cnt, s.obs_ego, s.ego_actions, REC_EGO_NOT_DONE + (d1 ? 2 : 0), s.ego_id ? s.ego_id[e] : 0) < 0) lost += 1;
  if (run) {
    pend = rec_put(L, e, cnt, s.obs_next, s.alt_actions, REC_ALT_NOT_DONE, s.alt_id ? s.alt_id[e] : 0);
    if (pend < 0) lost += 1;
    else alt_rows = 1;
  }
  L.count[e] = cnt;
  if (alt_rows) L.count_alt[e] += alt_rows;
  if (lost) L.dropped[e] += lost;
  L.pending[e] = pend;
}

// B: behind the opening forward, in front of after_opening
__global__ __launch_bounds__(256) void record_opening_kernel(RecordLog L, RecordStep s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L.n) return;
  const int pend = L.pending[e];
  const bool opens = s.alt_opens[e] != 0, d2 = s.done2[e] != 0;
  if (pend >= 0) {
    if (pend < L.cap && d2) L.rows[((size_t)e * L.cap + pend) * REC_ROW + REC_OBS + REC_ACT] = (float)(REC_ALT_NOT_DONE + 2);
    L.pending[e] = -1;
  }
  if (!opens) return;
  int cnt = L.count[e];
  if (rec_put(L, e, cnt, s.obs_alt, s.alt_actions, REC_ALT_NOT_DONE, s.alt_id ? s.alt_id[e] : 0) < 0) {
    L.dropped[e] += 1;
    return;
  }
  L.count[e] = cnt;
  L.count_alt[e] += 1;
}

// rows of table e the seat filter selects (cursors clamped to the table: nothing is read past rows[e])
__device__ __forceinline__ int rec_rows(const RecordLog& L, int e) {
  const int c = L.count[e];
  return c < 0 ? 0 : (c > L.cap ? L.cap : c);
}
__device__ __forceinline__ int rec_selected(const RecordLog& L, int e, int seat) {
  const int c = rec_rows(L, e);
  if (seat < 0) return c;
  int a = L.count_alt[e];
  a = a < 0 ? 0 : (a > c ? c : a);
  return seat == 1 ? a : c - a;
}

// exclusive scan of the selected counts: ONE block walks the tables 1024 at a time with a running carry (n is a few thousand at
// most and the export runs once per recording)
__global__ __launch_bounds__(1024) void record_scan_kernel(RecordLog L, int seat, long long* __restrict__ offsets) {
  __shared__ long long part[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  for (int base = 0; base < L.n; base += 1024) {
    const int e = base + tid;
    const long long c = e < L.n ? (long long)rec_selected(L, e, seat) : 0ll;
    long long v = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (lane == 63) part[wave] = v;
    __syncthreads();
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      before += w < wave ? part[w] : 0ll;
      total += part[w];
    }
    if (e < L.n) offsets[e] = carry + before + v - c;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) offsets[L.n] = carry;
}

// one wave per table: the table's rows in order, lane l < REC_ROW copies component l, lane REC_ROW the member
__global__ __launch_bounds__(64) void record_copy_kernel(RecordLog L, int seat, const long long* __restrict__ offsets,
                                                         float* __restrict__ rows_out, int* __restrict__ member_out, long long out_cap) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= L.n) return;
  const int c = rec_rows(L, e);
  long long k = offsets[e];
  const long long end = offsets[e + 1] < out_cap ? offsets[e + 1] : out_cap;
  for (int r = 0; r < c && k < end; ++r) {
    const size_t slot = (size_t)e * L.cap + r;
    const float* row = L.rows + slot * REC_ROW;
    if (seat >= 0 && (((int)row[REC_OBS + REC_ACT]) & 1) != seat) continue;
    if (lane < REC_ROW) rows_out[(size_t)k * REC_ROW + lane] = row[lane];
    else if (lane == REC_ROW && member_out) member_out[k] = L.member ? L.member[slot] : 0;
    ++k;
  }
}

}  // namespace

hipError_t launch_record_moves(const RecordLog& log, const RecordStep& s, hipStream_t st) {
  hipLaunchKernelGGL(record_moves_kernel, dim3((log.n + 255) / 256), dim3(256), 0, st, log, s);
  return hipGetLastError();
}
hipError_t launch_record_opening(const RecordLog& log, const RecordStep& s, hipStream_t st) {
  hipLaunchKernelGGL(record_opening_kernel, dim3((log.n + 255) / 256), dim3(256), 0, st, log, s);
  return hipGetLastError();
}
hipError_t launch_record_export(const RecordLog& log, int seat, long long* offsets, float* rows_out, int* member_out, long long out_cap,
                                hipStream_t st) {
  hipLaunchKernelGGL(record_scan_kernel, dim3(1), dim3(1024), 0, st, log, seat, offsets);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !rows_out || out_cap <= 0) return e;
  hipLaunchKernelGGL(record_copy_kernel, dim3(log.n), dim3(64), 0, st, log, seat, (const long long*)offsets, rows_out, member_out,
                     out_cap);
  return hipGetLastError();
}

}  // namespace ph
