// Episode statistics of a filled rollout buffer (ph_episode.h): one launch behind the rollout.
// Reference: the Monitor wrapper's per-episode (r, l) records that OnPolicyAgent averages out of ep_info_buffer
// (pantheonrl/common/agents.py:132-158) -- here over every episode that ended, per pool member, summed on the device.
//
// A workgroup owns EPISODE_TABLES consecutive tables and takes the rollout in blocks of EPISODE_CHUNK rows, three passes a block:
//   stage  ALL lanes load the block's rows of the two planes into LDS: lane (row group, table) issues its 2 x 16 loads before
//          anything waits for one (they do not depend on any running sum), lanes of a row read adjacent columns (one 128-byte line);
//   walk   one lane per table runs the only dependent chain -- return += reward in f32, row by row -- out of LDS, and leaves an
//          EVENT in place of each row that ended a counted episode: (f32 return, length and member);
//   sum    ALL lanes again: lane (row group, table) adds the events of its rows to f64 sums it keeps in registers per member.
// (Measured, profiles/episode_stats_speed.txt: walking HBM directly with 16 rows of loads in flight took 27 us at T = 128 against
// GAE's 5 -- and so did staging alone: the time was the walk's, 0.17 us a row, because it kept its f64 sums in LDS and every row's
// read-modify-write waited for the row before.  Hence events: the chain carries four words and stores without reading back.)
// Sums: per-episode returns are f32 in row order, carry first (bitwise the sequential NumPy loop); sums over episodes are f64,
// reduced in a fixed order -- a lane's rows in row order, the wave's butterfly, the workgroup's waves in index order through LDS,
// then the workgroups' partials by whichever workgroup stores its partials last (an integer ticket; no floating-point atomics):
// eight contiguous ranges of workgroups each in index order, the eight range sums in index order -- two runs give the same bits.
#include "ph_episode.h"
#include "ph_pool.h"

namespace ph {

namespace {

constexpr int EP_GROUPS = EPISODE_WG / EPISODE_TABLES;          // row groups of the stage and sum passes
constexpr int EP_STAGE = EPISODE_CHUNK / EP_GROUPS;             // rows of a block per lane in those passes
constexpr int EP_UNROLL = 16;                                   // rows the walk reads out of LDS ahead of its chain
constexpr int EP_WAVES = EPISODE_WG / 64;
constexpr int EP_PARTS = EPISODE_WG / 32;                       // ranges of workgroups in the last phase
constexpr int EP_SLOTS = PH_MAX_POOL * EPISODE_NSTAT;           // statistics of one scan
static_assert(EPISODE_TABLES == 32 && EPISODE_WG % 64 == 0 && EPISODE_CHUNK % EP_GROUPS == 0 && EP_SLOTS == 32, "episode scan tiling");
static_assert(PH_MAX_POOL <= 15, "an event's member field is four bits");

__device__ __forceinline__ double episode_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

}  // namespace

// MEMBERS: K > 1, the member at seat 1 is replayed.  Without members a row of the walk is branch-free (selects): the walk is one wave
// issuing a dependent chain, so its time is its instruction count per row -- 25 with the end of a game behind a branch (exec mask
// saved and restored twice, three scalar branches), 0.12 us a row measured; see profiles/episode_stats_speed.txt for this form's.
template <bool MEMBERS>
__global__ __launch_bounds__(EPISODE_WG) void episode_scan_kernel(EpisodeScan a) {
#pragma clang fp contract(off)
  __shared__ float s_r[EPISODE_CHUNK * EPISODE_TABLES];      // [row][table] staged rewards; behind the walk: an event's return
  __shared__ float s_d[EPISODE_CHUNK * EPISODE_TABLES];      // staged end flags; behind the walk: an event's (length << 4 | member + 1) or 0
  __shared__ double s_wave[EP_WAVES * EP_SLOTS];             // the waves' sums
  __shared__ double s_part[EP_PARTS * EP_SLOTS];             // the last phase's range sums
  __shared__ int s_last;
  const int K = a.K, T = a.T, E = a.E, lane = threadIdx.x;
  const int el = lane % EPISODE_TABLES, grp = lane / EPISODE_TABLES;
  const int e = blockIdx.x * EPISODE_TABLES + el;
  const bool walker = grp == 0 && e < E;          // one lane per table walks
  const int ec = e < E ? e : E - 1;               // a lane past the last table stages a copy of it (never walked, never summed)
  float ret = 0.f;
  int len = 0, m = 0;
  bool valid = false;
  if (walker) {
    ret = a.carry_return[e];
    len = a.carry_length[e];
    valid = a.carry_valid[e] != 0;
    if constexpr (MEMBERS) {
      m = a.member[e];
      m = m < 0 ? 0 : (m >= K ? K - 1 : m);
    }
  }
  const uint64_t c0 = a.counter0 + (a.epoch ? (uint64_t)(*a.epoch) << 32 : 0ull);   // the step's counter word (ph_liar_step.h)
  double sum[PH_MAX_POOL], sq[PH_MAX_POOL];
  unsigned cnt[PH_MAX_POOL], lsum[PH_MAX_POOL];
#pragma unroll
  for (int k = 0; k < PH_MAX_POOL; ++k) {
    sum[k] = 0.0;
    sq[k] = 0.0;
    cnt[k] = 0u;
    lsum[k] = 0u;
  }
  // one row of the walk: the event (stored, never read back by the chain), then the carries
  int vmask = valid ? -1 : 0;      // `valid` of the member-free walk as a mask: its row is bit operations, nothing the compiler
                                   // turns back into exec-mask regions
  auto row = [&](int t, int i, float r, float end) {
    ret = ret + r;
    len += 1;
    const bool ended = end != 0.f;
    s_r[i] = ret;
    if constexpr (!MEMBERS) {
      const int emask = ended ? -1 : 0;
      s_d[i] = __int_as_float(((len << 4) | 1) & emask & vmask);
      ret = __int_as_float(__float_as_int(ret) & ~emask);      // +0.0f behind an end
      len &= ~emask;
      vmask |= emask;
      return;
    }
    s_d[i] = __int_as_float(ended && valid ? (len << 4) | (m + 1) : 0);
    if constexpr (MEMBERS) {
      if (ended) {
        ret = 0.f;
        len = 0;
        valid = true;
        m = pool_resample(m, K, a.resample, a.pool_seed, c0 + (uint64_t)t, e);
      }
    }
  };
  for (int t0 = 0; t0 < T; t0 += EPISODE_CHUNK) {
    const int rows = T - t0 < EPISODE_CHUNK ? T - t0 : EPISODE_CHUNK;
    // stage: every load of the block is issued before the first LDS store waits for one.  Rows past the block's end re-read row
    // T - 1 (in bounds, never walked): addresses are selected, no load sits behind a branch
    {
      float r[EP_STAGE], d[EP_STAGE];
#pragma unroll
      for (int u = 0; u < EP_STAGE; ++u) {
        int t = t0 + grp + u * EP_GROUPS;
        t = t < T ? t : T - 1;
        const float* p = t + 1 < T ? a.starts + (size_t)(t + 1) * E + ec : a.last_dones + ec;   // episode_starts[t + 1] = "ended in row t"
        r[u] = a.rewards[(size_t)t * E + ec];
        d[u] = *p;
      }
#pragma unroll
      for (int u = 0; u < EP_STAGE; ++u) {
        const int i = (grp + u * EP_GROUPS) * EPISODE_TABLES + el;
        s_r[i] = r[u];
        s_d[i] = d[u];
      }
    }
    __syncthreads();
    if (walker) {
      int tl = 0;
      for (; tl + EP_UNROLL <= rows; tl += EP_UNROLL) {
        float wr[EP_UNROLL], wd[EP_UNROLL];
#pragma unroll
        for (int u = 0; u < EP_UNROLL; ++u) {
          wr[u] = s_r[(tl + u) * EPISODE_TABLES + el];
          wd[u] = s_d[(tl + u) * EPISODE_TABLES + el];
        }
#pragma unroll
        for (int u = 0; u < EP_UNROLL; ++u) row(t0 + tl + u, (tl + u) * EPISODE_TABLES + el, wr[u], wd[u]);
      }
      for (; tl < rows; ++tl) {
        const int i = tl * EPISODE_TABLES + el;
        row(t0 + tl, i, s_r[i], s_d[i]);
      }
    }
    __syncthreads();
    // sum: the events of this lane's rows, in row order, into the member's registers (a select per member: no indexed registers)
    if (e < E) {
#pragma unroll
      for (int u = 0; u < EP_STAGE; ++u) {
        const int tl = grp + u * EP_GROUPS;
        if (tl < rows) {
          const int i = tl * EPISODE_TABLES + el;
          const int code = __float_as_int(s_d[i]);
          if (code != 0) {
            const double x = (double)s_r[i];
            const double xx = x * x;
            const int mk = (code & 15) - 1;
            const unsigned l = (unsigned)(code >> 4);
#pragma unroll
            for (int k = 0; k < PH_MAX_POOL; ++k)
              if (k < K && mk == k) {
                cnt[k] += 1u;
                lsum[k] += l;
                sum[k] += x;
                sq[k] += xx;
              }
          }
        }
      }
    }
    __syncthreads();      // the next block's staging overwrites the events
  }
  if (walker) {
    a.carry_return[e] = ret;
    a.carry_length[e] = len;
    a.carry_valid[e] = (MEMBERS ? valid : vmask != 0) ? 1 : 0;
    if constexpr (MEMBERS) a.member[e] = m;
  }
  // the wave's lanes (butterfly: a fixed tree), then the workgroup's waves in index order
  const int NS = K * EPISODE_NSTAT;
  const int wave = lane >> 6;
#pragma unroll
  for (int k = 0; k < PH_MAX_POOL; ++k)
    if (k < K) {
      const double c = episode_wave_sum((double)cnt[k]);
      const double s = episode_wave_sum(sum[k]);
      const double q = episode_wave_sum(sq[k]);
      const double l = episode_wave_sum((double)lsum[k]);
      if ((lane & 63) == 0) {
        double* w = s_wave + wave * EP_SLOTS + k * EPISODE_NSTAT;
        w[0] = c;
        w[1] = s;
        w[2] = q;
        w[3] = l;
      }
    }
  __syncthreads();
  if (lane < NS) {
    double p = s_wave[lane];
#pragma unroll
    for (int w = 1; w < EP_WAVES; ++w) p += s_wave[w * EP_SLOTS + lane];
    a.partial[(size_t)blockIdx.x * NS + lane] = p;
    __threadfence();
  }
  __syncthreads();
  // the workgroup whose ticket is the last one adds every workgroup's partials to stats -- in an order that does not depend on
  // which workgroup that is: EP_PARTS contiguous ranges of workgroups, each in index order, then the ranges in index order
  if (lane == 0) s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  {
    const int j = lane % EP_SLOTS, part = lane / EP_SLOTS;
    const unsigned nb = gridDim.x, per = (nb + EP_PARTS - 1) / EP_PARTS;
    const unsigned b0 = part * per, b1 = b0 + per < nb ? b0 + per : nb;
    double s = 0.0;
    if (j < NS) {
      unsigned b = b0;
      for (; b + 8 <= b1; b += 8) {
        unsigned long long v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(a.partial + (size_t)(b + u) * NS + j), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += __longlong_as_double((long long)v[u]);
      }
      for (; b < b1; ++b)
        s += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(a.partial + (size_t)b * NS + j),
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    s_part[part * EP_SLOTS + j] = s;
  }
  __syncthreads();
  if (lane < NS) {
    double s = a.stats[lane];
#pragma unroll
    for (int p = 0; p < EP_PARTS; ++p) s += s_part[p * EP_SLOTS + lane];
    a.stats[lane] = s;
  }
  if (lane == 0) *a.ticket = 0u;      // the next launch (or the next replay of this one) starts from zero again
}

hipError_t launch_episode_scan(const EpisodeScan& a, hipStream_t st) {
  if (a.K > 1) hipLaunchKernelGGL(episode_scan_kernel<true>, dim3(episode_workgroups(a.E)), dim3(EPISODE_WG), 0, st, a);
  else hipLaunchKernelGGL(episode_scan_kernel<false>, dim3(episode_workgroups(a.E)), dim3(EPISODE_WG), 0, st, a);
  return hipGetLastError();
}

}  // namespace ph
