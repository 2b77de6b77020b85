// Cross-play evaluation of Liar's Dice (ph_xplay.h): the three book-keeping launches between the seat forwards, one lane per
// table, and the statistics reduction.  The rules are ph_liar.h's lane functions; the forwards are the pool's (ph_pool.hip,
// ph_policy.hip).  As in ph_pool.hip a pass reads a table's flags ONCE, at its top, and never reads one back behind a store.
#include "ph_xplay.h"

namespace ph {

// seat 0 has moved in every playing table (its forward wrote ego_actions): play the move, find the tables that go on
__global__ void xplay_after_ego_kernel(XplayStep s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  if (!s.playing[e]) return;   // idle: running[e] was cleared when the budget ran out
  LiarTable t;
  liar_load(t, e, s.hands, s.history, s.nmoves);
  const LiarOutcome o1 = liar_move(t, e, s.history, s.nmoves, s.ego_actions, true, s.obs_next, s.rew1, s.done1);
  s.running[e] = o1.done ? 0 : 1;
}

// seat 1 has replied where the game went on: play that move, add both transitions to the game's return (multiagentenv.py:201-202),
// and at the end of a game log it, count it, and either deal the next game with the dice counter or -- budget spent -- retire the
// table.  deal_only: the first deal of the tables flagged in `done`.
__global__ void xplay_after_reply_kernel(XplayStep s, uint64_t counter, const unsigned long long* __restrict__ epoch, int deal_only) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  const bool playing = s.playing[e] != 0;
  const bool run = s.running[e] != 0, d1 = s.done1[e] != 0;
  const float r1_ego = s.rew1[2 * e];
  bool ego_first = s.ego_first[e] != 0;
  bool fresh = s.done[e] != 0;             // a deal-only call: the caller's flags
  float ret = s.ep_return[e];
  int len = s.ep_length[e], g = s.games[e];
  if (!playing) return;
  LiarTable t;
  liar_load(t, e, s.hands, s.history, s.nmoves);
  if (!deal_only) {
    LiarOutcome o2{0.f, 0.f, false};
    if (run) o2 = liar_move(t, e, s.history, s.nmoves, s.alt_actions, false, s.obs_next, s.rew2, s.done2);
    const bool d2 = run && o2.done;
    const bool done = d1 || d2;
    ret += r1_ego + (run ? o2.r_ego : 0.f);
    len += 1;
    if (run && !d2) liar_write_obs(t, true, s.obs_ego + (size_t)e * 30);   // = obs_next of the move just played
    s.done[e] = done ? 1 : 0;
    fresh = done;
    if (done) {
      if (g >= 0 && g < s.G) {
        s.returns[(size_t)e * s.G + g] = ret;
        s.lengths[(size_t)e * s.G + g] = len;
      }
      g += 1;
      s.games[e] = g;
      ret = 0.f;
      len = 0;
    }
    s.ep_return[e] = ret;
    s.ep_length[e] = len;
    if (done && g >= s.G) {   // the budget is spent: the table leaves every later forward and pass
      s.playing[e] = 0;
      s.running[e] = 0;
      s.alt_opens[e] = 0;
      s.ego_opens[e] = 0;
      atomicSub(s.tables_left, 1);
      return;
    }
  }
  if (fresh)   // (the context's RNG epoch word, when one is attached, is the dice counter's high half -- as in ph_liar_reset)
    ego_first = liar_deal(t, e, s.hands, s.history, s.nmoves, s.ego_first, s.dice_seed,
                          counter + (epoch ? (uint64_t)(*epoch) << 32 : 0ull), s.probegostart);
  s.alt_opens[e] = (fresh && !ego_first) ? 1 : 0;
  s.ego_opens[e] = (fresh && ego_first) ? 1 : 0;
  if (fresh && !ego_first) liar_write_obs(t, false, s.obs_alt + (size_t)e * 30);
}

// seat 1 has opened the new games it starts: play that move; seat 0's observation of every fresh table
__global__ void xplay_after_opening_kernel(XplayStep s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  const bool alt_opens = s.alt_opens[e] != 0, ego_opens = s.ego_opens[e] != 0;
  if (!alt_opens && !ego_opens) return;   // (an idle table's flags are both clear)
  LiarTable t;
  liar_load(t, e, s.hands, s.history, s.nmoves);
  if (alt_opens) (void)liar_move(t, e, s.history, s.nmoves, s.alt_actions, false, s.obs_next, s.rew2, s.done2);
  liar_write_obs(t, true, s.obs_ego + (size_t)e * 30);
}

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

#define PH_XPLAY_GRID(s) dim3(((s).n + 255) / 256), dim3(256)
hipError_t launch_xplay_after_ego(const XplayStep& s, hipStream_t st) {
  hipLaunchKernelGGL(xplay_after_ego_kernel, PH_XPLAY_GRID(s), 0, st, s);
  return hipGetLastError();
}
hipError_t launch_xplay_after_reply(const XplayStep& s, unsigned long long counter, const unsigned long long* epoch, int deal_only,
                                    hipStream_t st) {
  hipLaunchKernelGGL(xplay_after_reply_kernel, PH_XPLAY_GRID(s), 0, st, s, (uint64_t)counter, epoch, deal_only);
  return hipGetLastError();
}
hipError_t launch_xplay_after_opening(const XplayStep& s, hipStream_t st) {
  hipLaunchKernelGGL(xplay_after_opening_kernel, PH_XPLAY_GRID(s), 0, st, s);
  return hipGetLastError();
}
hipError_t launch_xplay_stats(const float* returns, const int* lengths, const int* games, int n, int G, int n_pairs, double* stats,
                              hipStream_t st) {
  hipLaunchKernelGGL(xplay_stats_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, returns, lengths, games, n, G, n_pairs, stats);
  return hipGetLastError();
}

}  // namespace ph
