// Episode returns and lengths of the ego, per pool member, from what a rollout already left in HBM (ph_episode.hip): one scan of
// the rollout buffer's reward and episode-start planes behind the rollout, nothing in the step.  An episode of table e ends at row t
// iff episode_starts[t + 1][e] is set (t + 1 < T) or last_dones[e] is (t = T - 1); its return is the f32 sum of rewards[.][e] over
// its rows in row order, carry first, its length its number of rows; games span rollouts, so (return, length, valid) are carried per
// table.  In the pool the member at seat 1 is replayed, not logged: the lane credits an ending episode to the member it holds for
// the table and advances it with the step's own pool_resample (ph_pool.h) under the step's counter -- row t was step counter0 + t,
// the epoch word, when one is attached, its high half.
#pragma once
#include <hip/hip_runtime.h>

namespace ph {

constexpr int EPISODE_NSTAT = 4;     // count, sum of returns, sum of squared returns, sum of lengths
constexpr int EPISODE_WG = 256;      // lanes of a workgroup: all of them stage rows into LDS, one per table walks them
constexpr int EPISODE_TABLES = 32;   // tables of a workgroup: one 128-byte line per row and plane
constexpr int EPISODE_CHUNK = 128;   // rows staged per pass: a rollout of T <= 128 rows is one round trip to HBM

struct EpisodeScan {
  const float* rewards;          // (T, E)
  const float* starts;           // (T, E) row t + 1 = "ended in row t"; row 0 is never read
  const float* last_dones;       // (E) the same for row T - 1
  int T, E;
  float* carry_return;           // (E) in/out
  int* carry_length;             // (E) in/out
  unsigned char* carry_valid;    // (E) in/out: 0 = the game in progress is dropped when it ends
  int K;                         // members; 1 = no attribution
  int* member;                   // (E) in/out, null when K == 1
  int resample;
  unsigned long long pool_seed, counter0;
  const unsigned long long* epoch;   // device RNG epoch word or null
  double* stats;                 // (K, EPISODE_NSTAT) accumulated into
  double* partial;               // workspace [workgroups][K][EPISODE_NSTAT]
  unsigned int* ticket;          // workspace [1]: workgroups that have stored their partials; zero between launches
};

inline int episode_workgroups(int E) { return (E + EPISODE_TABLES - 1) / EPISODE_TABLES; }
hipError_t launch_episode_scan(const EpisodeScan& a, hipStream_t st);

}  // namespace ph
