// The block worlds on the device (BlockEnv-v0 / BlockEnv-v1): the masked per-call kernels, the two book-keeping launches of
// the vectorised self-play step, the scripted constructors and the two book-keeping launches of the cross-play step and of the partner-pool step.  One lane per table; the rules are ph_block.h's, the partner seat's ragged book-keeping is
// ph_liar.h's (liar_sp_credit / liar_sp_prepare / liar_sp_commit).
#include "ph_block.h"
#include "ph_liar.h"
#include "ph_pool.h"

namespace ph {

// a table's 12 words as three 16-byte accesses
__device__ __forceinline__ void bw_load(BwTable& t, int variant, const int* state, int e) {
  int w[BW_WORDS];
  const int4* p = reinterpret_cast<const int4*>(state + (size_t)e * BW_WORDS);
#pragma unroll
  for (int i = 0; i < BW_WORDS / 4; ++i) {
    const int4 v = p[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  bw_unpack(t, variant, w);
}
__device__ __forceinline__ void bw_store(const BwTable& t, int variant, int* state, int e) {
  int w[BW_WORDS];
  bw_pack(t, variant, w);
  int4* p = reinterpret_cast<int4*>(state + (size_t)e * BW_WORDS);
#pragma unroll
  for (int i = 0; i < BW_WORDS / 4; ++i) p[i] = make_int4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
__device__ __forceinline__ uint64_t bw_counter(uint64_t counter, const unsigned long long* epoch) {
  return counter + (epoch ? (uint64_t)(*epoch) << 32 : 0ull);
}

__global__ void block_reset_kernel(int variant, int* __restrict__ state, const unsigned char* __restrict__ reset_mask,
                                   uint64_t seed, uint64_t counter, const unsigned long long* __restrict__ epoch, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (reset_mask && !reset_mask[e]) return;
  BwTable t;
  bw_reset(t, variant, seed, bw_counter(counter, epoch), (uint32_t)e, BW_MAX_DRAWS);
  bw_store(t, variant, state, e);
}
hipError_t launch_block_reset(int variant, int* state, const unsigned char* reset_mask, unsigned long long seed,
                              unsigned long long counter, const unsigned long long* epoch, int n, hipStream_t s) {
  hipLaunchKernelGGL(block_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, s, variant, state, reset_mask, (uint64_t)seed,
                     (uint64_t)counter, epoch, n);
  return hipGetLastError();
}

// ego_step (is_ego) or alt_step of every active table: the OTHER seat's observation, rewards (ego, partner), done
__global__ void block_step_kernel(int variant, int* __restrict__ state, const int* __restrict__ actions, int is_ego,
                                  const unsigned char* __restrict__ active, float* __restrict__ obs_next,
                                  float* __restrict__ rewards, unsigned char* __restrict__ done, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (active && !active[e]) return;
  BwTable t;
  bw_load(t, variant, state, e);
  BwOutcome o{0.f, false};
  if (is_ego) {
    o = bw_ego_step(t, variant, actions[e]);
    bw_write_alt_obs(t, variant, obs_next + (size_t)e * bw_alt_obs_len(variant));
  } else {
    const int A = bw_alt_act_len(variant);
    int a[3] = {actions[(size_t)e * A], actions[(size_t)e * A + 1], variant ? actions[(size_t)e * A + 2] : 0};
    bw_alt_step(t, variant, a);
    bw_write_ego_obs(t, variant, obs_next + (size_t)e * bw_ego_obs_len(variant));
  }
  bw_store(t, variant, state, e);
  rewards[2 * (size_t)e] = o.reward;
  rewards[2 * (size_t)e + 1] = o.reward;
  done[e] = o.done ? 1 : 0;
}
hipError_t launch_block_step(int variant, int* state, const int* actions, int is_ego, const unsigned char* active, float* obs_next,
                             float* rewards, unsigned char* done, int n, hipStream_t s) {
  hipLaunchKernelGGL(block_step_kernel, dim3((n + 255) / 256), dim3(256), 0, s, variant, state, actions, is_ego, active, obs_next,
                     rewards, done, n);
  return hipGetLastError();
}

__global__ void block_obs_kernel(int variant, const int* __restrict__ state, int is_ego, const unsigned char* __restrict__ active,
                                 float* __restrict__ obs_out, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (active && !active[e]) return;
  BwTable t;
  bw_load(t, variant, state, e);
  if (is_ego) bw_write_ego_obs(t, variant, obs_out + (size_t)e * bw_ego_obs_len(variant));
  else bw_write_alt_obs(t, variant, obs_out + (size_t)e * bw_alt_obs_len(variant));
}
hipError_t launch_block_obs(int variant, const int* state, int is_ego, const unsigned char* active, float* obs_out, int n,
                            hipStream_t s) {
  hipLaunchKernelGGL(block_obs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, variant, state, is_ego, active, obs_out, n);
  return hipGetLastError();
}

// ---- vectorised self-play: ego forward | after_ego | partner forward (ragged) | after_alt -------------------------------------
// The planner always opens, so a step needs no opening pass: every table is at the planner's turn before and after it.
//
// after_ego: the planner's token is played.  The partner is credited where it already moved in this game (MultiAgentEnv.
// _update_players), the ego's reward row / episode flag / the episode count follow; a finished table gets its next world at once
// (the step's counter) and its planner observation, a running one the constructor's observation and the partner's record flags.
__global__ void block_sp_after_ego_kernel(ph_block_selfplay s, float* alt_rewards, int alt_T, float* ego_rew_row, uint64_t counter,
                                          const unsigned long long* __restrict__ epoch) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  BwTable t;
  bw_load(t, s.variant, s.state, e);
  LiarSeat q = liar_seat_load(s, e);
  const BwOutcome o = bw_ego_step(t, s.variant, s.ego_actions[e]);
  liar_sp_credit(s, q, alt_rewards, alt_T, e, o.reward, o.done, q.acted);
  liar_add_f32(ego_rew_row + e, o.reward);
  s.ego_episode_start[e] = o.done ? 1.f : 0.f;
  s.done[e] = o.done ? 1 : 0;
  s.running[e] = o.done ? 0 : 1;
  if (o.done) {
    atomicAdd(s.episodes, 1ull);
    bw_reset(t, s.variant, s.world_seed, bw_counter(counter, epoch), (uint32_t)e, BW_MAX_DRAWS);
    s.alt_acted[e] = 0;
    bw_write_ego_obs(t, s.variant, s.obs_ego + (size_t)e * bw_ego_obs_len(s.variant));
  } else {
    bw_write_alt_obs(t, s.variant, s.obs_alt + (size_t)e * bw_alt_obs_len(s.variant));
  }
  bw_store(t, s.variant, s.state, e);
  liar_sp_prepare(s, q, alt_T, e, !o.done);
}
// after_alt: where the game goes on the constructor's move is played (it pays nothing and never ends a game) and the planner
// sees the result
__global__ void block_sp_after_alt_kernel(ph_block_selfplay s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  if (!s.running[e]) return;
  BwTable t;
  bw_load(t, s.variant, s.state, e);
  LiarSeat q = liar_seat_load(s, e);
  liar_sp_commit(s, q, e, s.can[e] != 0);
  const int A = bw_alt_act_len(s.variant);
  int a[3] = {s.alt_actions[(size_t)e * A], s.alt_actions[(size_t)e * A + 1], s.variant ? s.alt_actions[(size_t)e * A + 2] : 0};
  bw_alt_step(t, s.variant, a);
  bw_store(t, s.variant, s.state, e);
  bw_write_ego_obs(t, s.variant, s.obs_ego + (size_t)e * bw_ego_obs_len(s.variant));
}
hipError_t launch_block_sp_after_ego(const ph_block_selfplay& s, float* ego_rew_row, unsigned long long counter,
                                     const unsigned long long* epoch, hipStream_t st) {
  hipLaunchKernelGGL(block_sp_after_ego_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s, s.alt_rb->rewards, s.alt_rb->T,
                     ego_rew_row, (uint64_t)counter, epoch);
  return hipGetLastError();
}
hipError_t launch_block_sp_after_alt(const ph_block_selfplay& s, hipStream_t st) {
  hipLaunchKernelGGL(block_sp_after_alt_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s);
  return hipGetLastError();
}

// ---- the scripted constructors (ph_block.h: bw_scripted_move), one lane per table -------------------------------------------------
__device__ __forceinline__ void bw_store_move(int variant, int* actions, int e, const int* a) {
  const int A = bw_alt_act_len(variant);
  actions[(size_t)e * A] = a[0];
  actions[(size_t)e * A + 1] = a[1];
  if (variant) actions[(size_t)e * A + 2] = a[2];
}
__global__ void block_scripted_actions_kernel(int variant, int rule, const float* __restrict__ obs,
                                              const unsigned char* __restrict__ active, int* __restrict__ actions, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n || (active && !active[e])) return;
  int a[3];
  bw_scripted_move(variant, rule, obs + (size_t)e * bw_alt_obs_len(variant), a);
  bw_store_move(variant, actions, e, a);
}
hipError_t launch_block_scripted_actions(int variant, int rule, const float* obs, const unsigned char* active, int* actions, int n,
                                         hipStream_t s) {
  hipLaunchKernelGGL(block_scripted_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, s, variant, rule, obs, active, actions, n);
  return hipGetLastError();
}
// the scripted members' rows of a grouped forward: the member and its rule come from the member table in device memory
__global__ void block_group_scripted_kernel(int variant, const float* __restrict__ obs, const PoolMemberDev* __restrict__ members,
                                            const int* __restrict__ member_of, const unsigned char* __restrict__ active,
                                            int* __restrict__ actions, int n, int K) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n || !active[e]) return;
  const int k = member_of[e];
  if (k < 0 || k >= K) return;
  if (members[k].kind != PH_POOL_SCRIPTED) return;
  int a[3];
  bw_scripted_move(variant, members[k].rb_T, obs + (size_t)e * bw_alt_obs_len(variant), a);
  bw_store_move(variant, actions, e, a);
}
hipError_t launch_block_group_scripted(int variant, const float* obs, const PoolMemberDev* members, const int* member_of,
                                       const unsigned char* active, int* actions, int n, int K, hipStream_t s) {
  hipLaunchKernelGGL(block_group_scripted_kernel, dim3((n + 255) / 256), dim3(256), 0, s, variant, obs, members, member_of, active,
                     actions, n, K);
  return hipGetLastError();
}

// ---- cross-play evaluation: grouped planner forward | after_ego | grouped constructor forward | after_alt ------------------------
// after_ego of a playing table: the token is played and counted; the end token logs the game's return and length at [e, games[e]],
// counts the game and either generates the next world (the step's counter) with its planner observation or -- budget spent --
// retires the table (playing = running = 0, tables_left -= 1: it leaves every later launch, its state and logs stay as they are).
// Where the game goes on the constructor's observation is written and the table is `running`.
__global__ void block_xp_after_ego_kernel(ph_block_xplay s, uint64_t counter, const unsigned long long* __restrict__ epoch) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  if (!s.playing[e]) return;
  BwTable t;
  bw_load(t, s.variant, s.state, e);
  const BwOutcome o = bw_ego_step(t, s.variant, s.ego_actions[e]);
  float ret = s.ep_return[e] + o.reward;
  int len = s.ep_length[e] + 1;
  bool running = !o.done;
  if (o.done) {
    const int G = s.episodes_per_table;
    int g = s.games[e];
    if (g >= 0 && g < G) {
      s.returns[(size_t)e * G + g] = ret;
      s.lengths[(size_t)e * G + g] = len;
    }
    g += 1;
    s.games[e] = g;
    ret = 0.f;
    len = 0;
    if (g >= G) {
      s.playing[e] = 0;
      atomicSub(s.tables_left, 1);
    } else {
      bw_reset(t, s.variant, s.world_seed, bw_counter(counter, epoch), (uint32_t)e, BW_MAX_DRAWS);
      bw_write_ego_obs(t, s.variant, s.obs_ego + (size_t)e * bw_ego_obs_len(s.variant));
    }
  } else {
    bw_write_alt_obs(t, s.variant, s.obs_alt + (size_t)e * bw_alt_obs_len(s.variant));
  }
  s.running[e] = running ? 1 : 0;
  s.ep_return[e] = ret;
  s.ep_length[e] = len;
  bw_store(t, s.variant, s.state, e);
}
// after_alt: where the game goes on the constructor's move is played and the planner sees the result
__global__ void block_xp_after_alt_kernel(ph_block_xplay s) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  if (!s.running[e]) return;
  BwTable t;
  bw_load(t, s.variant, s.state, e);
  const int A = bw_alt_act_len(s.variant);
  int a[3] = {s.alt_actions[(size_t)e * A], s.alt_actions[(size_t)e * A + 1], s.variant ? s.alt_actions[(size_t)e * A + 2] : 0};
  bw_alt_step(t, s.variant, a);
  bw_store(t, s.variant, s.state, e);
  bw_write_ego_obs(t, s.variant, s.obs_ego + (size_t)e * bw_ego_obs_len(s.variant));
}
hipError_t launch_block_xp_after_ego(const ph_block_xplay& s, unsigned long long counter, const unsigned long long* epoch, hipStream_t st) {
  hipLaunchKernelGGL(block_xp_after_ego_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s, (uint64_t)counter, epoch);
  return hipGetLastError();
}
hipError_t launch_block_xp_after_alt(const ph_block_xplay& s, hipStream_t st) {
  hipLaunchKernelGGL(block_xp_after_alt_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s);
  return hipGetLastError();
}

// ---- the partner pool: ego forward | after_ego | bucket pass + grouped constructor forward (+ scripted rows) | after_alt ---------
// The self-play kernels' lane logic with PoolBook (ph_pool.h) in place of the single learner's seat: the member that holds the
// constructor's seat of table e is partnerid[e], resampled where the table's game ends -- under the counter of the table's next
// world, epoch word included, so that ph_episode_stats replays it.  One lane per table; a pass loads each flag once at its top
// (ph_liar_step.h) -- the book's cursor behind a deal is the NEW member's, a second load by necessity.
//
// after_ego: the token is played, the member that has acted in this game is credited, the ego's reward row / episode flag / the
// episode count follow; a finished table gets its next world, PoolBook::on_deal (alt_acted cleared, the next member bound) and its
// planner observation, a running one the constructor's observation.  prepare states what the seat's forward records: nothing in a
// finished table.  first != 0 (the constructor's call): nothing is played -- world counter 0, a resample under counter 0, the
// planner's observation.
__global__ void block_pool_after_ego_kernel(ph_block_pool s, PoolBook book, float* ego_rew_row, uint64_t counter,
                                            const unsigned long long* __restrict__ epoch, int first) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  PoolBook::Lane b = book.load(e);
  BwTable t;
  bool done = true;
  if (!first) {
    bw_load(t, s.variant, s.state, e);
    const BwOutcome o = bw_ego_step(t, s.variant, s.ego_actions[e]);
    done = o.done;
    book.credit(b, e, o.reward, o.done, book.acted(b));
    liar_add_f32(ego_rew_row + e, o.reward);
    s.ego_episode_start[e] = o.done ? 1.f : 0.f;
    if (o.done) atomicAdd(s.episodes, 1ull);
  }
  s.done[e] = (done && !first) ? 1 : 0;
  s.running[e] = done ? 0 : 1;
  if (done) {
    const uint64_t c = bw_counter(first ? 0ull : counter, epoch);
    bw_reset(t, s.variant, s.world_seed, c, (uint32_t)e, BW_MAX_DRAWS);
    book.on_deal(b, e, c);
    bw_write_ego_obs(t, s.variant, s.obs_ego + (size_t)e * bw_ego_obs_len(s.variant));
  } else {
    bw_write_alt_obs(t, s.variant, s.obs_alt + (size_t)e * bw_alt_obs_len(s.variant));
  }
  bw_store(t, s.variant, s.state, e);
  book.prepare(b, e, !done);
}
// after_alt: where the game goes on the member's forward is committed (a non-learner only marks alt_acted), its move is played and
// the planner sees the result
__global__ void block_pool_after_alt_kernel(ph_block_pool s, PoolBook book) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n) return;
  if (!s.running[e]) return;
  PoolBook::Lane b = book.load(e);
  BwTable t;
  bw_load(t, s.variant, s.state, e);
  book.commit(b, e);
  const int A = bw_alt_act_len(s.variant);
  int a[3] = {s.alt_actions[(size_t)e * A], s.alt_actions[(size_t)e * A + 1], s.variant ? s.alt_actions[(size_t)e * A + 2] : 0};
  bw_alt_step(t, s.variant, a);
  bw_store(t, s.variant, s.state, e);
  bw_write_ego_obs(t, s.variant, s.obs_ego + (size_t)e * bw_ego_obs_len(s.variant));
}
hipError_t launch_block_pool_after_ego(const ph_block_pool& s, const PoolBook& book, float* ego_rew_row, unsigned long long counter,
                                       const unsigned long long* epoch, int first, hipStream_t st) {
  hipLaunchKernelGGL(block_pool_after_ego_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s, book, ego_rew_row, (uint64_t)counter,
                     epoch, first);
  return hipGetLastError();
}
hipError_t launch_block_pool_after_alt(const ph_block_pool& s, const PoolBook& book, hipStream_t st) {
  hipLaunchKernelGGL(block_pool_after_alt_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s, book);
  return hipGetLastError();
}

}  // namespace ph
