// The two block worlds (pantheonrl/envs/blockworldgym: blockworld.py:34-83, simpleblockworld.py:36-131, gridutils.py:8-64) as
// __host__ __device__ functions of one table's packed state: what the per-call kernels and the self-play book-keeping run with
// one lane per table (ph_block.hip) and what ph_block_replay_host runs on the CPU (ph_abi.hip) -- one text, so the rules are
// pinned to the reference's traces where there is no GPU.
//
// A table is PH_BLOCK_STATE_WORDS = 12 int32 words (48 bytes, moved as three 16-byte accesses):
//   variant 1 (BlockEnv-v1)  words 0-3 the target grid, words 4-7 the built grid: 49 two-bit cells, row major (row 0 = top),
//                            16 per word; a lane holds a grid as two 64-bit halves (cells 0-31, 32-48), so gravity reads the
//                            column tops by shifts -- no 49-entry private array that would live in scratch
//   variant 0 (BlockEnv-v0)  words 0-4 the five true blocks (orientation | y << 1 | x << 4 | colour << 7), word 5 the
//                            constructor's five colours, two bits each (its blocks differ from the true ones in colour only)
//   both                     word 8 the planner's last token; the other words are zero
#pragma once
#include "ph_launch.h"

namespace ph {

constexpr int BW_GRID = 7, BW_CELLS = 49, BW_BLOCKS = 5, BW_WORDS = PH_BLOCK_STATE_WORDS;
// world generation: one Philox block per draw (slot = draw number); after this many draws in total the blocks still missing are
// placed deterministically (first position that fits, colour 1), so the loop is bounded
constexpr int BW_MAX_DRAWS = 64;

__host__ __device__ inline int bw_tokens(int variant) { return variant ? 30 : 16; }
__host__ __device__ inline int bw_ego_obs_len(int variant) { return variant ? 2 * BW_CELLS : 8 * BW_BLOCKS; }
__host__ __device__ inline int bw_alt_obs_len(int variant) { return variant ? 1 + BW_CELLS : 1 + 4 * BW_BLOCKS; }
__host__ __device__ inline int bw_alt_act_len(int variant) { return variant ? 3 : 2; }

struct BwGrid {
  uint64_t lo, hi;   // cells 0-31, cells 32-48
};
struct BwTable {
  BwGrid target, built;    // variant 1
  uint32_t block[BW_BLOCKS];   // variant 0: true blocks
  uint32_t view;               // variant 0: constructor's colours
  int token;
};

__host__ __device__ inline int bw_cell(const BwGrid& g, int k) {
  return (int)((k < 32 ? g.lo >> (2 * k) : g.hi >> (2 * (k - 32))) & 3ull);
}
__host__ __device__ inline void bw_set_cell(BwGrid& g, int k, int c) {
  if (k < 32) g.lo |= (uint64_t)c << (2 * k);
  else g.hi |= (uint64_t)c << (2 * (k - 32));
}
// smallest occupied row of column x, BW_GRID when the column is empty
__host__ __device__ inline int bw_top(const BwGrid& g, int x) {
  int top = BW_GRID;
#pragma unroll
  for (int y = BW_GRID - 1; y >= 0; --y) top = bw_cell(g, y * BW_GRID + x) ? y : top;
  return top;
}
// gridutils.gravity: resting row of a block dropped in column x (horizontal: x <= 5), -1 when its entry cells are taken
__host__ __device__ inline int bw_gravity(const BwGrid& g, int vertical, int x) {
  const int t0 = bw_top(g, x);
  if (vertical) return t0 <= 1 ? -1 : t0 - 2;
  const int t1 = bw_top(g, x + 1);
  const int t = t0 < t1 ? t0 : t1;
  return t == 0 ? -1 : t - 1;
}
__host__ __device__ inline void bw_place(BwGrid& g, int x, int y, int colour, int vertical) {
  bw_set_cell(g, y * BW_GRID + x, colour);
  bw_set_cell(g, vertical ? (y + 1) * BW_GRID + x : y * BW_GRID + x + 1, colour);
}
// a drop as alt_step and the world generator make it; false = nothing happened
__host__ __device__ inline bool bw_drop(BwGrid& g, int x, int vertical, int colour) {
  if (x < 0 || x >= BW_GRID || (!vertical && x == BW_GRID - 1)) return false;
  const int y = bw_gravity(g, vertical, x);
  if (y < 0) return false;
  bw_place(g, x, y, colour, vertical);
  return true;
}

__host__ __device__ inline void bw_unpack(BwTable& t, int variant, const int* w) {
  const uint32_t* u = reinterpret_cast<const uint32_t*>(w);
  t.target.lo = (uint64_t)u[0] | (uint64_t)u[1] << 32;
  t.target.hi = (uint64_t)u[2] | (uint64_t)u[3] << 32;
  t.built.lo = (uint64_t)u[4] | (uint64_t)u[5] << 32;
  t.built.hi = (uint64_t)u[6] | (uint64_t)u[7] << 32;
#pragma unroll
  for (int i = 0; i < BW_BLOCKS; ++i) t.block[i] = u[i];
  t.view = u[5];
  t.token = w[8];
  (void)variant;
}
__host__ __device__ inline void bw_pack(const BwTable& t, int variant, int* w) {
  uint32_t* u = reinterpret_cast<uint32_t*>(w);
  if (variant) {
    u[0] = (uint32_t)t.target.lo; u[1] = (uint32_t)(t.target.lo >> 32); u[2] = (uint32_t)t.target.hi; u[3] = (uint32_t)(t.target.hi >> 32);
    u[4] = (uint32_t)t.built.lo; u[5] = (uint32_t)(t.built.lo >> 32); u[6] = (uint32_t)t.built.hi; u[7] = (uint32_t)(t.built.hi >> 32);
  } else {
#pragma unroll
    for (int i = 0; i < BW_BLOCKS; ++i) u[i] = t.block[i];
    u[5] = t.view;
    u[6] = 0; u[7] = 0;
  }
  w[8] = t.token;
  w[9] = 0; w[10] = 0; w[11] = 0;
}

// ---- variant 0: the block list -------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t bw_make_block(int o, int y, int x, int c) { return (uint32_t)(o | y << 1 | x << 4 | c << 7); }
// the two cells of a block as a 49-bit occupancy mask
__host__ __device__ inline uint64_t bw_block_mask(uint32_t b) {
  const int o = b & 1, y = (b >> 1) & 7, x = (b >> 4) & 7;
  const int k = y * BW_GRID + x;
  return 1ull << k | 1ull << (o ? k + BW_GRID : k + 1);
}

// ---- reset: a fresh world from the Philox stream keyed (seed, counter, table, draw) ----------------------------------------
// One draw = one Philox block: words 0 orientation, 1 column, 2 row (variant 0 only), 3 colour -- the reference's draw order; a
// draw that does not fit is discarded and the next one taken, max_draws draws at most (BW_MAX_DRAWS on the device).
__host__ __device__ inline int bw_pick(float u, int n) {
  const int v = (int)(u * (float)n);
  return v >= n ? n - 1 : v;
}
__host__ __device__ inline void bw_reset(BwTable& t, int variant, uint64_t seed, uint64_t counter, uint32_t table, int max_draws) {
  t.target = BwGrid{0ull, 0ull};
  t.built = BwGrid{0ull, 0ull};
  t.view = 0u;
  t.token = 0;
#pragma unroll
  for (int i = 0; i < BW_BLOCKS; ++i) t.block[i] = 0u;
  int placed = 0;
  uint64_t taken = 0ull;    // variant 0: occupied cells
  for (int draw = 0; draw < max_draws && placed < BW_BLOCKS; ++draw) {
    float u[4];
    philox_uniform4(seed, counter, table, (uint32_t)draw, u);
    const int vertical = bw_pick(u[0], 2);
    const int colour = bw_pick(u[3], 2) + 1;
    if (variant) {
      const int x = bw_pick(u[1], vertical ? BW_GRID : BW_GRID - 1);
      if (bw_drop(t.target, x, vertical, colour)) ++placed;
    } else {
      const int x = bw_pick(u[1], vertical ? BW_GRID : BW_GRID - 1);
      const int y = bw_pick(u[2], vertical ? BW_GRID - 1 : BW_GRID);
      const uint32_t b = bw_make_block(vertical, y, x, colour);
      const uint64_t m = bw_block_mask(b);
      if (taken & m) continue;
      taken |= m;
#pragma unroll
      for (int i = 0; i < BW_BLOCKS; ++i) t.block[i] = (i == placed) ? b : t.block[i];
      ++placed;
    }
  }
  // the bounded fall-back.  Variant 1: a vertical block in the first column that takes one -- four blocks cannot close the top two
  // rows of all seven columns.  Variant 0: the first free horizontal pair in row-major order -- eight cells cannot break all 42.
  // (every sweep over the columns places at least one block, so BW_BLOCKS sweeps are enough)
  if (variant) {
    for (int sweep = 0; sweep < BW_BLOCKS; ++sweep)
      for (int x = 0; x < BW_GRID && placed < BW_BLOCKS; ++x)
        if (bw_drop(t.target, x, 1, 1)) ++placed;
    return;
  }
  for (int p = 0; p < BW_CELLS && placed < BW_BLOCKS; ++p) {
    const int y = p / BW_GRID, x = p - y * BW_GRID;
    if (x == BW_GRID - 1) continue;
    const uint32_t b = bw_make_block(0, y, x, 1);
    const uint64_t m = bw_block_mask(b);
    if (taken & m) continue;
    taken |= m;
#pragma unroll
    for (int i = 0; i < BW_BLOCKS; ++i) t.block[i] = (i == placed) ? b : t.block[i];
    ++placed;
  }
}

// ---- the two moves -----------------------------------------------------------------------------------------------------------
struct BwOutcome {
  float reward;   // paid to both seats
  bool done;
};
__host__ __device__ inline int bw_popcount64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}
// one bit per two-bit cell: set where the cell is not zero
__host__ __device__ inline uint64_t bw_nonzero(uint64_t g) { return (g | g >> 1) & 0x5555555555555555ull; }
// ego_step: the token is stored; the last token ends the game and pays
__host__ __device__ inline BwOutcome bw_ego_step(BwTable& t, int variant, int token) {
  t.token = token;
  if (token != bw_tokens(variant) - 1) return BwOutcome{0.f, false};
  if (variant) {
    // F1 = 2 tp / (selected + relevant): tp = cells that are non-zero and equal in both grids
    const uint64_t dlo = t.built.lo ^ t.target.lo, dhi = t.built.hi ^ t.target.hi;
    const uint64_t eqlo = ~(dlo | dlo >> 1) & 0x5555555555555555ull, eqhi = ~(dhi | dhi >> 1) & 0x5555555555555555ull;
    const int tp = bw_popcount64(eqlo & bw_nonzero(t.built.lo)) + bw_popcount64(eqhi & bw_nonzero(t.built.hi));
    const int selected = bw_popcount64(bw_nonzero(t.built.lo)) + bw_popcount64(bw_nonzero(t.built.hi));
    const int relevant = bw_popcount64(bw_nonzero(t.target.lo)) + bw_popcount64(bw_nonzero(t.target.hi));
    return BwOutcome{(float)(2 * tp) / (float)(selected + relevant), true};   // one correctly rounded division
  }
  int correct = 0;
#pragma unroll
  for (int i = 0; i < BW_BLOCKS; ++i) correct += ((t.block[i] >> 7) & 3u) == ((t.view >> (2 * i)) & 3u) ? 1 : 0;
  return BwOutcome{(float)(20 * correct), true};   // 100 * correct / 5
}
// alt_step: a (actions of bw_alt_act_len ints).  Variant 1 (x, orientation, colour - 1): a drop, nothing when it does not fit.
// Variant 0 (block, colour): recolour the constructor's block.  Out-of-range components (a categorical head gives none) change nothing.
__host__ __device__ inline void bw_alt_step(BwTable& t, int variant, const int* a) {
  if (variant) {
    if (a[1] < 0 || a[1] > 1 || a[2] < 0 || a[2] > 1) return;
    (void)bw_drop(t.built, a[0], a[1], a[2] + 1);
  } else {
    if (a[0] < 0 || a[0] >= BW_BLOCKS || a[1] < 0 || a[1] > 2) return;
    t.view = (t.view & ~(3u << (2 * a[0]))) | (uint32_t)a[1] << (2 * a[0]);
  }
}

// ---- observations (get_obs): raw integer components as floats, the form the policy kernels one-hot ----------------------------
__host__ __device__ inline void bw_write_grid(const BwGrid& g, float* o) {
#pragma unroll
  for (int k = 0; k < BW_CELLS; ++k) o[k] = (float)bw_cell(g, k);
}
__host__ __device__ inline void bw_write_blocks(const BwTable& t, bool true_colours, float* o) {
#pragma unroll
  for (int i = 0; i < BW_BLOCKS; ++i) {
    const uint32_t b = t.block[i];
    o[4 * i] = (float)(b & 1u);
    o[4 * i + 1] = (float)((b >> 1) & 7u);
    o[4 * i + 2] = (float)((b >> 4) & 7u);
    o[4 * i + 3] = (float)(true_colours ? (b >> 7) & 3u : (t.view >> (2 * i)) & 3u);
  }
}
// planner: target then built (98) / true blocks then the constructor's view (40)
__host__ __device__ inline void bw_write_ego_obs(const BwTable& t, int variant, float* o) {
  if (variant) {
    bw_write_grid(t.target, o);
    bw_write_grid(t.built, o + BW_CELLS);
  } else {
    bw_write_blocks(t, true, o);
    bw_write_blocks(t, false, o + 4 * BW_BLOCKS);
  }
}
// constructor: last token then the built grid (50) / its view of the blocks (21)
__host__ __device__ inline void bw_write_alt_obs(const BwTable& t, int variant, float* o) {
  o[0] = (float)t.token;
  if (variant) bw_write_grid(t.built, o + 1);
  else bw_write_blocks(t, false, o + 1);
}

// ---- the scripted constructors (envs/blockworld.py: DefaultConstructorAgent, SBWDefaultAgent, SBWEasyPartner) --------------------
// One function of a constructor observation row o (bw_alt_obs_len floats) and a rule; a[] gets bw_alt_act_len ints (a[2] = 0 for
// variant 0).  Integer rules, the reference's quirks included:
//   variant 1, DEFAULT  token - 1 = 4 x + 2 orientation + colour; the first and the last token get (6, vertical, blue)
//   variant 0, DEFAULT  tokens 1-7 / 8-14 name a grid row: the first still uncoloured block met along it (a cell covered twice
//                       belongs to the later block) turns red / blue; a red-range token whose row is done looks at row token - 8,
//                       counted from the bottom, for a block to turn blue; otherwise the pass move (0, colour of block 0)
//   variant 0, EASY     tokens above 10 are halved; 1-5 turn block token - 1 red, 6-10 block token - 8 blue.  The host agent answers
//                       the negative index -2 / -1 for tokens 6 / 7 (and 12-15), which the host game reads from the end of its
//                       list; here the index is given modulo BW_BLOCKS (3 / 4): the move the host game makes, inside the action space
constexpr int BW_RULE_DEFAULT = PH_BLOCK_RULE_DEFAULT, BW_RULE_EASY = PH_BLOCK_RULE_EASY;
// SBWDefaultAgent.first_uncoloured: `row` as a Python index into the seven grid rows (negative: from the bottom)
__host__ __device__ inline int bw_first_uncoloured(const float* o, int row) {
  if (row < 0) row += BW_GRID;
  for (int x = 0; x < BW_GRID; ++x) {
    int owner = -1;
#pragma unroll
    for (int i = 0; i < BW_BLOCKS; ++i) {
      const int v = (int)o[1 + 4 * i], y = (int)o[2 + 4 * i], bx = (int)o[3 + 4 * i];
      const bool covers = (y == row && bx == x) || (v ? (y + 1 == row && bx == x) : (y == row && bx + 1 == x));
      owner = covers ? i : owner;
    }
    if (owner < 0) continue;
    int colour = 0;
#pragma unroll
    for (int i = 0; i < BW_BLOCKS; ++i) colour = (i == owner) ? (int)o[4 + 4 * i] : colour;
    if (colour == 0) return owner;
  }
  return -1;
}
__host__ __device__ inline void bw_scripted_move(int variant, int rule, const float* o, int* a) {
  int token = (int)o[0];
  a[2] = 0;
  if (variant) {
    if (token <= 0 || token >= bw_tokens(1) - 1) {
      a[0] = BW_GRID - 1; a[1] = 1; a[2] = 0;
      return;
    }
    const int t = token - 1;
    a[0] = t / 4; a[1] = (t / 2) % 2; a[2] = t % 2;
    return;
  }
  a[0] = 0;
  a[1] = (int)o[4];   // the pass move: block 0 keeps its colour
  if (rule == BW_RULE_EASY) {
    if (token > 10) token /= 2;
    if (token >= 1 && token <= 5) { a[0] = token - 1; a[1] = 2; }
    else if (token >= 6 && token <= 10) { a[0] = (token - 8 + BW_BLOCKS) % BW_BLOCKS; a[1] = 1; }
    return;
  }
  if (token <= 0) return;
  if (token <= 7) {
    const int i = bw_first_uncoloured(o, token - 1);
    if (i >= 0) { a[0] = i; a[1] = 2; return; }
  }
  if (token <= 14) {
    const int i = bw_first_uncoloured(o, token - 8);
    if (i >= 0) { a[0] = i; a[1] = 1; }
  }
}

// ---- launchers (ph_block.hip) ----------------------------------------------------------------------------------------------------
hipError_t launch_block_scripted_actions(int variant, int rule, const float* obs, const unsigned char* active, int* actions, int n,
                                         hipStream_t s);
// the scripted members' rows of a grouped forward: one lane per table, which reads its member from the device-side member table
// (ph_pool.h; a scripted member's `rb_T` word holds its rule) and moves where the table is active and that member is scripted
struct PoolMemberDev;
hipError_t launch_block_group_scripted(int variant, const float* obs, const PoolMemberDev* members, const int* member_of,
                                       const unsigned char* active, int* actions, int n, int K, hipStream_t s);
hipError_t launch_block_xp_after_ego(const ph_block_xplay& s, unsigned long long counter, const unsigned long long* epoch, hipStream_t st);
hipError_t launch_block_xp_after_alt(const ph_block_xplay& s, hipStream_t st);
// the partner-pool step's two book-keeping launches (ph_pool.h: PoolBook is seat 1's book; first: the constructor's call, no token)
struct PoolBook;
hipError_t launch_block_pool_after_ego(const ph_block_pool& s, const PoolBook& book, float* ego_rew_row, unsigned long long counter,
                                       const unsigned long long* epoch, int first, hipStream_t st);
hipError_t launch_block_pool_after_alt(const ph_block_pool& s, const PoolBook& book, hipStream_t st);
hipError_t launch_block_reset(int variant, int* state, const unsigned char* reset_mask, unsigned long long seed,
                              unsigned long long counter, const unsigned long long* epoch, int n, hipStream_t s);
hipError_t launch_block_step(int variant, int* state, const int* actions, int is_ego, const unsigned char* active, float* obs_next,
                             float* rewards, unsigned char* done, int n, hipStream_t s);
hipError_t launch_block_obs(int variant, const int* state, int is_ego, const unsigned char* active, float* obs_out, int n,
                            hipStream_t s);
hipError_t launch_block_sp_after_ego(const ph_block_selfplay& s, float* ego_rew_row, unsigned long long counter,
                                     const unsigned long long* epoch, hipStream_t st);
hipError_t launch_block_sp_after_alt(const ph_block_selfplay& s, hipStream_t st);

}  // namespace ph
