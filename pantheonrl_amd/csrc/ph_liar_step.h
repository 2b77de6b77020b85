// The vectorised Liar's Dice step, written once: what runs between the policy forwards of
//   seat-0 forward | after_ego | seat-1 forward (reply) | after_reply (ends of games, re-deal) | seat-1 forward (openers) | after_opening
// as lane functions (one lane per table, ph_liar.h's rules) over two small policy types:
//   a BOOK     what seat 1 keeps of table e -- one learner's cursor (LearnerBook, self-play), the cursor of the pool member that
//              sits there, resampled at the deal (PoolBook, ph_pool.h), or nothing (NoBook, cross-play);
//   a GAME END what the end of a game means -- training adds to the ego's reward row, flags the episode start and counts episodes
//              (TrainEnd); evaluation gates on `playing`, accumulates return and length, logs the game, spends the budget and
//              retires the table (EvalEnd, ph_xplay.h).
// Self-play = <LearnerBook, TrainEnd>, the pool = <PoolBook, TrainEnd>, cross-play = <NoBook, EvalEnd>: three kernels per pass
// (ph_envs.hip), no run-time mode in any of them.  (The persistent rollout runs the self-play instantiation with a table spread
// over 32 lanes, ph_liar_group.h, where these lanes go by their earlier names liar_sp_after_ego_lane / _reply_lane / _opening_lane.)
//
// Memory order is part of the behaviour (ph_liar.h): a pass loads every flag it needs ONCE, at its top -- the book's, the game
// end's, the game's, all independent: one round trip, and in front of the game end's early-out -- carries them in registers and
// never reads one back behind a store or behind the late-reward atomic.
#pragma once
#include "ph_liar.h"

namespace ph {

// the game as the lanes see it: what all three modes share, filled once on the host from whichever public description came in
struct LiarGame {
  int n;
  int *hands, *history, *nmoves;
  unsigned char* ego_first;
  unsigned long long dice_seed;
  float probegostart;
  const int *ego_actions, *alt_actions;
  float *obs_ego, *obs_alt, *obs_next, *rew1, *rew2;
  unsigned char *done1, *done2, *running, *alt_opens, *ego_opens, *done;
};
template <class Desc>   // ph_liar_selfplay, ph_liar_pool, ph_liar_xplay
inline LiarGame liar_game_of(const Desc& s) {
  return LiarGame{s.n,       s.hands,   s.history,  s.nmoves, s.ego_first, s.dice_seed, s.probegostart, s.ego_actions, s.alt_actions,
                  s.obs_ego, s.obs_alt, s.obs_next, s.rew1,   s.rew2,      s.done1,     s.done2,        s.running,     s.alt_opens,
                  s.ego_opens, s.done};
}

// ---- books ---------------------------------------------------------------------------------------------------------------------
// A book's Lane is its state of table e in registers.  load: at the top of a pass -- or in its two halves, seat (who sits at
// the table: the addresses of its cursor) and cursor (the cursor itself).  acted: seat 1 has moved in this game.
// credit: a reward / an end that follows seat 1's last forward.  commit: seat 1's forward ran (b.can: it recorded a row).
// prepare: what its next forward records.  on_deal: the table was re-dealt with dice counter c.

// the partner-seat fields ph_liar.h's LiarSeat helpers work on, bound to one learner
struct SeatFields {
  int n;
  int* alt_pos;
  unsigned char *alt_boundary, *alt_term, *alt_open, *alt_acted, *can;
  float* es_alt;
};
struct LearnerBook {
  SeatFields v;
  float* rewards;   // the learner's ragged buffer
  int T;
  struct Lane {
    LiarSeat q;
    bool can;
  };
  __device__ __forceinline__ Lane load(int e) const { return Lane{liar_seat_load(v, e), v.can[e] != 0}; }
  __device__ __forceinline__ Lane seat(int e) const { return load(e); }   // one learner: the addresses are the arguments
  __device__ __forceinline__ void cursor(Lane&, int) const {}
  __device__ __forceinline__ bool acted(const Lane& b) const { return b.q.acted; }
  __device__ __forceinline__ void credit(Lane& b, int e, float r, bool done, bool credited) const {
    liar_sp_credit(v, b.q, rewards, T, e, r, done, credited);
  }
  __device__ __forceinline__ void commit(Lane& b, int e) const { liar_sp_commit(v, b.q, e, b.can); }
  __device__ __forceinline__ void prepare(const Lane& b, int e, bool requested) const { liar_sp_prepare(v, b.q, T, e, requested); }
  __device__ __forceinline__ void on_deal(Lane&, int e, uint64_t) const { v.alt_acted[e] = 0; }
};
// frozen and scripted players keep no book: nothing is loaded and nothing written, not even can / es_alt
struct NoBook {
  struct Lane {};
  __device__ __forceinline__ Lane load(int) const { return Lane{}; }
  __device__ __forceinline__ Lane seat(int) const { return Lane{}; }
  __device__ __forceinline__ void cursor(Lane&, int) const {}
  __device__ __forceinline__ bool acted(const Lane&) const { return false; }
  __device__ __forceinline__ void credit(Lane&, int, float, bool, bool) const {}
  __device__ __forceinline__ void commit(Lane&, int) const {}
  __device__ __forceinline__ void prepare(const Lane&, int, bool) const {}
  __device__ __forceinline__ void on_deal(Lane&, int, uint64_t) const {}
};

// ---- game ends -----------------------------------------------------------------------------------------------------------------
// load: the table's accounting, at the top of a pass.  plays: the table takes part in the pass.  account: the ego's reward of
// this step (both transitions, agents.py:44-47) and whether its game ended.  finish: the end of the game; true = the table
// retired and the pass is over for it.
struct TrainEnd {
  float* ego_rew_row;          // row ego_pos of the ego's rectangular buffer (null in a deal-only call)
  float* ego_episode_start;
  unsigned long long* episodes;
  struct Acc {};
  __device__ __forceinline__ Acc load(int) const { return Acc{}; }
  __device__ __forceinline__ bool plays(const Acc&) const { return true; }
  __device__ __forceinline__ void account(Acc&, int e, float r, bool done) const {
    liar_add_f32(ego_rew_row + e, r);
    ego_episode_start[e] = done ? 1.f : 0.f;
  }
  __device__ __forceinline__ bool finish(Acc&, const LiarGame&, int, bool done) const {
    if (done) atomicAdd(episodes, 1ull);
    return false;
  }
};

// ---- the three passes ----------------------------------------------------------------------------------------------------------
// seat 0 has moved (its forward wrote ego_actions): play the move, credit seat 1 where it already acted this game, find the
// tables that go on and prepare seat 1's reply there
template <class Book, class End>
__device__ __forceinline__ void liar_after_ego_lane(const LiarGame& g, const Book& book, const End& end, int e) {
  if (!end.plays(end.load(e))) return;   // idle: running[e] was cleared when the table retired
  typename Book::Lane b = book.seat(e);
  LiarTable t;
  liar_load(t, e, g.hands, g.history, g.nmoves);
  const LiarOutcome o1 = liar_move(t, e, g.history, g.nmoves, g.ego_actions, true, g.obs_next, g.rew1, g.done1);
  book.cursor(b, e);   // needed from here on: a cursor that hangs on dependent loads (the pool's) arrives while the move's stores drain
  book.credit(b, e, o1.r_alt, o1.done, book.acted(b));
  g.running[e] = o1.done ? 0 : 1;
  book.prepare(b, e, !o1.done);
}
// seat 1 has replied where the game went on: play that move, credit both seats, seat 0's next observation, the end of the game;
// then (also the whole of a deal-only call, for the tables flagged in `done`) re-deal the finished tables, find who opens the
// new games and prepare seat 1's opening forward.  The context's RNG epoch word, when one is attached, is the dice counter's
// high half (as in ph_liar_reset).
template <class Book, class End>
__device__ __forceinline__ void liar_after_reply_lane(const LiarGame& g, const Book& book, const End& end, int e, uint64_t counter,
                                                      const unsigned long long* epoch, int deal_only) {
  typename End::Acc a = end.load(e);
  const bool run = g.running[e] != 0, d1 = g.done1[e] != 0;
  const float r1_ego = g.rew1[2 * e];
  bool ego_first = g.ego_first[e] != 0;    // of the game in progress; a re-deal below replaces it
  bool fresh = g.done[e] != 0;             // a deal-only call: the caller's flags
  if (!end.plays(a)) return;
  LiarTable t;
  liar_load(t, e, g.hands, g.history, g.nmoves);
  typename Book::Lane b = book.load(e);
  if (!deal_only) {
    LiarOutcome o2{0.f, 0.f, false};
    if (run) {
      book.commit(b, e);
      o2 = liar_move(t, e, g.history, g.nmoves, g.alt_actions, false, g.obs_next, g.rew2, g.done2);
    }
    const bool d2 = run && o2.done;
    book.credit(b, e, o2.r_alt, d2, run);
    const bool done = d1 || d2;
    end.account(a, e, r1_ego + (run ? o2.r_ego : 0.f), done);
    if (run && !d2) liar_write_obs(t, true, g.obs_ego + (size_t)e * 30);   // = obs_next of the move just played
    g.done[e] = done ? 1 : 0;
    fresh = done;
    if (end.finish(a, g, e, done)) return;
  }
  if (fresh) {
    const uint64_t c = counter + (epoch ? (uint64_t)(*epoch) << 32 : 0ull);
    ego_first = liar_deal(t, e, g.hands, g.history, g.nmoves, g.ego_first, g.dice_seed, c, g.probegostart);
    book.on_deal(b, e, c);
  }
  g.alt_opens[e] = (fresh && !ego_first) ? 1 : 0;
  g.ego_opens[e] = (fresh && ego_first) ? 1 : 0;
  book.prepare(b, e, fresh && !ego_first);
  if (fresh && !ego_first) liar_write_obs(t, false, g.obs_alt + (size_t)e * 30);
}
// seat 1 has opened the new games it starts: play that move; seat 0's observation of every fresh table (a retired table's
// flags are both clear)
template <class Book>
__device__ __forceinline__ void liar_after_opening_lane(const LiarGame& g, const Book& book, int e) {
  const bool alt_opens = g.alt_opens[e] != 0, ego_opens = g.ego_opens[e] != 0;
  if (!alt_opens && !ego_opens) return;
  LiarTable t;
  liar_load(t, e, g.hands, g.history, g.nmoves);
  if (alt_opens) {
    typename Book::Lane b = book.load(e);
    book.commit(b, e);
    (void)liar_move(t, e, g.history, g.nmoves, g.alt_actions, false, g.obs_next, g.rew2, g.done2);
  }
  liar_write_obs(t, true, g.obs_ego + (size_t)e * 30);   // after seat 1's opening move, or of the fresh deal
}

// pass 0 / 1 / 2 = after_ego / after_reply / after_opening of one mode; instantiated for the three modes in ph_envs.hip
template <class Book, class End>
hipError_t launch_liar_pass(int pass, const LiarGame& g, const Book& book, const End& end, unsigned long long counter,
                            const unsigned long long* epoch, int deal_only, hipStream_t st);

}  // namespace ph
