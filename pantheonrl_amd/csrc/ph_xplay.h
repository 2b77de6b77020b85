// Cross-play evaluation of Liar's Dice (tester.py:41-63 over E tables): both seats of table e are held by members of ONE member table
// (ph_pool.h) -- seat 0 by ego_id[e], seat 1 by alt_id[e], fixed for the whole evaluation -- every table plays exactly G games, and
// every game's ego return and length go into a per-table log.  The seat forwards are the pool's bucket pass + grouped forward
// (indexed by ego_id or alt_id); this header holds the game end of what runs between them and the statistics reduction (ph_xplay.hip).
#pragma once
#include "ph_pool.h"

namespace ph {

// The end of a game in an evaluation (ph_liar_step.h; the book is NoBook: frozen and scripted members keep none, so the passes
// between the forwards need the game, the budget and the logs only).  A table takes part while `playing`; a step adds both
// transitions to the game's return (multiagentenv.py:201-202) and one to its length; the end of a game logs both at
// [e, games[e]], counts the game and -- budget spent -- retires the table: it leaves every later forward and pass.
struct EvalEnd {
  int G;
  int* games;                // (n) games finished
  unsigned char* playing;    // (n) 1 while games[e] < G: the idle mask's complement, the seat-0 forward's active mask
  int* tables_left;          // [1] tables with budget left
  float* ep_return;          // (n) ego return of the game in progress
  int* ep_length;            // (n) ego moves of the game in progress
  float* returns;            // (n, G)
  int* lengths;              // (n, G)
  struct Acc {
    bool playing;
    float ret;
    int len, g;
  };
  __device__ __forceinline__ Acc load(int e) const { return Acc{playing[e] != 0, ep_return[e], ep_length[e], games[e]}; }
  __device__ __forceinline__ bool plays(const Acc& a) const { return a.playing; }
  __device__ __forceinline__ void account(Acc& a, int, float r, bool) const {
    a.ret += r;
    a.len += 1;
  }
  __device__ __forceinline__ bool finish(Acc& a, const LiarGame& g, int e, bool done) const {
    if (done) {
      if (a.g >= 0 && a.g < G) {
        returns[(size_t)e * G + a.g] = a.ret;
        lengths[(size_t)e * G + a.g] = a.len;
      }
      a.g += 1;
      games[e] = a.g;
      a.ret = 0.f;
      a.len = 0;
    }
    ep_return[e] = a.ret;
    ep_length[e] = a.len;
    if (!(done && a.g >= G)) return false;
    playing[e] = 0;
    g.running[e] = 0;
    g.alt_opens[e] = 0;
    g.ego_opens[e] = 0;
    atomicSub(tables_left, 1);
    return true;
  }
};

constexpr int XPLAY_NSTAT = 4;   // count, sum, sum of squares, sum of lengths

hipError_t launch_xplay_stats(const float* returns, const int* lengths, const int* games, int n, int G, int n_pairs, double* stats,
                              hipStream_t st);

}  // namespace ph
