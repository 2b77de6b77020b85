// Cross-play evaluation of Liar's Dice (tester.py:41-63 over E tables): both seats of table e are held by members of ONE member table
// (ph_pool.h) -- seat 0 by ego_id[e], seat 1 by alt_id[e], fixed for the whole evaluation -- every table plays exactly G games, and
// every game's ego return and length go into a per-table log.  The seat forwards are the pool's bucket pass + grouped forward
// (indexed by ego_id or alt_id); this header holds what runs between them (ph_xplay.hip) and the statistics reduction.
#pragma once
#include "ph_pool.h"

namespace ph {

// the step's description as the book-keeping kernels take it.  No member sits in it: frozen and scripted members keep no book, so
// the passes between the forwards need the game, the budget and the logs only.
struct XplayStep {
  int n, G;
  int *hands, *history, *nmoves;
  unsigned char* ego_first;
  unsigned long long dice_seed;
  float probegostart;
  const int *ego_actions, *alt_actions;
  float *obs_ego, *obs_alt;
  int* games;                // (n) games finished
  unsigned char* playing;    // (n) 1 while games[e] < G: the idle mask's complement, the seat-0 forward's active mask
  int* tables_left;          // [1] tables with budget left
  float* ep_return;          // (n) ego return of the game in progress
  int* ep_length;            // (n) ego moves of the game in progress
  float* returns;            // (n, G)
  int* lengths;              // (n, G)
  float *obs_next, *rew1, *rew2;
  unsigned char *done1, *done2, *running, *alt_opens, *ego_opens, *done;
};

constexpr int XPLAY_NSTAT = 4;   // count, sum, sum of squares, sum of lengths

hipError_t launch_xplay_after_ego(const XplayStep& s, hipStream_t st);
hipError_t launch_xplay_after_reply(const XplayStep& s, unsigned long long counter, const unsigned long long* epoch, int deal_only,
                                    hipStream_t st);
hipError_t launch_xplay_after_opening(const XplayStep& s, hipStream_t st);
hipError_t launch_xplay_stats(const float* returns, const int* lengths, const int* games, int n, int G, int n_pairs, double* stats,
                              hipStream_t st);

}  // namespace ph
