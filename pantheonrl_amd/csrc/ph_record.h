// A move log of the vectorised Liar's Dice step that lives on the device: the rows TurnBasedRecorder (common/wrappers.py) would
// have produced for each table -- [obs 30 | action 2 | flag], flag = EGO_NOT_DONE 0, ALT_NOT_DONE 1, EGO_DONE 2, ALT_DONE 3 --
// filled between the launches of ph_liar_step.h's protocol by two launches of their own, one lane per table:
//   seat-0 forward | after_ego | seat-1 forward (reply) | RECORD A | after_reply | seat-1 forward (openers) | RECORD B | after_opening
// A: the ego's row (obs_ego, ego_actions, done1) and, where `running`, the reply's row (obs_next as after_ego left it,
//    alt_actions) with a provisional flag; the reply's row index is remembered in pending[e].  It runs before after_reply
//    overwrites obs_next / obs_ego and before the opening forward overwrites alt_actions.
// B: the pending reply's flag from done2 (after_reply wrote it; after_opening overwrites it in re-dealt tables), then seat 1's
//    opening row (obs_alt, alt_actions) where alt_opens -- flag ALT_NOT_DONE: an opening never ends a game.  It reads who sits at
//    seat 1 AFTER after_reply's resample, so the opening belongs to the newly seated member.  A deal-only call runs B alone.
// The recorder only reads the step's arrays; the passes know nothing of it.  Table e owns rows[e], count[e], count_alt[e] (the
// rows of seat 1 among them), dropped[e] and pending[e]; a move that finds the table full is dropped and counted, so a table's
// log stays a prefix of its stream.
#pragma once
#include "ph_launch.h"

namespace ph {

constexpr int REC_OBS = 30, REC_ACT = 2, REC_ROW = REC_OBS + REC_ACT + 1;
constexpr int REC_EGO_NOT_DONE = 0, REC_ALT_NOT_DONE = 1;   // + 2: that move ended the game

struct RecordLog {
  int n, cap;
  float* rows;      // (n, cap, REC_ROW)
  int* member;      // (n, cap) who moved, or null
  int* count;       // (n) rows logged
  int* count_alt;   // (n) ... of which seat 1's
  int* dropped;     // (n) moves that found the table full
  int* pending;     // (n) row of the reply that waits for its flag, -1: none
};
// what the recorder reads of a step: the game's arrays, and who sits where (null: member 0; `playing` null: every table plays)
struct RecordStep {
  const float *obs_ego, *obs_alt, *obs_next;
  const int *ego_actions, *alt_actions;
  const unsigned char *done1, *done2, *running, *alt_opens;
  const int *ego_id, *alt_id;
  const unsigned char* playing;
};

hipError_t launch_record_moves(const RecordLog& log, const RecordStep& s, hipStream_t st);      // A
hipError_t launch_record_opening(const RecordLog& log, const RecordStep& s, hipStream_t st);    // B
// seat: -1 every row, 0 / 1 that seat's rows (flag % 2).  offsets (n + 1) int64 = exclusive scan of the selected counts; then --
// rows_out non-null -- the selected rows, table-major, each table's in its own order, into rows_out (out_cap, REC_ROW) and
// member_out (out_cap) (either member side may be null); a row at or past out_cap is not written.
hipError_t launch_record_export(const RecordLog& log, int seat, long long* offsets, float* rows_out, int* member_out,
                                long long out_cap, hipStream_t st);

}  // namespace ph
