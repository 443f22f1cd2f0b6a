// stage_times.h — the events of a slot by name, and what each shape of call reports in qtr_stage_times from them: plain
// data and integers, no HIP (tests/test_stage_times_cpu.py compiles it into a CPU program).
#pragma once

// Slot::ev (capi.hip).  A registration records them in this order on the slot's stream:
//   EV_BEGIN | voxel grids | EV_VOX | FPFH chain | EV_FPFH | matcher, gather | EV_MATCH | graph | EV_GRAPH | clique |
//   EV_CLIQUE | estimation | EV_SOLVE
// (the follow-up chains of a solve record EV_SOLVE again: solve_followup).
enum SlotEvent {
  EV_BEGIN = 0, EV_VOX, EV_GRAPH, EV_CLIQUE, EV_SOLVE,
  EV_JOIN2,  // no stage time: the second stream's work (means, clean slates) joins the slot's stream in front of the matcher
  EV_FPFH, EV_MATCH,
  EV_BE0,    // qtr_register_pair_corr, back end beside the front end: its start on the third stream
  EV_END,    // ... and the call's end on the slot's stream, behind the join of the third stream
  EV_COUNT,
  // The same events under the meaning other calls give them:
  EV_STAGED = EV_VOX,                  // qtr_solve: the correspondences are staged (no voxel stage)
  EV_STAGE_BEGIN = EV_BEGIN,           // a call that is ONE stage (qtr_voxelize, qtr_fpfh, qtr_match, qtr_patchwork,
  EV_STAGE_END = EV_VOX,               // qtr_segment_cloud and the batch pre-processing built from the last two)
  EV_ICP_BEGIN = EV_BEGIN, EV_ICP_GRID = EV_VOX, EV_ICP_END = EV_GRAPH,  // icp_loop: grid build | iterations
};

// the float fields of qtr_stage_times a row can fill (capi.hip maps them to members)
enum StageField { SF_VOXELIZE = 0, SF_FPFH, SF_MATCH, SF_GRAPH, SF_CLIQUE, SF_SOLVE, SF_TOTAL, SF_COUNT };

// Slot::times_pending: the shape of the slot's last call, until its times have been read off the events
enum TimesShape {
  TIMES_NONE = 0,       // nothing to read (the times are final, or the call reports none)
  TIMES_EVENTS_OFF,     // QTR_STAGE_EVENTS=0 / qtr_set_stage_events(0): no event was recorded, every stage reads 0
  TIMES_SOLVE,          // qtr_solve
  TIMES_PAIR,           // qtr_register_pair, and qtr_register_pair_corr in the serial order
  TIMES_FRONT,          // qtr_feature_pair: the front end alone
  TIMES_KEYFRAMES,      // qtr_register_keyframes: no voxel grid, no FPFH chain; match = load + matcher
  TIMES_PAIR_OVERLAP,   // qtr_register_pair_corr, back end beside the front end: graph / clique / solve were measured on
                        // the third stream WHILE voxelize / fpfh / match ran — they add up to more than total
  TIMES_SHAPES
};

struct StageRow {
  int field, from, to;  // StageField <- elapsed time from SlotEvent to SlotEvent
};
struct ShapeTimes {
  int sync;   // the event that is synchronised before any is read (-1: none)
  bool nn;    // nn_kernel / nn_launches are filled from the matcher's own event pairs (when its last match was timed)
  int nrows;
  StageRow rows[SF_COUNT];  // fields without a row read 0
};

// (the rows most shapes share: the front end's three stages, the back end's last two)
#define ROWS_FRONT {SF_VOXELIZE, EV_BEGIN, EV_VOX}, {SF_FPFH, EV_VOX, EV_FPFH}, {SF_MATCH, EV_FPFH, EV_MATCH}
#define ROWS_BACK {SF_CLIQUE, EV_GRAPH, EV_CLIQUE}, {SF_SOLVE, EV_CLIQUE, EV_SOLVE}
static constexpr ShapeTimes k_shape_times[TIMES_SHAPES] = {
    /* TIMES_NONE */ {-1, false, 0, {}},
    /* TIMES_EVENTS_OFF */ {-1, true, 0, {}},
    /* TIMES_SOLVE */ {EV_SOLVE, false, 4, {{SF_GRAPH, EV_STAGED, EV_GRAPH}, ROWS_BACK, {SF_TOTAL, EV_BEGIN, EV_SOLVE}}},
    /* TIMES_PAIR */ {EV_SOLVE, true, 7, {ROWS_FRONT, {SF_GRAPH, EV_MATCH, EV_GRAPH}, ROWS_BACK, {SF_TOTAL, EV_BEGIN, EV_SOLVE}}},
    /* TIMES_FRONT */ {EV_MATCH, true, 4, {ROWS_FRONT, {SF_TOTAL, EV_BEGIN, EV_MATCH}}},
    /* TIMES_KEYFRAMES */
    {EV_SOLVE, true, 5, {{SF_MATCH, EV_BEGIN, EV_MATCH}, {SF_GRAPH, EV_MATCH, EV_GRAPH}, ROWS_BACK, {SF_TOTAL, EV_BEGIN, EV_SOLVE}}},
    /* TIMES_PAIR_OVERLAP */ {EV_END, true, 7, {ROWS_FRONT, {SF_GRAPH, EV_BE0, EV_GRAPH}, ROWS_BACK, {SF_TOTAL, EV_BEGIN, EV_END}}},
};
#undef ROWS_FRONT
#undef ROWS_BACK
