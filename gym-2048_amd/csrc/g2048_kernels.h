// g2048_kernels.h -- launch interface between the C ABI (g2048_api.hip) and the gfx950 kernels
// (g2048_kernels.hip).  Internal; the public contract is include/g2048.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g2048 {

// Engine-owned device state (one slab).
struct DeviceState {
    uint4 *boards;      // [n] 16-byte board RECORDS: 16 x 5-bit exponents + the 24-bit score deficit in the spare
                        //     bits of bytes 8..15 (g2048_device.h "board RECORD"); there is no separate score
                        //     array -- self.score (game2048_env.py:86) = potential - deficit
    uint4 *last_record; // [n] record a board's most recent episode ENDED on (all-zero: none yet); its score is
                        //     that episode's return.  Written only by lanes whose episode ended.
    unsigned long long *ep_counters; // one 32-byte SLOT per 64 boards: finished episodes, of which ended on an illegal move,
                                     // G = summed merge scores (return accounting), pending mask -- as eight dwords, the
                                     // four low halves first; updated by ONE lane of the wavefront that owns the boards
                                     // (old values via the scalar cache); g2048_kernels.hip "episode SLOT"
    uint64_t *rng;      // numpy-RNG mode only: [5][n] planes (state_lo, state_hi, inc_lo, inc_hi, buf); else NULL
};

constexpr uint32_t kSlotWords = 4; // uint64 per wavefront slot of ep_counters

// bytes of the numpy-RNG allocation for n boards: 5 planes of uint64
inline size_t numpy_rng_bytes(uint64_t n) { return static_cast<size_t>(n * 40); }
// launch blocks never straddle the end of the slot array: slots exist for whole blocks of the LARGEST block size in use
// (the 512 lanes of step_numpy_kernel)
constexpr uint32_t kSlotBlockLanes = 512;

struct StepArgs {
    DeviceState st;
    const void *actions;
    float *reward;
    uint8_t *terminated;
    uint8_t *illegal;
    uint8_t *highest;
    uint4 *terminal_boards;
    uint4 *boards_out;  // [n][16] plain cells of the board AFTER the step (and its auto-reset), or NULL
    unsigned long long *done_seq; // host-visible completion word (mapped pinned memory) or NULL: a launch of ONE block writes
    unsigned long long done_value; //   done_value there after all of its outputs (system-scope release); see g2048_step_host
    unsigned long long *action_err; // strict actions (g2048_set_strict_actions): host-visible word that receives a report when a
                                    //   lane reads an action outside 0..3 (game2048_env.py:49 Discrete(4)); NULL = not checked
    void *obs;          // [n][16][4][4] one-hot observation of the board AFTER the step (and its auto-reset), or NULL
    uint32_t obs_dtype; // G2048_OBS_*
    uint32_t n;
    uint32_t board_offset;
    uint32_t seed_lo, seed_hi;
    uint32_t t_lo, t_hi;
    float illegal_reward;
    uint32_t max_exp;
    uint32_t auto_reset;
    uint32_t k_steps; // fused rollout only
};

struct StatsOut {
    unsigned long long episodes;      // all finished episodes since create / seed
    unsigned long long illegal_ends;
    unsigned long long last_count;    // boards that have finished at least one episode
    unsigned long long last_score_sum; // sum / max of those boards' most recent final scores
    int last_score_max;
    unsigned int max_exp;
    unsigned int highest_hist[32]; // boards whose highest tile is 2^k right now (game2048_env.py:190-192)
    long long return_sum;          // sum of the final scores of ALL finished episodes (exact)
};

// Launchers that take StepArgs run the kernel of the engine's RNG mode: numpy-RNG mode when a.st.rng is set.
hipError_t launch_reset(const StepArgs &a, uint32_t first_slot, const uint8_t *mask, hipStream_t s);
hipError_t launch_step(const StepArgs &a, int action_dtype, hipStream_t s);
hipError_t launch_rollout_random(const StepArgs &a, hipStream_t s);
// a k-step launch train as a cached hipGraph: k x step (t read from *t_dev, written by a launch in front); see g2048_kernels.hip
struct RolloutGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    unsigned long long *t_dev = nullptr;
};
bool rollout_graph_supported(const StepArgs &a); // the standard configuration: reward + terminated, nothing optional, spawn stream
hipError_t build_rollout_graph(const StepArgs &first, int action_dtype, uint32_t k_steps, uint64_t stride, unsigned long long *t_dev,
                               RolloutGraph *out);
hipError_t launch_rollout_graph(RolloutGraph &g, unsigned long long t_first, hipStream_t s);
void destroy_rollout_graph(RolloutGraph &g);
hipError_t launch_rollout_fused(const StepArgs &a, int action_dtype, uint64_t stride, hipStream_t s);
hipError_t launch_move(uint4 *boards, uint32_t n, const void *actions, int action_dtype, bool trial,
                       int32_t *score_out, uint8_t *legal_out, hipStream_t s);
hipError_t launch_query(const uint4 *boards, uint32_t n, uint32_t max_exp, uint8_t *isend_out, uint8_t *highest_out,
                        hipStream_t s);
hipError_t launch_legal_mask(const uint4 *boards, uint32_t n, uint8_t *mask_out, hipStream_t s);
// g2048_afterstates: outputs of the four trial moves (g2048_afterstate_io, checked by the caller; NULL = not wanted)
struct AfterstateOut {
    uint4 *boards;      // [n][4] afterstate cells, one 16-byte chunk per direction
    uint4 *score;       // [n] four int32 merge scores per chunk
    uint8_t *legal;     // [n] bit d = move d legal
    void *obs;          // [n][4][16][4][4] of obs_dtype
    uint32_t obs_dtype; // G2048_OBS_*
};
// The boards a read-only launch works on: n engine records, or (`plain`) n rows of plain exponents (taken mod 32)
struct Boards {
    const uint4 *ptr;
    uint32_t n;
    bool plain;
};
hipError_t launch_afterstates(const Boards &b, const AfterstateOut &o, hipStream_t s);
// g2048_expectimax: weights and outputs (g2048_search_io, checked by the caller; NULL = not wanted)
struct SearchArgs {
    uint32_t base, w_empty, w_merge, w_mono; // = g2048::SearchWeights (g2048_device.h)
    uint8_t *action; // [n]
    int32_t *value;  // [n][4]
};
// depth 1..3
hipError_t launch_expectimax(const Boards &b, uint32_t depth, const SearchArgs &a, hipStream_t s);
// g2048_mc_search: parameters and outputs (g2048_mc_io, checked by the caller; NULL = not wanted)
struct McArgs {
    uint32_t rollouts, max_steps; // R in 1..65536, L in 1..65535
    uint32_t seed_lo, seed_hi;
    uint32_t index_offset;        // board index of row 0 in the Philox counter
    uint8_t *action;              // [n]
    int64_t *value;               // [n][4]
    int64_t *steps;               // [n][4]
};
hipError_t launch_mc_search(const Boards &b, const McArgs &a, hipStream_t s);
// g2048_ntuple_*: the network (g2048_ntuple_net) and evaluate's outputs (g2048_ntuple_io), both checked by the caller
struct NtupleNet {
    uint32_t n_tuples, tuple_len, frac_bits; // T in 1..8, L in 1..6, F in 0..16
    uint8_t cells[8][6];                     // < 16, distinct within a tuple
    int32_t *weights;                        // [S][T][16^L]
    uint32_t n_stages = 1;                   // S in 1..8 (g2048_ntuple_staged_net); 1 = the unstaged network
    uint16_t thresholds[7] = {};             // the first S - 1: strictly ascending, >= 1
};
struct NtupleOut {
    int64_t *value;       // [n][4]
    uint8_t *action;      // [n]
    int64_t *best;        // [n]
    uint4 *after;         // [n] plain cells of the chosen afterstate
    int64_t *after_value; // [n]
};
hipError_t launch_ntuple_eval(const Boards &b, const NtupleNet &net, const NtupleOut &o, hipStream_t s);
// g2048_ntuple_search's outputs (g2048_ntuple_search_io), checked by the caller; depth in 1..2
struct NtupleSearchOut {
    uint8_t *action; // [n]
    int64_t *value;  // [n][4]
    const uint32_t *active = nullptr; // [n] or NULL (g2048_ntuple_search_active): a board at 0 is not searched, its outputs
                                      //     are those of a board with no legal move
};
hipError_t launch_ntuple_search(const Boards &b, uint32_t depth, const NtupleNet &net, const NtupleSearchOut &o, hipStream_t s);
// g2048_ntuple_deep_search: the same outputs from the workgroup-per-board kernel; depth in 2..3
hipError_t launch_ntuple_deep_search(const Boards &b, uint32_t depth, const NtupleNet &net, const NtupleSearchOut &o, hipStream_t s);
// g2048_ntuple_adaptive_search: the workgroup-per-board kernel at a depth per board, schedule[E0] in 0..4 (checked by the caller)
struct NtupleAdaptiveOut {
    uint8_t *action;        // [n] or NULL
    int64_t *value;         // [n][4] or NULL
    uint8_t *depth;         // [n] or NULL: the depth used, kNtupleAdaptiveSkipped where active is 0
    const uint32_t *active; // [n] or NULL, as NtupleSearchOut::active
};
hipError_t launch_ntuple_adaptive_search(const Boards &b, const uint8_t schedule[17], const NtupleNet &net, const NtupleAdaptiveOut &o,
                                         hipStream_t s);
// g2048_ntuple_reduced_search: the same outputs with the children of a 4 spawn searched reduce4 (1..2, checked by the caller)
// plies shallower
hipError_t launch_ntuple_reduced_search(const Boards &b, const uint8_t schedule[17], uint32_t reduce4, const NtupleNet &net,
                                        const NtupleAdaptiveOut &o, hipStream_t s);
// g2048_ntuple_play: a.k_steps greedy steps with auto-reset in one launch (spawn stream only: a.st.rng is refused by the
// caller); the side outputs (g2048_ntuple_play_io, checked by the caller; NULL = not wanted)
struct NtuplePlayOut {
    uint32_t *games_left;      // [n] in/out: games a board may still finish; 0 = the board rests
    unsigned long long *hist;  // [32] += episodes that ended with highest exponent k
    unsigned long long *moves; // [1] += (board, step) pairs played
};
hipError_t launch_ntuple_play(const StepArgs &a, const NtupleNet &net, const NtuplePlayOut &io, hipStream_t s);
// Tile-downgrading (g2048_downgrade, checked by the caller): min_exp in 1..31, floor_exp in 4..31
struct DowngradeArgs {
    uint32_t min_exp, floor_exp;
};
// g2048_ntuple_play_downgraded: launch_ntuple_play with every move chosen on the translated board
hipError_t launch_ntuple_play_downgraded(const StepArgs &a, const NtupleNet &net, const DowngradeArgs &rule, const NtuplePlayOut &io,
                                         hipStream_t s);
// g2048_downgrade_plain / _boards: out[i] = the translation of boards[i] (plain boards or records; out may be boards),
// missing[i] (or NULL) = its k; active (or NULL): a board at 0 gets the empty board and G2048_DOWNGRADE_SKIPPED
hipError_t launch_downgrade(const uint4 *boards, uint32_t n, const DowngradeArgs &rule, const uint32_t *active, uint4 *out,
                            uint8_t *missing, hipStream_t s);
// g2048_play_step: one step of that launch with the actions of a.actions (action_dtype G2048_ACT_*, checked by the caller)
hipError_t launch_play_step(const StepArgs &a, int action_dtype, const NtuplePlayOut &io, hipStream_t s);
// g2048_ntuple_td_step: one greedy step with auto-reset and the evaluate on either side of it in one launch (spawn stream
// only, as launch_ntuple_play); the outputs (g2048_ntuple_td_io, checked by the caller; NULL = not wanted)
struct NtupleTdIo {
    uint8_t *action;      // [n]
    uint4 *after;         // [n] plain cells of the afterstate played
    int64_t *after_value; // [n]
    int64_t *best_next;   // [n] `best` of the board after the step, not masked
    uint8_t *terminated;  // [n]
    int64_t *delta;       // [n] (terminated ? 0 : best_next) - after_value
};
hipError_t launch_ntuple_td_step(const StepArgs &a, const NtupleNet &net, const NtupleTdIo &io, hipStream_t s);
// g2048_ntuple_play_log and g2048_ntuple_log_delta: the move log (g2048_ntuple_log, checked by the caller): depth M in
// 1..1024, M + 1 slots of n entries each, slot-major
struct NtupleLog {
    uint32_t depth;
    uint4 *after;  // [M + 1][n] plain boards
    int64_t *gain; // [M + 1][n]
    uint8_t *flag; // [M + 1][n]
};
// log.depth greedy steps with auto-reset in one launch, as launch_ntuple_play without side outputs (a.k_steps == log.depth,
// spawn stream only); slot 0 takes what slot M held, slot m the entry of move m
hipError_t launch_ntuple_play_log(const StepArgs &a, const NtupleNet &net, const NtupleLog &log, hipStream_t s);
// delta[i] of slot m < log.depth for the n boards of the log; reads the log and the weights only
hipError_t launch_ntuple_log_delta(uint32_t n, const NtupleNet &net, const NtupleLog &log, uint32_t m, int64_t *delta, hipStream_t s);
hipError_t launch_ntuple_values(const uint4 *boards, uint32_t n, const NtupleNet &net, int64_t *v, hipStream_t s);
// g2048_ntuple_stage_plain: stage[i] of n plain boards; reads the network's shape and thresholds, not its weights
hipError_t launch_ntuple_stage(const uint4 *boards, uint32_t n, const NtupleNet &net, uint8_t *stage, hipStream_t s);
// The accumulators of a TC update (g2048_ntuple_tc, checked by the caller): err and mag [T][16^L]; phases in 1..3: phase W
// (kNtupleTcWeights = G2048_NTUPLE_TC_WEIGHTS), then phase A (kNtupleTcAccum = G2048_NTUPLE_TC_ACCUM), a launch each
constexpr uint32_t kNtupleTcWeights = 1u, kNtupleTcAccum = 2u;
struct NtupleTc {
    uint32_t phases;
    int64_t *err, *mag;
};
// The three updates, one per item source (plain boards, trace, delay ring); tc: NULL for the TD update, else the TC update
hipError_t launch_ntuple_update(const uint4 *boards, uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                const NtupleTc *tc, hipStream_t s);
// g2048_ntuple_trace_*: the history (g2048_ntuple_trace), checked by the caller: depth in 1..8, lambda <= 65536, slot < depth
struct NtupleTrace {
    uint32_t depth, lambda;
    uint4 *hist;  // [depth][n] plain boards
    uint8_t *len; // [n]
};
// g2048_ntuple_delay_*: the delay ring (g2048_ntuple_delay), checked by the caller as the history; mode is kNtupleDelayStep or
// kNtupleDelayFlush (g2048_device.h)
struct NtupleDelay : NtupleTrace {
    int64_t *acc; // [depth][n]
};
// g2048_ntuple_trace_push and g2048_ntuple_delay_push: the kernel of the history's kind
hipError_t launch_ntuple_push(const uint4 *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                              uint32_t n, const NtupleTrace &tr, uint32_t slot, int64_t *delta, hipStream_t s);
hipError_t launch_ntuple_push(const uint4 *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                              uint32_t n, const NtupleDelay &dl, uint32_t slot, int64_t *delta, hipStream_t s);
hipError_t launch_ntuple_trace_update(uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                      const NtupleTrace &tr, uint32_t slot, const NtupleTc *tc, hipStream_t s);
hipError_t launch_ntuple_delay_update(uint32_t n, uint32_t lr_shift, uint32_t mode, const NtupleNet &net, const NtupleDelay &dl,
                                      uint32_t slot, const NtupleTc *tc, hipStream_t s);
// The state of a batch-mean update (g2048_ntuple_mean, checked by the caller): sum and count shaped like the weights; phases
// in 1..3: phase SUM (kNtupleMeanSum = G2048_NTUPLE_MEAN_SUM), then phase APPLY (kNtupleMeanApply = G2048_NTUPLE_MEAN_APPLY), a
// launch each
constexpr uint32_t kNtupleMeanSum = 1u, kNtupleMeanApply = 2u;
struct NtupleMean {
    uint32_t phases;
    int64_t *sum;
    uint32_t *count;
};
// g2048_ntuple_mean_update_plain and g2048_ntuple_mean_trace_update: the batch-mean update over plain boards and over a trace
hipError_t launch_ntuple_mean_update(const uint4 *boards, uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                     const NtupleMean &mean, hipStream_t s);
hipError_t launch_ntuple_mean_trace_update(uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                           const NtupleTrace &tr, uint32_t slot, const NtupleMean &mean, hipStream_t s);
// g2048_carousel_step: the carousel (g2048_carousel) and the records it works on, both checked by the caller
struct CarouselArgs {
    uint4 *records;            // [n] engine records, restarted in place
    const uint8_t *terminated; // [n]
    uint32_t n, index_offset;  // index_offset + n <= 2^32
    uint32_t n_stages, capacity; // S in 2..8, C in 1..65536
    uint16_t thresholds[7];    // the first S - 1: strictly ascending, >= 1
    uint32_t seed_lo, seed_hi;
    uint4 *pool;               // [S][C] records
    uint64_t *count;           // [S]
    uint8_t *seen;             // [n]
    uint32_t *episodes;        // [n]
    uint32_t *scratch;         // kCarouselScratchBytes
};
// The carousel's kernels give every workgroup a contiguous range of boards; the cap on workgroups bounds the scratch
// (their entry counts per stage, the scanned counts, the totals and count mod C) whatever n is.
constexpr uint32_t kCarouselMaxGroups = 1024;
constexpr size_t kCarouselScratchBytes = (2 * 8 * kCarouselMaxGroups + 16) * sizeof(uint32_t);
// three launches on s: restart (reads the pool), scan, scatter (writes the pool)
hipError_t launch_carousel_step(const CarouselArgs &a, hipStream_t s);
// g2048_restart_step and g2048_ntuple_play_log_restart: the midpoint restart (g2048_restart, checked by the caller)
struct RestartArgs {
    uint32_t stride_log2, capacity; // k in 0..16, C in 1..4096
    uint32_t min_span, max_restarts;
    uint4 *snap;                    // [C][n] engine records, slot-major
    uint32_t *pos, *start, *restarts; // [n] each
};
// restart_step_kernel strides over the boards: the cap on its workgroups
constexpr uint32_t kRestartMaxGroups = 1024;
// one launch on s: the restart step on n records in place
hipError_t launch_restart_step(uint4 *records, const uint8_t *terminated, uint32_t n, const RestartArgs &rs, hipStream_t s);
// launch_ntuple_play_log with the restart step behind every move, in the same launch
hipError_t launch_ntuple_play_log_restart(const StepArgs &a, const NtupleNet &net, const NtupleLog &log, const RestartArgs &rs, hipStream_t s);
hipError_t launch_add_tile(const StepArgs &a, uint32_t slot, hipStream_t s);
// numpy-RNG mode: every board's PCG64 generator, seeded as numpy seeds it, into the DeviceState::rng planes
hipError_t launch_seed_numpy(uint64_t *planes, uint32_t n, uint64_t first_seed, hipStream_t s);
hipError_t launch_fill_actions(uint8_t *out, uint32_t n, uint32_t board_offset, uint32_t seed_lo, uint32_t seed_hi,
                               uint64_t t_first, uint32_t k_steps, hipStream_t s);
hipError_t launch_onehot(const uint4 *boards, uint32_t n, void *out, int obs_dtype, hipStream_t s);
hipError_t launch_augment(const uint4 *boards, const uint4 *next_boards, const uint8_t *actions, uint32_t n,
                          uint4 *boards_out, uint4 *next_out, uint8_t *actions_out, hipStream_t s);
// partials: kStatsPartialWords uint64 of device scratch (stage 1 -> stage 2; field-major, one column per block)
constexpr uint32_t kStatsBlocks = 2048;
constexpr uint32_t kStatsPartialWords = (7 + 32) * kStatsBlocks;
// summary_scratch: kSummaryScratchWords uint64, ZERO when first used (the one-launch returns summary keeps its block / group
// partials and its "last one out" counters there and leaves the counters at zero)
constexpr uint32_t kSummaryBlocks = 256;
constexpr uint32_t kSummaryScratchWords = 2048;
hipError_t launch_stats(const DeviceState &st, uint32_t n, unsigned long long *partials, unsigned long long *summary_scratch,
                        StatsOut *dev_out, bool returns_only, hipStream_t s);
// record <-> plain views (cells uint8[n][16], scores int32[n]); device pointers
hipError_t launch_export_boards(const uint4 *records, uint32_t n, uint4 *cells_out, hipStream_t s);
hipError_t launch_import_boards(uint4 *records, uint32_t n, const uint4 *cells_in, hipStream_t s);
hipError_t launch_export_scores(const uint4 *records, uint32_t n, int32_t *scores_out, hipStream_t s); // also last_record -> returns
hipError_t launch_import_scores(uint4 *records, uint32_t n, const int32_t *scores_in, unsigned long long *ep_counters,
                                hipStream_t s);
hipError_t launch_clear_stats(const DeviceState &st, uint32_t n, hipStream_t s);
hipError_t launch_export_last_scores(const DeviceState &st, uint32_t n, int32_t *out, hipStream_t s);
// host-resident I/O: boards + scores of the current state in one launch; the completion word (see StepArgs::done_seq)
hipError_t launch_fetch(const uint4 *records, uint32_t n, uint4 *cells_out, int32_t *scores_out, unsigned long long *done_seq,
                        unsigned long long done_value, hipStream_t s);
hipError_t launch_signal(unsigned long long *done_seq, unsigned long long done_value, hipStream_t s);
// stream-to-stream ordering by a ticket in device memory (two-chain rollouts): set behind the work it stands for, wait (bounded) before what depends on it
hipError_t launch_flag_set(unsigned long long *flag, unsigned long long value, hipStream_t s);
// `timed_out`: host-visible word that receives `value` when the wait gives up after `max_polls` polls (~1 us each)
hipError_t launch_flag_wait(const unsigned long long *flag, unsigned long long value, unsigned long long *timed_out,
                            uint32_t max_polls, hipStream_t s);
constexpr uint32_t kFlagWaitPolls = 1u << 26;
hipError_t launch_canonicalize(uint4 *boards, uint4 *next_boards, uint8_t *actions, uint32_t n, uint8_t *sym_out,
                               hipStream_t s);

} // namespace g2048
