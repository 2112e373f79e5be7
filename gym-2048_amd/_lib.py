"""ctypes binding of ``libg2048_hip.so`` (the C ABI declared in ``include/g2048.h``).

There is exactly one compute path: the HIP library.  If it is missing, cannot be loaded, or finds
no GPU, everything here raises -- nothing falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libg2048_hip.so")

ACT_RANDOM, ACT_U8, ACT_I32, ACT_I64 = 0, 1, 2, 3
OBS_U8, OBS_F16, OBS_F32 = 0, 1, 2
ABI_VERSION = 16


class G2048Error(RuntimeError):
    """A call into libg2048_hip.so failed (message from g2048_last_error())."""


class StepIO(C.Structure):
    """g2048_step_io (include/g2048.h)."""
    _fields_ = [
        ("actions", C.c_void_p),
        ("action_dtype", C.c_int32),
        ("reward", C.c_void_p),
        ("terminated", C.c_void_p),
        ("illegal", C.c_void_p),
        ("highest", C.c_void_p),
        ("terminal_boards", C.c_void_p),
        ("obs", C.c_void_p),
        ("obs_dtype", C.c_int32),
        ("boards_out", C.c_void_p),
    ]


class HostIO(C.Structure):
    """g2048_host_io (include/g2048.h): host addresses of the engine's pinned, device-mapped I/O block."""
    _fields_ = [
        ("actions", C.c_void_p),
        ("reward", C.c_void_p),
        ("terminated", C.c_void_p),
        ("illegal", C.c_void_p),
        ("highest", C.c_void_p),
        ("boards", C.c_void_p),
        ("terminal_boards", C.c_void_p),
        ("scores", C.c_void_p),
    ]


class AfterstateIO(C.Structure):
    """g2048_afterstate_io (include/g2048.h): device pointers, NULL = not wanted."""
    _fields_ = [
        ("boards", C.c_void_p),
        ("score", C.c_void_p),
        ("legal", C.c_void_p),
        ("obs", C.c_void_p),
        ("obs_dtype", C.c_int32),
    ]


class SearchIO(C.Structure):
    """g2048_search_io (include/g2048.h): depth, weights and device output pointers (NULL = not wanted)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("base", C.c_int32),
        ("w_empty", C.c_int32),
        ("w_merge", C.c_int32),
        ("w_mono", C.c_int32),
        ("action", C.c_void_p),
        ("value", C.c_void_p),
    ]


class MCIO(C.Structure):
    """g2048_mc_io (include/g2048.h): playouts per move, playout cap, seed and device output pointers (NULL = not wanted)."""
    _fields_ = [
        ("rollouts", C.c_uint32),
        ("max_steps", C.c_uint32),
        ("seed", C.c_uint64),
        ("action", C.c_void_p),
        ("value", C.c_void_p),
        ("steps", C.c_void_p),
    ]


class NTupleNetC(C.Structure):
    """g2048_ntuple_net (include/g2048.h): T tuples of L cells, F fraction bits, the cell lists and the device weights.  A
    list shorter than tuple_len ends with G2048_NTUPLE_END (0xff) entries: a mixed network, weights [W]."""
    _fields_ = [
        ("n_tuples", C.c_uint32),
        ("tuple_len", C.c_uint32),
        ("frac_bits", C.c_uint32),
        ("cells", (C.c_uint8 * 6) * 8),
        ("weights", C.c_void_p),
    ]


class NTupleStagedNetC(C.Structure):
    """g2048_ntuple_staged_net (include/g2048.h): the network with weights [S][T][16^L], S and the S - 1 stage thresholds."""
    _fields_ = [
        ("net", NTupleNetC),
        ("n_stages", C.c_uint32),
        ("thresholds", C.c_uint16 * 7),
    ]


class NTupleIO(C.Structure):
    """g2048_ntuple_io (include/g2048.h): device output pointers of evaluate (NULL = not wanted)."""
    _fields_ = [
        ("value", C.c_void_p),
        ("action", C.c_void_p),
        ("best", C.c_void_p),
        ("after", C.c_void_p),
        ("after_value", C.c_void_p),
    ]


class NTuplePlayIO(C.Structure):
    """g2048_ntuple_play_io (include/g2048.h): the device side outputs of play (NULL = not wanted; games_left NULL = no
    limit)."""
    _fields_ = [
        ("games_left", C.c_void_p),
        ("hist", C.c_void_p),
        ("moves", C.c_void_p),
    ]


class NTupleTDIO(C.Structure):
    """g2048_ntuple_td_io (include/g2048.h): device output pointers of the fused TD step (NULL = not wanted)."""
    _fields_ = [
        ("action", C.c_void_p),
        ("after", C.c_void_p),
        ("after_value", C.c_void_p),
        ("best_next", C.c_void_p),
        ("terminated", C.c_void_p),
        ("delta", C.c_void_p),
    ]


class NTupleLogC(C.Structure):
    """g2048_ntuple_log (include/g2048.h): depth M and the device tensors of the move log, M + 1 slots each, slot-major."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("after", C.c_void_p),
        ("gain", C.c_void_p),
        ("flag", C.c_void_p),
    ]


class NTupleSearchIO(C.Structure):
    """g2048_ntuple_search_io (include/g2048.h): depth and device output pointers (NULL = not wanted)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("action", C.c_void_p),
        ("value", C.c_void_p),
    ]


class NTupleDeepIO(C.Structure):
    """g2048_ntuple_deep_io (include/g2048.h): depth, device output pointers (NULL = not wanted) and the mask of the engine
    forms (NULL = every board)."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("action", C.c_void_p),
        ("value", C.c_void_p),
        ("active", C.c_void_p),
    ]


class NTupleAdaptiveIO(C.Structure):
    """g2048_ntuple_adaptive_io (include/g2048.h): the depth of a board per empty-cell count, device output pointers (NULL = not
    wanted) and the mask of the engine forms (NULL = every board)."""
    _fields_ = [
        ("schedule", C.c_uint8 * 17),
        ("action", C.c_void_p),
        ("value", C.c_void_p),
        ("depth", C.c_void_p),
        ("active", C.c_void_p),
    ]


class NTupleReducedIO(C.Structure):
    """g2048_ntuple_reduced_io (include/g2048.h): g2048_ntuple_adaptive_io with ``reduce4``, the plies by which the children of
    a 4 spawn are searched shallower."""
    _fields_ = [
        ("schedule", C.c_uint8 * 17),
        ("reduce4", C.c_uint32),
        ("action", C.c_void_p),
        ("value", C.c_void_p),
        ("depth", C.c_void_p),
        ("active", C.c_void_p),
    ]


class NTupleTCC(C.Structure):
    """g2048_ntuple_tc (include/g2048.h): the device accumulators of temporal-coherence learning, int64 each, laid out as
    the weights."""
    _fields_ = [
        ("err", C.c_void_p),
        ("mag", C.c_void_p),
    ]


class NTupleMeanC(C.Structure):
    """g2048_ntuple_mean (include/g2048.h): the device state of the batch-mean update, int64 sums and uint32 counts, laid out
    as the weights."""
    _fields_ = [
        ("sum", C.c_void_p),
        ("count", C.c_void_p),
    ]


class NTupleTraceC(C.Structure):
    """g2048_ntuple_trace (include/g2048.h): depth H, lambda in Q16 and the device history of the n-tuple traces."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("lambda_", C.c_uint32),
        ("hist", C.c_void_p),
        ("len", C.c_void_p),
    ]


class NTupleDelayC(C.Structure):
    """g2048_ntuple_delay (include/g2048.h): the trace history plus the accumulators of the delayed learners."""
    _fields_ = [
        ("depth", C.c_uint32),
        ("lambda_", C.c_uint32),
        ("hist", C.c_void_p),
        ("len", C.c_void_p),
        ("acc", C.c_void_p),
    ]


class CarouselC(C.Structure):
    """g2048_carousel (include/g2048.h): S, the thresholds, the ring size, the seed and the device state of a carousel."""
    _fields_ = [
        ("n_stages", C.c_uint32),
        ("thresholds", C.c_uint16 * 7),
        ("capacity", C.c_uint32),
        ("seed", C.c_uint64),
        ("pool", C.c_void_p),
        ("count", C.c_void_p),
        ("seen", C.c_void_p),
        ("episodes", C.c_void_p),
        ("scratch", C.c_void_p),
    ]


class RestartC(C.Structure):
    """g2048_restart (include/g2048.h): the rule (stride_log2, capacity, min_span, max_restarts) and the device state of a midpoint
    restart."""
    _fields_ = [
        ("stride_log2", C.c_uint32),
        ("capacity", C.c_uint32),
        ("min_span", C.c_uint32),
        ("max_restarts", C.c_uint32),
        ("snap", C.c_void_p),
        ("pos", C.c_void_p),
        ("start", C.c_void_p),
        ("restarts", C.c_void_p),
    ]


class DowngradeC(C.Structure):
    """g2048_downgrade (include/g2048.h): the rule of tile-downgrading, in exponents."""
    _fields_ = [
        ("min_exp", C.c_uint32),
        ("floor_exp", C.c_uint32),
    ]


class Stats(C.Structure):
    """g2048_stats (include/g2048.h)."""
    _fields_ = [
        ("episodes", C.c_uint64),
        ("illegal_ends", C.c_uint64),
        ("last_count", C.c_uint64),
        ("last_score_sum", C.c_int64),
        ("last_score_max", C.c_int32),
        ("max_exp", C.c_uint32),
        ("highest_hist", C.c_uint32 * 32),
        ("return_sum", C.c_int64),
    ]


_E = C.c_void_p      # g2048_engine*
_S = C.c_void_p      # hipStream_t
_u64, _u32, _i32 = C.c_uint64, C.c_uint32, C.c_int32

# name -> (restype, argtypes); the single source of truth for tests/test_abi.py as well
SIGNATURES = {
    "g2048_last_error": (C.c_char_p, []),
    "g2048_abi_version": (C.c_int, []),
    "g2048_create": (C.c_int, [_u64, C.c_int, _u64, _u64, C.POINTER(_E)]),
    "g2048_destroy": (C.c_int, [_E]),
    "g2048_seed": (C.c_int, [_E, _u64, _S]),
    "g2048_get_clock": (C.c_int, [_E, C.POINTER(_u64)]),
    "g2048_set_clock": (C.c_int, [_E, _u64]),
    "g2048_num_boards": (_u64, [_E]),
    "g2048_set_illegal_move_reward": (C.c_int, [_E, C.c_float]),
    "g2048_set_max_tile": (C.c_int, [_E, C.c_int]),
    "g2048_set_strict_actions": (C.c_int, [_E, C.c_int]),
    "g2048_get_strict_actions": (C.c_int, [_E]),
    "g2048_reset": (C.c_int, [_E, C.c_int, _u32, C.c_void_p, _S]),
    "g2048_step": (C.c_int, [_E, C.POINTER(StepIO), C.c_int, _S]),
    "g2048_host_io_map": (C.c_int, [_E, C.POINTER(HostIO)]),
    "g2048_step_host": (C.c_int, [_E, C.c_int, _S]),
    "g2048_fetch_host": (C.c_int, [_E, _S]),
    "g2048_stream_signal": (C.c_int, [_E, _S, C.POINTER(_u64)]),
    "g2048_stream_wait": (C.c_int, [_E, _u64, _S]),
    "g2048_rollout": (C.c_int, [_E, _u32, C.POINTER(StepIO), _u64, C.c_int, _S]),
    "g2048_rollout_prepare": (C.c_int, [_E, _u32, C.POINTER(StepIO), _u64, C.c_int]),
    "g2048_set_chains": (C.c_int, [_E, C.c_int]),
    "g2048_get_chains": (C.c_int, [_E]),
    "g2048_get_chains_used": (C.c_int, [_E]),
    "g2048_get_graph_replays": (C.c_uint64, [_E]),
    "g2048_graph_status": (C.c_char_p, [_E]),
    "g2048_rollout_fused": (C.c_int, [_E, _u32, C.POINTER(StepIO), _u64, C.c_int, _S]),
    "g2048_rollout_random": (C.c_int, [_E, _u32, _S]),
    "g2048_move": (C.c_int, [_E, C.c_void_p, _i32, C.c_int, C.c_void_p, C.c_void_p, _S]),
    "g2048_query": (C.c_int, [_E, C.c_void_p, C.c_void_p, _S]),
    "g2048_legal_actions": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_afterstates": (C.c_int, [_E, C.POINTER(AfterstateIO), _S]),
    "g2048_afterstates_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(AfterstateIO), _S]),
    "g2048_expectimax": (C.c_int, [_E, C.POINTER(SearchIO), _S]),
    "g2048_expectimax_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(SearchIO), _S]),
    "g2048_mc_search": (C.c_int, [_E, C.POINTER(MCIO), _S]),
    "g2048_mc_search_plain": (C.c_int, [C.c_void_p, _u64, _u32, C.POINTER(MCIO), _S]),
    "g2048_ntuple_evaluate": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleIO), _S]),
    "g2048_ntuple_evaluate_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleNetC), C.POINTER(NTupleIO), _S]),
    "g2048_ntuple_play": (C.c_int, [_E, C.POINTER(NTupleNetC), _u32, C.POINTER(NTuplePlayIO), _S]),
    "g2048_ntuple_staged_play": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), _u32, C.POINTER(NTuplePlayIO), _S]),
    "g2048_play_step": (C.c_int, [_E, C.c_void_p, _i32, C.POINTER(NTuplePlayIO), _S]),
    "g2048_downgrade_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(DowngradeC), C.c_void_p, C.c_void_p, _S]),
    "g2048_downgrade_boards": (C.c_int, [_E, C.POINTER(DowngradeC), C.c_void_p, C.c_void_p, C.c_void_p, _S]),
    "g2048_ntuple_play_downgraded": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(DowngradeC), _u32, C.POINTER(NTuplePlayIO), _S]),
    "g2048_ntuple_staged_play_downgraded": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(DowngradeC), _u32,
                                                     C.POINTER(NTuplePlayIO), _S]),
    "g2048_ntuple_td_step": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleTDIO), _S]),
    "g2048_ntuple_staged_td_step": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleTDIO), _S]),
    "g2048_ntuple_td_train": (C.c_int, [_E, C.POINTER(NTupleNetC), _u32, _u32, C.POINTER(NTupleTDIO), C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_staged_td_train": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), _u32, _u32, C.POINTER(NTupleTDIO),
                                              C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_play_log": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleLogC), _S]),
    "g2048_ntuple_staged_play_log": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleLogC), _S]),
    "g2048_ntuple_log_delta": (C.c_int, [_u64, C.POINTER(NTupleNetC), C.POINTER(NTupleLogC), _u32, C.c_void_p, _S]),
    "g2048_ntuple_staged_log_delta": (C.c_int, [_u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleLogC), _u32, C.c_void_p, _S]),
    "g2048_ntuple_log_sweep": (C.c_int, [_u64, C.POINTER(NTupleNetC), C.POINTER(NTupleLogC), _u32, C.c_void_p, C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_staged_log_sweep": (C.c_int, [_u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleLogC), _u32, C.c_void_p,
                                               C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_log_train": (C.c_int, [_E, C.POINTER(NTupleNetC), _u32, _u32, C.POINTER(NTupleLogC), C.c_void_p, C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_staged_log_train": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), _u32, _u32, C.POINTER(NTupleLogC), C.c_void_p,
                                               C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_search": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleSearchIO), _S]),
    "g2048_ntuple_search_active": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleSearchIO), C.c_void_p, _S]),
    "g2048_ntuple_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleNetC), C.POINTER(NTupleSearchIO), _S]),
    "g2048_ntuple_deep_search": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleDeepIO), _S]),
    "g2048_ntuple_deep_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleNetC), C.POINTER(NTupleDeepIO), _S]),
    "g2048_ntuple_staged_deep_search": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleDeepIO), _S]),
    "g2048_ntuple_staged_deep_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleDeepIO), _S]),
    "g2048_ntuple_adaptive_search": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleAdaptiveIO), _S]),
    "g2048_ntuple_adaptive_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleNetC), C.POINTER(NTupleAdaptiveIO), _S]),
    "g2048_ntuple_staged_adaptive_search": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleAdaptiveIO), _S]),
    "g2048_ntuple_staged_adaptive_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleAdaptiveIO), _S]),
    "g2048_ntuple_reduced_search": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleReducedIO), _S]),
    "g2048_ntuple_reduced_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleNetC), C.POINTER(NTupleReducedIO), _S]),
    "g2048_ntuple_staged_reduced_search": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleReducedIO), _S]),
    "g2048_ntuple_staged_reduced_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleReducedIO), _S]),
    "g2048_ntuple_values_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleNetC), C.c_void_p, _S]),
    "g2048_ntuple_update_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, _u32, C.POINTER(NTupleNetC), _S]),
    "g2048_ntuple_tc_update_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleNetC),
                                              C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_trace_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _u64, C.POINTER(NTupleTraceC), _u32,
                                         C.c_void_p, _S]),
    "g2048_ntuple_trace_update": (C.c_int, [_u64, C.c_void_p, _u32, C.POINTER(NTupleNetC), C.POINTER(NTupleTraceC), _u32, _S]),
    "g2048_ntuple_tc_trace_update": (C.c_int, [_u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleNetC), C.POINTER(NTupleTCC),
                                              C.POINTER(NTupleTraceC), _u32, _S]),
    "g2048_ntuple_mean_update_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleNetC),
                                                C.POINTER(NTupleMeanC), _S]),
    "g2048_ntuple_mean_trace_update": (C.c_int, [_u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleNetC), C.POINTER(NTupleMeanC),
                                                C.POINTER(NTupleTraceC), _u32, _S]),
    "g2048_ntuple_staged_mean_update_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleStagedNetC),
                                                       C.POINTER(NTupleMeanC), _S]),
    "g2048_ntuple_staged_mean_trace_update": (C.c_int, [_u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleStagedNetC),
                                                       C.POINTER(NTupleMeanC), C.POINTER(NTupleTraceC), _u32, _S]),
    "g2048_ntuple_delay_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _u64, C.POINTER(NTupleDelayC), _u32,
                                         C.c_void_p, _S]),
    "g2048_ntuple_delay_update": (C.c_int, [_u64, _u32, _u32, C.POINTER(NTupleNetC), C.POINTER(NTupleDelayC), _u32, _S]),
    "g2048_ntuple_tc_delay_update": (C.c_int, [_u64, _u32, _u32, _u32, C.POINTER(NTupleNetC), C.POINTER(NTupleTCC),
                                              C.POINTER(NTupleDelayC), _u32, _S]),
    "g2048_ntuple_staged_evaluate": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleIO), _S]),
    "g2048_ntuple_staged_evaluate_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleIO), _S]),
    "g2048_ntuple_staged_search": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleSearchIO), _S]),
    "g2048_ntuple_staged_search_active": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleSearchIO), C.c_void_p, _S]),
    "g2048_ntuple_staged_search_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleSearchIO), _S]),
    "g2048_ntuple_staged_values_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.c_void_p, _S]),
    "g2048_ntuple_staged_update_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, _u32, C.POINTER(NTupleStagedNetC), _S]),
    "g2048_ntuple_staged_tc_update_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleStagedNetC),
                                                     C.POINTER(NTupleTCC), _S]),
    "g2048_ntuple_staged_trace_update": (C.c_int, [_u64, C.c_void_p, _u32, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleTraceC),
                                                  _u32, _S]),
    "g2048_ntuple_staged_tc_trace_update": (C.c_int, [_u64, C.c_void_p, _u32, _u32, C.POINTER(NTupleStagedNetC),
                                                     C.POINTER(NTupleTCC), C.POINTER(NTupleTraceC), _u32, _S]),
    "g2048_ntuple_staged_delay_update": (C.c_int, [_u64, _u32, _u32, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleDelayC), _u32, _S]),
    "g2048_ntuple_staged_tc_delay_update": (C.c_int, [_u64, _u32, _u32, _u32, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleTCC),
                                                     C.POINTER(NTupleDelayC), _u32, _S]),
    "g2048_ntuple_stage_plain": (C.c_int, [C.c_void_p, _u64, C.POINTER(NTupleStagedNetC), C.c_void_p, _S]),
    "g2048_carousel_scratch_bytes": (_u64, [_u64]),
    "g2048_carousel_step": (C.c_int, [_E, C.POINTER(CarouselC), C.c_void_p, _S]),
    "g2048_carousel_step_plain": (C.c_int, [C.c_void_p, _u64, _u64, C.c_void_p, C.POINTER(CarouselC), _S]),
    "g2048_restart_step": (C.c_int, [_E, C.POINTER(RestartC), C.c_void_p, _S]),
    "g2048_restart_step_plain": (C.c_int, [C.c_void_p, _u64, C.c_void_p, C.POINTER(RestartC), _S]),
    "g2048_ntuple_play_log_restart": (C.c_int, [_E, C.POINTER(NTupleNetC), C.POINTER(NTupleLogC), C.POINTER(RestartC), _S]),
    "g2048_ntuple_staged_play_log_restart": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), C.POINTER(NTupleLogC), C.POINTER(RestartC), _S]),
    "g2048_ntuple_log_train_restart": (C.c_int, [_E, C.POINTER(NTupleNetC), _u32, _u32, C.POINTER(NTupleLogC), C.c_void_p,
                                                C.POINTER(NTupleTCC), C.POINTER(RestartC), _S]),
    "g2048_ntuple_staged_log_train_restart": (C.c_int, [_E, C.POINTER(NTupleStagedNetC), _u32, _u32, C.POINTER(NTupleLogC), C.c_void_p,
                                                       C.POINTER(NTupleTCC), C.POINTER(RestartC), _S]),
    "g2048_add_tile": (C.c_int, [_E, _u32, _S]),
    "g2048_fill_random_actions": (C.c_int, [_E, _u64, _u32, C.c_void_p, _S]),
    "g2048_onehot": (C.c_int, [_E, C.c_void_p, _i32, _S]),
    "g2048_get_boards": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_set_boards": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_get_scores": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_set_scores": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_get_last_scores": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_set_last_records": (C.c_int, [_E, C.c_int, _S]),
    "g2048_get_last_records": (C.c_int, [_E]),
    "g2048_records_ptr": (C.c_void_p, [_E]),
    "g2048_last_records_ptr": (C.c_void_p, [_E]),
    "g2048_episode_stats": (C.c_int, [_E, C.POINTER(Stats), _S]),
    "g2048_episode_stats_async": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_returns_summary_async": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_set_numpy_rng": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_get_numpy_rng": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_seed_numpy": (C.c_int, [_E, _u64, _S]),
    "g2048_augment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _u64, C.c_void_p, C.c_void_p, C.c_void_p, _S]),
    "g2048_state_bytes": (_u64, [_E]),
    "g2048_get_state": (C.c_int, [_E, C.c_void_p, _S]),
    "g2048_set_state": (C.c_int, [_E, C.c_void_p, _u64, _S]),
    "g2048_canonicalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _u64, C.c_void_p, _S]),
    "g2048_comm_unique_id": (C.c_int, [C.c_void_p]),
    "g2048_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "g2048_comm_destroy": (C.c_int, [C.c_void_p]),
    "g2048_allgather_returns": (C.c_int, [_E, C.c_void_p, C.c_void_p, _S]),
    "g2048_allgather_summary": (C.c_int, [_E, C.c_void_p, C.c_void_p, _S]),
    "g2048_comm_world": (C.c_int, [C.c_void_p]),
    "g2048_comm_rank": (C.c_int, [C.c_void_p]),
    "g2048_comm_local_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "g2048_comm_local_destroy": (C.c_int, [C.c_void_p]),
    "g2048_allgather_returns_local": (C.c_int, [C.c_void_p, C.POINTER(_E), C.POINTER(C.c_void_p), C.POINTER(_S)]),
}
COMM_ID_BYTES = 128

_lib = None


def load():
    """Load libg2048_hip.so (once).  Raises G2048Error when it is not built or not loadable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise G2048Error(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the machine
        raise G2048Error(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.g2048_abi_version() != ABI_VERSION:
        raise G2048Error(f"ABI mismatch: library {lib.g2048_abi_version()}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise G2048Error(f"libg2048_hip error {rc}: {load().g2048_last_error().decode(errors='replace')}")
