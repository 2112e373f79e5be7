"""N-tuple network value function (``g2048_ntuple_*``): table look-ups indexed by cell exponents,
summed over the eight board symmetries, with int32 fixed-point weights -- evaluated on the afterstates of the four moves
(a greedy player: one launch for the whole batch) and learned by afterstate TD(0) (Szubert & Jaskowski 2014), one launch
per update.  Everything is an integer: the same bits however the batch is split over lanes, launches or shards.

``NTupleNet`` owns the weights (a device tensor); ``Batched2048.ntuple_evaluate`` evaluates the engine's live boards;
``td_step`` / ``train`` chain evaluate, ``g2048_step`` and update on the device with no host synchronisation;
``NTupleTC`` and ``tc_step`` / ``tc_train`` do the same with temporal-coherence learning, a learning rate per weight
(``g2048_ntuple_tc_update_plain``).  ``NTupleTrace`` and ``tdl_step`` / ``tdl_train`` / ``tcl_step`` /
``tcl_train`` are the multi-step forms, TD(lambda) and TC(lambda): the error of a step also moves, decayed, the last few
afterstates of the same board (``g2048_ntuple_trace_*``).
``NTupleDelay`` and ``delayed_tdl_step`` / ``delayed_tdl_train`` / ``delayed_tcl_step`` / ``delayed_tcl_train`` are the delayed
forms of those two (Jaskowski 2017): the errors an afterstate earns are collected per board and applied to the tables once,
when it leaves the ring (``g2048_ntuple_delay_*``).
``NTupleNet.search`` / ``Batched2048.ntuple_search`` play the network through a depth-1..2 expectimax
(``g2048_ntuple_search``), one launch for the whole batch.
``NTupleNet.deep_search`` / ``Batched2048.ntuple_deep_search`` are the same search at depth 2..3 from a kernel that gives a
board a whole workgroup (``g2048_ntuple_deep_search``), and ``DeepPlayer`` plays it in :func:`play_games`:
the 3-ply row of the papers.
``NTupleNet.adaptive_search`` / ``Batched2048.ntuple_adaptive_search`` search every board at a depth 0..4 chosen by a fixed
rule from its own empty cells, one launch (``g2048_ntuple_adaptive_search``); :func:`schedule_by_empties`
and ``SCHEDULES`` make the rule, and ``AdaptivePlayer`` plays it in :func:`play_games`.
``NTupleNet.reduced_search`` / ``Batched2048.ntuple_reduced_search`` are that search with the children of a 4 spawn searched
``reduce4`` plies shallower (``g2048_ntuple_reduced_search``); ``ReducedPlayer`` plays it.
``NTupleNet(..., stages=...)`` is the multi-stage network: a weight set per game stage, chosen per board by the tiles it
holds (``g2048_ntuple_staged_*``); every method and trainer above works on it unchanged.
``Carousel`` is carousel shaping for such a network (``g2048_carousel_*``): it remembers, per stage, the
boards on which recent episodes entered that stage and restarts finished episodes from them, cycling over the stages, so
that the late weight sets are trained too; every trainer takes it as ``carousel=``.
``Batched2048.ntuple_play`` plays K greedy moves of every board in one launch and :func:`play_games` turns that into the
game report of the papers -- exactly G games per board, mean score and the share of games that reach each tile
(``g2048_ntuple_play``).  ``play_games(depth=1 or 2)`` is that report for the expectimax player over the
network and ``play_games(player=...)`` for any policy, through ``Batched2048.play_step`` and ``ntuple_search(active=)``
(``g2048_play_step``, ``g2048_ntuple_search_active``).
``NTupleNet(..., mixed=True)`` and the ragged presets of ``TUPLES`` are networks with tuples of mixed length (redundant
encoding): tables of 16^L_t weights back to back in one ``[W]`` tensor; everything above works on them.
``Batched2048.ntuple_td_step`` is the front half of every learner above -- evaluate, play, evaluate, form the error -- in one
launch, and ``Batched2048.ntuple_td_train`` runs K whole TD(0) or TC steps in one library call (``g2048_ntuple_td_step``,
``g2048_ntuple_td_train``); every trainer takes ``fused=True`` for them, the same bits.  Measured, the
composition is the faster form, so ``fused=False`` is the default.
``NTupleMean`` and ``mean_step`` / ``mean_train`` / ``mean_tdl_step`` / ``mean_tdl_train`` are the batch-mean learners: every
table entry a batch reaches moves once, by the mean of the errors that reached it, so its learning rate does not grow with the
batch (``g2048_ntuple_mean_update_plain``, ``g2048_ntuple_mean_trace_update``).  Opt-in.
``NTupleLog``, ``Batched2048.ntuple_play_log``, ``NTupleNet.log_delta``, :func:`log_sweep` and :func:`backward_train` are backward
learning over logged segments (Matsuzaki 2017): M moves of every board played and kept in one launch, then updated from the
last to the first (``g2048_ntuple_play_log``, ``g2048_ntuple_log_delta``, ``g2048_ntuple_log_sweep``, ``g2048_ntuple_log_train``,
INTEGRATION.md §24).  A learner of its own.  Opt-in.
``Restart`` is the midpoint restart of the same paper (``g2048_restart_*``): a finished episode goes back to
the last snapshot at or below the middle of the run that ended -- per board, integers only, for any network, the same bits
across shards; every trainer takes it as ``restart=`` (keyword only) where it takes ``carousel=``, and ``Batched2048.ntuple_play_log`` and
:func:`backward_train` run it inside the play-log launch (``g2048_ntuple_play_log_restart``,
``g2048_ntuple_log_train_restart``).  Opt-in.
``Downgrade``, :func:`downgrade`, ``Batched2048.downgraded_boards``, ``Batched2048.ntuple_play(..., downgrade=)``,
``play_games(..., downgrade=)`` and ``DowngradedPlayer`` are tile-downgrading, and ``NTupleNet.fill_value`` /
``NTupleNet(..., init_value=)`` optimistic initialisation -- the two ideas of Guei, Chen & Wu 2022 (``g2048_downgrade_*``,
``g2048_ntuple_play_downgraded``).  Opt-in.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import CarouselC, DowngradeC, RestartC, NTupleAdaptiveIO, NTupleDeepIO, NTupleReducedIO, NTupleDelayC, NTupleIO, NTupleMeanC, NTupleNetC, NTuplePlayIO, NTupleSearchIO, NTupleStagedNetC, NTupleTCC, NTupleTDIO, NTupleTraceC, check
from .analysis import _bind_out, _int_arg, _plain_boards

MAX_TUPLES, MAX_LEN, MAX_FRAC_BITS, MAX_LR_SHIFT = 8, 6, 16, 40   # G2048_NTUPLE_MAX_* (include/g2048.h)
ILLEGAL = -(1 << 63)                                              # G2048_NTUPLE_ILLEGAL: q of an illegal move
SEARCH_MAX_DEPTH = 2                                              # G2048_NTUPLE_SEARCH_MAX_DEPTH
DEEP_MIN_DEPTH, DEEP_MAX_DEPTH = 2, 3                             # G2048_NTUPLE_DEEP_MIN_DEPTH, G2048_NTUPLE_DEEP_MAX_DEPTH
ADAPTIVE_MAX_DEPTH, ADAPTIVE_SKIPPED = 4, 0xff                    # G2048_NTUPLE_ADAPTIVE_MAX_DEPTH, G2048_NTUPLE_ADAPTIVE_SKIPPED
REDUCE4_MIN, REDUCE4_MAX = 1, 2                                     # G2048_NTUPLE_REDUCE4_MIN, G2048_NTUPLE_REDUCE4_MAX
TC_WEIGHTS, TC_ACCUM = 1, 2                                       # G2048_NTUPLE_TC_WEIGHTS, G2048_NTUPLE_TC_ACCUM
MEAN_SUM, MEAN_APPLY = 1, 2                                       # G2048_NTUPLE_MEAN_SUM, G2048_NTUPLE_MEAN_APPLY
TRACE_MAX = 8                                                     # G2048_NTUPLE_TRACE_MAX
DELAY_STEP, DELAY_FLUSH = 0, 1                                    # G2048_NTUPLE_DELAY_STEP, G2048_NTUPLE_DELAY_FLUSH
MAX_STAGES = 8                                                    # G2048_NTUPLE_MAX_STAGES
CAROUSEL_MAX_CAPACITY = 65536                                     # G2048_CAROUSEL_MAX_CAPACITY
RESTART_MAX_STRIDE_LOG2, RESTART_MAX_CAPACITY = 16, 4096          # G2048_RESTART_MAX_STRIDE_LOG2, G2048_RESTART_MAX_CAPACITY
RESTART_MAX_RESTARTS = 2**32 - 1                                  # g2048_restart.max_restarts: 1..2^32 - 1
LOG_MAX_DEPTH, LOG_VALID, LOG_ENDED = 1024, 1, 2                  # G2048_NTUPLE_LOG_MAX_DEPTH, G2048_NTUPLE_LOG_VALID, G2048_NTUPLE_LOG_ENDED
NTUPLE_END = 0xff                                                 # G2048_NTUPLE_END: pads a cell list shorter than tuple_len
SEEN_UNKNOWN = 0xff                                               # Carousel.seen: the stage of the episode is not known yet
DOWNGRADE_MIN_FLOOR, DOWNGRADE_SKIPPED = 4, 0xff                  # G2048_DOWNGRADE_MIN_FLOOR, G2048_DOWNGRADE_SKIPPED

# Default shapes, as row-major cell indices (cell 4r + c).  The value sums every tuple over the eight symmetries of the
# board, so a shape lists each tuple once, not once per placement.
TUPLES = {
    # the 4 x 6-tuple network of Szubert & Jaskowski 2014: two 2x3 rectangles and two "axes"
    "4x6": ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10)),
    # all 17 straight and square 4-tuples -- 4 rows, 4 columns, 9 2x2 squares -- as the symmetric images of five: the
    # outer and the inner row, the corner, the edge and the centre square
    "17x4": ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (1, 2, 5, 6), (5, 6, 9, 10)),
    # redundant encoding (Jaskowski 2017): the 4x6 network plus four 4-tuples, each a sub-shape of one of its 6-tuples, so
    # that a rarely visited 6-tuple entry generalises through an often visited 4-tuple entry.  A mixed network.
    "4x6+4x4": ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10),
                (0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (5, 6, 9, 10)),
}


def stage_mask(*tiles) -> int:
    """The stage threshold "the board holds all of these tiles": the OR of ``1 << min(log2(tile), 15)`` over ``tiles`` (tile
    values, powers of two from 2 on), e.g. ``stage_mask(16384, 8192) == 0x6000``.  A board's mask has one bit per distinct
    cell value (bit 0: an empty cell), and its stage is the number of thresholds its mask is not below -- so a threshold is
    reached by every board that holds these tiles or any larger one."""
    if not tiles:
        raise ValueError("stage_mask needs at least one tile value")
    mask = 0
    for tile in tiles:
        tile = _int_arg("tile", tile, 2, 1 << 31)
        if tile & (tile - 1):
            raise ValueError(f"tile must be a power of two, not {tile}")
        mask |= 1 << min(tile.bit_length() - 1, 15)
    return mask


def _stage_thresholds(stages):
    """``stages`` of NTupleNet as a tuple of ints: at most 7, each 1..65535, strictly ascending."""
    try:
        stages = tuple(stages)
    except TypeError:
        raise ValueError("stages must be a sequence of thresholds (ints in 1..65535)") from None
    if len(stages) > MAX_STAGES - 1:
        raise ValueError(f"stages: at most {MAX_STAGES - 1} thresholds ({MAX_STAGES} stages), not {len(stages)}")
    stages = tuple(_int_arg("stages threshold", t, 1, 65535) for t in stages)
    if any(b <= a for a, b in zip(stages, stages[1:])):
        raise ValueError(f"stages: thresholds must be strictly ascending, not {stages}")
    return stages


class NTupleEval(NamedTuple):
    """Result of evaluate (``g2048_ntuple_evaluate``).  Device tensors; a field that is None was not asked for (``out``)."""
    value: Optional[torch.Tensor]        # int64 [n, 4]: q[d] = (merge score << F) + V(afterstate d); ILLEGAL where d is illegal
    action: Optional[torch.Tensor]       # uint8 [n]: the smallest d of largest q among the legal d; 0 when none is legal
    best: Optional[torch.Tensor]         # int64 [n]: q[action]; 0 when no move is legal
    after: Optional[torch.Tensor]        # uint8 [n, 16]: the afterstate of `action`; the board itself when no move is legal
    after_value: Optional[torch.Tensor]  # int64 [n]: V(after); 0 when no move is legal


def _check_tensor(name, t, dtypes, shape, device):
    """``t`` is a contiguous tensor of one of ``dtypes`` and of ``shape`` on ``device``, or ValueError."""
    if (not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
            or t.device != device):
        raise ValueError(f"{name} must be a contiguous {str(dtypes[0]).replace('torch.', '')} {list(shape)} tensor on {device}")


def _on_stream(fn, device, *args):
    """One library call on the current stream of ``device``."""
    with torch.cuda.device(device):
        check(fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))


def _eval_io(n, device, out):
    """(NTupleIO, NTupleEval) for n boards: ``out`` checked field by field, or freshly allocated outputs."""
    if out is None:
        i64 = dict(dtype=torch.int64, device=device)
        out = NTupleEval(torch.empty((n, 4), **i64), torch.empty(n, dtype=torch.uint8, device=device), torch.empty(n, **i64),
                         torch.empty((n, 16), dtype=torch.uint8, device=device), torch.empty(n, **i64))
    else:
        out = NTupleEval(*out)
        if all(t is None for t in out):
            raise ValueError("out requests no output (value, action, best, after and after_value are all None)")
    io = NTupleIO()
    _bind_out(io, out, {"value": ((n, 4), (torch.int64,)), "action": ((n,), (torch.uint8,)), "best": ((n,), (torch.int64,)),
                        "after": ((n, 16), (torch.uint8,)), "after_value": ((n,), (torch.int64,))}, device)
    return io, out


class NTupleSearch(NamedTuple):
    """Result of search (``g2048_ntuple_search``).  Device tensors; a field that is None was not asked for (``out``)."""
    action: Optional[torch.Tensor]       # uint8 [n]: the smallest d of largest value among the legal d; 0 when none is legal
    value: Optional[torch.Tensor]        # int64 [n, 4]: (merge score << F) + A_depth(afterstate d); ILLEGAL where d is illegal


def _search_io(n, device, depth, out, io_type=NTupleSearchIO, depths=(1, SEARCH_MAX_DEPTH)):
    """(io_type(depth, ...), NTupleSearch) for n boards: ``depth`` checked against ``depths``, ``out`` checked field by field or
    freshly allocated."""
    depth = _int_arg("depth", depth, *depths)
    if out is None:
        out = NTupleSearch(torch.empty(n, dtype=torch.uint8, device=device), torch.empty((n, 4), dtype=torch.int64, device=device))
    else:
        out = NTupleSearch(*out)
        if out.action is None and out.value is None:
            raise ValueError("out requests no output (action and value are both None)")
    io = io_type(depth)
    _bind_out(io, out, {"action": ((n,), (torch.uint8,)), "value": ((n, 4), (torch.int64,))}, device)
    return io, out


def _deep_io(n, device, depth, out, active=None):
    """``_search_io`` for the deep search: (NTupleDeepIO, NTupleSearch), depth 2..3, and ``active`` (engine forms) checked as
    ``_check_tensor`` checks."""
    io, out = _search_io(n, device, depth, out, NTupleDeepIO, (DEEP_MIN_DEPTH, DEEP_MAX_DEPTH))
    if active is not None:
        _check_tensor("active", active, (torch.uint32,), (n,), device)
        io.active = active.data_ptr()
    return io, out


class NTupleAdaptive(NamedTuple):
    """Result of adaptive_search (``g2048_ntuple_adaptive_search``).  Device tensors; a field that is None was not asked for."""
    action: Optional[torch.Tensor]       # uint8 [n]: as NTupleSearch.action, at the board's own depth
    value: Optional[torch.Tensor]        # int64 [n, 4]: as NTupleSearch.value (evaluate's q at depth 0)
    depth: Optional[torch.Tensor]        # uint8 [n]: the depth used, schedule[empty cells]; ADAPTIVE_SKIPPED for a masked-out board


def schedule_by_empties(depths, default) -> tuple:
    """The 17 entries of a search schedule, ``schedule[E]`` = the depth of a board with ``E`` empty cells, from
    ``{max_empty: depth, ...}``: a board gets the depth of the smallest ``max_empty`` that is not below its ``E``, and
    ``default`` above the largest.  ``schedule_by_empties({5: 3, 9: 2}, 1)`` is depth 3 for E <= 5, 2 for 6..9 and 1 above."""
    default = _int_arg("default", default, 0, ADAPTIVE_MAX_DEPTH)
    if not isinstance(depths, dict):
        raise ValueError("depths must be a dict {max_empty: depth}")
    steps = sorted((_int_arg("max_empty", e, 0, 16), _int_arg("depth", d, 0, ADAPTIVE_MAX_DEPTH)) for e, d in depths.items())
    return tuple(next((d for m, d in steps if e <= m), default) for e in range(17))


# Starting values: NOBODY HAS TIMED OR PLAYED THESE schedules against each other or against a fixed depth.  They follow
# the cost of a ply on a late-game board, about 37 times the ply before it (profiles/r21_ntuple_deep_probe.txt), and give
# the deepest level to the boards where one wrong move ends the game.
SCHEDULES = {
    "3-ply-late": schedule_by_empties({5: 3, 9: 2}, 1),
    "4-ply-late": schedule_by_empties({1: 4, 5: 3, 9: 2}, 1),
}


def _schedule(schedule) -> tuple:
    """``schedule`` as 17 depths in 0..ADAPTIVE_MAX_DEPTH: the name of a preset in SCHEDULES, or a sequence."""
    if isinstance(schedule, str):
        if schedule not in SCHEDULES:
            raise ValueError(f"schedule {schedule!r}: the presets are {sorted(SCHEDULES)}")
        return SCHEDULES[schedule]
    try:
        schedule = tuple(schedule)
    except TypeError:
        raise ValueError("schedule must be a preset name or a sequence of 17 depths") from None
    if len(schedule) != 17:
        raise ValueError(f"schedule needs 17 entries (0..16 empty cells), not {len(schedule)}")
    return tuple(_int_arg("schedule entry", d, 0, ADAPTIVE_MAX_DEPTH) for d in schedule)


def _adaptive_io(n, device, schedule, out, active=None, reduce4=None):
    """(NTupleAdaptiveIO, NTupleAdaptive) for n boards: ``schedule`` checked, ``out`` checked field by field or freshly
    allocated, ``active`` (engine forms) checked as ``_check_tensor`` checks.  With ``reduce4`` (checked) the structure is the
    NTupleReducedIO of the reduced search."""
    schedule = _schedule(schedule)
    if reduce4 is not None:
        reduce4 = _int_arg("reduce4", reduce4, REDUCE4_MIN, REDUCE4_MAX)
    if out is None:
        u8 = dict(dtype=torch.uint8, device=device)
        out = NTupleAdaptive(torch.empty(n, **u8), torch.empty((n, 4), dtype=torch.int64, device=device), torch.empty(n, **u8))
    else:
        out = NTupleAdaptive(*out)
        if out.action is None and out.value is None:
            raise ValueError("out requests no output (action and value are both None)")
    sched = (C.c_uint8 * 17)(*schedule)
    io = NTupleAdaptiveIO(sched) if reduce4 is None else NTupleReducedIO(sched, reduce4)
    _bind_out(io, out, {"action": ((n,), (torch.uint8,)), "value": ((n, 4), (torch.int64,)), "depth": ((n,), (torch.uint8,))}, device)
    if active is not None:
        _check_tensor("active", active, (torch.uint32,), (n,), device)
        io.active = active.data_ptr()
    return io, out


def _play_io(n, device, games_left, hist, moves):
    """NTuplePlayIO for n boards: every side output that is not None checked as ``_check_tensor`` checks."""
    io = NTuplePlayIO()
    for name, t, dtype, shape in (("games_left", games_left, torch.uint32, (n,)), ("hist", hist, torch.uint64, (32,)),
                                  ("moves", moves, torch.uint64, (1,))):
        if t is not None:
            _check_tensor(name, t, (dtype,), shape, device)
            setattr(io, name, t.data_ptr())
    return io


def _tile_exp(name, tile, lo, hi):
    """log2 of ``tile``, a power of two in 2^lo .. 2^hi."""
    tile = _int_arg(name, tile, 1 << lo, 1 << hi)
    if tile & (tile - 1):
        raise ValueError(f"{name} must be a power of two, not {tile}")
    return tile.bit_length() - 1


class Downgrade:
    """The rule of tile-downgrading (``g2048_downgrade``; after Guei, Chen & Wu 2022): at play time a board
    whose largest tile is at least ``min_tile`` is translated into a board the network knows better -- the largest tile value
    ``2^k >= floor_tile`` below its largest tile that is missing from the board, and not about to be made by two tiles
    ``2^(k-1)``, is picked and every tile above it is halved -- and the move is chosen on the translated board.  ``min_tile``: a
    power of two in 2..2^31; ``floor_tile``: one in 16..2^31.  The choice of the missing tile and its guard are this project's
    own, and activation is a parameter here (the paper activates on the 32768 tile)."""

    def __init__(self, min_tile=32768, floor_tile=16):
        self._c = DowngradeC(_tile_exp("min_tile", min_tile, 1, 31), _tile_exp("floor_tile", floor_tile, DOWNGRADE_MIN_FLOOR, 31))
        self.min_tile, self.floor_tile = int(min_tile), int(floor_tile)

    def __repr__(self):
        return f"Downgrade(min_tile={self.min_tile}, floor_tile={self.floor_tile})"


def _rule(rule):
    if not isinstance(rule, Downgrade):
        raise ValueError("rule must be a Downgrade")
    return C.byref(rule._c)


class Downgraded(NamedTuple):
    """Result of :func:`downgrade` / ``Batched2048.downgraded_boards``."""
    boards: torch.Tensor              # uint8 [n, 16]: the translated boards, plain exponents
    missing: Optional[torch.Tensor]   # uint8 [n]: the exponent k of the missing tile, 0 = unchanged, 0xff = masked out


def _downgraded_out(n, device, out):
    """(boards, missing) tensors of a translation: fresh ones, or those of ``out`` (missing may be None), checked."""
    if out is None:
        return Downgraded(torch.empty((n, 16), dtype=torch.uint8, device=device), torch.empty(n, dtype=torch.uint8, device=device))
    boards, missing = out
    _check_tensor("out.boards", boards, (torch.uint8,), (n, 16), device)
    if missing is not None:
        _check_tensor("out.missing", missing, (torch.uint8,), (n,), device)
    return Downgraded(boards, missing)


def downgrade(boards, rule, out=None) -> Downgraded:
    """Tile-downgrading of plain boards (``g2048_downgrade_plain``): ``boards`` a device ``uint8``
    ``[n, 16]`` or ``[n, 4, 4]`` tensor of exponents, ``rule`` a :class:`Downgrade`.  One launch on the current stream of the
    boards' device.  ``out``: a preallocated :class:`Downgraded` (``missing`` may be None); ``out.boards`` may be ``boards``
    itself (in place)."""
    n, device = _plain_boards(boards)
    ref = _rule(rule)
    out = _downgraded_out(n, device, out)
    _on_stream(_lib.load().g2048_downgrade_plain, device, boards.data_ptr(), n, ref, out.boards.data_ptr(),
               None if out.missing is None else out.missing.data_ptr())
    return out


class NTupleNet:
    """T tuples of L cells with a table of 16^L int32 weights each; a weight is a score in units of 2^-``frac_bits``.

    ``tuples``: a name in ``TUPLES`` or a sequence of equally long sequences of distinct cell indices 0..15 (at most 8
    tuples of at most 6 cells).  ``weights`` is the int32 ``[T, 16^L]`` tensor on ``device``, zero-initialised; the
    kernels read and update it in place, so it can be shared between engines.

    ``mixed``: True allows sequences of different lengths -- a mixed network (redundant encoding); a
    ragged name of ``TUPLES`` needs no flag, and with equal lengths the flag changes nothing.  Tuple t then has
    ``tuple_lens[t]`` cells and a table of ``16^tuple_lens[t]`` weights, the tables lie back to back from
    ``table_offsets[t]`` on, and ``weights`` is int32 ``[W]``, ``W = n_weights`` = the sum of the table sizes (``[S, W]``
    when staged); :meth:`table` views one table.  ``tuple_len`` is the longest length.

    ``init_value``: None (zero weights), or a score for :meth:`fill_value` -- optimistic initialisation.

    ``stages``: None, or a sequence of at most 7 strictly ascending thresholds in 1..65535 (:func:`stage_mask`) for a
    multi-stage network of ``S = len(stages) + 1`` weight sets: ``weights`` is then ``[S, T, 16^L]``,
    a board reads and updates the set ``stage(board)`` = the number of thresholds its tile mask is not below, and every
    method goes to its ``g2048_ntuple_staged_`` symbol.  The stage is a function of the board alone: the afterstates of one
    board, the leaves of a search and the slots of a trace may all be in different stages.  Memory: S times the unstaged
    network's."""

    def __init__(self, tuples="4x6", frac_bits=10, device="cuda:0", stages=None, mixed=False, init_value=None):
        if isinstance(tuples, str):
            if tuples not in TUPLES:
                raise ValueError(f"tuples must be one of {sorted(TUPLES)} or a sequence of cell lists, not {tuples!r}")
            tuples, mixed = TUPLES[tuples], True
        try:
            tuples = tuple(tuple(t) for t in tuples)
        except TypeError:
            raise ValueError("tuples must be a sequence of sequences of cell indices") from None
        if not 1 <= len(tuples) <= MAX_TUPLES:
            raise ValueError(f"tuples: need 1..{MAX_TUPLES} tuples, not {len(tuples)}")
        length = max(len(t) for t in tuples)
        if not all(1 <= len(t) <= MAX_LEN for t in tuples):
            raise ValueError(f"tuples: every tuple needs a length in 1..{MAX_LEN}")
        if not mixed and any(len(t) != length for t in tuples):
            raise ValueError(f"tuples: every tuple needs the same length in 1..{MAX_LEN} (mixed=True allows tuples of mixed length)")
        for t in tuples:
            cells = [_int_arg("tuples cell", c, 0, 15) for c in t]
            if len(set(cells)) != len(cells):
                raise ValueError(f"tuples: cell repeated within tuple {t}")
        self.tuples = tuple(tuple(int(c) for c in t) for t in tuples)
        self.frac_bits = _int_arg("frac_bits", frac_bits, 0, MAX_FRAC_BITS)
        self.device = torch.device(device)
        self.stages = None if stages is None else _stage_thresholds(stages)
        self.tuple_lens = tuple(len(t) for t in tuples)
        self.mixed = any(n != length for n in self.tuple_lens)
        sizes = [16 ** n for n in self.tuple_lens]
        self.table_offsets = tuple(sum(sizes[:t]) for t in range(len(sizes)))
        self.n_weights = sum(sizes)
        shape = (self.n_weights,) if self.mixed else (len(tuples), 16 ** length)
        if self.stages is None:
            self.weights = torch.zeros(shape, dtype=torch.int32, device=self.device)
            self._c = c_net = NTupleNetC(len(tuples), length, self.frac_bits)
        else:
            self.weights = torch.zeros((len(self.stages) + 1,) + shape, dtype=torch.int32, device=self.device)
            self._c = NTupleStagedNetC(NTupleNetC(len(tuples), length, self.frac_bits), len(self.stages) + 1)
            self._c.thresholds[:len(self.stages)] = self.stages
            c_net = self._c.net
        for t, cells in enumerate(self.tuples):
            for k in range(length):
                c_net.cells[t][k] = cells[k] if k < len(cells) else NTUPLE_END
        c_net.weights = self.weights.data_ptr()
        if init_value is not None:
            self.fill_value(init_value)

    def fill_value(self, score):
        """Optimistic initialisation (Guei, Chen & Wu 2022): every weight of every table and stage is set to
        ``floor((score << frac_bits) / (8 * T))``, so that ``V(b)`` is that constant times ``8 T`` -- ``score``, to within the
        rounding -- for every board, and an afterstate that was never tried looks as good as ``score`` until it is tried.
        ``score``: an int, in points.  ValueError when the weight does not fit in int32.  On the current stream of the weights'
        device; the accumulators of an :class:`NTupleTC` are not touched.  ``NTupleNet(..., init_value=score)`` is the same at
        construction."""
        score = _int_arg("score", score, -(1 << 62), 1 << 62)
        weight = (score << self.frac_bits) // (8 * self.n_tuples)
        if not -(1 << 31) <= weight < 1 << 31:
            raise ValueError(f"fill_value: score {score} needs the weight {weight}, which does not fit in int32 "
                             f"(frac_bits={self.frac_bits}, {self.n_tuples} tuples)")
        self.weights.fill_(weight)
        return self

    @property
    def n_tuples(self):
        return len(self.tuples)

    @property
    def tuple_len(self):
        return max(self.tuple_lens)

    def table(self, t, stage=None) -> torch.Tensor:
        """The table of tuple ``t`` as an int32 ``[16^tuple_lens[t]]`` view of ``weights``, of either layout; ``stage``: the
        weight set of a staged network (required there, None otherwise)."""
        t = _int_arg("t", t, 0, self.n_tuples - 1)
        if self.stages is None:
            if stage is not None:
                raise ValueError("table: stage is for a staged network (NTupleNet(..., stages=...))")
            flat = self.weights.reshape(-1)
        else:
            if stage is None:
                raise ValueError(f"table: a staged network needs stage in 0..{self.n_stages - 1}")
            flat = self.weights[_int_arg("stage", stage, 0, self.n_stages - 1)].reshape(-1)
        return flat[self.table_offsets[t]:self.table_offsets[t] + 16 ** self.tuple_lens[t]]

    @property
    def n_stages(self):
        return 1 if self.stages is None else len(self.stages) + 1

    def _ref(self, device):
        """The C descriptor, for a launch on ``device``."""
        if self.device != device:
            raise ValueError(f"the network's weights are on {self.device}, the boards on {device}")
        return C.byref(self._c)

    def _fn(self, name):
        """The library's ``g2048_ntuple_<name>``, or its ``g2048_ntuple_staged_<name>`` sibling for a staged network."""
        return getattr(_lib.load(), ("g2048_ntuple_" if self.stages is None else "g2048_ntuple_staged_") + name)

    def _launch(self, fn, boards, *args):
        _on_stream(fn, boards.device, boards.data_ptr(), boards.shape[0], *args)

    def _own_tc(self, tc):
        if not isinstance(tc, NTupleTC) or tc.net is not self:
            raise ValueError("tc must be the NTupleTC of this network")

    def _own_mean(self, mean):
        if not isinstance(mean, NTupleMean) or mean.net is not self:
            raise ValueError("mean must be the NTupleMean of this network")

    def values(self, boards, out=None) -> torch.Tensor:
        """V of plain boards (``g2048_ntuple_values_plain``): ``boards`` a device ``uint8`` ``[n, 16]`` or ``[n, 4, 4]``
        tensor of exponents; returns int64 ``[n]``."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=device)
        else:
            _check_tensor("out", out, (torch.int64,), (n,), device)
        self._launch(self._fn("values_plain"), boards, net, out.data_ptr())
        return out

    def stage(self, boards, out=None) -> torch.Tensor:
        """The stage of plain boards (``g2048_ntuple_stage_plain``): ``boards`` as in :meth:`values`; returns uint8 ``[n]``,
        the index of the weight set each board reads.  A staged network only."""
        if self.stages is None:
            raise ValueError("stage() needs a staged network (NTupleNet(..., stages=...))")
        n, device = _plain_boards(boards)
        net = self._ref(device)
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=device)
        else:
            _check_tensor("out", out, (torch.uint8,), (n,), device)
        self._launch(_lib.load().g2048_ntuple_stage_plain, boards, net, out.data_ptr())
        return out

    def promote(self, src, dst, tc=None):
        """Whole-stage weight promotion (Yeh et al. 2016): ``weights[dst] = weights[src]`` on the current stream -- a stage
        that is first reached starts from what an earlier stage has learned.  With ``tc`` (the :class:`NTupleTC` of this
        network) ``err[dst]`` and ``mag[dst]`` are zeroed, so the promoted stage learns at full rate again.  A staged
        network only; ``src != dst``.  (Lazy per-weight promotion is not offered: it would read weights that other lanes
        of the same launch update, and the result would depend on their order.)"""
        if self.stages is None:
            raise ValueError("promote() needs a staged network (NTupleNet(..., stages=...))")
        src = _int_arg("src", src, 0, self.n_stages - 1)
        dst = _int_arg("dst", dst, 0, self.n_stages - 1)
        if src == dst:
            raise ValueError(f"promote: src and dst are both stage {src}")
        if tc is not None:
            self._own_tc(tc)
        self.weights[dst].copy_(self.weights[src])          # torch: the current stream of the tensors' device
        if tc is not None:
            tc.err[dst].zero_()
            tc.mag[dst].zero_()

    def evaluate(self, boards, out=None) -> NTupleEval:
        """The greedy player on plain boards (``g2048_ntuple_evaluate_plain``): q of the four moves, the best move, its
        q, its afterstate and the afterstate's value, in one launch on the current stream of the boards' device.
        ``out``: a preallocated :class:`NTupleEval` (a field that is None is not written)."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        io, out = _eval_io(n, device, out)
        self._launch(self._fn("evaluate_plain"), boards, net, C.byref(io))
        return out

    def search(self, boards, depth=1, out=None) -> NTupleSearch:
        """Expectimax over the network's afterstate values on plain boards (``g2048_ntuple_search_plain``, INTEGRATION.md
        §10): ``depth`` 1..2 chance levels below the root move, :meth:`evaluate`'s ``best`` at the leaves (depth 0 is
        :meth:`evaluate`).  One launch on the current stream of the boards' device.  ``out``: a preallocated
        :class:`NTupleSearch` (a field that is None is not written)."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        io, out = _search_io(n, device, depth, out)
        self._launch(self._fn("search_plain"), boards, net, C.byref(io))
        return out

    def deep_search(self, boards, depth=3, out=None) -> NTupleSearch:
        """:meth:`search` at ``depth`` 2..3 on plain boards (``g2048_ntuple_deep_search_plain``): the same
        definition and the same :class:`NTupleSearch`, from the kernel that gives every board a workgroup; depth 2 gives the
        bits of ``search(boards, 2)``.  One launch on the current stream of the boards' device.  The cost grows steeply with
        the empty cells of a board: about 10^4..10^5 network evaluations on a board with 1..6 empty cells at depth 3, up to
        about 2 * 10^6 on a nearly empty one (counts from the definition).  Measured on the MI355X
        (``profiles/r21_ntuple_deep_probe.txt``): 14.6 ms per launch for 1 024 late-game boards and 120 ms for 1 024 mid-game
        boards with the 4x6 network; other shapes, sizes above 4 096 boards and staged networks have not been timed."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        io, out = _deep_io(n, device, depth, out)
        self._launch(self._fn("deep_search_plain"), boards, net, C.byref(io))
        return out

    def adaptive_search(self, boards, schedule, out=None) -> NTupleAdaptive:
        """:meth:`search` at a depth per board on plain boards (``g2048_ntuple_adaptive_search_plain``):
        board ``i`` is searched at ``schedule[E]`` in 0..4 for its own number ``E`` of empty cells, in one launch on the current
        stream of the boards' device.  ``schedule``: 17 depths (:func:`schedule_by_empties`) or the name of a preset in
        ``SCHEDULES``.  Depth 0 gives the bits of :meth:`evaluate`, 1..2 those of :meth:`search`, 2..3 those of
        :meth:`deep_search`; depth 4 exists here only.  ``out``: a preallocated :class:`NTupleAdaptive` (a field that is None is
        not written; ``action`` or ``value`` must be given)."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        io, out = _adaptive_io(n, device, schedule, out)
        self._launch(self._fn("adaptive_search_plain"), boards, net, C.byref(io))
        return out

    def reduced_search(self, boards, schedule, reduce4=1, out=None) -> NTupleAdaptive:
        """:meth:`adaptive_search` with the rare branches searched shallower (``g2048_ntuple_reduced_search_plain``,
        INTEGRATION.md §23): a child board made by a 4 spawn, a tenth of its chance node's weight, is searched ``reduce4``
        (1..2) plies shallower than its 2 sibling, at every level of the tree.  ``schedule`` and ``out`` as
        :meth:`adaptive_search` takes them; ``depth`` of the result is the schedule's depth, not a reduced one.  Depth 0 gives
        the bits of :meth:`evaluate` and depth 1 those of :meth:`search` at depth 1."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        io, out = _adaptive_io(n, device, schedule, out, reduce4=reduce4)
        self._launch(self._fn("reduced_search_plain"), boards, net, C.byref(io))
        return out

    def update(self, boards, delta, lr_shift):
        """``weights[t][idx_t(s(board_i))] += sat_int32(delta_i >> lr_shift)`` for every symmetry s and tuple t of every
        board (``g2048_ntuple_update_plain``): ``boards`` as in :meth:`values`, ``delta`` a device int64 ``[n]`` tensor,
        ``lr_shift`` 0..40.  One launch of integer atomic adds: the result does not depend on their order."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        _check_tensor("delta", delta, (torch.int64,), (n,), device)
        shift = _int_arg("lr_shift", lr_shift, 0, MAX_LR_SHIFT)
        self._launch(self._fn("update_plain"), boards, delta.data_ptr(), shift, net)

    def tc_update(self, boards, delta, lr_shift, tc, phases=3):
        """The temporal-coherence update (``g2048_ntuple_tc_update_plain``) with the accumulators of
        ``tc`` (an :class:`NTupleTC` of this network): phase W (``phases`` bit 1) adds
        ``sat_int32((d_i * rate(err, mag)) >> (16 + lr_shift))`` to every weight a board reaches, with the accumulators of
        before the call; phase A (bit 2) adds ``d_i`` to ``err`` and ``|d_i|`` to ``mag``.  ``boards``, ``delta`` and
        ``lr_shift`` as in :meth:`update`.  ``phases=3`` is two launches, W then A; shards that share the network run
        W on every shard, then A on every shard."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        _check_tensor("delta", delta, (torch.int64,), (n,), device)
        shift = _int_arg("lr_shift", lr_shift, 0, MAX_LR_SHIFT)
        phases = _int_arg("phases", phases, TC_WEIGHTS, TC_WEIGHTS | TC_ACCUM)
        self._own_tc(tc)
        self._launch(self._fn("tc_update_plain"), boards, delta.data_ptr(), shift, phases, net, C.byref(tc._c))

    def _trace_args(self, trace, delta, lr_shift):
        """(net, lr_shift) for a trace update: ``trace`` and ``delta`` checked as :meth:`update` checks its arguments."""
        if not isinstance(trace, NTupleTrace):
            raise ValueError("trace must be an NTupleTrace")
        net = self._ref(trace.device)
        _check_tensor("delta", delta, (torch.int64,), (trace.n,), trace.device)
        return net, _int_arg("lr_shift", lr_shift, 0, MAX_LR_SHIFT)

    def trace_update(self, trace, delta, lr_shift):
        """The TD(lambda) update (``g2048_ntuple_trace_update``): for the k-th last afterstate pushed
        into ``trace`` (an :class:`NTupleTrace`), k below the board's history length, :meth:`update` with
        ``d_k = (clamp(delta) * lam^k) >> 16``.  ``delta`` a device int64 ``[trace.n]`` tensor, ``lr_shift`` 0..40.  One
        launch of integer atomic adds."""
        net, shift = self._trace_args(trace, delta, lr_shift)
        _on_stream(self._fn("trace_update"), trace.device, trace.n, delta.data_ptr(), shift, net, C.byref(trace._c), trace.slot)

    def tc_trace_update(self, trace, delta, lr_shift, tc, phases=3):
        """The TC(lambda) update (``g2048_ntuple_tc_trace_update``): :meth:`tc_update` with ``d_k`` for
        the k-th last afterstate of ``trace``.  ``phases=3`` is two launches, W then A; shards that share the network run W
        on every shard, then A on every shard."""
        net, shift = self._trace_args(trace, delta, lr_shift)
        phases = _int_arg("phases", phases, TC_WEIGHTS, TC_WEIGHTS | TC_ACCUM)
        self._own_tc(tc)
        _on_stream(self._fn("tc_trace_update"), trace.device, trace.n, delta.data_ptr(), shift, phases, net, C.byref(tc._c),
                   C.byref(trace._c), trace.slot)

    def mean_update(self, boards, delta, lr_shift, mean, phases=3):
        """The batch-mean update (``g2048_ntuple_mean_update_plain``) with the state of ``mean`` (an
        :class:`NTupleMean` of this network): every entry the boards reach moves ONCE, by
        ``sat_int32(floor(sum / count) >> lr_shift)``, the mean of the clamped deltas that reached it -- not once per reach as in
        :meth:`update` -- so the learning rate of an entry does not grow with the batch.  Phase SUM (``phases`` bit 1) adds every
        ``d_i`` to ``mean.sum`` and 1 to ``mean.count``; phase APPLY (bit 2) moves the weights and zeroes both.  ``boards``,
        ``delta`` and ``lr_shift`` as in :meth:`update`; fewer than 2^29 boards.  ``phases=3`` is two launches, SUM then APPLY;
        shards that share the network and ``mean`` run SUM on every shard, then APPLY on every shard."""
        n, device = _plain_boards(boards)
        net = self._ref(device)
        _check_tensor("delta", delta, (torch.int64,), (n,), device)
        shift = _int_arg("lr_shift", lr_shift, 0, MAX_LR_SHIFT)
        phases = _int_arg("phases", phases, MEAN_SUM, MEAN_SUM | MEAN_APPLY)
        self._own_mean(mean)
        self._launch(self._fn("mean_update_plain"), boards, delta.data_ptr(), shift, phases, net, C.byref(mean._c))

    def mean_trace_update(self, trace, delta, lr_shift, mean, phases=3):
        """The batch-mean TD(lambda) update (``g2048_ntuple_mean_trace_update``): :meth:`mean_update` with
        ``d_k`` for the k-th last afterstate of ``trace``, the items of :meth:`trace_update`; ``trace.depth * trace.n`` below
        2^29.  ``phases=3`` is two launches, SUM then APPLY; shards run SUM on every shard, then APPLY on every shard."""
        net, shift = self._trace_args(trace, delta, lr_shift)
        phases = _int_arg("phases", phases, MEAN_SUM, MEAN_SUM | MEAN_APPLY)
        self._own_mean(mean)
        _on_stream(self._fn("mean_trace_update"), trace.device, trace.n, delta.data_ptr(), shift, phases, net, C.byref(mean._c),
                   C.byref(trace._c), trace.slot)

    def log_delta(self, log, m, out=None) -> torch.Tensor:
        """The backward error of slot ``m`` (0..M-1) of ``log`` (an :class:`NTupleLog`; ``g2048_ntuple_log_delta``, INTEGRATION.md
        §24), int64 ``[n]``, one launch on the current stream: 0 where slot ``m`` holds nothing; ``-V(after[m])`` where its move
        ended the episode; 0 where slot ``m + 1`` holds nothing; else ``gain[m+1] + V(after[m+1]) - V(after[m])``.  Reads the log
        and the weights only; ``V`` is :meth:`values` of the slot.  ``out``: a preallocated tensor."""
        if not isinstance(log, NTupleLog):
            raise ValueError("log must be an NTupleLog")
        net = self._ref(log.device)
        m = _int_arg("m", m, 0, log.depth - 1)
        if out is None:
            out = torch.empty(log.n, dtype=torch.int64, device=log.device)
        else:
            _check_tensor("out", out, (torch.int64,), (log.n,), log.device)
        _on_stream(self._fn("log_delta"), log.device, log.n, net, C.byref(log._c), m, out.data_ptr())
        return out

    def _delay_args(self, delay, lr_shift, flush):
        """(net, lr_shift, mode) for a delay update: ``delay`` checked as :meth:`trace_update` checks its trace."""
        if not isinstance(delay, NTupleDelay):
            raise ValueError("delay must be an NTupleDelay")
        net = self._ref(delay.device)
        if not isinstance(flush, (bool, int)) or int(flush) not in (DELAY_STEP, DELAY_FLUSH):
            raise ValueError(f"flush must be False (the step update) or True (the flush), not {flush!r}")
        return net, _int_arg("lr_shift", lr_shift, 0, MAX_LR_SHIFT), int(flush)

    def delay_update(self, delay, lr_shift, flush=False):
        """The delayed TD(lambda) update (``g2048_ntuple_delay_update``): :meth:`update` of every
        afterstate of ``delay`` (an :class:`NTupleDelay`) that is due, with the error it has collected, clamped to
        +-2^40.  ``flush=False`` is the update after every push: due are the afterstate that leaves the ring at the next push
        and every afterstate of a board whose episode ended at the last push.  ``flush=True`` applies what is still pending,
        once, right after a step update and before ``delay.reset()``; twice, or without that step update, errors are
        applied twice or not at all.  One launch of integer atomic adds.  Measured (profiles/r22_ntuple_delay_probe.txt): at
        2^20 boards and H = 4 it takes 1.08 to 1.2 times the one-step update where the trace update takes 4.2 to 4.4 times; at
        1 024 boards a training step is bound by launch issue and the delayed trainers are not faster end to end."""
        net, shift, mode = self._delay_args(delay, lr_shift, flush)
        _on_stream(self._fn("delay_update"), delay.device, delay.n, shift, mode, net, C.byref(delay._c), delay.slot)

    def tc_delay_update(self, delay, lr_shift, tc, phases=3, flush=False):
        """The delayed TC(lambda) update (``g2048_ntuple_tc_delay_update``): :meth:`tc_update` of every
        due afterstate of ``delay`` with its collected error; ``flush`` as in :meth:`delay_update`.  ``phases=3`` is two
        launches, W then A; shards that share the network run W on every shard, then A on every shard."""
        net, shift, mode = self._delay_args(delay, lr_shift, flush)
        phases = _int_arg("phases", phases, TC_WEIGHTS, TC_WEIGHTS | TC_ACCUM)
        self._own_tc(tc)
        _on_stream(self._fn("tc_delay_update"), delay.device, delay.n, shift, phases, mode, net, C.byref(tc._c), C.byref(delay._c),
                   delay.slot)

    def state_dict(self):
        return {"tuples": self.tuples, "frac_bits": self.frac_bits, "stages": self.stages, "weights": self.weights.clone()}

    def load_state_dict(self, state):
        """Copy the weights of a ``state_dict()`` of a network of the same shape into this one's tensor (in place)."""
        if tuple(tuple(t) for t in state["tuples"]) != self.tuples or int(state["frac_bits"]) != self.frac_bits:
            raise ValueError("state_dict is of a network with other tuples or frac_bits")
        stages = state.get("stages")                       # absent in the state of a network saved before stages existed
        if (None if stages is None else tuple(int(t) for t in stages)) != self.stages:
            raise ValueError(f"state_dict is of a network with stages {stages}, this one has {self.stages}")
        w = torch.as_tensor(state["weights"])
        if w.dtype != torch.int32 or w.shape != self.weights.shape:
            raise ValueError(f"state_dict weights must be int32 {tuple(self.weights.shape)}")
        self.weights.copy_(w)


class NTupleTC:
    """The accumulators of temporal-coherence learning for ``net`` (``g2048_ntuple_tc``): ``err``, the
    signed sum of the deltas every weight has seen, and ``mag``, the sum of their magnitudes (read as unsigned), both
    int64 tensors of the shape of ``net.weights`` (``[T, 16^L]``, ``[S, T, 16^L]`` for a staged network, ``[W]`` or ``[S, W]``
    for a mixed one) on the network's device, zero-initialised; a weight learns at rate ``|err| / mag``.

    Memory: 16 bytes per weight on top of the weight's own 4 -- 256 MiB per table for the 4x6 network (1 GiB in all), 5 MiB
    in all for the 17x4 network, 1 GiB + 4 MiB for the mixed "4x6+4x4" (the uniform eight 6-tuples it replaces: 2 GiB); a
    staged network takes S times that."""

    def __init__(self, net):
        if not isinstance(net, NTupleNet):
            raise ValueError("net must be an NTupleNet")
        self.net = net
        self.err = torch.zeros(tuple(net.weights.shape), dtype=torch.int64, device=net.device)
        self.mag = torch.zeros(tuple(net.weights.shape), dtype=torch.int64, device=net.device)
        self._c = NTupleTCC(self.err.data_ptr(), self.mag.data_ptr())

    def state_dict(self):
        return {"err": self.err.clone(), "mag": self.mag.clone()}

    def load_state_dict(self, state):
        """Copy the accumulators of a ``state_dict()`` of the same shape into this one's tensors (in place)."""
        err, mag = torch.as_tensor(state["err"]), torch.as_tensor(state["mag"])
        for name, t in (("err", err), ("mag", mag)):
            if t.dtype != torch.int64 or t.shape != self.err.shape:
                raise ValueError(f"state_dict {name} must be int64 {tuple(self.err.shape)}")
        self.err.copy_(err)
        self.mag.copy_(mag)


class NTupleMean:
    """The state of the batch-mean update for ``net`` (``g2048_ntuple_mean``): ``sum``, int64, the sum of
    the errors that have reached every weight in the call under way, and ``count``, int32 storage read as unsigned 32-bit, the
    number of reaches -- both of the shape of ``net.weights`` on the network's device.  Both are zero between calls: phase APPLY
    zeroes what phase SUM wrote.  :meth:`reset` zeroes them by hand, after a call that ran SUM without APPLY.

    Memory: 12 bytes per weight on top of the weight's own 4 -- 768 MiB in all for the 4x6 network."""

    def __init__(self, net):
        if not isinstance(net, NTupleNet):
            raise ValueError("net must be an NTupleNet")
        self.net = net
        self.sum = torch.zeros(tuple(net.weights.shape), dtype=torch.int64, device=net.device)
        self.count = torch.zeros(tuple(net.weights.shape), dtype=torch.int32, device=net.device)
        self._c = NTupleMeanC(self.sum.data_ptr(), self.count.data_ptr())

    def reset(self):
        """Zero ``sum`` and ``count`` on the current stream: drops whatever a phase SUM without its APPLY left pending."""
        self.sum.zero_()
        self.count.zero_()


class _NTupleHistory:
    """What :class:`NTupleTrace` and :class:`NTupleDelay` share: the ring of the last ``depth`` afterstates of ``n`` boards
    and the slot of the last push.  A subclass names itself in messages (``_noun``), its push in the library (``_push``)
    and its tensors (``_tensors``, the ``hist`` and ``len`` made here first), and builds ``_c`` over them."""

    _noun = _push = None
    _tensors = ("hist", "len")

    def __init__(self, n, depth=4, lam=0.5, device="cuda:0"):
        self.n = _int_arg("n", n, 1, 0xffffff00)
        self.depth = _int_arg("depth", depth, 1, TRACE_MAX)
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= lam <= 1.0:
            raise ValueError(f"lam must be a number in 0..1, not {lam!r}")
        self.lam_q16 = int(round(lam * 65536))
        self.device = torch.device(device)
        self.hist = torch.zeros((self.depth, self.n, 16), dtype=torch.uint8, device=self.device)
        self.len = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self.slot = self.depth - 1                      # the slot of the last push: the first push goes into slot 0

    def reset(self):
        """Forget every board's history (``len`` = 0) -- of a delay, pending errors included: flush first.  The slot counter
        keeps running."""
        self.len.zero_()

    def push(self, after, after_value, best_next, terminated, out):
        """Advance the slot and push (``g2048_ntuple_trace_push`` or ``g2048_ntuple_delay_push``), one launch on the current
        stream: store ``after`` (uint8 ``[n, 16]``) into the slot, update ``len`` with ``terminated`` (uint8 or bool ``[n]``),
        and write ``out = (0 if terminated else best_next) - after_value`` (int64 ``[n]`` each); a delay also adds
        ``clamp(out)``, decayed, to the accumulators of the board's valid slots.  Returns ``out``."""
        n, dev = self.n, self.device
        for name, t, shape, dtypes in (("after", after, (n, 16), (torch.uint8,)), ("after_value", after_value, (n,), (torch.int64,)),
                                       ("best_next", best_next, (n,), (torch.int64,)),
                                       ("terminated", terminated, (n,), (torch.uint8, torch.bool)), ("out", out, (n,), (torch.int64,))):
            _check_tensor(name, t, dtypes, shape, dev)
        slot = (self.slot + 1) % self.depth
        _on_stream(getattr(_lib.load(), self._push), dev, after.data_ptr(), after_value.data_ptr(), best_next.data_ptr(),
                   terminated.data_ptr(), n, C.byref(self._c), slot, out.data_ptr())
        self.slot = slot
        return out

    def state_dict(self):
        return {"depth": self.depth, "lam_q16": self.lam_q16, "slot": self.slot,
                **{name: getattr(self, name).clone() for name in self._tensors}}

    def load_state_dict(self, state):
        """Copy the tensors and the slot counter of a ``state_dict()`` of one of the same kind and shape into this one (in
        place)."""
        if int(state["depth"]) != self.depth or int(state["lam_q16"]) != self.lam_q16:
            raise ValueError(f"state_dict is of a {self._noun} with another depth or lam")
        new = {name: torch.as_tensor(state[name]) for name in self._tensors}
        for name in self._tensors:
            mine = getattr(self, name)
            if new[name].dtype != mine.dtype or new[name].shape != mine.shape:
                raise ValueError(f"state_dict {name} must be {str(mine.dtype).replace('torch.', '')} {tuple(mine.shape)}")
        slot = _int_arg("state_dict slot", state["slot"], 0, self.depth - 1)
        for name in self._tensors:
            getattr(self, name).copy_(new[name])
        self.slot = slot


class NTupleTrace(_NTupleHistory):
    """The history of the n-tuple traces for ``n`` boards (``g2048_ntuple_trace``): ``hist``, the last
    ``depth`` (H, 1..8) afterstates of every board as a uint8 ``[H, n, 16]`` ring, ``len``, uint8 ``[n]`` (bits 0..6 the
    number of valid slots, bit 7 "the episode ended at the last push"), and the slot of the last push.  ``lam`` is a float in
    0..1, stored as ``lam_q16 = round(lam * 65536)``.  One per engine or shard; call :meth:`reset` after ``engine.reset()``.

    Memory: 16 H + 1 bytes per board."""

    _noun, _push = "trace", "g2048_ntuple_trace_push"

    def __init__(self, n, depth=4, lam=0.5, device="cuda:0"):
        super().__init__(n, depth, lam, device)
        self._c = NTupleTraceC(self.depth, self.lam_q16, self.hist.data_ptr(), self.len.data_ptr())


class NTupleDelay(_NTupleHistory):
    """The delay ring of the delayed learners for ``n`` boards (``g2048_ntuple_delay``): the ``hist`` and
    ``len`` of an :class:`NTupleTrace`, plus ``acc``, int64 ``[H, n]``, the error every afterstate of the ring has collected
    so far, and the slot of the last push.  ``depth`` (H) in 1..8, ``lam`` a float in 0..1 stored as
    ``lam_q16 = round(lam * 65536)``.  One per engine or shard.  An afterstate is applied to the tables once, by
    ``NTupleNet.delay_update`` / ``tc_delay_update``, when it leaves the ring or its episode ends; before the ring is dropped
    or :meth:`reset`, the pending errors are applied by one update with ``flush=True`` (the ``delayed_*_train`` functions
    do that).

    Memory: 24 H + 1 bytes per board."""

    _noun, _push = "delay", "g2048_ntuple_delay_push"
    _tensors = ("hist", "len", "acc")

    def __init__(self, n, depth=4, lam=0.5, device="cuda:0"):
        super().__init__(n, depth, lam, device)
        self.acc = torch.zeros((self.depth, self.n), dtype=torch.int64, device=self.device)
        self._c = NTupleDelayC(self.depth, self.lam_q16, self.hist.data_ptr(), self.len.data_ptr(), self.acc.data_ptr())


class Carousel:
    """Carousel shaping for ``n`` boards (``g2048_carousel``; Jaskowski 2017): stage-balanced restarts.

    Every episode starts from an empty board, so the late weight sets of a staged network see only the rare boards that
    survive that long.  The carousel keeps, per stage ``k >= 1``, a ring ``pool[k]`` of the last ``capacity`` engine records
    on which an episode *entered* stage ``k`` (its stage rose above every stage the episode had been in), and :meth:`step`,
    run right after a step with auto-reset on, restarts a board whose episode has just ended from ``pool[k]``,
    ``k = (global board index + episodes the board has ended) mod (highest stage entered so far + 1)``; ``k = 0``, and a
    stage nothing has entered yet, keep the fresh board.  Everything is integers and index-ordered: the same bits whatever
    the launch geometry.

    ``net_or_stages``: a staged :class:`NTupleNet`, or the sequence of thresholds (as its ``stages``).  Tensors on ``device``:
    ``pool`` uint8 ``[S, capacity, 16]`` (records, verbatim: cells and packed score), ``count`` int64 ``[S]`` (read as
    unsigned: entries ever made), ``seen`` uint8 ``[n]`` (the highest stage of the running episode, 0xff: not yet known),
    ``episodes`` int32 ``[n]`` (read as unsigned, wraps).  One per engine or shard -- a pool depends on which boards feed it,
    so a sharded run does *not* repeat the unsharded one.  A restarted board carries the score it was recorded with:
    ``engine.scores()`` and the episode statistics then describe composite episodes.  Call :meth:`reset` after
    ``engine.reset()``.

    Memory: 16 S capacity + 5 n bytes, and 64 KiB of scratch."""

    def __init__(self, net_or_stages, n, capacity=1024, seed=0, device="cuda:0"):
        if isinstance(net_or_stages, NTupleNet):
            if net_or_stages.stages is None:
                raise ValueError("a carousel needs a staged network (NTupleNet(..., stages=...))")
            stages = net_or_stages.stages
        else:
            stages = _stage_thresholds(net_or_stages)
        if not stages:
            raise ValueError("a carousel needs at least one stage threshold (two stages)")
        self.stages = stages
        self.n = _int_arg("n", n, 1, 0xffffff00)
        self.capacity = _int_arg("capacity", capacity, 1, CAROUSEL_MAX_CAPACITY)
        self.seed = _int_arg("seed", seed, 0, 2**64 - 1)
        self.device = torch.device(device)
        S = self.n_stages
        self.pool = torch.zeros((S, self.capacity, 16), dtype=torch.uint8, device=self.device)
        self.count = torch.zeros(S, dtype=torch.int64, device=self.device)
        self.seen = torch.full((self.n,), SEEN_UNKNOWN, dtype=torch.uint8, device=self.device)
        self.episodes = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self._scratch = torch.empty(int(_lib.load().g2048_carousel_scratch_bytes(self.n)) // 4, dtype=torch.int32, device=self.device)
        self._c = CarouselC(S, (C.c_uint16 * 7)(*stages), self.capacity, self.seed, self.pool.data_ptr(), self.count.data_ptr(),
                            self.seen.data_ptr(), self.episodes.data_ptr(), self._scratch.data_ptr())

    @property
    def n_stages(self):
        return len(self.stages) + 1

    def reset(self):
        """Forget which stage every running episode has been in (``seen`` = 0xff); the pool and ``episodes`` stay."""
        self.seen.fill_(SEEN_UNKNOWN)

    def step(self, engine):
        """The carousel step on the live records of ``engine`` (``g2048_carousel_step``) with ``engine.terminated`` of the
        step just made (auto-reset on): three launches at most on the engine's stream, no host synchronisation."""
        if engine.n_envs != self.n or engine.device != self.device:
            raise ValueError(f"the carousel is for {self.n} boards on {self.device}, the engine has {engine.n_envs} on {engine.device}")
        check(_lib.load().g2048_carousel_step(engine._h, C.byref(self._c), engine.terminated.data_ptr(), engine._stream()))

    def step_plain(self, records, terminated, index_offset=0):
        """The same on any device uint8 ``[n, 16]`` tensor of engine records, updated in place (``g2048_carousel_step_plain``);
        ``terminated`` uint8 or bool ``[n]``; the global index of row i is ``index_offset + i``."""
        _check_tensor("records", records, (torch.uint8,), (self.n, 16), self.device)
        _check_tensor("terminated", terminated, (torch.uint8, torch.bool), (self.n,), self.device)
        index_offset = _int_arg("index_offset", index_offset, 0, 2**32 - self.n)
        _on_stream(_lib.load().g2048_carousel_step_plain, self.device, records.data_ptr(), self.n, index_offset, terminated.data_ptr(),
                   C.byref(self._c))

    def state_dict(self):
        return {"stages": self.stages, "capacity": self.capacity, "seed": self.seed, "pool": self.pool.clone(),
                "count": self.count.clone(), "seen": self.seen.clone(), "episodes": self.episodes.clone()}

    def load_state_dict(self, state):
        """Copy the pool, the counters and the per-board state of a ``state_dict()`` of a carousel of the same shape into this
        one (in place)."""
        if tuple(int(t) for t in state["stages"]) != self.stages or int(state["capacity"]) != self.capacity:
            raise ValueError("state_dict is of a carousel with other stages or another capacity")
        if int(state["seed"]) != self.seed:
            raise ValueError(f"state_dict is of a carousel with seed {state['seed']}, this one has {self.seed}")
        new = {}
        for name, mine in (("pool", self.pool), ("count", self.count), ("seen", self.seen), ("episodes", self.episodes)):
            t = torch.as_tensor(state[name])
            if t.dtype != mine.dtype or t.shape != mine.shape:
                raise ValueError(f"state_dict {name} must be {str(mine.dtype).replace('torch.', '')} {tuple(mine.shape)}")
            new[name] = t
        seen = new["seen"]
        if bool(((seen >= self.n_stages) & (seen != SEEN_UNKNOWN)).any()):
            raise ValueError(f"state_dict seen must hold stages below {self.n_stages} or 0xff")
        for name, mine in (("pool", self.pool), ("count", self.count), ("seen", self.seen), ("episodes", self.episodes)):
            mine.copy_(new[name])


class _Rides:
    """A :class:`Restart` given as ``restart=``, on its way through the ``carousel`` argument of the trainers (``_restart_keyword``)."""

    def __init__(self, restart):
        self.restart = restart


def _carousel_of(engine, carousel):
    """``carousel`` checked against the engine: the object whose ``step(engine)`` runs right behind the step."""
    if isinstance(carousel, _Rides):
        return _restart_of(engine, carousel.restart)
    if not isinstance(carousel, Carousel) or carousel.n != engine.n_envs or carousel.device != engine.device:
        raise ValueError(f"carousel must be a Carousel of {engine.n_envs} boards on {engine.device}")
    return carousel


class Restart:
    """Midpoint restart for ``n`` boards (``g2048_restart``; the restart of Matsuzaki 2017): a board whose
    episode has just ended goes back to the middle of the run that ended, so that late-game positions -- where the value function
    is worst -- are met more often.  For any network: no stages, no pool, no batch-wide rank.

    Every ``stride`` (a power of two, 1..65536) positions the board's engine record is kept in the next of ``capacity`` (1..4096)
    slots, ``snap`` uint8 ``[capacity, n, 16]`` (records, verbatim: cells and packed score).  :meth:`step`, run right after a step
    with auto-reset on, counts the position of every board that goes on (``pos``) and, where an episode ended after a run of
    ``R = pos - start`` positions, restarts it from the last snapshot at or below ``start + R // 2`` -- if ``R >= min_span``, the
    lineage has made fewer than ``max_restarts`` restarts and that snapshot lies beyond ``start``; otherwise the fresh board stays
    and ``pos``, ``start`` and ``restarts`` (int32 ``[n]`` each, read as unsigned) return to 0.  Everything is integers and a
    function of the board's own history: the same bits whatever the launch geometry, and -- unlike :class:`Carousel` -- the
    shards of a batch reproduce the unsharded run.  The paper records whole games and restarts exactly at the middle; here the
    restart point is up to ``stride - 1`` positions earlier, and earlier still once the middle lies beyond ``capacity * stride``.
    A restarted board carries the score it was recorded with: ``engine.scores()`` and the episode statistics then describe
    composite episodes.  One per engine or shard; call :meth:`reset` after ``engine.reset()``.

    Memory: 16 capacity + 12 bytes per board."""

    def __init__(self, n, stride=16, capacity=256, min_span=64, max_restarts=RESTART_MAX_RESTARTS, device="cuda:0"):
        self.n = _int_arg("n", n, 1, 0xffffff00)
        self.stride = _int_arg("stride", stride, 1, 1 << RESTART_MAX_STRIDE_LOG2)
        if self.stride & (self.stride - 1):
            raise ValueError(f"stride={stride}: need a power of two")
        self.capacity = _int_arg("capacity", capacity, 1, RESTART_MAX_CAPACITY)
        self.min_span = _int_arg("min_span", min_span, 2, 1 << 31)
        self.max_restarts = _int_arg("max_restarts", max_restarts, 1, RESTART_MAX_RESTARTS)
        self.device = torch.device(device)
        self.snap = torch.zeros((self.capacity, self.n, 16), dtype=torch.uint8, device=self.device)
        self.pos = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.start = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.restarts = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self._c = RestartC(self.stride.bit_length() - 1, self.capacity, self.min_span, self.max_restarts, self.snap.data_ptr(),
                           self.pos.data_ptr(), self.start.data_ptr(), self.restarts.data_ptr())

    def reset(self):
        """Every board is at the start of a fresh game again (``pos`` = ``start`` = ``restarts`` = 0); no snapshot is read before
        it is written again, so ``snap`` stays."""
        self.pos.zero_()
        self.start.zero_()
        self.restarts.zero_()

    def step(self, engine):
        """The restart step on the live records of ``engine`` (``g2048_restart_step``) with ``engine.terminated`` of the step just
        made (auto-reset on): one launch on the engine's stream, no host synchronisation."""
        if engine.n_envs != self.n or engine.device != self.device:
            raise ValueError(f"the restart is for {self.n} boards on {self.device}, the engine has {engine.n_envs} on {engine.device}")
        check(_lib.load().g2048_restart_step(engine._h, C.byref(self._c), engine.terminated.data_ptr(), engine._stream()))

    def step_plain(self, records, terminated):
        """The same on any device uint8 ``[n, 16]`` tensor of engine records, updated in place (``g2048_restart_step_plain``);
        ``terminated`` uint8 or bool ``[n]``."""
        _check_tensor("records", records, (torch.uint8,), (self.n, 16), self.device)
        _check_tensor("terminated", terminated, (torch.uint8, torch.bool), (self.n,), self.device)
        _on_stream(_lib.load().g2048_restart_step_plain, self.device, records.data_ptr(), self.n, terminated.data_ptr(), C.byref(self._c))

    def state_dict(self):
        return {"stride": self.stride, "capacity": self.capacity, "snap": self.snap.clone(), "pos": self.pos.clone(),
                "start": self.start.clone(), "restarts": self.restarts.clone()}

    def load_state_dict(self, state):
        """Copy the snapshots and the per-board counters of a ``state_dict()`` of a restart of the same shape into this one (in
        place)."""
        if int(state["stride"]) != self.stride or int(state["capacity"]) != self.capacity:
            raise ValueError("state_dict is of a restart with another stride or another capacity")
        new = {}
        for name in ("snap", "pos", "start", "restarts"):
            t, mine = torch.as_tensor(state[name]), getattr(self, name)
            if t.dtype != mine.dtype or t.shape != mine.shape:
                raise ValueError(f"state_dict {name} must be {str(mine.dtype).replace('torch.', '')} {tuple(mine.shape)}")
            new[name] = t
        for name, t in new.items():
            getattr(self, name).copy_(t)


def _restart_of(engine, restart):
    if not isinstance(restart, Restart) or restart.n != engine.n_envs or restart.device != engine.device:
        raise ValueError(f"restart must be a Restart of {engine.n_envs} boards on {engine.device}")
    return restart


class TDWork(NamedTuple):
    """Preallocated buffers of :func:`td_step` for one engine."""
    before: NTupleEval   # action, after, after_value of the boards before the step
    after: NTupleEval    # best of the boards after the step
    delta: torch.Tensor  # int64 [n]


def td_work(engine) -> TDWork:
    n, dev = engine.n_envs, engine.device
    i64 = dict(dtype=torch.int64, device=dev)
    return TDWork(NTupleEval(None, torch.empty(n, dtype=torch.uint8, device=dev), None,
                             torch.empty((n, 16), dtype=torch.uint8, device=dev), torch.empty(n, **i64)),
                  NTupleEval(None, None, torch.empty(n, **i64), None, None), torch.empty(n, **i64))


def _td_io(engine, work, delta=True):
    """NTupleTDIO over the buffers of ``work`` (a :class:`TDWork` of ``engine``) and ``engine.terminated``, each checked as
    ``_check_tensor`` checks; ``delta=False`` leaves ``work.delta`` out (NULL: not written)."""
    if not isinstance(work, TDWork) or not isinstance(work.before, NTupleEval) or not isinstance(work.after, NTupleEval):
        raise ValueError("work must be a TDWork (td_work(engine))")
    n, dev = engine.n_envs, engine.device
    io = NTupleTDIO()
    for name, t, dtype, shape in (("action", work.before.action, torch.uint8, (n,)), ("after", work.before.after, torch.uint8, (n, 16)),
                                  ("after_value", work.before.after_value, torch.int64, (n,)),
                                  ("best_next", work.after.best, torch.int64, (n,)),
                                  ("terminated", engine.terminated, torch.uint8, (n,)), ("delta", work.delta, torch.int64, (n,))):
        _check_tensor("work " + name, t, (dtype,), shape, dev)
        if delta or name != "delta":
            setattr(io, name, t.data_ptr())
    return io


def _restart_keyword(fn):
    """``fn`` -- a function with ``carousel=None, fused=False`` -- with the keyword-only ``restart=`` (a :class:`Restart`,
    INTEGRATION.md §25) added.  Positional arguments are ``fn``'s, unchanged.  ``restart=`` with ``carousel=`` is a ValueError,
    and so is ``restart=`` with ``fused=True``, both raised before anything is looked at or launched; otherwise the restart
    rides where a carousel rides (``_Rides``), and its ``step(engine)`` runs at exactly the place ``carousel.step(engine)``
    runs."""
    params = inspect.signature(fn)

    @functools.wraps(fn)
    def call(*args, restart=None, **kw):
        if restart is None:
            return fn(*args, **kw)
        bound = params.bind(*args, **kw)
        bound.apply_defaults()
        if bound.arguments["carousel"] is not None:
            raise ValueError("carousel= and restart= are two ways to restart a finished episode: give one of them")
        if bound.arguments["fused"]:
            raise ValueError("fused=True cannot run a restart: its launch sits between the step and the second evaluate and needs "
                             "the whole batch's terminated (use fused=False)")
        bound.arguments["carousel"] = _Rides(restart)
        return fn(*bound.args, **bound.kwargs)
    return call


def _fused_args(fused, carousel):
    """``fused`` as a bool; ValueError for ``fused=True`` with a carousel."""
    if fused and carousel is not None:
        raise ValueError("fused=True cannot run a carousel: its launches sit between the step and the second evaluate and need "
                         "the whole batch's terminated (use fused=False)")
    return bool(fused)


@_restart_keyword
def td_evaluate(engine, net, work, carousel=None, fused=False) -> TDWork:
    """Points 1-3 of the TD(0) step and the delta of point 4, leaving the weights alone: evaluate, play the greedy move
    (auto-reset on), evaluate the new boards, ``work.delta = (0 if terminated else best') - V(after)``.  Shards that share
    one weight tensor run this on every shard before :func:`td_update` on any, so that all of them see the same weights.
    ``carousel`` (a :class:`Carousel` of this engine): ``carousel.step(engine)`` right behind the step, so a finished
    episode restarts from the carousel's pool; the second evaluate sees the restarted board, and its ``best`` is masked by
    ``terminated`` as before.  None: exactly the launches above.
    ``restart=`` (keyword only; a :class:`Restart` of this engine): ``restart.step(engine)`` at that same place -- the midpoint
    restart, one launch, for any network.  Not together with ``carousel`` and not with ``fused=True`` (ValueError).  Every
    ``*_evaluate``, ``*_step`` and ``*_train`` function below that takes ``carousel=`` takes ``restart=`` the same way.
    ``fused=True``: all seven launches as ONE (``Batched2048.ntuple_td_step``, ``g2048_ntuple_td_step``) --
    the same bits in ``work``, ``engine.terminated`` and the engine; ``engine.reward`` is not written.  A spawn-stream engine
    only, and not with a ``carousel`` (ValueError): the carousel's three launches sit between the step and the second
    evaluate and need the whole batch's ``terminated``.  Measured on the MI355X (INTEGRATION.md §21,
    profiles/r25_ntuple_td_probe.txt): the fused step is NOT faster at any size timed -- 88 against 66 µs per TD(0) step at
    1 024 boards ("4x6"), 15 % slower at 16 384, a tie at 65 536, 7 % slower at 2^20 -- so ``fused=False`` is the faster
    choice below 65 536 boards and no slower above."""
    if _fused_args(fused, carousel):
        return engine.ntuple_td_step(net, work)
    if carousel is not None:
        carousel = _carousel_of(engine, carousel)
    engine.ntuple_evaluate(net, out=work.before)
    engine.step(work.before.action, auto_reset=True, want_info=False)
    if carousel is not None:
        carousel.step(engine)
    engine.ntuple_evaluate(net, out=work.after)
    work.delta.copy_(work.after.best)
    work.delta.masked_fill_(engine.terminated.bool(), 0)
    work.delta.sub_(work.before.after_value)
    return work


def td_update(net, work, lr_shift):
    """Point 4: ``net.update(after, delta, lr_shift)`` with what :func:`td_evaluate` left in ``work``."""
    net.update(work.before.after, work.delta, lr_shift)


@_restart_keyword
def td_step(engine, net, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """One afterstate TD(0) step of every board of ``engine`` (a ``Batched2048``) under ``net``, on the engine's stream:
    evaluate, play the greedy move, evaluate the new boards, and move V of the afterstate just played towards what
    followed it (:func:`td_evaluate`, then :func:`td_update`).  The weights change only in that last launch.  No host
    synchronisation; ``work`` (:func:`td_work`) is reused.  ``carousel`` and ``fused``: as in :func:`td_evaluate`."""
    work = td_evaluate(engine, net, td_work(engine) if work is None else work, carousel, fused)
    td_update(net, work, lr_shift)
    return work


@_restart_keyword
def train(engine, net, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`td_step` calls with one set of buffers.  ``fused=True``: ONE library call for all of them
    (``Batched2048.ntuple_td_train``, ``g2048_ntuple_td_train``) -- two launches per step and no Python
    between the steps, the same bits; not with a ``carousel`` (:func:`td_evaluate`).  Measured: no faster than ``fused=False``
    at any size timed, and 34 % slower at 1 024 boards (:func:`td_evaluate`)."""
    if _fused_args(fused, carousel):
        engine.ntuple_td_train(net, td_work(engine), n_steps, lr_shift)
        return net
    work = td_work(engine)
    for _ in range(int(n_steps)):
        td_step(engine, net, lr_shift, work, carousel)
    return net


def tc_update(net, tc, work, lr_shift, phases=3):
    """``net.tc_update(after, delta, lr_shift, tc, phases)`` with what :func:`td_evaluate` left in ``work``.  Shards that
    share one network and one :class:`NTupleTC` run :func:`td_evaluate` on every shard, then this with ``phases=1`` on
    every shard, then with ``phases=2`` on every shard: the bits of the unsharded step."""
    net.tc_update(work.before.after, work.delta, lr_shift, tc, phases)


@_restart_keyword
def tc_step(engine, net, tc, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """:func:`td_step` with the temporal-coherence update in place of the TD(0) one: :func:`td_evaluate`, then
    :func:`tc_update` (two launches).  No host synchronisation; ``work`` (:func:`td_work`) is reused.  ``fused``: as in
    :func:`td_evaluate`."""
    work = td_evaluate(engine, net, td_work(engine) if work is None else work, carousel, fused)
    tc_update(net, tc, work, lr_shift)
    return work


@_restart_keyword
def tc_train(engine, net, tc, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`tc_step` calls with one set of buffers.  ``fused=True``: ONE library call for all of them, as in
    :func:`train` (three launches per step); not with a ``carousel``."""
    if _fused_args(fused, carousel):
        net._own_tc(tc)
        engine.ntuple_td_train(net, td_work(engine), n_steps, lr_shift, tc)
        return net
    work = td_work(engine)
    for _ in range(int(n_steps)):
        tc_step(engine, net, tc, lr_shift, work, carousel)
    return net


def mean_update(net, mean, work, lr_shift, phases=3):
    """``net.mean_update(after, delta, lr_shift, mean, phases)`` with what :func:`td_evaluate` left in ``work``.  Shards that
    share one network and one :class:`NTupleMean` run :func:`td_evaluate` on every shard, then this with ``phases=1`` on every
    shard, then with ``phases=2`` on every shard: the bits of the unsharded step."""
    net.mean_update(work.before.after, work.delta, lr_shift, mean, phases)


@_restart_keyword
def mean_step(engine, net, mean, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """:func:`td_step` with the batch-mean update in place of the summed one: :func:`td_evaluate`, then :func:`mean_update` (two
    launches).  Measured (profiles/r26_ntuple_mean_probe.txt): "4x6" with ``lr_shift`` 6 scores the same at
    1 024 and at 65 536 boards for the same number of board-steps, where the summed update loses more than half its score; not
    at 2^20 boards, where 2^28 board-steps are 256 updates; a step costs 1.8 to 2.15 times a :func:`td_step`.  No host synchronisation;
    ``work`` (:func:`td_work`) is reused.  ``carousel`` and ``fused``: as in :func:`td_evaluate`."""
    work = td_evaluate(engine, net, td_work(engine) if work is None else work, carousel, fused)
    mean_update(net, mean, work, lr_shift)
    return work


@_restart_keyword
def mean_train(engine, net, mean, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`mean_step` calls with one set of buffers.  ``fused=True`` is the fused front half per step; there is no
    one-call trainer for this update."""
    net._own_mean(mean)
    _fused_args(fused, carousel)
    work = td_work(engine)
    for _ in range(int(n_steps)):
        mean_step(engine, net, mean, lr_shift, work, carousel, fused)
    return net


@_restart_keyword
def tdl_evaluate(engine, net, trace, work, carousel=None, fused=False) -> TDWork:
    """:func:`td_evaluate` for the trace learners: evaluate, play the greedy move, evaluate the new boards, then one
    ``trace.push`` that stores the afterstate just played and forms ``work.delta`` in the same launch (in place of
    td_evaluate's three element-wise ones).  Shards that share one network run this on every shard before an update on any.
    ``carousel``: as in :func:`td_evaluate`; the trace needs nothing, its push already sees ``terminated``.
    ``fused=True``: the first three launches as one (``Batched2048.ntuple_td_step`` without its ``delta``: the push writes the
    same values); the same bits, and the exclusions of :func:`td_evaluate`."""
    if _fused_args(fused, carousel):
        engine.ntuple_td_step(net, work, delta=False)
        trace.push(work.before.after, work.before.after_value, work.after.best, engine.terminated, work.delta)
        return work
    if carousel is not None:
        carousel = _carousel_of(engine, carousel)
    engine.ntuple_evaluate(net, out=work.before)
    engine.step(work.before.action, auto_reset=True, want_info=False)
    if carousel is not None:
        carousel.step(engine)
    engine.ntuple_evaluate(net, out=work.after)
    trace.push(work.before.after, work.before.after_value, work.after.best, engine.terminated, work.delta)
    return work


def _trace_of(engine, trace):
    if not isinstance(trace, NTupleTrace) or trace.n != engine.n_envs or trace.device != engine.device:
        raise ValueError(f"trace must be an NTupleTrace of {engine.n_envs} boards on {engine.device}")
    return trace


@_restart_keyword
def tdl_step(engine, net, trace, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """One afterstate TD(lambda) step of every board of ``engine`` under ``net``: :func:`tdl_evaluate`, then
    ``net.trace_update``.  No host synchronisation; ``work`` (:func:`td_work`) is reused.  ``fused``: as in
    :func:`tdl_evaluate`."""
    work = tdl_evaluate(engine, net, _trace_of(engine, trace), td_work(engine) if work is None else work, carousel, fused)
    net.trace_update(trace, work.delta, lr_shift)
    return work


@_restart_keyword
def tdl_train(engine, net, trace, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`tdl_step` calls with one set of buffers."""
    work = td_work(engine)
    for _ in range(int(n_steps)):
        tdl_step(engine, net, trace, lr_shift, work, carousel, fused)
    return net


@_restart_keyword
def mean_tdl_step(engine, net, mean, trace, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """:func:`tdl_step` with the batch-mean trace update: :func:`tdl_evaluate`, then ``net.mean_trace_update`` (two launches, SUM
    then APPLY)."""
    work = tdl_evaluate(engine, net, _trace_of(engine, trace), td_work(engine) if work is None else work, carousel, fused)
    net.mean_trace_update(trace, work.delta, lr_shift, mean)
    return work


@_restart_keyword
def mean_tdl_train(engine, net, mean, trace, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`mean_tdl_step` calls with one set of buffers."""
    work = td_work(engine)
    for _ in range(int(n_steps)):
        mean_tdl_step(engine, net, mean, trace, lr_shift, work, carousel, fused)
    return net


@_restart_keyword
def tcl_step(engine, net, tc, trace, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """:func:`tdl_step` with the temporal-coherence trace update: :func:`tdl_evaluate`, then ``net.tc_trace_update`` (two
    launches, W then A)."""
    work = tdl_evaluate(engine, net, _trace_of(engine, trace), td_work(engine) if work is None else work, carousel, fused)
    net.tc_trace_update(trace, work.delta, lr_shift, tc)
    return work


@_restart_keyword
def tcl_train(engine, net, tc, trace, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`tcl_step` calls with one set of buffers."""
    work = td_work(engine)
    for _ in range(int(n_steps)):
        tcl_step(engine, net, tc, trace, lr_shift, work, carousel, fused)
    return net


def _delay_of(engine, delay):
    if not isinstance(delay, NTupleDelay) or delay.n != engine.n_envs or delay.device != engine.device:
        raise ValueError(f"delay must be an NTupleDelay of {engine.n_envs} boards on {engine.device}")
    return delay


@_restart_keyword
def delayed_evaluate(engine, net, delay, work, carousel=None, fused=False) -> TDWork:
    """:func:`tdl_evaluate` for the delayed learners: the same launches with ``delay.push`` (an :class:`NTupleDelay`) in place
    of ``trace.push``.  Shards that share one network run this on every shard before an update on any.  ``fused``: as in
    :func:`tdl_evaluate`."""
    return tdl_evaluate(engine, net, _delay_of(engine, delay), work, carousel, fused)


@_restart_keyword
def delayed_tdl_step(engine, net, delay, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """One delayed TD(lambda) step of every board of ``engine`` under ``net``: :func:`delayed_evaluate`, then
    ``net.delay_update``.  No host synchronisation; ``work`` (:func:`td_work`) is reused.  Errors stay pending in ``delay``:
    see :func:`delayed_tdl_train`."""
    work = delayed_evaluate(engine, net, _delay_of(engine, delay), td_work(engine) if work is None else work, carousel, fused)
    net.delay_update(delay, lr_shift)
    return work


@_restart_keyword
def delayed_tdl_train(engine, net, delay, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`delayed_tdl_step` calls with one set of buffers, then the flush and ``delay.reset()``: no collected
    error is lost, and the next call starts every board's history anew."""
    _delay_of(engine, delay)
    work = td_work(engine)
    for _ in range(int(n_steps)):
        delayed_tdl_step(engine, net, delay, lr_shift, work, carousel, fused)
    net.delay_update(delay, lr_shift, flush=True)
    delay.reset()
    return net


@_restart_keyword
def delayed_tcl_step(engine, net, tc, delay, lr_shift, work=None, carousel=None, fused=False) -> TDWork:
    """:func:`delayed_tdl_step` with the temporal-coherence update: :func:`delayed_evaluate`, then ``net.tc_delay_update``
    (two launches, W then A)."""
    work = delayed_evaluate(engine, net, _delay_of(engine, delay), td_work(engine) if work is None else work, carousel, fused)
    net.tc_delay_update(delay, lr_shift, tc)
    return work


@_restart_keyword
def delayed_tcl_train(engine, net, tc, delay, n_steps, lr_shift, carousel=None, fused=False):
    """``n_steps`` :func:`delayed_tcl_step` calls with one set of buffers, then the flush and ``delay.reset()``, as
    :func:`delayed_tdl_train`."""
    _delay_of(engine, delay)
    work = td_work(engine)
    for _ in range(int(n_steps)):
        delayed_tcl_step(engine, net, tc, delay, lr_shift, work, carousel, fused)
    net.tc_delay_update(delay, lr_shift, tc, flush=True)
    delay.reset()
    return net


class NTupleLog:
    """The move log of backward learning for ``n`` boards (``g2048_ntuple_log``): ``depth`` (M, 1..1024)
    moves per segment in ``M + 1`` slots, slot-major -- ``after`` uint8 ``[M+1, n, 16]``, the afterstates played, ``gain`` int64
    ``[M+1, n]``, the merge gain of each move ``<< frac_bits``, and ``flag`` uint8 ``[M+1, n]``: 0 (nothing played: the board had
    no legal move, or the slot is still empty), ``LOG_VALID``, or ``LOG_VALID | LOG_ENDED`` (the move ended the episode).
    ``Batched2048.ntuple_play_log`` writes slots 1..M and carries slot M into slot 0; :func:`log_sweep` learns from slots
    M-1..0.  Zero-initialised; one per engine or shard; :meth:`reset` after ``engine.reset()``.

    Memory: 25 (M + 1) bytes per board."""

    def __init__(self, n, depth=16, device="cuda:0"):
        self.n = _int_arg("n", n, 1, 0xffffff00)
        self.depth = _int_arg("depth", depth, 1, LOG_MAX_DEPTH)
        self.device = torch.device(device)
        slots = self.depth + 1
        self.after = torch.zeros((slots, self.n, 16), dtype=torch.uint8, device=self.device)
        self.gain = torch.zeros((slots, self.n), dtype=torch.int64, device=self.device)
        self.flag = torch.zeros((slots, self.n), dtype=torch.uint8, device=self.device)
        self._c = _lib.NTupleLogC(self.depth, self.after.data_ptr(), self.gain.data_ptr(), self.flag.data_ptr())

    def reset(self):
        """Empty every slot on the current stream: the next segment has no predecessor (slot 0 carries nothing)."""
        self.after.zero_()
        self.gain.zero_()
        self.flag.zero_()

    def slot(self, m) -> torch.Tensor:
        """Slot ``m`` (0..M) of ``after`` as a uint8 ``[n, 16]`` view: a plain-board batch for ``values`` and the updates."""
        return self.after[_int_arg("m", m, 0, self.depth)]

    def state_dict(self):
        return {"depth": self.depth, "after": self.after.clone(), "gain": self.gain.clone(), "flag": self.flag.clone()}

    def load_state_dict(self, state):
        """Copy the tensors of a ``state_dict()`` of a log of the same shape into this one (in place)."""
        if int(state["depth"]) != self.depth:
            raise ValueError(f"state_dict is of a log of depth {state['depth']}, this one has {self.depth}")
        new = {name: torch.as_tensor(state[name]) for name in ("after", "gain", "flag")}
        for name, t in new.items():
            mine = getattr(self, name)
            if t.dtype != mine.dtype or t.shape != mine.shape:
                raise ValueError(f"state_dict {name} must be {str(mine.dtype).replace('torch.', '')} {tuple(mine.shape)}")
        for name, t in new.items():
            getattr(self, name).copy_(t)


def _log_of(engine, log):
    if not isinstance(log, NTupleLog) or log.n != engine.n_envs or log.device != engine.device:
        raise ValueError(f"log must be an NTupleLog of {engine.n_envs} boards on {engine.device}")
    return log


def _log_delta_buffer(log, delta):
    """``delta`` checked as the int64 ``[log.n]`` work buffer of a sweep, or a fresh one."""
    if delta is None:
        return torch.empty(log.n, dtype=torch.int64, device=log.device)
    _check_tensor("delta", delta, (torch.int64,), (log.n,), log.device)
    return delta


def log_sweep(net, log, lr_shift, tc=None, mean=None, delta=None) -> torch.Tensor:
    """The backward sweep over ``log`` (an :class:`NTupleLog`): for ``m`` = M-1 down to 0, ``net.log_delta``
    of slot ``m`` into ``delta`` and then the update of ``log.slot(m)`` by it, so that the target of slot ``m`` is formed with
    the value slot ``m + 1`` has after its own update.  ``tc`` and ``mean`` None: ``net.update``, ``tc`` (an :class:`NTupleTC` of
    ``net``): ``net.tc_update`` with ``phases=3`` -- both ONE library call, 2M or 3M plain launches
    (``g2048_ntuple_log_sweep``); ``mean`` (an :class:`NTupleMean` of ``net``): ``net.mean_update``, composed here launch by
    launch.  Slot M is not updated: it is slot 0 of the next segment.  ``delta``: the int64 ``[n]`` work buffer, returned (the
    errors of slot 0 afterwards).  No host synchronisation.  Shards that share ``net`` do not call this: per ``m`` they run
    ``net.log_delta`` on every shard, then the update on every shard."""
    if not isinstance(net, NTupleNet):
        raise ValueError("net must be an NTupleNet")
    if not isinstance(log, NTupleLog):
        raise ValueError("log must be an NTupleLog")
    if tc is not None and mean is not None:
        raise ValueError("log_sweep takes tc or mean, not both")
    ref = net._ref(log.device)
    shift = _int_arg("lr_shift", lr_shift, 0, MAX_LR_SHIFT)
    delta = _log_delta_buffer(log, delta)
    if mean is not None:
        net._own_mean(mean)
        for m in range(log.depth - 1, -1, -1):
            net.log_delta(log, m, out=delta)
            net.mean_update(log.slot(m), delta, shift, mean)
        return delta
    if tc is not None:
        net._own_tc(tc)
    _on_stream(net._fn("log_sweep"), log.device, log.n, ref, C.byref(log._c), shift, delta.data_ptr(),
               None if tc is None else C.byref(tc._c))
    return delta


def backward_train(engine, net, log, rounds, lr_shift, tc=None, mean=None, carousel=None, restart=None):
    """Backward learning over logged segments (Matsuzaki 2017): ``rounds`` times
    { ``engine.ntuple_play_log(net, log)``; :func:`log_sweep` } -- play ``log.depth`` moves of every board under frozen weights
    in one launch, then update the logged afterstates from the last to the first.  ``tc`` and ``mean`` None (TD) or ``tc``: ONE
    library call for all rounds (``Batched2048.ntuple_log_train``, ``g2048_ntuple_log_train``); ``mean``: the same loop in
    Python.  The afterstates of slot M are updated by the next round, those of the last round never.  A learner of its own, not
    :func:`train` at ``depth=1``.  ``carousel`` is not offered (ValueError): its launches sit between a step and the next
    evaluate, and the moves of a segment are one launch.  ``restart`` (a :class:`Restart` of this engine) is: its step is per
    board and runs behind every move inside the play-log launch (``g2048_ntuple_play_log_restart``,
    ``g2048_ntuple_log_train_restart``).  A spawn-stream engine only."""
    if carousel is not None:
        raise ValueError("backward_train cannot run a carousel: its launches sit between a step and the next evaluate, and the "
                         "moves of a segment are one launch (use the forward trainers)")
    if tc is not None and mean is not None:
        raise ValueError("backward_train takes tc or mean, not both")
    _log_of(engine, log)
    if restart is not None:
        _restart_of(engine, restart)
    if mean is None:
        engine.ntuple_log_train(net, log, rounds, lr_shift, _log_delta_buffer(log, None), tc, restart=restart)
        return net
    if not isinstance(net, NTupleNet):
        raise ValueError("net must be an NTupleNet")
    net._own_mean(mean)
    delta = _log_delta_buffer(log, None)
    for _ in range(_int_arg("rounds", rounds, 0, (1 << 32) - 1)):
        engine.ntuple_play_log(net, log, restart=restart)
        log_sweep(net, log, lr_shift, mean=mean, delta=delta)
    return net


class PlayReport(NamedTuple):
    """Result of :func:`play_games`: the table the n-tuple papers report."""
    games: int                        # games played to the end
    unfinished: int                   # games still owed when max_steps ran out (0 otherwise)
    mean_score: float                 # return_sum of those games / games: exact integers, one division (0.0 for no game)
    hist: list                        # [32]: games whose highest tile was 2^k
    reach: dict                       # {2048: share, ..., 32768: share} of the games whose highest tile was at least that tile
    moves: int                        # moves played, the last (possibly illegal) move of every game included
    scores: Optional[torch.Tensor]    # int32 [n]: every game's score when games == 1 and the engine keeps terminal records


REACH_TILES = (2048, 4096, 8192, 16384, 32768)


class DeepPlayer:
    """The expectimax player over ``net`` at ``depth`` 2..3 for :func:`play_games` (``g2048_ntuple_deep_search``,
    INTEGRATION.md §18): ``play_games(engine, net, games, player=DeepPlayer(net))`` is the 3-ply row of the n-tuple papers.
    A callable ``player(engine, actions, active=None)``; ``takes_active`` tells :func:`play_games` to pass the boards' games
    left as ``active``, so that boards that have finished their games are not searched."""
    takes_active = True

    def __init__(self, net, depth=3):
        if not isinstance(net, NTupleNet):
            raise ValueError("net must be an NTupleNet")
        self.net, self.depth = net, _int_arg("depth", depth, DEEP_MIN_DEPTH, DEEP_MAX_DEPTH)

    def __call__(self, engine, actions, active=None):
        engine.ntuple_deep_search(self.net, self.depth, out=NTupleSearch(actions, None), active=active)


class AdaptivePlayer:
    """The expectimax player over ``net`` at a depth per board for :func:`play_games` (``g2048_ntuple_adaptive_search``,
    INTEGRATION.md §20): ``play_games(engine, net, games, player=AdaptivePlayer(net, "4-ply-late"))``.  ``schedule`` as
    :meth:`NTupleNet.adaptive_search` takes it.  A callable ``player(engine, actions, active=None)`` with ``takes_active``, as
    :class:`DeepPlayer`."""
    takes_active = True

    def __init__(self, net, schedule):
        if not isinstance(net, NTupleNet):
            raise ValueError("net must be an NTupleNet")
        self.net, self.schedule = net, _schedule(schedule)

    def __call__(self, engine, actions, active=None):
        engine.ntuple_adaptive_search(self.net, self.schedule, out=NTupleAdaptive(actions, None, None), active=active)


class ReducedPlayer:
    """The expectimax player over ``net`` at a depth per board with the children of a 4 spawn searched ``reduce4`` plies
    shallower, for :func:`play_games` (``g2048_ntuple_reduced_search``):
    ``play_games(engine, net, games, player=ReducedPlayer(net, "4-ply-late"))``.  ``schedule`` as
    :meth:`NTupleNet.adaptive_search` takes it.  A callable ``player(engine, actions, active=None)`` with ``takes_active``, as
    :class:`AdaptivePlayer`."""
    takes_active = True

    def __init__(self, net, schedule, reduce4=1):
        if not isinstance(net, NTupleNet):
            raise ValueError("net must be an NTupleNet")
        self.net, self.schedule = net, _schedule(schedule)
        self.reduce4 = _int_arg("reduce4", reduce4, REDUCE4_MIN, REDUCE4_MAX)

    def __call__(self, engine, actions, active=None):
        engine.ntuple_reduced_search(self.net, self.schedule, self.reduce4, out=NTupleAdaptive(actions, None, None), active=active)


class DowngradedPlayer:
    """A :class:`DeepPlayer`, :class:`AdaptivePlayer` or :class:`ReducedPlayer` searching translated boards (tile-downgrading,
    INTEGRATION.md §26), for :func:`play_games`: per move ``engine.downgraded_boards(rule, active)`` and then the wrapped
    player's search of its own network on those plain boards (``net.deep_search`` / ``adaptive_search`` / ``reduced_search``).
    A board that rests comes out of the translation as the empty board, which every plain search answers at once with action
    0, so resting boards are not searched and nothing is read by the host.  A callable ``player(engine, actions, active=None)``
    with ``takes_active``."""
    takes_active = True

    def __init__(self, player, rule):
        if not isinstance(player, (DeepPlayer, AdaptivePlayer, ReducedPlayer)):
            raise ValueError("player must be a DeepPlayer, an AdaptivePlayer or a ReducedPlayer")
        _rule(rule)
        self.player, self.rule, self._boards = player, rule, None

    def __call__(self, engine, actions, active=None):
        if self._boards is None or self._boards.shape[0] != engine.n_envs or self._boards.device != engine.device:
            self._boards = torch.empty((engine.n_envs, 16), dtype=torch.uint8, device=engine.device)
        boards = engine.downgraded_boards(self.rule, active=active, out=Downgraded(self._boards, None)).boards
        p = self.player            # (the plain searches run on the current stream of the boards' device: the engine's)
        if isinstance(p, DeepPlayer):
            p.net.deep_search(boards, p.depth, out=NTupleSearch(actions, None))
        elif isinstance(p, ReducedPlayer):
            p.net.reduced_search(boards, p.schedule, p.reduce4, out=NTupleAdaptive(actions, None, None))
        else:
            p.net.adaptive_search(boards, p.schedule, out=NTupleAdaptive(actions, None, None))


def _play_games(engine, net, games, chunk, max_steps, depth, player, downgrade) -> PlayReport:
    """:func:`play_games`, every argument given."""
    games = _int_arg("games", games, 1, (1 << 32) - 1)
    chunk = _int_arg("chunk", chunk, 1, (1 << 32) - 1)
    if max_steps is not None:
        max_steps = _int_arg("max_steps", max_steps, 1, 1 << 62)
    depth = _int_arg("depth", depth, 0, SEARCH_MAX_DEPTH)
    if player is not None:
        if not callable(player):
            raise ValueError("player must be a callable player(engine, actions)")
        if depth != 0:
            raise ValueError(f"depth={depth} with a player: depth searches net, a player chooses its own actions")
    elif not isinstance(net, NTupleNet):
        raise ValueError("net must be an NTupleNet (or give a player)")
    if downgrade is not None:
        _rule(downgrade)
        if player is not None:
            raise ValueError("downgrade with a player: wrap the player in DowngradedPlayer(player, rule) instead")
    n, dev = engine.n_envs, engine.device
    engine.reset()
    # (filled as the signed types of the same width and viewed: every torch build fills and sums those on the device)
    left = torch.full((n,), games - (1 << 32) if games >> 31 else games, dtype=torch.int32, device=dev).view(torch.uint32)
    hist = torch.zeros(32, dtype=torch.int64, device=dev).view(torch.uint64)
    moves = torch.zeros(1, dtype=torch.int64, device=dev).view(torch.uint64)
    before, steps = engine.episode_stats(), 0
    act = torch.empty(n, dtype=torch.uint8, device=dev) if player is not None or depth else None
    takes_active = bool(getattr(player, "takes_active", False))
    low = Downgraded(torch.empty((n, 16), dtype=torch.uint8, device=dev), None) if downgrade is not None and depth else None
    while max_steps is None or steps < max_steps:
        if act is None:
            engine.ntuple_play(net, chunk, games_left=left, hist=hist, moves=moves, downgrade=downgrade)
        else:
            for _ in range(chunk):        # (a chunk that outlives every game steps resting boards: launches, no work)
                if takes_active:
                    player(engine, act, active=left)
                elif player is not None:
                    player(engine, act)
                elif low is not None:
                    engine.downgraded_boards(downgrade, active=left, out=low)
                    net.search(low.boards, depth, out=NTupleSearch(act, None))
                else:
                    engine.ntuple_search(net, depth, out=NTupleSearch(act, None), active=left)
                engine.play_step(act, games_left=left, hist=hist, moves=moves)
        steps += chunk
        if not bool(left.view(torch.int32).any()):
            break
    after = engine.episode_stats()
    played = after["episodes"] - before["episodes"]
    counts = [int(c) for c in hist.view(torch.int64).tolist()]
    reach = {tile: (sum(counts[tile.bit_length() - 1:]) / played if played else 0.0) for tile in REACH_TILES}
    scores = engine.last_scores() if games == 1 and engine.last_records_enabled else None
    return PlayReport(played, n * games - played, (after["return_sum"] - before["return_sum"]) / played if played else 0.0, counts,
                      reach, int(moves.view(torch.int64).item()), scores)


def _downgrade_keyword(fn):
    """``fn`` with the keyword-only ``downgrade=`` (a :class:`Downgrade`) added; the positional arguments are
    ``fn``'s, unchanged."""
    params = inspect.signature(fn)

    @functools.wraps(fn)
    def call(*args, downgrade=None, **kw):
        bound = params.bind(*args, **kw)
        bound.apply_defaults()
        return _play_games(*bound.args, **bound.kwargs, downgrade=downgrade)
    return call


@_downgrade_keyword
def play_games(engine, net, games=1, chunk=1024, max_steps=None, depth=0, player=None) -> PlayReport:
    """Exactly ``games`` games on every board of ``engine`` (a spawn-stream ``Batched2048``), played to the end, by one of
    three players.  ``depth=0`` (the default): the greedy player of ``net`` -- resets the engine, then
    ``engine.ntuple_play(net, chunk, ...)`` until no board has a game left, with one host read per chunk.  ``depth`` 1..2: the
    expectimax player over ``net`` -- per move ``engine.ntuple_search(net, depth, active=left)``
    into one preallocated action tensor, then ``engine.play_step`` of it; boards that have finished their games are not
    searched.  ``player``: any policy, a callable ``player(engine, actions)`` that fills the uint8 ``[n]`` device tensor
    ``actions`` on the engine's stream; ``net`` may then be None and ``depth`` must be 0.  A player with a true attribute
    ``takes_active`` (:class:`DeepPlayer`) is called as ``player(engine, actions, active=left)`` with the uint32 ``[n]`` tensor
    of the games each board still owes, 0 for a board that rests.  Either way the loop runs
    ``chunk`` moves between two host reads.  A board that has finished its games rests, so short games are not
    over-weighted the way counting every episode of a fixed step budget over-weights them.  ``max_steps``: stop after at
    least that many steps per board (a multiple of ``chunk``) and report what is missing as ``unfinished``.  The engine's
    statistics keep running: the report is the difference of two ``episode_stats()`` readings.  The games are a function of
    the engine's seed and of its clock at the reset: ``engine.seed(s)`` first makes a report reproducible.
    ``downgrade`` (a :class:`Downgrade`): every move is chosen on the translated board -- the greedy player
    through ``engine.ntuple_play(..., downgrade=)``, one launch per chunk as before; ``depth`` 1..2 through
    ``engine.downgraded_boards(downgrade, active=left)`` and ``net.search`` of those boards.  A ``player`` is wrapped by the
    caller (:class:`DowngradedPlayer`); ``downgrade`` with a ``player`` is refused.  Keyword only; None: today's call."""
    return _play_games(engine, net, games, chunk, max_steps, depth, player, None)
