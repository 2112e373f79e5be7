"""The calls that look at every board and write nothing back: afterstates, expectimax search and Monte-Carlo rollout
search (``g2048_afterstates`` / ``g2048_expectimax`` / ``g2048_mc_search`` and their ``_plain`` forms).

The module functions take plain boards; ``Batched2048`` (batched.py) has the same three calls as methods on its live
boards and re-exports every public name of this module.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import AfterstateIO, MCIO, SearchIO, check

_OBS_DTYPES = {torch.uint8: _lib.OBS_U8, torch.float16: _lib.OBS_F16, torch.float32: _lib.OBS_F32}


def _plain_boards(boards):
    """(n, device) of a plain board tensor, or ValueError."""
    if (not isinstance(boards, torch.Tensor) or boards.dtype != torch.uint8 or boards.device.type != "cuda"
            or boards.dim() not in (2, 3) or tuple(boards.shape[1:]) not in ((16,), (4, 4)) or not boards.is_contiguous()):
        raise ValueError("boards must be a contiguous uint8 [n, 16] or [n, 4, 4] tensor on a GPU")
    return boards.shape[0], boards.device


def _int_arg(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an int in {lo}..{hi}, not {v!r}")
    return int(v)


def _bind_out(io, out, spec, device):
    """Check the fields of ``out`` that are not None against ``spec`` (name -> (shape, allowed dtypes)) and put their
    addresses into the C struct ``io``."""
    for name, (shape, dtypes) in spec.items():
        t = getattr(out, name)
        if t is None:
            continue
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype not in dtypes or not t.is_contiguous()
                or t.device != device):
            raise ValueError(f"out.{name} must be a contiguous {shape} tensor of {' / '.join(map(str, dtypes))} on {device}")
        setattr(io, name, t.data_ptr())


def _launch_plain(fn, boards, *args):
    """``fn(boards, n, *args, stream)`` on the current stream of the boards' device."""
    with torch.cuda.device(boards.device):
        stream = C.c_void_p(torch.cuda.current_stream(boards.device).cuda_stream)
        check(fn(boards.data_ptr(), boards.shape[0], *args, stream))


class Afterstates(NamedTuple):
    """What the four moves of every board produce, before the spawn (``g2048_afterstates``).  Device tensors; a field
    that is None was not asked for (``out``) -- ``obs`` is None unless an ``obs_dtype`` was given."""
    boards: Optional[torch.Tensor]   # uint8 [n, 4, 16]: afterstate d of board i (the board itself where d is illegal)
    score: Optional[torch.Tensor]    # int32 [n, 4]: merge score of move d, 0 where illegal
    legal: Optional[torch.Tensor]    # uint8 [n]: bit d = move d legal (legal_actions())
    obs: Optional[torch.Tensor]      # [n, 4, 16, 4, 4] stack() of each afterstate; .view(4n, 16, 4, 4) feeds a network


def _afterstate_io(n, device, obs_dtype, out):
    """(AfterstateIO, Afterstates) for n boards: ``out`` checked field by field, or freshly allocated outputs."""
    if out is None:
        out = Afterstates(torch.empty((n, 4, 16), dtype=torch.uint8, device=device),
                          torch.empty((n, 4), dtype=torch.int32, device=device),
                          torch.empty(n, dtype=torch.uint8, device=device),
                          None if obs_dtype is None else torch.empty((n, 4, 16, 4, 4), dtype=obs_dtype, device=device))
    else:
        out = Afterstates(*out)
        if obs_dtype is not None and (out.obs is None or out.obs.dtype != obs_dtype):
            raise ValueError("obs_dtype does not match out.obs (leave obs_dtype None when passing out)")
    io = AfterstateIO()
    _bind_out(io, out, {"boards": ((n, 4, 16), (torch.uint8,)), "score": ((n, 4), (torch.int32,)),
                        "legal": ((n,), (torch.uint8,)), "obs": ((n, 4, 16, 4, 4), tuple(_OBS_DTYPES))}, device)
    if out.obs is not None:
        io.obs_dtype = _OBS_DTYPES[out.obs.dtype]
    return io, out


def afterstates(boards, obs_dtype=None, out=None) -> Afterstates:
    """Afterstates of plain boards (``g2048_afterstates_plain``): ``boards`` is a device ``uint8`` tensor ``[n, 16]`` or
    ``[n, 4, 4]`` of exponents (taken mod 32) -- replay-buffer rows, a search frontier.  No engine; enqueued on the current
    stream of the boards' device.  See :class:`Afterstates` and :meth:`Batched2048.afterstates`."""
    io, out = _afterstate_io(*_plain_boards(boards), obs_dtype, out)
    _launch_plain(_lib.load().g2048_afterstates_plain, boards, C.byref(io))
    return out


class SearchWeights(NamedTuple):
    """Integer weights of the expectimax heuristic (include/g2048.h G2048_SEARCH_*): ``base`` in 0..2^24, the others in
    0..65535.  H(b) = base + sum over the 4 rows and 4 columns of w_empty * empty + w_merge * merge + w_mono * mono."""
    base: int = 4096
    w_empty: int = 256
    w_merge: int = 128
    w_mono: int = 16


class Search(NamedTuple):
    """Result of ``expectimax`` (``g2048_expectimax``).  Device tensors; a field that is None was not asked for (``out``)."""
    action: Optional[torch.Tensor]  # uint8 [n]: the smallest direction of largest value; 0 when no move is legal
    value: Optional[torch.Tensor]   # int32 [n, 4]: C_depth(move(b, d)), -1 where d is illegal


def _search_io(n, device, depth, weights, out):
    """(SearchIO, Search) for n boards: arguments checked, ``out`` checked field by field or freshly allocated."""
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= int(depth) <= 3:
        raise ValueError(f"depth must be 1, 2 or 3, not {depth!r}")
    w = SearchWeights() if weights is None else SearchWeights(*weights)
    w = [_int_arg("weights." + name, v, 0, hi) for name, v, hi in zip(w._fields, w, (1 << 24, 65535, 65535, 65535))]
    if out is None:
        out = Search(torch.empty(n, dtype=torch.uint8, device=device), torch.empty((n, 4), dtype=torch.int32, device=device))
    else:
        out = Search(*out)
        if out.action is None and out.value is None:
            raise ValueError("out requests no output (action and value are both None)")
    io = SearchIO(int(depth), *w)
    _bind_out(io, out, {"action": ((n,), (torch.uint8,)), "value": ((n, 4), (torch.int32,))}, device)
    return io, out


def expectimax(boards, depth=2, weights=None, out=None) -> Search:
    """Expectimax search of plain boards (``g2048_expectimax_plain``): ``boards`` is a device
    ``uint8`` tensor ``[n, 16]`` or ``[n, 4, 4]`` of exponents (taken mod 32).  ``depth`` 1..3 move plies, each followed
    by a chance node over every spawn; ``weights`` a :class:`SearchWeights` (defaults when None); ``out`` a preallocated
    :class:`Search` (a field that is None is not written).  One launch, enqueued on the current stream of the boards'
    device.  Returns ``Search(action [n] uint8, value [n, 4] int32)``."""
    io, out = _search_io(*_plain_boards(boards), depth, weights, out)
    _launch_plain(_lib.load().g2048_expectimax_plain, boards, C.byref(io))
    return out


MC_DEFAULT_MAX_STEPS = 65535  # G2048_MC_MAX_STEPS: a playout runs to the end of its game (random play ends within ~10^3 moves)


class MCSearch(NamedTuple):
    """Result of ``mc_search`` (``g2048_mc_search``).  Device tensors; a field that is None was not asked for (``out``)."""
    action: Optional[torch.Tensor]  # uint8 [n]: the smallest direction of largest value; 0 when no move is legal
    value: Optional[torch.Tensor]   # int64 [n, 4]: summed scores of the R playouts of direction d, -1 where d is illegal
    steps: Optional[torch.Tensor]   # int64 [n, 4]: moves those playouts played after the root move, -1 where d is illegal


def _mc_io(n, device, rollouts, max_steps, seed, index_offset, out):
    """(MCIO, MCSearch) for n boards: arguments checked, ``out`` checked field by field or freshly allocated."""
    io = MCIO(_int_arg("rollouts", rollouts, 1, 65536), _int_arg("max_steps", max_steps, 1, 65535),
              _int_arg("seed", seed, 0, (1 << 64) - 1))
    _int_arg("index_offset", index_offset, 0, (1 << 32) - n)
    if out is None:
        out = MCSearch(torch.empty(n, dtype=torch.uint8, device=device), torch.empty((n, 4), dtype=torch.int64, device=device),
                       torch.empty((n, 4), dtype=torch.int64, device=device))
    else:
        out = MCSearch(*out)
        if out.action is None and out.value is None and out.steps is None:
            raise ValueError("out requests no output (action, value and steps are all None)")
    _bind_out(io, out, {"action": ((n,), (torch.uint8,)), "value": ((n, 4), (torch.int64,)), "steps": ((n, 4), (torch.int64,))},
              device)
    return io, out


def mc_search(boards, rollouts=64, max_steps=MC_DEFAULT_MAX_STEPS, seed=0, index_offset=0, out=None) -> MCSearch:
    """Monte-Carlo rollout search of plain boards (``g2048_mc_search_plain``): for each legal move,
    ``rollouts`` random playouts of at most ``max_steps`` moves; the action is the move with the largest summed score.
    ``boards`` is a device ``uint8`` tensor ``[n, 16]`` or ``[n, 4, 4]`` of exponents (taken mod 32); row ``k`` draws
    the random stream of board index ``index_offset + k`` under ``seed``.  ``max_steps`` defaults to the largest cap,
    i.e. playouts run to the end of the game.  ``out``: a preallocated :class:`MCSearch` (a field that is None is not
    written).  One launch, enqueued on the current stream of the boards' device.  Returns ``MCSearch(action [n] uint8,
    value [n, 4] int64, steps [n, 4] int64)``."""
    io, out = _mc_io(*_plain_boards(boards), rollouts, max_steps, seed, index_offset, out)
    _launch_plain(_lib.load().g2048_mc_search_plain, boards, int(index_offset), C.byref(io))
    return out
