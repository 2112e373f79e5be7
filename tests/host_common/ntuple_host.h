// ntuple_host.h -- what every host-check program (tests/host_*/*_check.cpp) needs around g2048_device.h, the header the kernels
// are compiled from, built for the host (-DG2048_HOST_CHECK): the tables a device function takes, the loads of a 16-byte board,
// the description of an n-tuple network that a test hands over through ctypes (tests/host_build.py holds the other side), and
// the dispatch from that description to the tuple count and shape type a call instantiates.  Not part of the product.
#pragma once
#define G2048_HOST_CHECK 1
#include "../../gym-2048_amd/csrc/g2048_device.h"

#include <cstring>
#include <type_traits>

using namespace g2048;

namespace { // a host-check program is one translation unit: nothing here is exported from its library

constexpr uint32_t kLut[32] = {G2048_MOVE_LUT_WORDS};

struct HostTables { // what LdsTables is on the device (g2048_kernels.hip)
    MoveSel move_sel(uint32_t action) const
    {
        const uint32_t *r = kLut + 8 * (action & 3u);
        return MoveSel{r[0], r[1], r[2], r[3], r[4], r[5]};
    }
    Board onehot_cell(uint32_t p) const
    {
        return Board{{onehot_cell_word(p, 0), onehot_cell_word(p, 1), onehot_cell_word(p, 2), onehot_cell_word(p, 3)}};
    }
};

// the 16 bytes as they are: an engine record (score-deficit bits in bits 5..7 of bytes 8..15), or what ntuple_pack sees of one
inline Board load_raw(const uint8_t *p)
{
    Board b;
    memcpy(b.r, p, 16);
    return b;
}

// plain cells, taken mod 32 as input_cells<true> takes them on the device
inline Board load_cells(const uint8_t *p)
{
    Board b = load_raw(p);
    for (uint32_t &r : b.r)
        r &= kCellBits;
    return b;
}

constexpr uint64_t kBlockLanes = 256; // kBlock of g2048_kernels.h

// the network a test describes (ctypes: host_build.Desc): a g2048_ntuple_staged_net without its pointers
struct Desc {
    uint32_t T, L, F, S; // L = tuple_len: how many entries of cells[t][] are read; a list of a mixed network may end early with kNtupleEnd
    uint32_t kind;       // the shape type the call instantiates: 0 NtupleShape (S == 1), 1 NtupleStagedShape, 2 NtupleMixedShape
    uint16_t thr[8];     // the first S - 1 used
    uint8_t cells[8][6];
};

// max_kind: the largest kind the program's calls instantiate
inline bool desc_ok(const Desc *d, uint32_t max_kind)
{
    return d && d->T >= 1 && d->T <= kNtupleMaxTuples && d->L >= 1 && d->L <= kNtupleMaxLen && d->F <= kNtupleMaxFrac && d->S >= 1 &&
           d->S <= kNtupleMaxStages && d->kind <= max_kind && (d->kind != 0 || d->S == 1);
}

template <uint32_t T = 1, class Shape, class F> void with_tuple_count(uint32_t n_tuples, const Shape &sh, F &&f)
{
    if constexpr (T <= kNtupleMaxTuples) {
        if (n_tuples == T)
            f(std::integral_constant<uint32_t, T>(), sh);
        else
            with_tuple_count<T + 1>(n_tuples, sh, f);
    }
}

// f(std::integral_constant<uint32_t, T>(), shape) for the description's T in 1..8 and its shape type
template <class F> void with_tuples(const Desc *d, F &&f)
{
    const NtupleShape sh = ntuple_shape(d->T, d->L, d->cells);
    if (d->kind == 2)
        with_tuple_count(d->T, ntuple_mixed_shape(d->T, d->L, d->cells, d->S, d->thr), f);
    else if (d->kind == 1)
        with_tuple_count(d->T, ntuple_staged_shape(sh, d->S, d->thr), f);
    else
        with_tuple_count(d->T, sh, f);
}

} // namespace
