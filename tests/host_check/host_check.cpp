// host_check.cpp -- TEST HARNESS ONLY: compiles the device header g2048_device.h with g++
// (-DG2048_HOST_CHECK) so that the exact byte-parallel arithmetic the gfx950 kernels run can be
// unit-tested against the oracle in a container that has no GPU.  It mirrors the bodies of
// step_kernel / reset_kernel (g2048_kernels.hip) one board at a time; the last two sections do the same for the
// expectimax and Monte-Carlo search.  Not part of the product.
#include "../host_common/ntuple_host.h" // g2048_device.h for the host, HostTables, load_raw, load_cells

#include "../../gym-2048_amd/csrc/g2048_pcg64.h"
#include "../../oracle/g2048_oracle.h"

static void store_board(uint8_t *b, const Board &bd) { std::memcpy(b, bd.r, 16); }

extern "C" {

void hostcheck_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    const Words w = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    std::memcpy(out, w.w, 16);
}

// one line through shift4 (byte lane `lane` of the four SWAR registers; other lanes get junk rows)
uint32_t hostcheck_shift(const uint8_t row[4], uint8_t out[4], int lane, const uint8_t junk[12])
{
    uint32_t r[4] = {0, 0, 0, 0};
    int j = 0;
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 4; ++k)
            r[k] |= (uint32_t)(l == lane ? row[k] : junk[j++ % 12]) << (8 * l);
    // score of the junk lanes alone
    uint32_t rj[4];
    for (int k = 0; k < 4; ++k)
        rj[k] = r[k] & ~(0xffu << (8 * lane));
    uint32_t a = r[0], b = r[1], c = r[2], d = r[3];
    const uint32_t total = shift4(a, b, c, d);
    const uint32_t junk_score = shift4(rj[0], rj[1], rj[2], rj[3]);
    out[0] = (a >> (8 * lane)) & 0xff;
    out[1] = (b >> (8 * lane)) & 0xff;
    out[2] = (c >> (8 * lane)) & 0xff;
    out[3] = (d >> (8 * lane)) & 0xff;
    return total - junk_score;
}

int hostcheck_move(const uint8_t in[16], uint32_t action, uint8_t out[16], uint32_t *score)
{
    Board bd = load_raw(in);
    const bool legal = move(bd, action, *score);
    store_board(out, bd);
    return legal;
}

uint32_t hostcheck_highest(const uint8_t in[16]) { return highest(load_raw(in)); }
uint32_t hostcheck_count_empty(const uint8_t in[16]) { return count_empty(load_raw(in)); }
int hostcheck_has_equal_neighbours(const uint8_t in[16]) { return has_equal_neighbours(load_raw(in)); }

void hostcheck_add_tile(uint8_t b[16], uint32_t w)
{
    Board bd = load_raw(b);
    add_tile(bd, w);
    store_board(b, bd);
}

void hostcheck_reset_batch(g2048o_batch *s, uint64_t n, uint64_t seed, uint64_t t, uint64_t board_offset,
                           uint32_t first_slot, int)
{
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t b = (uint32_t)(board_offset + i);
        const Words w = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), b, first_slot >> 2, (uint32_t)seed,
                                      (uint32_t)(seed >> 32));
        const uint32_t sl = first_slot & 3u;
        const uint32_t w1 = select_word(w, sl);
        uint32_t w2;
        if (sl == 3u)
            w2 = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), b, (first_slot >> 2) + 1u, (uint32_t)seed,
                               (uint32_t)(seed >> 32)).w[0];
        else
            w2 = select_word(w, sl + 1u);
        store_board(s->boards + 16 * i, fresh_board(w1, w2));
        s->score[i] = 0;
        s->ep_start[i] = (uint32_t)t;
    }
}

void hostcheck_step_batch(g2048o_batch *s, uint64_t n, uint64_t seed, uint64_t t, uint64_t board_offset,
                          float illegal_move_reward, int max_exp, int auto_reset, int)
{
    for (uint64_t i = 0; i < n; ++i) {
        Board bd = load_raw(s->boards + 16 * i);
        int32_t score = s->score[i];
        const Words w = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)(board_offset + i), 0u,
                                      (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t action = s->actions ? (s->actions[i] & 3u) : (w.w[3] >> 30);
        const StepResult r = step_env(bd, score, action, w, illegal_move_reward, (uint32_t)max_exp, auto_reset != 0);
        if (s->reward) s->reward[i] = r.reward;
        if (s->terminated) s->terminated[i] = r.terminated;
        if (s->illegal) s->illegal[i] = r.illegal;
        if (s->highest) s->highest[i] = (uint8_t)highest(r.terminal);
        if (r.terminated) {
            if (s->terminal_boards) store_board(s->terminal_boards + 16 * i, r.terminal);
            s->last_score[i] = r.terminal_score;
            s->last_len[i] = (int32_t)((uint32_t)t - s->ep_start[i]);
            s->ep_count[i] += 1;
            if (auto_reset) s->ep_start[i] = (uint32_t)t;
        }
        store_board(s->boards + 16 * i, bd);
        s->score[i] = score;
    }
}

// ---- the RECORD layout and the per-step kernel's flow (step_kernel in g2048_kernels.hip), one board
// at a time: state lives in `records` (16 B per board: cells + packed score deficit); the plain boards /
// scores of the batch struct are exported after every call so the test can compare them with the oracle's.
static void export_record(g2048o_batch *s, uint64_t i, const Board &rec)
{
    store_board(s->boards + 16 * i, record_cells(rec));
    s->score[i] = (int32_t)record_score(rec);
}

int hostcheck_move_sel(const uint8_t in[16], uint32_t action, uint8_t out[16], uint32_t *score)
{
    Board bd = load_raw(in);
    const bool legal = move_sel(bd, HostTables().move_sel(action), *score);
    store_board(out, bd);
    return legal;
}

uint32_t hostcheck_potential(const uint8_t in[16]) { return potential(load_raw(in)); }

void hostcheck_make_record(const uint8_t cells[16], uint32_t score, uint8_t rec[16])
{
    store_board(rec, make_record(load_raw(cells), score));
}

uint32_t hostcheck_record_score(const uint8_t rec[16]) { return record_score(load_raw(rec)); }
uint32_t hostcheck_record_deficit(const uint8_t rec[16]) { return record_deficit(load_raw(rec)); }

// record_update with an arbitrary number of "+4" carries (exercises the ripple through the cell bits)
void hostcheck_record_bump(uint8_t rec[16], uint32_t times)
{
    Board raw = load_raw(rec);
    for (uint32_t k = 0; k < times; ++k)
        record_update(raw, record_cells(raw), 0x80u);
    store_board(rec, raw);
}

void hostcheck_reset_records(g2048o_batch *s, uint8_t *records, uint64_t n, uint64_t seed, uint64_t t,
                             uint64_t board_offset, uint32_t first_slot)
{
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t b = (uint32_t)(board_offset + i);
        const Words w = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), b, first_slot >> 2, (uint32_t)seed,
                                      (uint32_t)(seed >> 32));
        const uint32_t sl = first_slot & 3u;
        const uint32_t w1 = select_word(w, sl);
        uint32_t w2;
        if (sl == 3u)
            w2 = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), b, (first_slot >> 2) + 1u, (uint32_t)seed,
                               (uint32_t)(seed >> 32)).w[0];
        else
            w2 = select_word(w, sl + 1u);
        const Board rec = fresh_record(w1, w2);
        store_board(records + 16 * i, rec);
        export_record(s, i, rec);
        s->ep_start[i] = (uint32_t)t;
    }
}

void hostcheck_fresh_record_lut(uint32_t w1, uint32_t w2, uint8_t out_lut[16], uint8_t out_ref[16])
{
    store_board(out_lut, fresh_record_lut(w1, w2, HostTables{}));
    store_board(out_ref, fresh_record(w1, w2));
}

// step_kernel's body (g2048_kernels.hip): step_record + outputs + episode bookkeeping; last_records
// [n][16] is the engine's last_record array.
void hostcheck_step_records(g2048o_batch *s, uint8_t *records, uint8_t *last_records, uint64_t n, uint64_t seed, uint64_t t,
                            uint64_t board_offset, float illegal_move_reward, int max_exp, int auto_reset)
{
    for (uint64_t i = 0; i < n; ++i) {
        Board rec = load_raw(records + 16 * i);
        const Words w = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)(board_offset + i), 0u,
                                      (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t action = s->actions ? (s->actions[i] & 3u) : (w.w[3] >> 30);
        const StepOut o = step_record(rec, action, w, (uint32_t)max_exp, auto_reset != 0, HostTables{});
        store_board(records + 16 * i, rec);
        if (s->reward) s->reward[i] = o.legal ? (float)o.gain : illegal_move_reward;
        if (s->terminated) s->terminated[i] = o.terminated;
        if (s->illegal) s->illegal[i] = !o.legal;
        if (s->highest) s->highest[i] = (uint8_t)highest(record_cells(o.terminal));
        if (o.terminated) {
            store_board(last_records + 16 * i, o.terminal);
            if (s->terminal_boards) store_board(s->terminal_boards + 16 * i, record_cells(o.terminal));
            s->last_score[i] = (int32_t)record_score(load_raw(last_records + 16 * i)); // g2048_get_last_scores
            s->last_len[i] = (int32_t)((uint32_t)t - s->ep_start[i]);
            s->ep_count[i] += 1;
            if (auto_reset) s->ep_start[i] = (uint32_t)t;
        }
        export_record(s, i, rec);
    }
}

// the fused kernels' way through the record: unpack once, step_env, pack
void hostcheck_step_records_unpacked(g2048o_batch *s, uint8_t *records, uint8_t *, uint64_t n, uint64_t seed, uint64_t t,
                                     uint64_t board_offset, float illegal_move_reward, int max_exp, int auto_reset)
{
    for (uint64_t i = 0; i < n; ++i) {
        const Board raw = load_raw(records + 16 * i);
        Board bd = record_cells(raw);
        int32_t score = (int32_t)record_score(raw);
        const Words w = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)(board_offset + i), 0u,
                                      (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t action = s->actions ? (s->actions[i] & 3u) : (w.w[3] >> 30);
        const StepResult r = step_env(bd, score, action, w, illegal_move_reward, (uint32_t)max_exp, auto_reset != 0);
        if (s->reward) s->reward[i] = r.reward;
        if (s->terminated) s->terminated[i] = r.terminated;
        if (s->illegal) s->illegal[i] = r.illegal;
        if (s->highest) s->highest[i] = (uint8_t)highest(r.terminal);
        if (r.terminated) {
            if (s->terminal_boards) store_board(s->terminal_boards + 16 * i, r.terminal);
            s->last_score[i] = r.terminal_score;
            s->last_len[i] = (int32_t)((uint32_t)t - s->ep_start[i]);
            s->ep_count[i] += 1;
            if (auto_reset) s->ep_start[i] = (uint32_t)t;
        }
        const Board rec = make_record(bd, (uint32_t)score);
        store_board(records + 16 * i, rec);
        export_record(s, i, rec);
    }
}

// ---- numpy-compatible RNG mode (g2048_pcg64.h); rng = [n][5] uint64 as in the oracle
static Pcg64 load_rng(const g2048o_pcg64 *r) { return Pcg64{r->state_lo, r->state_hi, r->inc_lo, r->inc_hi, r->buf}; }
static void store_rng(g2048o_pcg64 *r, const Pcg64 &p)
{
    r->state_lo = p.state_lo; r->state_hi = p.state_hi; r->inc_lo = p.inc_lo; r->inc_hi = p.inc_hi; r->buf = p.buf;
}

// The observation piece of ONE wavefront (64 boards, records with their spare bits set as the engine keeps them),
// built exactly as emit_onehot does on the device: records parked with the cells masked, chunk s * 64 + lane of store
// s from onehot_chunk<OBS>.  out: 64 boards x 16 channels x 16 cells of 1 / 2 / 4 bytes.
void hostcheck_onehot_wave(const uint8_t *records, int obs_dtype, uint8_t *out)
{
    Cells16 recs[64];
    for (int l = 0; l < 64; ++l) {
        const Board cells = record_cells(load_raw(records + 16 * l));
        for (int k = 0; k < 4; ++k)
            recs[l].r[k] = cells.r[k];
    }
    const uint32_t stores = 16u << obs_dtype;
    for (uint32_t s = 0; s < stores; ++s)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t board;
            const Chunk16 c = obs_dtype == 0 ? onehot_chunk<0>(recs, s, lane, board)
                              : obs_dtype == 1 ? onehot_chunk<1>(recs, s, lane, board) : onehot_chunk<2>(recs, s, lane, board);
            std::memcpy(out + (static_cast<size_t>(s) * 64 + lane) * 16, c.w, 16);
        }
}

uint64_t hostcheck_pcg64_next64(g2048o_pcg64 *r) { Pcg64 p = load_rng(r); const uint64_t v = pcg64_next64(p); store_rng(r, p); return v; }
uint32_t hostcheck_pcg64_next32(g2048o_pcg64 *r) { Pcg64 p = load_rng(r); const uint32_t v = pcg64_next32(p); store_rng(r, p); return v; }
uint32_t hostcheck_pcg64_interval(g2048o_pcg64 *r, uint32_t mx) { Pcg64 p = load_rng(r); const uint32_t v = pcg64_interval(p, mx); store_rng(r, p); return v; }
void hostcheck_pcg64_from_seed(uint64_t entropy, g2048o_pcg64 *out) { store_rng(out, pcg64_from_seed(entropy)); }
uint32_t hostcheck_empty_mask16(const uint8_t b[16]) { return empty_mask16(load_raw(b)); }

void hostcheck_reset_batch_numpy(g2048o_batch *s, g2048o_pcg64 *rng, uint64_t n, uint64_t t, int)
{
    for (uint64_t i = 0; i < n; ++i) {
        Pcg64 p = load_rng(&rng[i]);
        const Board rec = fresh_record_numpy(p); // what reset_numpy_kernel and the step kernel's in-block reset store
        store_rng(&rng[i], p);
        store_board(s->boards + 16 * i, record_cells(rec));
        s->score[i] = (int32_t)record_score(rec); // 0: the deficit of a fresh record is its potential
        s->ep_start[i] = (uint32_t)t;
    }
}

void hostcheck_step_batch_numpy(g2048o_batch *s, g2048o_pcg64 *rng, uint64_t n, uint64_t seed, uint64_t t,
                                uint64_t board_offset, float illegal_move_reward, int max_exp, int auto_reset, int)
{
    for (uint64_t i = 0; i < n; ++i) {
        Board bd = load_raw(s->boards + 16 * i);
        int32_t score = s->score[i];
        Pcg64 p = load_rng(&rng[i]);
        uint32_t action;
        if (s->actions)
            action = s->actions[i] & 3u;
        else
            action = philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)(board_offset + i), 0u, (uint32_t)seed,
                                   (uint32_t)(seed >> 32)).w[3] >> 30;
        // exactly step_numpy_kernel's sequence, on the RECORD: play_record_numpy, then (auto-reset) fresh_record_numpy
        Board rec = make_record(bd, (uint32_t)score);
        const NumpyStepOut o = play_record_numpy(rec, action, p, (uint32_t)max_exp, auto_reset != 0);
        if (s->reward) s->reward[i] = o.legal ? (float)o.gain : illegal_move_reward;
        if (s->terminated) s->terminated[i] = o.terminated;
        if (s->illegal) s->illegal[i] = !o.legal;
        if (s->highest) s->highest[i] = (uint8_t)o.top;
        if (o.terminated) {
            if (s->terminal_boards) store_board(s->terminal_boards + 16 * i, record_cells(rec));
            s->last_score[i] = (int32_t)record_score(rec);
            s->last_len[i] = (int32_t)((uint32_t)t - s->ep_start[i]);
            s->ep_count[i] += 1;
            if (auto_reset) {
                s->ep_start[i] = (uint32_t)t;
                rec = finish_record_numpy(p, o.have_first, o.first_cell, o.first_four);
            }
        }
        store_rng(&rng[i], p);
        store_board(s->boards + 16 * i, record_cells(rec));
        s->score[i] = (int32_t)record_score(rec);
    }
}

} // extern "C"

// ---- expectimax search (g2048_expectimax): the search code of g2048_device.h, one board at a time on one thread.
// tests/test_search_host.py compares it with the pure-Python reference (tests/search_ref.py), the GPU tests compare the
// kernels with it, and tools/search_probe.py times it as the host baseline.
namespace {

SearchWeights weights(const int32_t w[4])
{
    return SearchWeights{(uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3]};
}

template <int D> uint32_t root(const Board &b, const SearchWeights &w, int32_t value[4])
{
    return search_root<D>(b, w, HostTables(), value);
}

// the kernels' split: K lanes per direction, each summing its own chance items, then one sum and one divide
template <int D> void root_split(const Board &b, const SearchWeights &w, uint32_t K, int32_t value[4])
{
    for (uint32_t m = 0; m < 4; ++m) {
        Board a = b;
        uint32_t gain;
        if (!move_sel(a, HostTables().move_sel(m), gain)) {
            value[m] = -1;
            continue;
        }
        uint64_t sum = 0;
        for (uint32_t sub = 0; sub < K; ++sub)
            sum += chance_partial<D>(a, sub, K, w, HostTables());
        value[m] = (int32_t)(sum / (10u * count_empty(a)));
    }
}

// number of heuristic evaluations (leaves) of V_D(b), mirroring search_value / chance_partial
template <int D> uint64_t leaves_value(const Board &b)
{
    if constexpr (D == 0) {
        return 1;
    } else {
        uint64_t total = 0;
        for (uint32_t m = 0; m < 4; ++m) {
            Board a = b;
            uint32_t gain;
            if (move_sel(a, HostTables().move_sel(m), gain))
                for (uint32_t e = empty_bits(a); e; e &= e - 1)
                    for (uint32_t v = 1; v <= 2; ++v)
                        total += leaves_value<D - 1>(place(a, g2048_ctz(e), v));
        }
        return total;
    }
}

} // namespace

extern "C" {

// total leaves of a depth-`depth` search over n boards (the root is V_depth without its max)
uint64_t search_check_leaves(const uint8_t *boards, uint64_t n, uint32_t depth)
{
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        total += depth == 1 ? leaves_value<1>(b) : depth == 2 ? leaves_value<2>(b) : leaves_value<3>(b);
    }
    return total;
}

uint32_t search_check_heuristic(const uint8_t board[16], const int32_t w[4])
{
    return heuristic(load_cells(board), weights(w));
}

// action[n] and value[n][4] of g2048_expectimax_plain; returns 0, or -1 for a depth outside 1..3
int search_check_boards(const uint8_t *boards, uint64_t n, uint32_t depth, const int32_t w[4], uint8_t *action,
                        int32_t *value)
{
    if (depth < 1 || depth > 3)
        return -1;
    const SearchWeights sw = weights(w);
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        int32_t *v = value + 4 * i;
        action[i] = (uint8_t)(depth == 1 ? root<1>(b, sw, v) : depth == 2 ? root<2>(b, sw, v) : root<3>(b, sw, v));
    }
    return 0;
}

// the root values through the kernels' lane split with K lanes per direction
int search_check_split(const uint8_t *boards, uint64_t n, uint32_t depth, const int32_t w[4], uint32_t K, int32_t *value)
{
    if (depth < 1 || depth > 3 || K == 0)
        return -1;
    const SearchWeights sw = weights(w);
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        int32_t *v = value + 4 * i;
        if (depth == 1)
            root_split<1>(b, sw, K, v);
        else if (depth == 2)
            root_split<2>(b, sw, K, v);
        else
            root_split<3>(b, sw, K, v);
    }
    return 0;
}

} // extern "C"

// ---- Monte-Carlo rollout search (g2048_mc_search), likewise.  tests/test_mc_host.py compares it with the pure-Python
// reference (tests/mc_ref.py), the GPU tests compare the kernel with it, and tools/mc_probe.py's games run on it.
namespace {

bool any_legal(const Board &b)
{
    for (uint32_t d = 0; d < 4; ++d) {
        Board a = b;
        uint32_t g;
        if (move_sel(a, HostTables().move_sel(d), g))
            return true;
    }
    return false;
}

} // namespace

extern "C" {

// action[n], value[n][4], steps[n][4] of g2048_mc_search_plain; returns 0, or -1 for R or L outside their limits
int mc_check_boards(const uint8_t *boards, uint64_t n, uint32_t index_offset, uint32_t rollouts, uint32_t max_steps, uint64_t seed,
                    uint8_t *action, int64_t *value, int64_t *steps)
{
    if (rollouts < 1 || rollouts > kMcMaxRollouts || max_steps < 1 || max_steps > kMcMaxSteps)
        return -1;
    for (uint64_t i = 0; i < n; ++i)
        action[i] = (uint8_t)mc_root(load_cells(boards + 16 * i), index_offset + (uint32_t)i, rollouts, max_steps, (uint32_t)seed,
                                     (uint32_t)(seed >> 32), HostTables(), value + 4 * i, steps + 4 * i);
    return 0;
}

// the root sums through the kernel's lane split: K lanes per direction, lane sub sums the playouts sub, sub + K, ...
int mc_check_split(const uint8_t *boards, uint64_t n, uint32_t index_offset, uint32_t rollouts, uint32_t max_steps, uint64_t seed,
                   uint32_t K, int64_t *value, int64_t *steps)
{
    if (rollouts < 1 || rollouts > kMcMaxRollouts || max_steps < 1 || max_steps > kMcMaxSteps || K == 0)
        return -1;
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        for (uint32_t d = 0; d < 4; ++d) {
            Board after = b;
            uint32_t g;
            value[4 * i + d] = steps[4 * i + d] = -1;
            if (!move_sel(after, HostTables().move_sel(d), g))
                continue;
            uint64_t total = 0, st = 0;
            for (uint32_t sub = K; sub-- > 0;) // the lanes in another order than mc_root's r = 0, 1, ...
                mc_partial(after, g, index_offset + (uint32_t)i, d, sub, K, rollouts, (uint32_t)seed, (uint32_t)(seed >> 32), max_steps,
                           HostTables(), total, st);
            value[4 * i + d] = (int64_t)total;
            steps[4 * i + d] = (int64_t)st;
        }
    }
    return 0;
}

// Whole games on the CPU: game k starts from fresh_board and is played to its end by the Monte-Carlo player
// (rollouts > 0; the search of move t is seeded seed + t + 1 and sees board index k) or, with rollouts == 0, by the
// uniform random policy under the engine's rule that an illegal move ends the episode.  The game's own spawns and the
// random policy's actions come from Philox blocks keyed by `seed` with counter word 3 = 0xffffffff.  scores[k] = the
// summed merge scores, moves[k] = the moves played; illegal_picks counts searched moves that were illegal while a legal
// one existed.  Returns that count.
uint64_t mc_check_play(uint64_t n_games, uint64_t seed, uint32_t rollouts, uint32_t max_steps, int64_t *scores, int64_t *moves)
{
    const HostTables tb;
    uint64_t illegal_picks = 0;
    for (uint64_t k = 0; k < n_games; ++k) {
        const Words w0 = philox4x32_10(0u, 0u, (uint32_t)k, 0xffffffffu, (uint32_t)seed, (uint32_t)(seed >> 32));
        Board b = fresh_board(w0.w[0], w0.w[1]);
        int64_t score = 0, t = 0;
        while (any_legal(b)) {
            const Words w = philox4x32_10((uint32_t)(t + 1), 0u, (uint32_t)k, 0xffffffffu, (uint32_t)seed, (uint32_t)(seed >> 32));
            uint32_t action = w.w[3] >> 30;
            if (rollouts > 0) {
                int64_t value[4], steps[4];
                const uint64_t s = seed + (uint64_t)t + 1u;
                action = mc_root(b, (uint32_t)k, rollouts, max_steps, (uint32_t)s, (uint32_t)(s >> 32), tb, value, steps);
            }
            uint32_t g;
            if (!move_sel(b, tb.move_sel(action), g)) {
                illegal_picks += rollouts > 0;
                break; // the engine's rule: an illegal move ends the episode
            }
            score += g;
            ++t;
            add_tile(b, w.w[0]);
        }
        scores[k] = score;
        moves[k] = t;
    }
    return illegal_picks;
}

} // extern "C"
