// g2048_api.hip -- the C ABI of include/g2048.h on top of the gfx950 kernels.
// Host-side only: argument checking, the engine object, the transaction clock, launches.
#include "../../include/g2048.h"

#include "g2048_kernels.h"
#include "g2048_side_launcher.h"

#include <rccl/rccl.h> // declarations only: librccl is dlopen()ed by the first g2048_comm_* call

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>

namespace {

thread_local char g_error[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

#define G2048_HIP(call)                                                                                        \
    do {                                                                                                       \
        hipError_t err_ = (call);                                                                              \
        if (err_ != hipSuccess)                                                                                \
            return fail(G2048_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(err_));                       \
    } while (0)

using g2048::SideLauncher;
using g2048::cpu_relax;

// The engine's memory is held by two owner types; each frees what it holds when it is destroyed or reset, and its
// alloc() is the one place that memory of its kind is allocated.  alloc() does nothing when the owner already holds a
// buffer (every buffer of an engine has one size for the engine's lifetime), and names `what` the buffer is for when it
// fails.

// Device memory.  `zero`: cleared before alloc() returns -- hipMemset only ENQUEUES the fill (on the null stream: 3 us
// for a call that takes 1.4 ms on 8 GiB, tools/memset_probe.py), and a caller's non-blocking stream -- every torch
// stream but the default one -- is not ordered behind the null stream, so alloc() waits for it.
struct DeviceBuffer {
    void *p = nullptr;

    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { (void)reset(); }
    template <class T> T *as() const { return static_cast<T *>(p); }

    int alloc(size_t bytes, const char *what, bool zero = false)
    {
        if (p)
            return G2048_OK;
        hipError_t err = hipMalloc(&p, bytes);
        if (err != hipSuccess) {
            p = nullptr;
            return fail(G2048_ERR_NOMEM, "hipMalloc(%zu) for %s failed: %s", bytes, what, hipGetErrorString(err));
        }
        if (zero) {
            err = hipMemset(p, 0, bytes);
            if (err == hipSuccess)
                err = hipStreamSynchronize(nullptr);
            if (err != hipSuccess) {
                (void)reset();
                return fail(G2048_ERR_HIP, "hipMemset of %s failed: %s", what, hipGetErrorString(err));
            }
        }
        return G2048_OK;
    }

    hipError_t reset()
    {
        const hipError_t err = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        return err;
    }
};

// Pinned, device-mapped, coherent host memory: its host address and the device's alias of it.  Zeroed by alloc().
struct PinnedBlock {
    void *host = nullptr, *dev = nullptr;

    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock &) = delete;
    PinnedBlock &operator=(const PinnedBlock &) = delete;
    ~PinnedBlock()
    {
        if (host)
            (void)hipHostFree(host);
    }
    explicit operator bool() const { return host != nullptr; }

    int alloc(size_t bytes, const char *what)
    {
        if (host)
            return G2048_OK;
        void *h = nullptr;
        hipError_t err = hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (err != hipSuccess)
            return fail(G2048_ERR_NOMEM, "hipHostMalloc(%zu) for %s failed: %s", bytes, what, hipGetErrorString(err));
        err = hipHostGetDevicePointer(&dev, h, 0);
        if (err != hipSuccess) {
            (void)hipHostFree(h);
            dev = nullptr;
            return fail(G2048_ERR_HIP, "hipHostGetDevicePointer for %s failed: %s", what, hipGetErrorString(err));
        }
        std::memset(h, 0, bytes);
        host = h;
        return G2048_OK;
    }
};

// ONE side chain per device and process, shared by every engine on that device that runs two chains: the side stream
// (highest priority), its launch thread, and the time its last work is expected to end.  Shared so that it stays WARM:
// a stream that has idled for a few hundred milliseconds starts its next kernels late (a forced two-chain 20-step
// rollout takes 175 us after 0.2 ms of idle, 184-186 after 5-50 ms, 223 after 300 ms -- one chain: 195-209;
// tools/chain_gap_probe.py), and e.g. a warm-up on one engine should leave the chain ready for the next engine.  `use`
// serialises the engines' rollouts on it (an engine itself is single-threaded by contract).  The engines own it; it
// ends with the last of them.
struct SideChain {
    SideLauncher launcher;
    hipStream_t stream = nullptr;
    std::mutex use;
    std::atomic<int64_t> busy_until_ns{0}; // steady-clock time the side stream's queued work is expected to have ended + the warm window
    int device = 0;
    int priority = 0; // of `stream`: the highest the device offers

    ~SideChain()
    {
        launcher.stop();
        if (stream) {
            (void)hipSetDevice(device);
            // its launches retired first: destroyed with launches the runtime had not yet retired, the stream kept the
            // slab they used (the chain tickets are in it) from being freed -- one slab per engine, measured
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }
};

std::mutex g_side_mutex;
std::weak_ptr<SideChain> g_side[64]; // the side chain of each device, while an engine holds it

int64_t steady_now_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// "\0G2048v5": records carry the score, 4-word episode slots for whole 512-lane blocks, the bytes of the engine's work
// memory behind them (written as zeros, ignored when read back).
// v4 (ABI 14) is the same games in a slab of another size; v3 and older were played under the spawn rule before ABI 14
// (g2048.h "Randomness"): a game saved under the old rule would continue differently under the new one.  Both are refused
// with the reason instead of silently resumed.
constexpr uint64_t kStateMagic = 0x3576383430324700ull;

} // namespace

struct g2048_engine {
    uint64_t n = 0;
    int device = 0;
    uint64_t seed = 0;
    uint64_t board_offset = 0;
    uint64_t t = 0;       // transaction counter
    int fresh = 1;        // nothing consumed from the stream since seeding
    float illegal_reward = 0.0f; // game2048_env.py:53
    uint32_t max_exp = 0;        // game2048_env.py:54 (0 = None)
    // ONE slab (g2048_create), zeroed at create.  GAME region -- what a state blob carries: boards | last_record |
    // ep_counters, then the engine's own work memory (statistics struct, summary scratch, graph clock), which a blob
    // holds as zeros.  WORKSPACE region behind it: statistics partials, chain tickets.
    DeviceBuffer slab;
    size_t game_bytes = 0; // size of the game region
    size_t kept_bytes = 0; // boards | last_record | ep_counters: the bytes of the game region a state blob restores
    g2048::DeviceState st{}; // st.rng is set (numpy-RNG mode) exactly while `rng` holds the planes
    g2048::StatsOut *stats_dev = nullptr;
    unsigned long long *summary_scratch = nullptr; // partials + "last one out" counters of the one-launch returns summary (zero between launches)
    unsigned long long *stats_partials = nullptr;  // stage-1 output of the statistics reduction
    DeviceBuffer rng;     // numpy-RNG mode: the five PCG64 planes plus the per-wavefront lists of finished boards
    DeviceBuffer scratch; // staging for host-side get/set of boards and scores (16 B per board), lazily
    DeviceBuffer returns; // send buffer of the all-gather (int32[n]), lazily; NOT the staging buffer: a collective
                          // in flight on one stream must not be clobbered by a get_* call on another
    // host-resident I/O (g2048_host_io_map)
    PinnedBlock host_block;
    g2048_host_io host_io{};          // host addresses handed to the caller
    g2048_host_io host_io_dev{};      // the same arrays as the device sees them
    // the words the device reports to the host through (HostWord), each on its own 64-byte line; allocated on first
    // need by any of them: a word no kernel was ever given stays zero
    PinnedBlock words;
    unsigned long long done_count = 0; // tickets published to the completion word so far
    // two-chain rollouts (g2048_set_chains): the side stream, its launch thread and the fork / join tickets
    int chains = 1;
    std::shared_ptr<SideChain> side; // the device's shared side chain (held once chains == 2 was ever set)
    unsigned long long *chain_flags = nullptr; // in the workspace (256 B): [0] fork ticket, [16] join ticket (own cache lines), [24] scratch
    unsigned long long chain_seq = 0;
    // the measurement / test knobs of the two-chain form, read from the environment by g2048_set_chains (NOT per rollout)
    uint32_t chain_min_steps = 0;      // G2048_TWO_CHAIN_MIN_STEPS: split every rollout of at least that many steps (0: the warm / cold rule)
    uint32_t chain_wait_polls = g2048::kFlagWaitPolls; // G2048_FLAG_WAIT_POLLS: bound of a ticket wait, ~1 us per poll
    // set when a call left the engine in a state its caller cannot know (a two-chain rollout that failed half-way):
    // every later call fails with this message instead of continuing on half-stepped boards
    int poisoned = 0;
    char poison_msg[320] = "";
    int last_rollout_chains = 1; // what the most recent g2048_rollout did (g2048_get_chains_used)
    // A rollout over the SAME buffers as the one before it is replayed from a cached hipGraph when the batch is small
    // enough for the host's launch rate to be the limit (g2048_rollout; kGraphMaxBoards).  The key is everything the
    // graph's frozen kernel arguments depend on; the clock comes through *graph_t_dev.
    struct GraphKey {
        uint32_t k_steps = 0;
        uint64_t stride = 0, seed = 0, board_offset = 0;
        const void *actions = nullptr;
        float *reward = nullptr;
        uint8_t *terminated = nullptr;
        uint4 *last_record = nullptr;
        int32_t action_dtype = 0;
        int auto_reset = 0;
        float illegal_reward = 0.0f;
        bool operator==(const GraphKey &o) const
        {
            return k_steps == o.k_steps && stride == o.stride && seed == o.seed && board_offset == o.board_offset && actions == o.actions &&
                   reward == o.reward && terminated == o.terminated && last_record == o.last_record && action_dtype == o.action_dtype &&
                   auto_reset == o.auto_reset && std::memcmp(&illegal_reward, &o.illegal_reward, sizeof(float)) == 0;
        }
    };
    struct GraphEntry {
        GraphKey key{};
        g2048::RolloutGraph g{};
        hipStream_t last_stream = nullptr; // where it was last replayed (an entry is only evicted once that stream has drained)
    };
    static constexpr int kGraphSlots = 4;  // a trainer alternates between a few sets of rollout buffers at most
    GraphEntry graphs[kGraphSlots];        // the cached graphs, replaced round robin
    int graph_next = 0;
    GraphKey graph_seen{};                 // the key of the previous rollout that was eligible (cached or not)
    unsigned long long *graph_t_dev = nullptr;
    uint32_t graph_max_boards = 1u << 17; // batches up to this size use the form (G2048_GRAPH_MAX_BOARDS, read by g2048_create)
    int graph_enabled = 1;              // G2048_ROLLOUT_GRAPH=0 (read by g2048_create) turns the form off; a failing graph call too
    char graph_off_reason[200] = "";    // ... and says why here (g2048_graph_status)
    uint64_t graph_replays = 0;         // rollouts served from the cached graph (g2048_get_graph_replays)
    // strict actions (g2048_set_strict_actions): a step kernel reports an action outside 0..3 to kActionErrWord
    int strict_actions = 0;
    int track_last = 1;   // keep the terminal record of every board's most recent finished episode (g2048_set_last_records)
};

namespace {

struct StateHeader {
    uint64_t magic, n, seed, board_offset, t;
    int32_t fresh;
    uint32_t max_exp;
    float illegal_reward;
    uint32_t reserved;
};

size_t align_up(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// The words of g2048_engine::words: the completion word (published by the device, polled by the host), where a
// two-chain ticket wait that ran out reports (flag_wait_kernel), and where a step kernel reports an action outside 0..3
// under strict actions.  The two error words are checked at the entry of every call on the engine (usable).
enum HostWord { kDoneWord = 0, kChainErrWord = 1, kActionErrWord = 2 };

unsigned long long *host_word(const g2048_engine *e, HostWord w) { return static_cast<unsigned long long *>(e->words.host) + 8 * w; }
unsigned long long *dev_word(const g2048_engine *e, HostWord w) { return static_cast<unsigned long long *>(e->words.dev) + 8 * w; }

int ensure_words(g2048_engine *e) { return e->words.alloc(3 * 64, "the completion, chain timeout and strict-actions words"); }

// the device state as the kernels should see it: no terminal-record array when the engine does not keep them
g2048::DeviceState tracked_state(const g2048_engine *e)
{
    g2048::DeviceState st = e->st;
    if (!e->track_last)
        st.last_record = nullptr; // the kernels skip the terminal-record store
    return st;
}

g2048::StepArgs make_args(const g2048_engine *e, const g2048_step_io *io, int auto_reset)
{
    g2048::StepArgs a{};
    a.st = tracked_state(e);
    if (io) {
        a.actions = io->actions;
        a.reward = io->reward;
        a.terminated = io->terminated;
        a.illegal = io->illegal;
        a.highest = io->highest;
        a.terminal_boards = reinterpret_cast<uint4 *>(io->terminal_boards);
        a.obs = io->obs;
        a.obs_dtype = static_cast<uint32_t>(io->obs_dtype);
        a.boards_out = reinterpret_cast<uint4 *>(io->boards_out);
    }
    a.action_err = e->strict_actions ? dev_word(e, kActionErrWord) : nullptr;
    a.n = static_cast<uint32_t>(e->n);
    a.board_offset = static_cast<uint32_t>(e->board_offset);
    a.seed_lo = static_cast<uint32_t>(e->seed);
    a.seed_hi = static_cast<uint32_t>(e->seed >> 32);
    a.t_lo = static_cast<uint32_t>(e->t);
    a.t_hi = static_cast<uint32_t>(e->t >> 32);
    a.illegal_reward = e->illegal_reward;
    a.max_exp = e->max_exp;
    a.auto_reset = auto_reset ? 1u : 0u;
    return a;
}

int need_last_records(const g2048_engine *e, const char *what)
{
    if (e->track_last)
        return G2048_OK;
    return fail(G2048_ERR_INVALID, "%s reads the boards' terminal records, which this engine does not keep "
                                   "(g2048_set_last_records(e, 1, stream) turns them on)", what);
}

size_t obs_board_bytes(int dtype) { return static_cast<size_t>(256) << (dtype < 0 ? 0 : dtype); } // 16 channels x 16 cells

// Every call on an engine starts here: NULL, poisoned (a call that failed half-way), or a two-chain ticket wait that
// ran out on the device (the chains ran unordered since: whatever the engine holds is undefined).
int usable(const g2048_engine *e)
{
    if (!e)
        return fail(G2048_ERR_INVALID, "engine is NULL");
    if (e->poisoned)
        return fail(G2048_ERR_HIP, "%s", e->poison_msg);
    if (e->words) {
        const unsigned long long *chain_err = host_word(e, kChainErrWord);
        if (__atomic_load_n(chain_err, __ATOMIC_ACQUIRE) != 0ull)
            return fail(G2048_ERR_HIP, "a two-chain rollout's ordering ticket (%llu) did not arrive within the wait's bound "
                                       "(%u polls of ~1 us): its chains ran unordered from there on, the engine's boards and "
                                       "the rollout's outputs are undefined -- destroy the engine",
                        __atomic_load_n(chain_err, __ATOMIC_ACQUIRE), e->chain_wait_polls);
        // strict actions: a step kernel that has COMPLETED by now saw an action outside 0..3.  Reported once, by this call
        // (which does nothing else), and cleared; the step itself played the action's low two bits.
        const unsigned long long w = __atomic_exchange_n(host_word(e, kActionErrWord), 0ull, __ATOMIC_ACQ_REL);
        if (w != 0ull)
            return fail(G2048_ERR_INVALID, "strict actions: an earlier step was given an action outside 0..3 (e.g. global board %u, "
                                           "low byte 0x%02x); that step played the action's low two bits (the reference, "
                                           "game2048_env.py:210-212, would have played 4 as 'down' and -1 as 'right').  "
                                           "This call did nothing; the report is cleared",
                        static_cast<unsigned>(w & 0xffffffffull), static_cast<unsigned>((w >> 32) & 0xffu));
    }
    return G2048_OK;
}

int poison(g2048_engine *e, const char *what)
{
    e->poisoned = 1;
    snprintf(e->poison_msg, sizeof e->poison_msg, "%s; the engine is unusable from here on (a rollout was left half-done): destroy it", what);
    return fail(G2048_ERR_HIP, "%s", e->poison_msg);
}

size_t action_size(int dtype)
{
    switch (dtype) {
    case G2048_ACT_U8: return 1;
    case G2048_ACT_I32: return 4;
    case G2048_ACT_I64: return 8;
    default: return 0;
    }
}

int check_io(const g2048_step_io *io)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (io->action_dtype < G2048_ACT_RANDOM || io->action_dtype > G2048_ACT_I64)
        return fail(G2048_ERR_INVALID, "unknown action_dtype %d", io->action_dtype);
    if (io->action_dtype != G2048_ACT_RANDOM && !io->actions)
        return fail(G2048_ERR_INVALID, "actions is NULL but action_dtype is %d", io->action_dtype);
    // the kernels use natural-width loads and stores
    if ((reinterpret_cast<uintptr_t>(io->actions) & (action_size(io->action_dtype) ? action_size(io->action_dtype) - 1 : 0)) ||
        (reinterpret_cast<uintptr_t>(io->reward) & 3u) || (reinterpret_cast<uintptr_t>(io->terminal_boards) & 15u) ||
        (reinterpret_cast<uintptr_t>(io->boards_out) & 15u))
        return fail(G2048_ERR_INVALID, "misaligned buffer: actions need their element size, reward 4 bytes, "
                                       "terminal_boards and boards_out 16 bytes");
    if (io->obs) {
        if (io->obs_dtype < G2048_OBS_U8 || io->obs_dtype > G2048_OBS_F32)
            return fail(G2048_ERR_INVALID, "unknown obs_dtype %d", io->obs_dtype);
        if (reinterpret_cast<uintptr_t>(io->obs) & 15u)
            return fail(G2048_ERR_INVALID, "misaligned buffer: obs needs 16 bytes");
    }
    return G2048_OK;
}

} // namespace

extern "C" {

const char *g2048_last_error(void) { return g_error; }

int g2048_abi_version(void) { return 16; }

int g2048_create(uint64_t n_boards, int device, uint64_t seed, uint64_t board_offset, g2048_engine **out)
{
    if (!out)
        return fail(G2048_ERR_INVALID, "out is NULL");
    *out = nullptr;
    // (the launch grid is whole 256-lane blocks indexed in 32 bits, hence the 0xffffff00 cap)
    if (n_boards == 0 || n_boards > 0xffffff00ull || board_offset + n_boards > 0x100000000ull)
        return fail(G2048_ERR_INVALID, "n_boards=%llu board_offset=%llu: global board indices must fit 32 bits",
                    (unsigned long long)n_boards, (unsigned long long)board_offset);
    int count = 0;
    hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count == 0)
        return fail(G2048_ERR_HIP, "no HIP device available (%s); this library has no CPU path",
                    err != hipSuccess ? hipGetErrorString(err) : "device count is 0");
    if (device < 0 || device >= count)
        return fail(G2048_ERR_INVALID, "device %d out of range (have %d)", device, count);
    G2048_HIP(hipSetDevice(device));

    g2048_engine *e = new (std::nothrow) g2048_engine;
    if (!e)
        return fail(G2048_ERR_NOMEM, "out of host memory");
    e->n = n_boards;
    e->device = device;
    e->seed = seed;
    e->board_offset = board_offset;
    if (const char *v = std::getenv("G2048_ROLLOUT_GRAPH"))
        e->graph_enabled = std::atoi(v) != 0;
    if (const char *v = std::getenv("G2048_GRAPH_MAX_BOARDS")) { // measurement knob
        const long long m = std::atoll(v);
        if (m >= 0 && m <= 0xffffffffll)
            e->graph_max_boards = static_cast<uint32_t>(m);
    }

    const size_t n = n_boards;
    // game region (the layout tests/episode_slots.py decodes)
    const size_t off_boards = 0;
    const size_t off_last_record = off_boards + align_up(n * 16);
    const size_t off_counters = off_last_record + align_up(n * 16);
    // one slot of kSlotWords counters per 64 boards (whole launch blocks of the largest block size: a wavefront that lies
    // wholly past the end still loads and stores ITS slot)
    const size_t n_counters = ((n + g2048::kSlotBlockLanes - 1) / g2048::kSlotBlockLanes) * (g2048::kSlotBlockLanes / 64) * g2048::kSlotWords;
    const size_t off_stats = off_counters + align_up(n_counters * sizeof(unsigned long long));
    const size_t off_summary = off_stats + align_up(sizeof(g2048::StatsOut));
    // the clock word of the cached rollout graphs: in the slab, so that building one allocates nothing
    const size_t off_graph_t = off_summary + align_up(g2048::kSummaryScratchWords * sizeof(unsigned long long));
    // workspace region
    const size_t off_partials = off_graph_t + 256;
    const size_t off_chain = off_partials + align_up(g2048::kStatsPartialWords * sizeof(unsigned long long));
    if (int rc = e->slab.alloc(off_chain + 256, "the engine's boards and work memory", true)) {
        delete e;
        return rc;
    }
    e->game_bytes = off_partials;
    e->kept_bytes = off_stats;
    char *base = e->slab.as<char>();
    e->st.boards = reinterpret_cast<uint4 *>(base + off_boards);
    e->st.last_record = reinterpret_cast<uint4 *>(base + off_last_record);
    e->st.ep_counters = reinterpret_cast<unsigned long long *>(base + off_counters);
    e->stats_dev = reinterpret_cast<g2048::StatsOut *>(base + off_stats);
    e->summary_scratch = reinterpret_cast<unsigned long long *>(base + off_summary);
    e->graph_t_dev = reinterpret_cast<unsigned long long *>(base + off_graph_t);
    e->stats_partials = reinterpret_cast<unsigned long long *>(base + off_partials);
    e->chain_flags = reinterpret_cast<unsigned long long *>(base + off_chain);
    if (!e->graph_enabled)
        snprintf(e->graph_off_reason, sizeof e->graph_off_reason, "G2048_ROLLOUT_GRAPH=0 in the environment of g2048_create");
    *out = e;
    return G2048_OK;
}

int g2048_destroy(g2048_engine *e)
{
    if (!e)
        return G2048_OK;
    (void)hipSetDevice(e->device);
    e->side.reset(); // (the last engine of the device ends its side chain)
    bool any_graph = false;
    for (auto &entry : e->graphs)
        any_graph = any_graph || entry.g.exec;
    if (any_graph)
        (void)hipDeviceSynchronize(); // a replay may still be running: an executable graph is destroyed only at rest (freeing
                                      // the slab below waits for the device anyway)
    for (auto &entry : e->graphs)
        g2048::destroy_rollout_graph(entry.g);
    const hipError_t err = e->slab.reset();
    delete e; // (the owners free the rest: after the slab, so with the device at rest)
    if (err != hipSuccess)
        return fail(G2048_ERR_HIP, "hipFree failed: %s", hipGetErrorString(err));
    return G2048_OK;
}

int g2048_seed(g2048_engine *e, uint64_t seed, void *stream)
{
    if (int rc = usable(e))
        return rc;
    e->seed = seed;
    e->t = 0;
    e->fresh = 1;
    // episode statistics restart with the stream: cleared by a kernel ON THE CALLER'S STREAM, so the
    // clear is ordered against step kernels already enqueued there
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_clear_stats(tracked_state(e), static_cast<uint32_t>(e->n), static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_set_last_records(g2048_engine *e, int enable, void *stream)
{
    if (int rc = usable(e))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    if (enable && !e->track_last) // records from before the pause would be stale: start from "none yet"
        G2048_HIP(hipMemsetAsync(e->st.last_record, 0, e->n * 16, static_cast<hipStream_t>(stream)));
    e->track_last = enable ? 1 : 0;
    return G2048_OK;
}

int g2048_get_last_records(const g2048_engine *e)
{
    return e ? e->track_last : 0;
}

int g2048_get_clock(const g2048_engine *e, uint64_t *t)
{
    if (int rc = usable(e))
        return rc;
    if (!t)
        return fail(G2048_ERR_INVALID, "NULL argument");
    *t = e->t;
    return G2048_OK;
}

int g2048_set_clock(g2048_engine *e, uint64_t t)
{
    if (int rc = usable(e))
        return rc;
    e->t = t;
    e->fresh = 0;
    return G2048_OK;
}

uint64_t g2048_num_boards(const g2048_engine *e) { return e ? e->n : 0; }

int g2048_set_illegal_move_reward(g2048_engine *e, float reward)
{
    if (int rc = usable(e))
        return rc;
    e->illegal_reward = reward;
    return G2048_OK;
}

int g2048_set_strict_actions(g2048_engine *e, int enable)
{
    if (int rc = usable(e))
        return rc;
    if (enable) {
        G2048_HIP(hipSetDevice(e->device));
        if (int rc = ensure_words(e))
            return rc;
    }
    e->strict_actions = enable ? 1 : 0;
    return G2048_OK;
}

int g2048_get_strict_actions(const g2048_engine *e) { return e ? e->strict_actions : 0; }

int g2048_set_max_tile(g2048_engine *e, int max_exp)
{
    if (int rc = usable(e))
        return rc;
    if (max_exp < 0 || max_exp > 31)
        return fail(G2048_ERR_INVALID, "max_exp %d out of range 0..31", max_exp);
    e->max_exp = static_cast<uint32_t>(max_exp);
    return G2048_OK;
}

int g2048_reset(g2048_engine *e, int new_transaction, uint32_t first_slot, const uint8_t *mask, void *stream)
{
    if (int rc = usable(e))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    if (new_transaction)
        e->t += 1;
    e->fresh = 0;
    G2048_HIP(g2048::launch_reset(make_args(e, nullptr, 0), first_slot, mask, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_step(g2048_engine *e, const g2048_step_io *io, int auto_reset, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (int rc = check_io(io))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    e->t += 1;
    e->fresh = 0;
    G2048_HIP(g2048::launch_step(make_args(e, io, auto_reset), io->action_dtype, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// The buffers of step j of a rollout: the io pointers advanced by j * stride elements.
static g2048_step_io io_of_step(const g2048_step_io &io, uint32_t j, uint64_t stride)
{
    g2048_step_io s = io;
    const size_t off = static_cast<size_t>(j) * stride;
    if (s.actions) s.actions = static_cast<const char *>(io.actions) + off * action_size(io.action_dtype);
    if (s.reward) s.reward = io.reward + off;
    if (s.terminated) s.terminated = io.terminated + off;
    if (s.illegal) s.illegal = io.illegal + off;
    if (s.highest) s.highest = io.highest + off;
    if (s.terminal_boards) s.terminal_boards = io.terminal_boards + off * 16;
    if (s.obs) s.obs = static_cast<char *>(io.obs) + off * obs_board_bytes(io.obs_dtype);
    if (s.boards_out) s.boards_out = io.boards_out + off * 16;
    return s;
}

// Launch arguments restricted to the boards [first, first + count) of the engine (first is a multiple of 256: whole
// launch blocks and whole episode slots): every per-board pointer advanced by `first`, the global board index with it.
static g2048::StepArgs part_of(g2048::StepArgs a, int action_dtype, uint32_t first, uint32_t count)
{
    a.st.boards += first;
    if (a.st.last_record) a.st.last_record += first;
    a.st.ep_counters += static_cast<size_t>(first / 64u) * g2048::kSlotWords;
    if (a.actions) a.actions = static_cast<const char *>(a.actions) + static_cast<size_t>(first) * action_size(action_dtype);
    if (a.reward) a.reward += first;
    if (a.terminated) a.terminated += first;
    if (a.illegal) a.illegal += first;
    if (a.highest) a.highest += first;
    if (a.terminal_boards) a.terminal_boards += first;
    if (a.boards_out) a.boards_out += first;
    if (a.obs) a.obs = static_cast<char *>(a.obs) + static_cast<size_t>(first) * obs_board_bytes(static_cast<int>(a.obs_dtype));
    a.n = count;
    a.board_offset += first;
    return a;
}

// When do two chains pay?  WARM -- the device's side chain had work within the last ~50 ms -- they cost a fixed ~6 us per
// rollout more than one chain and save ~1.2 us per step at 2^20 boards: HIP-event time of a rollout of k steps, fitted
// over k = 8 .. 128 right behind a 128-step rollout (tools/chain_fixed_cost.py, profiles/r04_v_chain_fixed_cost.txt; two
// boxes): one chain 9.10 us/step + 12.9 us (8.92 + 21.0), two chains 7.91 us/step + 18.6 us (8.07 + 25.0; with HIP events
// instead of the ticket kernels: + 35.3 / + 46.3 us); k = 8 is a tie, k = 16 is 3-8 % faster.  A 20-step two-chain
// rollout after X of idle (tools/chain_gap_probe.py, profiles/r04_ab_chain_gap_probe.txt; one chain: 188-209 us):
// X = 0.2 ms 175 us, 5 ms 184 (the launch thread asleep by then: waking it costs ~10 us), 50 ms 186, 300 ms 223 -- COLD,
// the side stream's first kernels start late.  Hence: warm, two chains from kTwoChainMinSteps; cold, only from
// kTwoChainColdMinSteps, where 40 us are a few per cent.
constexpr uint32_t kTwoChainMinSteps = 12, kTwoChainColdMinSteps = 64;
// Cached-graph replay of a launch train (g2048_kernels.hip "a k-step launch train as a CACHED hipGraph"): up to 2^17 boards
// -- where one host thread cannot issue launches as fast as the device retires them -- and from 8 steps.
constexpr uint32_t kGraphMinSteps = 8; // (the size limit is g2048_engine::graph_max_boards)
constexpr double kSideWarmWindowUs = 50000.0; // after the estimated end of the side chain's last work

static int ensure_side_chain(g2048_engine *e)
{
    if (e->side)
        return G2048_OK;
    if (e->device < 0 || e->device >= 64)
        return fail(G2048_ERR_INVALID, "two chains are available on devices 0..63");
    if (int rc = ensure_words(e)) // (a ticket wait that runs out reports to kChainErrWord)
        return rc;
    std::lock_guard<std::mutex> lock(g_side_mutex);
    std::shared_ptr<SideChain> sc = g_side[e->device].lock();
    if (!sc) {
        // (a failure below returns with `sc` the only owner: ~SideChain undoes whatever was set up)
        try {
            sc = std::make_shared<SideChain>();
        } catch (const std::bad_alloc &) {
            return fail(G2048_ERR_NOMEM, "out of host memory");
        }
        sc->device = e->device;
        // The side stream is created at the HIGHEST priority the device offers.  In a process that also holds an RCCL
        // communicator (dozens of hardware queues) a normal-priority side queue shares its slot by time slices and the
        // two chains stop overlapping: 10.9-11.1 us per step instead of 8.0 at 2^20 boards, worse than one chain (9.1);
        // with the priority it is 8.0 with or without RCCL (bench.py, forced one-rank process group, K = 400).
        int least = 0, greatest = 0;
        hipError_t err = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (err == hipSuccess)
            err = hipStreamCreateWithPriority(&sc->stream, hipStreamNonBlocking, greatest);
        if (err != hipSuccess)
            return fail(G2048_ERR_HIP, "cannot create the side stream: %s", hipGetErrorString(err));
        sc->priority = greatest;
        SideLauncher *w = &sc->launcher;
        w->spin_us = g2048::side_spin_us_from_env(); // 200 us unless the caller opted into a longer window
        w->start();
        // prime it: a thread's first HIP calls set up per-thread runtime state (tens of microseconds) -- here, not in
        // somebody's first two-chain rollout
        unsigned long long *scratch_flag = e->chain_flags + 24; // (fork = 0 and join = 16 leave words 17..31 of the 256 bytes free)
        const int dev = e->device;
        hipStream_t side_stream = sc->stream;
        const uint64_t ticket = w->post([dev, scratch_flag, side_stream]() -> int {
            if (hipSetDevice(dev) != hipSuccess)
                return G2048_ERR_HIP;
            for (int k = 0; k < 4; ++k)
                (void)g2048::launch_flag_set(scratch_flag, 0ull, side_stream);
            return hipStreamSynchronize(side_stream) == hipSuccess ? G2048_OK : G2048_ERR_HIP;
        });
        if (w->wait(ticket) != G2048_OK)
            return fail(G2048_ERR_HIP, "the side launch thread could not reach device %d", e->device);
        g_side[e->device] = sc;
    }
    e->side = std::move(sc);
    return G2048_OK;
}

int g2048_set_chains(g2048_engine *e, int chains)
{
    if (int rc = usable(e))
        return rc;
    if (chains != 1 && chains != 2)
        return fail(G2048_ERR_INVALID, "chains must be 1 or 2 (got %d)", chains);
    if (chains == 2) {
        G2048_HIP(hipSetDevice(e->device));
        if (int rc = ensure_side_chain(e))
            return rc;
        // The knobs of this form are read HERE, once (not per rollout): a test or a measurement sets the environment and
        // calls g2048_set_chains(e, 2) again.
        const char *v = std::getenv("G2048_TWO_CHAIN_MIN_STEPS");
        const long forced = v ? std::atol(v) : 0l;
        e->chain_min_steps = forced >= 2 ? static_cast<uint32_t>(forced) : 0u;
        v = std::getenv("G2048_FLAG_WAIT_POLLS");
        const long polls = v ? std::atol(v) : 0l;
        e->chain_wait_polls = polls > 0 && polls < 0x7fffffffl ? static_cast<uint32_t>(polls) : g2048::kFlagWaitPolls;
    }
    e->chains = chains;
    return G2048_OK;
}

uint64_t g2048_get_graph_replays(const g2048_engine *e) { return e ? e->graph_replays : 0; }
const char *g2048_graph_status(const g2048_engine *e) { return e ? e->graph_off_reason : "engine is NULL"; }

int g2048_get_chains(const g2048_engine *e) { return e ? e->chains : 0; }
int g2048_get_chains_used(const g2048_engine *e) { return e ? e->last_rollout_chains : 0; }

// The one test of whether a rollout may be replayed from a cached graph: the form is on, the batch is small enough
// (graph_max_boards), the train long enough and its configuration one that step_graph_kernel supports.  When it may,
// *a0 is the launch arguments of step 0 (their clock is not used: a graph reads it through graph_t_dev) and *key is what
// the graph's frozen kernel arguments depend on.
static bool graph_key_for(const g2048_engine *e, uint32_t k_steps, const g2048_step_io *io, uint64_t stride, int auto_reset,
                          g2048::StepArgs *a0, g2048_engine::GraphKey *key)
{
    if (!e->graph_enabled || e->n > e->graph_max_boards || k_steps < kGraphMinSteps)
        return false;
    *a0 = make_args(e, io, auto_reset);
    if (!g2048::rollout_graph_supported(*a0))
        return false;
    key->k_steps = k_steps; key->stride = stride; key->seed = e->seed; key->board_offset = e->board_offset;
    key->actions = io->actions; key->reward = io->reward; key->terminated = io->terminated; key->last_record = a0->st.last_record;
    key->action_dtype = io->action_dtype; key->auto_reset = auto_reset ? 1 : 0; key->illegal_reward = e->illegal_reward;
    return true;
}

static g2048_engine::GraphEntry *find_graph(g2048_engine *e, const g2048_engine::GraphKey &key)
{
    for (auto &entry : e->graphs)
        if (entry.g.exec && entry.key == key)
            return &entry;
    return nullptr;
}

// Build the cached graph for `key` in the next slot (round robin).  A failure is not fatal: the engine keeps launching by
// stream, and stops trying.
// Builds (or rebuilds) a cached graph.  Nothing here is a stream operation -- no allocation, no memset, no synchronisation
// (the clock word lives in the engine's slab) -- so it is safe while the application has a stream capture open, in any
// capture mode.  An entry is evicted only when the stream it was last replayed on has drained (hipStreamQuery); otherwise
// this rollout simply is not cached (returns NULL, the form stays on).
static g2048_engine::GraphEntry *build_graph(g2048_engine *e, const g2048_engine::GraphKey &key, const g2048::StepArgs &a0,
                                             int action_dtype, uint32_t k_steps, uint64_t stride)
{
    g2048_engine::GraphEntry *slot = &e->graphs[e->graph_next];
    if (slot->g.exec) { // a fifth set of buffers: rare
        if (hipStreamQuery(slot->last_stream) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr; // its last replay may still be running: keep it, launch this rollout kernel by kernel
        }
    }
    e->graph_next = (e->graph_next + 1) % g2048_engine::kGraphSlots;
    g2048::destroy_rollout_graph(slot->g);
    const hipError_t err = g2048::build_rollout_graph(a0, action_dtype, k_steps, stride, e->graph_t_dev, &slot->g);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        e->graph_enabled = 0;
        snprintf(e->graph_off_reason, sizeof e->graph_off_reason, "building the graph of a %u-step rollout failed: %s", k_steps,
                 hipGetErrorString(err));
        return nullptr;
    }
    slot->key = key;
    slot->last_stream = nullptr;
    return slot;
}

int g2048_rollout_prepare(g2048_engine *e, uint32_t k_steps, const g2048_step_io *io, uint64_t stride, int auto_reset)
{
    if (int rc = usable(e))
        return rc;
    if (int rc = check_io(io))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    g2048::StepArgs a0;
    g2048_engine::GraphKey key; // (a rollout that cannot be replayed is launched kernel by kernel: nothing to prepare)
    if (graph_key_for(e, k_steps, io, stride, auto_reset, &a0, &key) && !find_graph(e, key))
        (void)build_graph(e, key, a0, io->action_dtype, k_steps, stride);
    return G2048_OK;
}

// Is `s` capturing a graph -- or can the runtime not tell (its error is cleared)?  Either way no other thread may launch
// for this rollout and no cached graph is replayed.  (refuse_capture asks the same question but goes on when it cannot
// tell.)
static bool capturing_or_unknown(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return st != hipStreamCaptureStatusNone;
}

// The launch arguments of step j of a rollout whose first step plays transaction t0 + 1 (make_args alone would read
// e->t, which already stands at the end of the rollout).
struct RolloutSteps {
    const g2048_engine *e;
    const g2048_step_io *io;
    uint64_t stride;
    int auto_reset;
    uint64_t t0;
    g2048::StepArgs operator()(uint32_t j) const
    {
        const g2048_step_io sj = io_of_step(*io, j, stride);
        g2048::StepArgs a = make_args(e, &sj, auto_reset);
        const uint64_t t = t0 + 1u + j;
        a.t_lo = static_cast<uint32_t>(t);
        a.t_hi = static_cast<uint32_t>(t >> 32);
        return a;
    }
};

// Two chains: the batch is cut at a block boundary and each half gets its own stream and launch thread.  Spawn-stream
// mode only (the numpy-RNG planes are indexed with the engine's board count), not while the caller captures a graph
// (another thread must not launch during a global capture), and only when both halves are whole blocks of work.  A
// rollout can only be split when ALL its k_steps actions are supplied up front, and the split only pays from
// kTwoChainMinSteps steps: a caller that steps one action at a time (ppo_train.py) never gets here, whatever
// g2048_set_chains said.
static bool use_two_chains(g2048_engine *e, uint32_t k_steps, hipStream_t s)
{
    const uint32_t first_half = (static_cast<uint32_t>(e->n) / 2u) & ~255u;
    if (e->chains != 2 || !e->side || e->st.rng || first_half < 256u || k_steps < 2)
        return false;
    // warm: the side chain had work until recently; need: the rollout length from which the split pays right now
    const bool warm = steady_now_ns() < e->side->busy_until_ns.load(std::memory_order_relaxed);
    const uint32_t need = e->chain_min_steps ? e->chain_min_steps : warm ? kTwoChainMinSteps : kTwoChainColdMinSteps;
    if (k_steps < need) {
        // Too short to split.  A rollout within reach of the threshold still wakes a sleeping launcher, so that a loop of
        // such rollouts finds it spinning when one of them qualifies; short ones (a step at a time) leave it asleep -- an
        // idle core is not spent on a caller that cannot use the second chain.
        if (k_steps >= kTwoChainMinSteps / 2u && e->side->launcher.sleeping.load())
            e->side->launcher.nudge();
        return false;
    }
    if (capturing_or_unknown(s))
        return false;
    // A caller's stream at the side stream's own priority may be given the SAME hardware queue by the runtime, and
    // streams that share one run in submission order: the caller's wait for the join ticket could then sit in front of
    // the side launches it waits for.  Such a stream gets one chain.  (Streams of other priorities have their own
    // queues; one runtime call per rollout.)
    if (s == nullptr)
        return true;
    int prio = 0;
    if (hipStreamGetPriority(s, &prio) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return prio != e->side->priority;
}

// Fork / join by tickets in device memory (flag_set_kernel / flag_wait_kernel): the side stream starts where the caller's
// stream stands, and whatever the caller enqueues next runs after both halves.
static int rollout_two_chains(g2048_engine *e, uint32_t k_steps, const RolloutSteps &args_of, hipStream_t s)
{
    const int dtype = args_of.io->action_dtype;
    const uint32_t n = static_cast<uint32_t>(e->n);
    const uint32_t first_half = (n / 2u) & ~255u;
    SideChain *sc = e->side.get();
    std::lock_guard<std::mutex> side_in_use(sc->use); // (another engine of this device may be using the side chain)
    hipStream_t side_stream = sc->stream;
    const unsigned long long seq = ++e->chain_seq;
    unsigned long long *fork_flag = e->chain_flags, *join_flag = e->chain_flags + 16;
    unsigned long long *err_word = dev_word(e, kChainErrWord);
    const uint32_t polls = e->chain_wait_polls;
    {   // nothing has been launched yet: a failure here leaves the engine as it was
        const hipError_t err = g2048::launch_flag_set(fork_flag, seq, s); // enqueued BEFORE the side thread can enqueue its wait
        if (err != hipSuccess) {
            e->t = args_of.t0;
            return fail(G2048_ERR_HIP, "cannot fork the two chains: %s", hipGetErrorString(err));
        }
    }
    SideLauncher *w = &sc->launcher;
    // The caller's chain gets a HEAD START of one launch (~3.3 us of host time, about half a half-batch kernel): two
    // chains that start together run their load phases together, like one big kernel.
    hipError_t mine = g2048::launch_step(part_of(args_of(0), dtype, 0u, first_half), dtype, s);
    const uint64_t ticket = w->post([e, w, args_of, k_steps, dtype, first_half, n, fork_flag, join_flag, seq, side_stream, err_word,
                                     polls]() -> int {
        if (hipSetDevice(e->device) != hipSuccess) {
            snprintf(w->error, sizeof w->error, "the side launch thread could not select device %d", e->device);
            return G2048_ERR_HIP;
        }
        hipError_t err = g2048::launch_flag_wait(fork_flag, seq, err_word, polls, side_stream);
        for (uint32_t j = 0; j < k_steps && err == hipSuccess; ++j)
            err = g2048::launch_step(part_of(args_of(j), dtype, first_half, n - first_half), dtype, side_stream);
        // the join ticket goes out even after a failed launch: the caller's stream must never wait for a ticket nobody sets
        const hipError_t tail = g2048::launch_flag_set(join_flag, seq, side_stream);
        if (err == hipSuccess)
            err = tail;
        if (err != hipSuccess) {
            snprintf(w->error, sizeof w->error, "launch on the side chain failed: %s", hipGetErrorString(err));
            return G2048_ERR_HIP;
        }
        return G2048_OK;
    });
    for (uint32_t j = 1; j < k_steps && mine == hipSuccess; ++j)
        mine = g2048::launch_step(part_of(args_of(j), dtype, 0u, first_half), dtype, s);
    const int theirs = w->wait(ticket); // (the side thread has ISSUED its launches; nothing waits for the device here)
    // The JOIN is enqueued whatever happened above: side-stream kernels that were launched may still be writing the
    // engine's and the caller's buffers, and whatever the caller enqueues next on `stream` must come after them.
    const hipError_t join = g2048::launch_flag_wait(join_flag, seq, err_word, polls, s);
    // the side stream has ~k_steps half-batch kernels ahead of it (they are only enqueued): warm until they are done + a bit
    sc->busy_until_ns.store(steady_now_ns() + static_cast<int64_t>((k_steps * (4.0e-6 * n + 0.5) + kSideWarmWindowUs) * 1000.0),
                            std::memory_order_relaxed);
    if (theirs != G2048_OK || mine != hipSuccess || join != hipSuccess) {
        // some launches of the rollout are enqueued and some are not: the halves of the batch no longer stand at the same
        // step, and nothing the caller could do would repair that
        char what[256];
        if (theirs != G2048_OK)
            snprintf(what, sizeof what, "two-chain rollout: %s", w->error);
        else
            snprintf(what, sizeof what, "two-chain rollout: %s failed: %s", mine != hipSuccess ? "a launch on the caller's stream" : "the join",
                     hipGetErrorString(mine != hipSuccess ? mine : join));
        return poison(e, what);
    }
    return G2048_OK;
}

// Same buffers as last time (or a prepared plan): replay the cached graph of this launch train.  Returns whether it
// served the rollout; when it did not, nothing of it has been enqueued.
static bool rollout_from_graph(g2048_engine *e, uint32_t k_steps, const RolloutSteps &args_of, hipStream_t s)
{
    g2048::StepArgs a0;
    g2048_engine::GraphKey key;
    if (!graph_key_for(e, k_steps, args_of.io, args_of.stride, args_of.auto_reset, &a0, &key))
        return false;
    const bool capturing = capturing_or_unknown(s);
    g2048_engine::GraphEntry *have = capturing ? nullptr : find_graph(e, key);
    if (!capturing && !have && key == e->graph_seen) // the second rollout over these buffers in a row: worth a graph
        have = build_graph(e, key, a0, args_of.io->action_dtype, k_steps, args_of.stride);
    e->graph_seen = key;
    if (!have)
        return false;
    const hipError_t err = g2048::launch_rollout_graph(have->g, args_of.t0 + 1u, s);
    if (err == hipSuccess) {
        have->last_stream = s;
        ++e->graph_replays;
        return true;
    }
    // no step was enqueued (the launch of a graph is all or nothing; at most the one-lane clock write went out, which
    // nobody else reads): the caller falls through to stream launches
    (void)hipGetLastError();
    g2048::destroy_rollout_graph(have->g);
    e->graph_enabled = 0;
    snprintf(e->graph_off_reason, sizeof e->graph_off_reason, "hipGraphLaunch of a cached %u-step rollout failed: %s", k_steps,
             hipGetErrorString(err));
    return false;
}

// One chain of k stream launches on the caller's stream.
static int rollout_launch_train(g2048_engine *e, uint32_t k_steps, const RolloutSteps &args_of, hipStream_t s)
{
    for (uint32_t j = 0; j < k_steps; ++j) {
        const hipError_t err = g2048::launch_step(args_of(j), args_of.io->action_dtype, s);
        if (err != hipSuccess) {
            // steps 0 .. j-1 are enqueued and will run: the clock says so, and the caller gets the error
            e->t = args_of.t0 + j;
            return fail(G2048_ERR_HIP, "launch of step %u of %u failed: %s", j, k_steps, hipGetErrorString(err));
        }
    }
    return G2048_OK;
}

int g2048_rollout(g2048_engine *e, uint32_t k_steps, const g2048_step_io *io, uint64_t stride, int auto_reset,
                  void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (int rc = check_io(io))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (k_steps == 0)
        return G2048_OK;
    const bool two = use_two_chains(e, k_steps, s);
    e->last_rollout_chains = two ? 2 : 1;
    const RolloutSteps args_of{e, io, stride, auto_reset, e->t};
    e->t += k_steps;
    e->fresh = 0;
    if (two)
        return rollout_two_chains(e, k_steps, args_of, s);
    if (rollout_from_graph(e, k_steps, args_of, s))
        return G2048_OK;
    return rollout_launch_train(e, k_steps, args_of, s);
}

int g2048_rollout_fused(g2048_engine *e, uint32_t k_steps, const g2048_step_io *io, uint64_t stride, int auto_reset,
                        void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (int rc = check_io(io))
        return rc;
    if (io->terminal_boards || io->obs || io->boards_out)
        return fail(G2048_ERR_INVALID, "g2048_rollout_fused writes neither terminal_boards, boards_out nor obs");
    if (k_steps == 0)
        return G2048_OK;
    G2048_HIP(hipSetDevice(e->device));
    e->t += 1; // transaction of the first fused step
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, io, auto_reset);
    a.k_steps = k_steps;
    G2048_HIP(g2048::launch_rollout_fused(a, io->action_dtype, stride, static_cast<hipStream_t>(stream)));
    e->t += k_steps - 1;
    return G2048_OK;
}

int g2048_rollout_random(g2048_engine *e, uint32_t k_steps, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (k_steps == 0)
        return G2048_OK;
    G2048_HIP(hipSetDevice(e->device));
    e->t += 1; // transaction of the first fused step
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, nullptr, 1);
    a.k_steps = k_steps;
    G2048_HIP(g2048::launch_rollout_random(a, static_cast<hipStream_t>(stream)));
    e->t += k_steps - 1;
    return G2048_OK;
}

int g2048_move(g2048_engine *e, const void *actions, int32_t action_dtype, int trial, int32_t *score_out,
               uint8_t *legal_out, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!actions)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (action_dtype < G2048_ACT_U8 || action_dtype > G2048_ACT_I64)
        return fail(G2048_ERR_INVALID, "g2048_move needs an action buffer (dtype %d)", action_dtype);
    if ((reinterpret_cast<uintptr_t>(actions) & (action_size(action_dtype) - 1)) || (reinterpret_cast<uintptr_t>(score_out) & 3u))
        return fail(G2048_ERR_INVALID, "misaligned buffer: actions need their element size, score_out 4 bytes");
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_move(e->st.boards, static_cast<uint32_t>(e->n), actions, action_dtype, trial != 0,
                                 score_out, legal_out, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_query(const g2048_engine *e, uint8_t *isend_out, uint8_t *highest_out, void *stream)
{
    if (int rc = usable(e))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_query(e->st.boards, static_cast<uint32_t>(e->n), e->max_exp, isend_out, highest_out,
                                  static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_legal_actions(const g2048_engine *e, uint8_t *mask_out, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!mask_out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_legal_mask(e->st.boards, static_cast<uint32_t>(e->n), mask_out, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

} // extern "C"

// A plain board array: n rows of 16 exponents
static int plain_boards(const uint8_t *boards, uint64_t n)
{
    if (!boards)
        return fail(G2048_ERR_INVALID, "boards is NULL");
    if (reinterpret_cast<uintptr_t>(boards) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: boards need 16 bytes");
    if (n == 0 || n > 0xffffff00ull) // (32-bit board indices, whole 256-lane blocks: the cap of g2048_create)
        return fail(G2048_ERR_INVALID, "n=%llu: need 1 <= n <= 2^32 - 256", (unsigned long long)n);
    return G2048_OK;
}

// Where a read-only call finds its boards.  Every such operation below is written once and entered twice, with an engine's
// records and with the caller's plain array: `rc` is the opening check of that form, and the body returns it before it
// looks at anything else.
struct Source {
    int rc;
    g2048::Boards boards;
    int device;            // the engine's, set before the launch; -1: a plain array is launched on the current device
    uint64_t index_offset; // global index of board 0 (g2048_mc_search): the engine's board_offset or the caller's
};

static Source from_engine(const g2048_engine *e)
{
    if (int rc = usable(e))
        return Source{rc, {}, -1, 0};
    return Source{G2048_OK, {e->st.boards, static_cast<uint32_t>(e->n), false}, e->device, e->board_offset};
}

static Source from_plain(const uint8_t *boards, uint64_t n, uint64_t index_offset = 0)
{
    if (int rc = plain_boards(boards, n))
        return Source{rc, {}, -1, 0};
    return Source{G2048_OK, {reinterpret_cast<const uint4 *>(boards), static_cast<uint32_t>(n), true}, -1, index_offset};
}

// after all validation, before the launch
static int select_device(const Source &src)
{
    if (src.device >= 0)
        G2048_HIP(hipSetDevice(src.device));
    return G2048_OK;
}

// g2048_afterstate_io -> the kernel's outputs, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int afterstate_out(const g2048_afterstate_io *io, g2048::AfterstateOut *o)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (!io->boards && !io->score && !io->legal && !io->obs)
        return fail(G2048_ERR_INVALID, "g2048_afterstate_io requests no output (boards, score, legal and obs are all NULL)");
    if ((reinterpret_cast<uintptr_t>(io->boards) | reinterpret_cast<uintptr_t>(io->score) | reinterpret_cast<uintptr_t>(io->obs)) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: afterstate boards, score and obs need 16 bytes");
    if (io->obs && (io->obs_dtype < G2048_OBS_U8 || io->obs_dtype > G2048_OBS_F32))
        return fail(G2048_ERR_INVALID, "unknown obs_dtype %d", io->obs_dtype);
    *o = g2048::AfterstateOut{reinterpret_cast<uint4 *>(io->boards), reinterpret_cast<uint4 *>(io->score), io->legal, io->obs,
                              io->obs ? static_cast<uint32_t>(io->obs_dtype) : 0u};
    return G2048_OK;
}

static int afterstates(const Source &src, const g2048_afterstate_io *io, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::AfterstateOut o;
    if (int rc = afterstate_out(io, &o))
        return rc;
    if (int rc = select_device(src))
        return rc;
    G2048_HIP(g2048::launch_afterstates(src.boards, o, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

extern "C" {

int g2048_afterstates(const g2048_engine *e, const g2048_afterstate_io *io, void *stream)
{
    return afterstates(from_engine(e), io, stream);
}

int g2048_afterstates_plain(const uint8_t *boards, uint64_t n, const g2048_afterstate_io *io, void *stream)
{
    return afterstates(from_plain(boards, n), io, stream);
}

} // extern "C"

// g2048_search_io -> the kernel's arguments, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int search_args(const g2048_search_io *io, g2048::SearchArgs *a)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (!io->action && !io->value)
        return fail(G2048_ERR_INVALID, "g2048_search_io requests no output (action and value are both NULL)");
    if (reinterpret_cast<uintptr_t>(io->value) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: search value needs 16 bytes");
    if (io->depth < 1 || io->depth > G2048_SEARCH_MAX_DEPTH)
        return fail(G2048_ERR_INVALID, "depth=%u: need 1 <= depth <= %d", io->depth, G2048_SEARCH_MAX_DEPTH);
    if (io->base < 0 || io->base > (1 << 24))
        return fail(G2048_ERR_INVALID, "base=%d: need 0 <= base <= 2^24", io->base);
    const int32_t w[3] = {io->w_empty, io->w_merge, io->w_mono};
    const char *names[3] = {"w_empty", "w_merge", "w_mono"};
    for (int k = 0; k < 3; ++k)
        if (w[k] < 0 || w[k] > 65535)
            return fail(G2048_ERR_INVALID, "%s=%d: need 0 <= %s <= 65535", names[k], w[k], names[k]);
    *a = g2048::SearchArgs{static_cast<uint32_t>(io->base), static_cast<uint32_t>(io->w_empty), static_cast<uint32_t>(io->w_merge),
                           static_cast<uint32_t>(io->w_mono), io->action, io->value};
    return G2048_OK;
}

static int expectimax(const Source &src, const g2048_search_io *io, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::SearchArgs a;
    if (int rc = search_args(io, &a))
        return rc;
    if (int rc = select_device(src))
        return rc;
    G2048_HIP(g2048::launch_expectimax(src.boards, io->depth, a, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

extern "C" {

int g2048_expectimax(const g2048_engine *e, const g2048_search_io *io, void *stream)
{
    return expectimax(from_engine(e), io, stream);
}

int g2048_expectimax_plain(const uint8_t *boards, uint64_t n, const g2048_search_io *io, void *stream)
{
    return expectimax(from_plain(boards, n), io, stream);
}

} // extern "C"

// g2048_mc_io -> the kernel's arguments, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int mc_args(const g2048_mc_io *io, uint64_t n, uint64_t index_offset, g2048::McArgs *a)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (!io->action && !io->value && !io->steps)
        return fail(G2048_ERR_INVALID, "g2048_mc_io requests no output (action, value and steps are all NULL)");
    if (reinterpret_cast<uintptr_t>(io->value) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: mc value needs 16 bytes");
    if (reinterpret_cast<uintptr_t>(io->steps) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: mc steps needs 16 bytes");
    if (io->rollouts < 1 || io->rollouts > G2048_MC_MAX_ROLLOUTS)
        return fail(G2048_ERR_INVALID, "rollouts=%u: need 1 <= rollouts <= %d", io->rollouts, G2048_MC_MAX_ROLLOUTS);
    if (io->max_steps < 1 || io->max_steps > G2048_MC_MAX_STEPS)
        return fail(G2048_ERR_INVALID, "max_steps=%u: need 1 <= max_steps <= %d", io->max_steps, G2048_MC_MAX_STEPS);
    if (index_offset + n > 0x100000000ull)
        return fail(G2048_ERR_INVALID, "index_offset=%llu n=%llu: global board indices must fit 32 bits",
                    (unsigned long long)index_offset, (unsigned long long)n);
    *a = g2048::McArgs{io->rollouts, io->max_steps, static_cast<uint32_t>(io->seed), static_cast<uint32_t>(io->seed >> 32),
                       static_cast<uint32_t>(index_offset), io->action, io->value, io->steps};
    return G2048_OK;
}

static int mc_search(const Source &src, const g2048_mc_io *io, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::McArgs a;
    if (int rc = mc_args(io, src.boards.n, src.index_offset, &a))
        return rc;
    if (int rc = select_device(src))
        return rc;
    G2048_HIP(g2048::launch_mc_search(src.boards, a, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

extern "C" {

int g2048_mc_search(const g2048_engine *e, const g2048_mc_io *io, void *stream)
{
    return mc_search(from_engine(e), io, stream);
}

int g2048_mc_search_plain(const uint8_t *boards, uint64_t n, uint32_t index_offset, const g2048_mc_io *io, void *stream)
{
    return mc_search(from_plain(boards, n, index_offset), io, stream);
}

} // extern "C"

// g2048_ntuple_net -> the launchers' network, or G2048_ERR_INVALID (before any HIP call: works without a device).
// need_weights = false for the one call that reads no table (g2048_ntuple_stage_plain).
static int ntuple_net(const g2048_ntuple_net *net, g2048::NtupleNet *out, bool need_weights = true)
{
    if (!net)
        return fail(G2048_ERR_INVALID, "net is NULL");
    if (net->n_tuples < 1 || net->n_tuples > G2048_NTUPLE_MAX_TUPLES)
        return fail(G2048_ERR_INVALID, "n_tuples=%u: need 1 <= n_tuples <= %d", net->n_tuples, G2048_NTUPLE_MAX_TUPLES);
    if (net->tuple_len < 1 || net->tuple_len > G2048_NTUPLE_MAX_LEN)
        return fail(G2048_ERR_INVALID, "tuple_len=%u: need 1 <= tuple_len <= %d", net->tuple_len, G2048_NTUPLE_MAX_LEN);
    if (net->frac_bits > G2048_NTUPLE_MAX_FRAC_BITS)
        return fail(G2048_ERR_INVALID, "frac_bits=%u: need 0 <= frac_bits <= %d", net->frac_bits, G2048_NTUPLE_MAX_FRAC_BITS);
    for (uint32_t t = 0; t < net->n_tuples; ++t) {
        uint32_t seen = 0;
        bool ended = false; // a G2048_NTUPLE_END at some k' < k: tuple t is shorter than tuple_len (a mixed network)
        for (uint32_t k = 0; k < net->tuple_len; ++k) {
            const uint32_t c = net->cells[t][k];
            if (c == G2048_NTUPLE_END) {
                if (k == 0)
                    return fail(G2048_ERR_INVALID, "cells[%u][0]=G2048_NTUPLE_END: tuple %u is empty, a tuple needs at least one cell", t, t);
                ended = true;
                continue;
            }
            if (ended)
                return fail(G2048_ERR_INVALID, "cells[%u][%u]=%u: a cell after G2048_NTUPLE_END in tuple %u (only G2048_NTUPLE_END may follow it)",
                            t, k, c, t);
            if (c > 15)
                return fail(G2048_ERR_INVALID, "cells[%u][%u]=%u: a cell index is 0..15", t, k, c);
            if (seen >> c & 1u)
                return fail(G2048_ERR_INVALID, "cells[%u][%u]=%u: cell repeated within tuple %u", t, k, c, t);
            seen |= 1u << c;
        }
    }
    if (need_weights && !net->weights)
        return fail(G2048_ERR_INVALID, "net weights is NULL");
    if (need_weights && reinterpret_cast<uintptr_t>(net->weights) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple weights need 16 bytes");
    *out = g2048::NtupleNet{};
    out->n_tuples = net->n_tuples;
    out->tuple_len = net->tuple_len;
    out->frac_bits = net->frac_bits;
    memcpy(out->cells, net->cells, sizeof(out->cells));
    out->weights = net->weights;
    return G2048_OK;
}

// the first n_stages - 1 thresholds of a staged network or a carousel: non-zero and strictly ascending
static int stage_thresholds(uint32_t n_stages, const uint16_t *thresholds)
{
    for (uint32_t j = 0; j + 1 < n_stages; ++j) {
        if (thresholds[j] == 0)
            return fail(G2048_ERR_INVALID, "thresholds[%u]=0: a stage threshold is 1..65535", j);
        if (j > 0 && thresholds[j] <= thresholds[j - 1])
            return fail(G2048_ERR_INVALID, "thresholds[%u]=%u: thresholds must be strictly ascending (thresholds[%u]=%u)", j,
                        thresholds[j], j - 1, thresholds[j - 1]);
    }
    return G2048_OK;
}

// g2048_ntuple_staged_net -> the same network with its stages: every ntuple entry point below is written once, for either
// descriptor, and reaches the same launchers and kernels (S = 1 is the unstaged network).
static int ntuple_net(const g2048_ntuple_staged_net *net, g2048::NtupleNet *out, bool need_weights = true)
{
    if (!net)
        return fail(G2048_ERR_INVALID, "net is NULL");
    if (net->n_stages < 1 || net->n_stages > G2048_NTUPLE_MAX_STAGES)
        return fail(G2048_ERR_INVALID, "n_stages=%u: need 1 <= n_stages <= %d", net->n_stages, G2048_NTUPLE_MAX_STAGES);
    if (int rc = stage_thresholds(net->n_stages, net->thresholds))
        return rc;
    if (int rc = ntuple_net(&net->net, out, need_weights))
        return rc;
    out->n_stages = net->n_stages;
    for (uint32_t j = 0; j + 1 < net->n_stages; ++j)
        out->thresholds[j] = net->thresholds[j];
    return G2048_OK;
}

static int ntuple_out(const g2048_ntuple_io *io, g2048::NtupleOut *o)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (!io->value && !io->action && !io->best && !io->after && !io->after_value)
        return fail(G2048_ERR_INVALID, "g2048_ntuple_io requests no output (value, action, best, after and after_value are all NULL)");
    if (reinterpret_cast<uintptr_t>(io->value) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple value needs 16 bytes");
    if (reinterpret_cast<uintptr_t>(io->after) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple after needs 16 bytes");
    if ((reinterpret_cast<uintptr_t>(io->best) | reinterpret_cast<uintptr_t>(io->after_value)) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple best and after_value need 8 bytes");
    *o = g2048::NtupleOut{io->value, io->action, io->best, reinterpret_cast<uint4 *>(io->after), io->after_value};
    return G2048_OK;
}

// g2048_ntuple_search_io -> the kernel's outputs, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int ntuple_search_out(const g2048_ntuple_search_io *io, g2048::NtupleSearchOut *o)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (!io->action && !io->value)
        return fail(G2048_ERR_INVALID, "g2048_ntuple_search_io requests no output (action and value are both NULL)");
    if (reinterpret_cast<uintptr_t>(io->value) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple search value needs 16 bytes");
    if (io->depth < 1 || io->depth > G2048_NTUPLE_SEARCH_MAX_DEPTH)
        return fail(G2048_ERR_INVALID, "depth=%u: need 1 <= depth <= %d", io->depth, G2048_NTUPLE_SEARCH_MAX_DEPTH);
    *o = g2048::NtupleSearchOut{io->action, io->value};
    return G2048_OK;
}

// the board count of a trace call (the cap of plain_boards: 32-bit board indices)
static int trace_boards(uint64_t n)
{
    if (n == 0 || n > 0xffffff00ull)
        return fail(G2048_ERR_INVALID, "n=%llu: need 1 <= n <= 2^32 - 256", (unsigned long long)n);
    return G2048_OK;
}

// g2048_ntuple_trace or g2048_ntuple_delay and a slot -> the launchers' history (g2048::NtupleTrace) or ring
// (g2048::NtupleDelay, which adds acc), or G2048_ERR_INVALID (before any HIP call: works without a device).  The messages
// call the descriptor `name`, the parameter it came in, and its buffers by `noun`.
template <class Desc, class Hist> static int ntuple_history(const Desc *h, const char *name, const char *noun, uint32_t slot, Hist *out)
{
    constexpr bool has_acc = std::is_same<Hist, g2048::NtupleDelay>::value;
    if (!h)
        return fail(G2048_ERR_INVALID, "%s is NULL", name);
    if (!h->hist)
        return fail(G2048_ERR_INVALID, "%s hist is NULL", noun);
    if (!h->len)
        return fail(G2048_ERR_INVALID, "%s len is NULL", noun);
    if constexpr (has_acc)
        if (!h->acc)
            return fail(G2048_ERR_INVALID, "%s acc is NULL", noun);
    if (h->depth < 1 || h->depth > G2048_NTUPLE_TRACE_MAX)
        return fail(G2048_ERR_INVALID, "depth=%u: need 1 <= depth <= %d", h->depth, G2048_NTUPLE_TRACE_MAX);
    if (h->lambda > 65536u)
        return fail(G2048_ERR_INVALID, "lambda=%u: need 0 <= lambda <= 65536 (Q16)", h->lambda);
    if (slot >= h->depth)
        return fail(G2048_ERR_INVALID, "slot=%u: need slot < depth=%u", slot, h->depth);
    if (reinterpret_cast<uintptr_t>(h->hist) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: %s hist needs 16 bytes", noun);
    if constexpr (has_acc)
        if (reinterpret_cast<uintptr_t>(h->acc) & 7u)
            return fail(G2048_ERR_INVALID, "misaligned buffer: %s acc needs 8 bytes", noun);
    static_cast<g2048::NtupleTrace &>(*out) = g2048::NtupleTrace{h->depth, h->lambda, reinterpret_cast<uint4 *>(h->hist), h->len};
    if constexpr (has_acc)
        out->acc = h->acc;
    return G2048_OK;
}

// lr_shift and mode of a delay update
static int ntuple_delay_mode(uint32_t lr_shift, uint32_t mode)
{
    if (lr_shift > G2048_NTUPLE_MAX_LR_SHIFT)
        return fail(G2048_ERR_INVALID, "lr_shift=%u: need 0 <= lr_shift <= %d", lr_shift, G2048_NTUPLE_MAX_LR_SHIFT);
    if (mode > G2048_NTUPLE_DELAY_FLUSH)
        return fail(G2048_ERR_INVALID, "mode=%u: need G2048_NTUPLE_DELAY_STEP (0) or G2048_NTUPLE_DELAY_FLUSH (1)", mode);
    return G2048_OK;
}

// delta and lr_shift of an update, as g2048_ntuple_update_plain checks them
static int ntuple_delta(const int64_t *delta, uint32_t lr_shift)
{
    if (!delta)
        return fail(G2048_ERR_INVALID, "delta is NULL");
    if (reinterpret_cast<uintptr_t>(delta) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple delta needs 8 bytes");
    if (lr_shift > G2048_NTUPLE_MAX_LR_SHIFT)
        return fail(G2048_ERR_INVALID, "lr_shift=%u: need 0 <= lr_shift <= %d", lr_shift, G2048_NTUPLE_MAX_LR_SHIFT);
    return G2048_OK;
}

// phases and the accumulators as a TC entry point got them.  The update bodies below take a pointer to one: NULL from the
// TD entry points, whose update it is then.
struct TcArgs {
    uint32_t phases;
    const g2048_ntuple_tc *tc;
};

// -> the launchers' accumulators; nothing to check, and *out is left alone, for the TD update
static int ntuple_tc(const TcArgs *in, g2048::NtupleTc *out)
{
    if (!in)
        return G2048_OK;
    if (in->phases < 1 || in->phases > (G2048_NTUPLE_TC_WEIGHTS | G2048_NTUPLE_TC_ACCUM))
        return fail(G2048_ERR_INVALID, "phases=%u: need G2048_NTUPLE_TC_WEIGHTS (1), G2048_NTUPLE_TC_ACCUM (2) or both (3)", in->phases);
    if (!in->tc)
        return fail(G2048_ERR_INVALID, "tc is NULL");
    if (!in->tc->err)
        return fail(G2048_ERR_INVALID, "tc err is NULL");
    if (!in->tc->mag)
        return fail(G2048_ERR_INVALID, "tc mag is NULL");
    if ((reinterpret_cast<uintptr_t>(in->tc->err) | reinterpret_cast<uintptr_t>(in->tc->mag)) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple tc err and mag need 8 bytes");
    *out = g2048::NtupleTc{in->phases, in->tc->err, in->tc->mag};
    return G2048_OK;
}

// phases and the state as a batch-mean entry point got them; NULL from every other entry point
struct MeanArgs {
    uint32_t phases;
    const g2048_ntuple_mean *mean;
};

// -> the launchers' state, for a call of `items` = H * n work items; nothing to check, and *out is left alone, for the other
// updates
static int ntuple_mean(const MeanArgs *in, uint64_t items, g2048::NtupleMean *out)
{
    if (!in)
        return G2048_OK;
    if (in->phases < 1 || in->phases > (G2048_NTUPLE_MEAN_SUM | G2048_NTUPLE_MEAN_APPLY))
        return fail(G2048_ERR_INVALID, "phases=%u: need G2048_NTUPLE_MEAN_SUM (1), G2048_NTUPLE_MEAN_APPLY (2) or both (3)", in->phases);
    if (!in->mean)
        return fail(G2048_ERR_INVALID, "mean is NULL");
    if (!in->mean->sum)
        return fail(G2048_ERR_INVALID, "mean sum is NULL");
    if (!in->mean->count)
        return fail(G2048_ERR_INVALID, "mean count is NULL");
    if (reinterpret_cast<uintptr_t>(in->mean->sum) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple mean sum needs 8 bytes");
    if (reinterpret_cast<uintptr_t>(in->mean->count) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple mean count needs 4 bytes");
    if (items >= (1ull << 29)) // 8 reaches of one entry per item: count stays below 2^32
        return fail(G2048_ERR_INVALID, "items=%llu: a batch-mean update needs H * n < 2^29", (unsigned long long)items);
    *out = g2048::NtupleMean{in->phases, in->mean->sum, in->mean->count};
    return G2048_OK;
}

// The entry points that take a network, once each for Net = g2048_ntuple_net and g2048_ntuple_staged_net (the extern "C"
// wrappers below): only ntuple_net() differs.
template <class Net> static int ntuple_evaluate(const Source &src, const Net *net, const g2048_ntuple_io *io, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleOut o;
    if (int rc = ntuple_out(io, &o))
        return rc;
    if (int rc = select_device(src))
        return rc;
    G2048_HIP(g2048::launch_ntuple_eval(src.boards, nn, o, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// g2048_ntuple_play_io -> the kernel's side outputs, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int ntuple_play_out(const g2048_ntuple_play_io *io, g2048::NtuplePlayOut *o)
{
    *o = g2048::NtuplePlayOut{};
    if (!io)
        return G2048_OK;
    if (reinterpret_cast<uintptr_t>(io->games_left) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple play games_left needs 4 bytes");
    if ((reinterpret_cast<uintptr_t>(io->hist) | reinterpret_cast<uintptr_t>(io->moves)) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple play hist and moves need 8 bytes");
    *o = g2048::NtuplePlayOut{io->games_left, reinterpret_cast<unsigned long long *>(io->hist),
                              reinterpret_cast<unsigned long long *>(io->moves)};
    return G2048_OK;
}

// The clock as in g2048_rollout_random: k_steps transactions, whatever the boards' budgets.
template <class Net> static int ntuple_play(g2048_engine *e, const Net *net, uint32_t k_steps, const g2048_ntuple_play_io *io, void *stream)
{
    if (int rc = usable(e))
        return rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtuplePlayOut o;
    if (int rc = ntuple_play_out(io, &o))
        return rc;
    if (e->st.rng)
        return fail(G2048_ERR_INVALID, "g2048_ntuple_play needs the spawn stream: this engine is in numpy-RNG mode, whose fused "
                                       "form is not offered (play it with g2048_ntuple_evaluate and g2048_step)");
    if (k_steps == 0)
        return G2048_OK;
    G2048_HIP(hipSetDevice(e->device));
    e->t += 1; // transaction of the first fused step
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, nullptr, 1);
    a.k_steps = k_steps;
    G2048_HIP(g2048::launch_ntuple_play(a, nn, o, static_cast<hipStream_t>(stream)));
    e->t += k_steps - 1;
    return G2048_OK;
}

// g2048_downgrade -> the kernels' rule, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int downgrade_rule(const g2048_downgrade *rule, g2048::DowngradeArgs *out)
{
    if (!rule)
        return fail(G2048_ERR_INVALID, "rule is NULL");
    if (rule->min_exp < 1u || rule->min_exp > 31u)
        return fail(G2048_ERR_INVALID, "downgrade min_exp=%u: need 1..31", rule->min_exp);
    if (rule->floor_exp < G2048_DOWNGRADE_MIN_FLOOR || rule->floor_exp > 31u)
        return fail(G2048_ERR_INVALID, "downgrade floor_exp=%u: need %d..31", rule->floor_exp, G2048_DOWNGRADE_MIN_FLOOR);
    *out = g2048::DowngradeArgs{rule->min_exp, rule->floor_exp};
    return G2048_OK;
}

// g2048_ntuple_play with every move chosen on the translated board: the same checks, clock and bookkeeping.  The engine is
// looked at after everything that can be refused without it.
template <class Net>
static int ntuple_play_downgraded(g2048_engine *e, const Net *net, const g2048_downgrade *rule, uint32_t k_steps,
                                  const g2048_ntuple_play_io *io, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::DowngradeArgs dr;
    if (int rc = downgrade_rule(rule, &dr))
        return rc;
    g2048::NtuplePlayOut o;
    if (int rc = ntuple_play_out(io, &o))
        return rc;
    if (int rc = usable(e))
        return rc;
    if (e->st.rng)
        return fail(G2048_ERR_INVALID, "g2048_ntuple_play_downgraded needs the spawn stream: this engine is in numpy-RNG mode, whose "
                                       "fused form is not offered (play it with g2048_downgrade_boards, g2048_ntuple_evaluate_plain "
                                       "and g2048_step)");
    if (k_steps == 0)
        return G2048_OK;
    G2048_HIP(hipSetDevice(e->device));
    e->t += 1; // transaction of the first fused step
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, nullptr, 1);
    a.k_steps = k_steps;
    G2048_HIP(g2048::launch_ntuple_play_downgraded(a, nn, dr, o, static_cast<hipStream_t>(stream)));
    e->t += k_steps - 1;
    return G2048_OK;
}

// The outputs of a translation: out [n][16], missing [n] or NULL
static int downgrade_out(const uint8_t *out)
{
    if (!out)
        return fail(G2048_ERR_INVALID, "out is NULL");
    if (reinterpret_cast<uintptr_t>(out) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: downgrade out needs 16 bytes");
    return G2048_OK;
}

// g2048_ntuple_td_io -> the kernel's outputs, or G2048_ERR_INVALID (before any HIP call: works without a device).  what: the
// entry point, for the one message that names it; train: after and delta are what its update reads
static int ntuple_td_out(const g2048_ntuple_td_io *io, const char *what, bool train, g2048::NtupleTdIo *o)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (reinterpret_cast<uintptr_t>(io->after) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple td after needs 16 bytes");
    if ((reinterpret_cast<uintptr_t>(io->after_value) | reinterpret_cast<uintptr_t>(io->best_next) | reinterpret_cast<uintptr_t>(io->delta)) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple td after_value, best_next and delta need 8 bytes");
    if (train && (!io->after || !io->delta))
        return fail(G2048_ERR_INVALID, "%s needs after and delta: its update reads them (%s is NULL)", what, io->after ? "delta" : "after");
    *o = g2048::NtupleTdIo{io->action, reinterpret_cast<uint4 *>(io->after), io->after_value, io->best_next, io->terminated, io->delta};
    return G2048_OK;
}

// The engine of a fused TD or play_log call, looked at after everything that can be refused without it
static int ntuple_td_engine(const g2048_engine *e, const char *what)
{
    if (int rc = usable(e))
        return rc;
    if (e->st.rng)
        return fail(G2048_ERR_INVALID, "%s needs the spawn stream: this engine is in numpy-RNG mode, whose fused "
                                       "form is not offered (play it with g2048_ntuple_evaluate and g2048_step)", what);
    return G2048_OK;
}

// One transaction of the clock and one launch, as g2048_ntuple_play with k_steps == 1
static hipError_t ntuple_td_launch(g2048_engine *e, const g2048::NtupleNet &nn, const g2048::NtupleTdIo &o, void *stream)
{
    e->t += 1;
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, nullptr, 1);
    a.k_steps = 1;
    return g2048::launch_ntuple_td_step(a, nn, o, static_cast<hipStream_t>(stream));
}

template <class Net> static int ntuple_td_step(g2048_engine *e, const Net *net, const g2048_ntuple_td_io *io, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleTdIo o;
    if (int rc = ntuple_td_out(io, "g2048_ntuple_td_step", false, &o))
        return rc;
    if (int rc = ntuple_td_engine(e, "g2048_ntuple_td_step"))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(ntuple_td_launch(e, nn, o, stream));
    return G2048_OK;
}

// k_steps times the fused step and the update of what it left in work, plain launches on one stream; tc: NULL for TD(0),
// else the TC update, W then A
template <class Net>
static int ntuple_td_train(g2048_engine *e, const Net *net, uint32_t k_steps, uint32_t lr_shift, const g2048_ntuple_td_io *work,
                           const g2048_ntuple_tc *tc, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleTdIo o;
    if (int rc = ntuple_td_out(work, "g2048_ntuple_td_train", true, &o))
        return rc;
    if (int rc = ntuple_delta(o.delta, lr_shift))
        return rc;
    const TcArgs tc_args{G2048_NTUPLE_TC_WEIGHTS | G2048_NTUPLE_TC_ACCUM, tc};
    g2048::NtupleTc t{};
    if (int rc = ntuple_tc(tc ? &tc_args : nullptr, &t))
        return rc;
    if (int rc = ntuple_td_engine(e, "g2048_ntuple_td_train"))
        return rc;
    if (k_steps == 0)
        return G2048_OK;
    G2048_HIP(hipSetDevice(e->device));
    for (uint32_t j = 0; j < k_steps; ++j) {
        G2048_HIP(ntuple_td_launch(e, nn, o, stream));
        G2048_HIP(g2048::launch_ntuple_update(o.after, static_cast<uint32_t>(e->n), o.delta, lr_shift, nn, tc ? &t : nullptr,
                                              static_cast<hipStream_t>(stream)));
    }
    return G2048_OK;
}

// g2048_restart -> the launchers' arguments, or G2048_ERR_INVALID (before any HIP call: works without a device): the rule, then
// NULL members, then alignment.  The records, terminated and n of a step are restart_records'.
static int restart_args(const g2048_restart *r, g2048::RestartArgs *a)
{
    if (!r)
        return fail(G2048_ERR_INVALID, "restart is NULL");
    if (r->stride_log2 > G2048_RESTART_MAX_STRIDE_LOG2)
        return fail(G2048_ERR_INVALID, "stride_log2=%u: need stride_log2 <= %d", r->stride_log2, G2048_RESTART_MAX_STRIDE_LOG2);
    if (r->capacity < 1 || r->capacity > G2048_RESTART_MAX_CAPACITY)
        return fail(G2048_ERR_INVALID, "capacity=%u: need 1 <= capacity <= %d", r->capacity, G2048_RESTART_MAX_CAPACITY);
    if (r->min_span < 2 || r->min_span > 0x80000000u)
        return fail(G2048_ERR_INVALID, "min_span=%u: need 2 <= min_span <= 2^31", r->min_span);
    if (r->max_restarts < 1)
        return fail(G2048_ERR_INVALID, "max_restarts=0: need max_restarts >= 1");
    if (!r->snap)
        return fail(G2048_ERR_INVALID, "restart snap is NULL");
    if (!r->pos)
        return fail(G2048_ERR_INVALID, "restart pos is NULL");
    if (!r->start)
        return fail(G2048_ERR_INVALID, "restart start is NULL");
    if (!r->restarts)
        return fail(G2048_ERR_INVALID, "restart restarts is NULL");
    if (reinterpret_cast<uintptr_t>(r->snap) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: restart snap needs 16 bytes");
    if ((reinterpret_cast<uintptr_t>(r->pos) | reinterpret_cast<uintptr_t>(r->start) | reinterpret_cast<uintptr_t>(r->restarts)) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: restart pos, start and restarts need 4 bytes");
    *a = g2048::RestartArgs{r->stride_log2, r->capacity, r->min_span, r->max_restarts, reinterpret_cast<uint4 *>(r->snap),
                            r->pos,         r->start,    r->restarts};
    return G2048_OK;
}

// the records, terminated and n of a restart step
static int restart_records(const uint8_t *records, uint64_t n, const uint8_t *terminated)
{
    if (!records)
        return fail(G2048_ERR_INVALID, "records is NULL");
    if (!terminated)
        return fail(G2048_ERR_INVALID, "terminated is NULL");
    if (reinterpret_cast<uintptr_t>(records) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: records need 16 bytes");
    if (n == 0 || n > 0xffffff00ull) // (the cap of g2048_create)
        return fail(G2048_ERR_INVALID, "n=%llu: need 1 <= n <= 2^32 - 256", (unsigned long long)n);
    return G2048_OK;
}

// g2048_ntuple_log -> the launchers' log, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int ntuple_log(const g2048_ntuple_log *log, g2048::NtupleLog *out)
{
    if (!log)
        return fail(G2048_ERR_INVALID, "log is NULL");
    if (!log->after)
        return fail(G2048_ERR_INVALID, "log after is NULL");
    if (!log->gain)
        return fail(G2048_ERR_INVALID, "log gain is NULL");
    if (!log->flag)
        return fail(G2048_ERR_INVALID, "log flag is NULL");
    if (log->depth < 1 || log->depth > G2048_NTUPLE_LOG_MAX_DEPTH)
        return fail(G2048_ERR_INVALID, "depth=%u: need 1 <= depth <= %d", log->depth, G2048_NTUPLE_LOG_MAX_DEPTH);
    if (reinterpret_cast<uintptr_t>(log->after) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: log after needs 16 bytes");
    if (reinterpret_cast<uintptr_t>(log->gain) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: log gain needs 8 bytes");
    *out = g2048::NtupleLog{log->depth, reinterpret_cast<uint4 *>(log->after), log->gain, log->flag};
    return G2048_OK;
}

// log.depth transactions of the clock and one launch, as g2048_ntuple_play with k_steps == log.depth; rs: NULL, or the restart
// whose step runs behind every move in that launch
static hipError_t ntuple_play_log_launch(g2048_engine *e, const g2048::NtupleNet &nn, const g2048::NtupleLog &lg, const g2048::RestartArgs *rs,
                                         void *stream)
{
    e->t += 1; // transaction of the first move
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, nullptr, 1);
    a.k_steps = lg.depth;
    const hipError_t err = rs ? g2048::launch_ntuple_play_log_restart(a, nn, lg, *rs, static_cast<hipStream_t>(stream))
                              : g2048::launch_ntuple_play_log(a, nn, lg, static_cast<hipStream_t>(stream));
    if (err == hipSuccess)
        e->t += lg.depth - 1;
    return err;
}

// for m = M - 1 down to 0: the error of slot m into delta, then the update of slot m by it; tc: NULL for the TD update, else
// the TC update, W then A.  Plain launches on one stream.
static hipError_t ntuple_log_sweep_launch(uint32_t n, const g2048::NtupleNet &nn, const g2048::NtupleLog &lg, uint32_t lr_shift, int64_t *delta,
                                          const g2048::NtupleTc *tc, void *stream)
{
    for (uint32_t m = lg.depth; m-- > 0u;) {
        if (hipError_t err = g2048::launch_ntuple_log_delta(n, nn, lg, m, delta, static_cast<hipStream_t>(stream)))
            return err;
        if (hipError_t err = g2048::launch_ntuple_update(lg.after + static_cast<uint64_t>(m) * n, n, delta, lr_shift, nn, tc,
                                                         static_cast<hipStream_t>(stream)))
            return err;
    }
    return hipSuccess;
}

// The optional restart of a play_log or log_train call: absent (today's entry points), or a g2048_restart that must be valid
struct RestartOpt {
    bool wanted;
    const g2048_restart *restart;
};
static int restart_opt(const RestartOpt &opt, g2048::RestartArgs *a) { return opt.wanted ? restart_args(opt.restart, a) : G2048_OK; }

template <class Net>
static int ntuple_play_log(g2048_engine *e, const Net *net, const g2048_ntuple_log *log, const RestartOpt &restart, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleLog lg;
    if (int rc = ntuple_log(log, &lg))
        return rc;
    g2048::RestartArgs rs{};
    if (int rc = restart_opt(restart, &rs))
        return rc;
    if (int rc = ntuple_td_engine(e, restart.wanted ? "g2048_ntuple_play_log_restart" : "g2048_ntuple_play_log"))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(ntuple_play_log_launch(e, nn, lg, restart.wanted ? &rs : nullptr, stream));
    return G2048_OK;
}

template <class Net>
static int ntuple_log_delta(uint64_t n, const Net *net, const g2048_ntuple_log *log, uint32_t m, int64_t *delta, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    if (int rc = trace_boards(n))
        return rc;
    g2048::NtupleLog lg;
    if (int rc = ntuple_log(log, &lg))
        return rc;
    if (m >= lg.depth)
        return fail(G2048_ERR_INVALID, "m=%u: need m < depth=%u (slot m + 1 is read)", m, lg.depth);
    if (int rc = ntuple_delta(delta, 0)) // (an output here: the same NULL and alignment checks, no lr_shift to refuse)
        return rc;
    G2048_HIP(g2048::launch_ntuple_log_delta(static_cast<uint32_t>(n), nn, lg, m, delta, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// What a sweep takes besides the network: the log, delta and lr_shift, and tc (NULL: the TD update) -> the launchers' forms
static int ntuple_log_sweep_args(const g2048_ntuple_log *log, uint32_t lr_shift, const int64_t *delta, const g2048_ntuple_tc *tc,
                                 g2048::NtupleLog *lg, g2048::NtupleTc *t)
{
    if (int rc = ntuple_log(log, lg))
        return rc;
    if (int rc = ntuple_delta(delta, lr_shift))
        return rc;
    const TcArgs tc_args{G2048_NTUPLE_TC_WEIGHTS | G2048_NTUPLE_TC_ACCUM, tc};
    return ntuple_tc(tc ? &tc_args : nullptr, t);
}

template <class Net>
static int ntuple_log_sweep(uint64_t n, const Net *net, const g2048_ntuple_log *log, uint32_t lr_shift, int64_t *delta,
                            const g2048_ntuple_tc *tc, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    if (int rc = trace_boards(n))
        return rc;
    g2048::NtupleLog lg;
    g2048::NtupleTc t{};
    if (int rc = ntuple_log_sweep_args(log, lr_shift, delta, tc, &lg, &t))
        return rc;
    G2048_HIP(ntuple_log_sweep_launch(static_cast<uint32_t>(n), nn, lg, lr_shift, delta, tc ? &t : nullptr, stream));
    return G2048_OK;
}

// rounds times { play_log; sweep }, plain launches on one stream
template <class Net>
static int ntuple_log_train(g2048_engine *e, const Net *net, uint32_t rounds, uint32_t lr_shift, const g2048_ntuple_log *log, int64_t *delta,
                            const g2048_ntuple_tc *tc, const RestartOpt &restart, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleLog lg;
    g2048::NtupleTc t{};
    if (int rc = ntuple_log_sweep_args(log, lr_shift, delta, tc, &lg, &t))
        return rc;
    g2048::RestartArgs rs{};
    if (int rc = restart_opt(restart, &rs))
        return rc;
    if (int rc = ntuple_td_engine(e, restart.wanted ? "g2048_ntuple_log_train_restart" : "g2048_ntuple_log_train"))
        return rc;
    if (rounds == 0)
        return G2048_OK;
    G2048_HIP(hipSetDevice(e->device));
    for (uint32_t r = 0; r < rounds; ++r) {
        G2048_HIP(ntuple_play_log_launch(e, nn, lg, restart.wanted ? &rs : nullptr, stream));
        G2048_HIP(ntuple_log_sweep_launch(static_cast<uint32_t>(e->n), nn, lg, lr_shift, delta, tc ? &t : nullptr, stream));
    }
    return G2048_OK;
}

// g2048_ntuple_search_active's mask.  Those entry points check it before they look at the engine (usable() consumes a
// pending strict-actions report, so it cannot run ahead of this).
static int ntuple_search_mask(const uint32_t *active)
{
    if (reinterpret_cast<uintptr_t>(active) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple search active needs 4 bytes");
    return G2048_OK;
}

// active: the mask, NULL for every board (and always for plain boards)
template <class Net>
static int ntuple_search(const Source &src, const Net *net, const g2048_ntuple_search_io *io, const uint32_t *active, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleSearchOut o;
    if (int rc = ntuple_search_out(io, &o))
        return rc;
    o.active = active;
    if (int rc = select_device(src))
        return rc;
    G2048_HIP(g2048::launch_ntuple_search(src.boards, io->depth, nn, o, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// g2048_ntuple_deep_io -> the kernel's outputs, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int ntuple_deep_out(const g2048_ntuple_deep_io *io, bool plain, g2048::NtupleSearchOut *o)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (!io->action && !io->value)
        return fail(G2048_ERR_INVALID, "g2048_ntuple_deep_io requests no output (action and value are both NULL)");
    if (reinterpret_cast<uintptr_t>(io->value) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple deep search value needs 16 bytes");
    if (io->depth < G2048_NTUPLE_DEEP_MIN_DEPTH || io->depth > G2048_NTUPLE_DEEP_MAX_DEPTH)
        return fail(G2048_ERR_INVALID, "depth=%u: need %d <= depth <= %d", io->depth, G2048_NTUPLE_DEEP_MIN_DEPTH,
                    G2048_NTUPLE_DEEP_MAX_DEPTH);
    if (plain && io->active)
        return fail(G2048_ERR_INVALID, "g2048_ntuple_deep_io active is for the engine forms: a plain form takes no mask");
    if (reinterpret_cast<uintptr_t>(io->active) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple deep search active needs 4 bytes");
    *o = g2048::NtupleSearchOut{io->action, io->value, io->active};
    return G2048_OK;
}

template <class Net> static int ntuple_deep_search(const Source &src, const Net *net, const g2048_ntuple_deep_io *io, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleSearchOut o;
    if (int rc = ntuple_deep_out(io, src.boards.plain, &o))
        return rc;
    if (int rc = select_device(src))
        return rc;
    G2048_HIP(g2048::launch_ntuple_deep_search(src.boards, io->depth, nn, o, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// The outputs of the two searches that take a schedule, g2048_ntuple_adaptive_io (`type`, "adaptive") and
// g2048_ntuple_reduced_io: the kernel's outputs, or G2048_ERR_INVALID (before any HIP call: works without a device)
static int ntuple_schedule_out(const char *type, const char *what, const uint8_t schedule[17], uint8_t *action, int64_t *value,
                               uint8_t *depth, const uint32_t *active, bool plain, g2048::NtupleAdaptiveOut *o)
{
    for (uint32_t e = 0; e < 17u; ++e)
        if (schedule[e] > G2048_NTUPLE_ADAPTIVE_MAX_DEPTH)
            return fail(G2048_ERR_INVALID, "schedule[%u]=%u: need a depth of 0..%d", e, schedule[e], G2048_NTUPLE_ADAPTIVE_MAX_DEPTH);
    if (!action && !value)
        return fail(G2048_ERR_INVALID, "%s requests no output (action and value are both NULL)", type);
    if (reinterpret_cast<uintptr_t>(value) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple %s search value needs 16 bytes", what);
    if (plain && active)
        return fail(G2048_ERR_INVALID, "%s active is for the engine forms: a plain form takes no mask", type);
    if (reinterpret_cast<uintptr_t>(active) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple %s search active needs 4 bytes", what);
    *o = g2048::NtupleAdaptiveOut{action, value, depth, active};
    return G2048_OK;
}

// *reduce4 = 0: the adaptive search, which reduces nothing
static int ntuple_adaptive_out(const g2048_ntuple_adaptive_io *io, bool plain, g2048::NtupleAdaptiveOut *o, uint32_t *reduce4)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    *reduce4 = 0u;
    return ntuple_schedule_out("g2048_ntuple_adaptive_io", "adaptive", io->schedule, io->action, io->value, io->depth, io->active, plain, o);
}

static int ntuple_adaptive_out(const g2048_ntuple_reduced_io *io, bool plain, g2048::NtupleAdaptiveOut *o, uint32_t *reduce4)
{
    if (!io)
        return fail(G2048_ERR_INVALID, "io is NULL");
    if (io->reduce4 == 0u)
        return fail(G2048_ERR_INVALID, "reduce4=0: need %d <= reduce4 <= %d; the search that reduces nothing is g2048_ntuple_adaptive_search",
                    G2048_NTUPLE_REDUCE4_MIN, G2048_NTUPLE_REDUCE4_MAX);
    if (io->reduce4 > G2048_NTUPLE_REDUCE4_MAX)
        return fail(G2048_ERR_INVALID, "reduce4=%u: need %d <= reduce4 <= %d", io->reduce4, G2048_NTUPLE_REDUCE4_MIN, G2048_NTUPLE_REDUCE4_MAX);
    *reduce4 = io->reduce4;
    return ntuple_schedule_out("g2048_ntuple_reduced_io", "reduced", io->schedule, io->action, io->value, io->depth, io->active, plain, o);
}

// Io: g2048_ntuple_adaptive_io or g2048_ntuple_reduced_io -- one body for both searches
template <class Net, class Io> static int ntuple_adaptive_search(const Source &src, const Net *net, const Io *io, void *stream)
{
    if (src.rc)
        return src.rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    g2048::NtupleAdaptiveOut o;
    uint32_t reduce4;
    if (int rc = ntuple_adaptive_out(io, src.boards.plain, &o, &reduce4))
        return rc;
    if (int rc = select_device(src))
        return rc;
    if (reduce4 != 0u)
        G2048_HIP(g2048::launch_ntuple_reduced_search(src.boards, io->schedule, reduce4, nn, o, static_cast<hipStream_t>(stream)));
    else
        G2048_HIP(g2048::launch_ntuple_adaptive_search(src.boards, io->schedule, nn, o, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

template <class Net> static int ntuple_values_plain(const uint8_t *boards, uint64_t n, const Net *net, int64_t *v, void *stream)
{
    if (int rc = plain_boards(boards, n))
        return rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    if (!v)
        return fail(G2048_ERR_INVALID, "v is NULL");
    if (reinterpret_cast<uintptr_t>(v) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: ntuple v needs 8 bytes");
    G2048_HIP(g2048::launch_ntuple_values(reinterpret_cast<const uint4 *>(boards), static_cast<uint32_t>(n), nn, v,
                                          static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// The three updates, one per item source; tc: the TC entry points' arguments, NULL for the TD update; mean: the batch-mean
// entry points', NULL for the others (never both)
template <class Net>
static int ntuple_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, const Net *net, const TcArgs *tc,
                               void *stream, const MeanArgs *mean = nullptr)
{
    if (int rc = plain_boards(boards, n))
        return rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    if (int rc = ntuple_delta(delta, lr_shift))
        return rc;
    g2048::NtupleTc t{};
    if (int rc = ntuple_tc(tc, &t))
        return rc;
    g2048::NtupleMean m{};
    if (int rc = ntuple_mean(mean, n, &m))
        return rc;
    if (mean) {
        G2048_HIP(g2048::launch_ntuple_mean_update(reinterpret_cast<const uint4 *>(boards), static_cast<uint32_t>(n), delta, lr_shift, nn, m,
                                                   static_cast<hipStream_t>(stream)));
        return G2048_OK;
    }
    G2048_HIP(g2048::launch_ntuple_update(reinterpret_cast<const uint4 *>(boards), static_cast<uint32_t>(n), delta, lr_shift, nn,
                                          tc ? &t : nullptr, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

template <class Net>
static int ntuple_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, const Net *net, const TcArgs *tc,
                               const g2048_ntuple_trace *tr, uint32_t slot, void *stream, const MeanArgs *mean = nullptr)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    if (int rc = trace_boards(n))
        return rc;
    if (int rc = ntuple_delta(delta, lr_shift))
        return rc;
    g2048::NtupleTc t{};
    if (int rc = ntuple_tc(tc, &t))
        return rc;
    g2048::NtupleTrace h;
    if (int rc = ntuple_history(tr, "tr", "trace", slot, &h))
        return rc;
    g2048::NtupleMean m{};
    if (int rc = ntuple_mean(mean, static_cast<uint64_t>(h.depth) * n, &m))
        return rc;
    if (mean) {
        G2048_HIP(g2048::launch_ntuple_mean_trace_update(static_cast<uint32_t>(n), delta, lr_shift, nn, h, slot, m,
                                                         static_cast<hipStream_t>(stream)));
        return G2048_OK;
    }
    G2048_HIP(g2048::launch_ntuple_trace_update(static_cast<uint32_t>(n), delta, lr_shift, nn, h, slot, tc ? &t : nullptr,
                                                static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

template <class Net>
static int ntuple_delay_update(uint64_t n, uint32_t lr_shift, uint32_t mode, const Net *net, const TcArgs *tc,
                               const g2048_ntuple_delay *dl, uint32_t slot, void *stream)
{
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn))
        return rc;
    if (int rc = trace_boards(n))
        return rc;
    if (int rc = ntuple_delay_mode(lr_shift, mode))
        return rc;
    g2048::NtupleTc t{};
    if (int rc = ntuple_tc(tc, &t))
        return rc;
    g2048::NtupleDelay h;
    if (int rc = ntuple_history(dl, "dl", "delay", slot, &h))
        return rc;
    G2048_HIP(g2048::launch_ntuple_delay_update(static_cast<uint32_t>(n), lr_shift, mode, nn, h, slot, tc ? &t : nullptr,
                                                static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// g2048_ntuple_trace_push (Hist = g2048::NtupleTrace) and g2048_ntuple_delay_push (g2048::NtupleDelay); name and noun as in
// ntuple_history
template <class Hist, class Desc>
static int ntuple_push(const uint8_t *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated, uint64_t n,
                       const Desc *desc, const char *name, const char *noun, uint32_t slot, int64_t *delta, void *stream)
{
    if (!after)
        return fail(G2048_ERR_INVALID, "after is NULL");
    if (!after_value)
        return fail(G2048_ERR_INVALID, "after_value is NULL");
    if (!best_next)
        return fail(G2048_ERR_INVALID, "best_next is NULL");
    if (!terminated)
        return fail(G2048_ERR_INVALID, "terminated is NULL");
    if (!delta)
        return fail(G2048_ERR_INVALID, "delta is NULL");
    if (int rc = trace_boards(n))
        return rc;
    Hist h;
    if (int rc = ntuple_history(desc, name, noun, slot, &h))
        return rc;
    if (reinterpret_cast<uintptr_t>(after) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: %s after needs 16 bytes", noun);
    if ((reinterpret_cast<uintptr_t>(after_value) | reinterpret_cast<uintptr_t>(best_next) | reinterpret_cast<uintptr_t>(delta)) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: %s after_value, best_next and delta need 8 bytes", noun);
    G2048_HIP(g2048::launch_ntuple_push(reinterpret_cast<const uint4 *>(after), after_value, best_next, terminated, static_cast<uint32_t>(n),
                                        h, slot, delta, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

extern "C" {

int g2048_ntuple_evaluate(const g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_io *io, void *stream)
{
    return ntuple_evaluate(from_engine(e), net, io, stream);
}

int g2048_ntuple_staged_evaluate(const g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_io *io, void *stream)
{
    return ntuple_evaluate(from_engine(e), net, io, stream);
}

int g2048_ntuple_play(g2048_engine *e, const g2048_ntuple_net *net, uint32_t k_steps, const g2048_ntuple_play_io *io, void *stream)
{
    return ntuple_play(e, net, k_steps, io, stream);
}

int g2048_ntuple_staged_play(g2048_engine *e, const g2048_ntuple_staged_net *net, uint32_t k_steps, const g2048_ntuple_play_io *io,
                             void *stream)
{
    return ntuple_play(e, net, k_steps, io, stream);
}

int g2048_ntuple_td_step(g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_td_io *io, void *stream)
{
    return ntuple_td_step(e, net, io, stream);
}

int g2048_ntuple_staged_td_step(g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_td_io *io, void *stream)
{
    return ntuple_td_step(e, net, io, stream);
}

int g2048_ntuple_td_train(g2048_engine *e, const g2048_ntuple_net *net, uint32_t k_steps, uint32_t lr_shift,
                          const g2048_ntuple_td_io *work, const g2048_ntuple_tc *tc, void *stream)
{
    return ntuple_td_train(e, net, k_steps, lr_shift, work, tc, stream);
}

int g2048_ntuple_staged_td_train(g2048_engine *e, const g2048_ntuple_staged_net *net, uint32_t k_steps, uint32_t lr_shift,
                                 const g2048_ntuple_td_io *work, const g2048_ntuple_tc *tc, void *stream)
{
    return ntuple_td_train(e, net, k_steps, lr_shift, work, tc, stream);
}

int g2048_ntuple_play_downgraded(g2048_engine *e, const g2048_ntuple_net *net, const g2048_downgrade *rule, uint32_t k_steps,
                                 const g2048_ntuple_play_io *io, void *stream)
{
    return ntuple_play_downgraded(e, net, rule, k_steps, io, stream);
}

int g2048_ntuple_staged_play_downgraded(g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_downgrade *rule,
                                        uint32_t k_steps, const g2048_ntuple_play_io *io, void *stream)
{
    return ntuple_play_downgraded(e, net, rule, k_steps, io, stream);
}

int g2048_downgrade_plain(const uint8_t *boards, uint64_t n, const g2048_downgrade *rule, uint8_t *out, uint8_t *missing, void *stream)
{
    if (int rc = plain_boards(boards, n))
        return rc;
    g2048::DowngradeArgs dr;
    if (int rc = downgrade_rule(rule, &dr))
        return rc;
    if (int rc = downgrade_out(out))
        return rc;
    G2048_HIP(g2048::launch_downgrade(reinterpret_cast<const uint4 *>(boards), static_cast<uint32_t>(n), dr, nullptr,
                                      reinterpret_cast<uint4 *>(out), missing, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_downgrade_boards(const g2048_engine *e, const g2048_downgrade *rule, const uint32_t *active, uint8_t *out, uint8_t *missing,
                           void *stream)
{
    g2048::DowngradeArgs dr;
    if (int rc = downgrade_rule(rule, &dr))
        return rc;
    if (int rc = downgrade_out(out))
        return rc;
    if (reinterpret_cast<uintptr_t>(active) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: downgrade active needs 4 bytes");
    if (int rc = usable(e)) // (after everything that can be refused without an engine)
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_downgrade(e->st.boards, static_cast<uint32_t>(e->n), dr, active, reinterpret_cast<uint4 *>(out), missing,
                                      static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_ntuple_play_log(g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_log *log, void *stream)
{
    return ntuple_play_log(e, net, log, RestartOpt{false, nullptr}, stream);
}

int g2048_ntuple_staged_play_log(g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_log *log, void *stream)
{
    return ntuple_play_log(e, net, log, RestartOpt{false, nullptr}, stream);
}

int g2048_ntuple_play_log_restart(g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_log *log, const g2048_restart *restart,
                                  void *stream)
{
    return ntuple_play_log(e, net, log, RestartOpt{true, restart}, stream);
}

int g2048_ntuple_staged_play_log_restart(g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_log *log,
                                         const g2048_restart *restart, void *stream)
{
    return ntuple_play_log(e, net, log, RestartOpt{true, restart}, stream);
}

int g2048_ntuple_log_delta(uint64_t n, const g2048_ntuple_net *net, const g2048_ntuple_log *log, uint32_t m, int64_t *delta, void *stream)
{
    return ntuple_log_delta(n, net, log, m, delta, stream);
}

int g2048_ntuple_staged_log_delta(uint64_t n, const g2048_ntuple_staged_net *net, const g2048_ntuple_log *log, uint32_t m, int64_t *delta,
                                  void *stream)
{
    return ntuple_log_delta(n, net, log, m, delta, stream);
}

int g2048_ntuple_log_sweep(uint64_t n, const g2048_ntuple_net *net, const g2048_ntuple_log *log, uint32_t lr_shift, int64_t *delta,
                           const g2048_ntuple_tc *tc, void *stream)
{
    return ntuple_log_sweep(n, net, log, lr_shift, delta, tc, stream);
}

int g2048_ntuple_staged_log_sweep(uint64_t n, const g2048_ntuple_staged_net *net, const g2048_ntuple_log *log, uint32_t lr_shift,
                                  int64_t *delta, const g2048_ntuple_tc *tc, void *stream)
{
    return ntuple_log_sweep(n, net, log, lr_shift, delta, tc, stream);
}

int g2048_ntuple_log_train(g2048_engine *e, const g2048_ntuple_net *net, uint32_t rounds, uint32_t lr_shift, const g2048_ntuple_log *log,
                           int64_t *delta, const g2048_ntuple_tc *tc, void *stream)
{
    return ntuple_log_train(e, net, rounds, lr_shift, log, delta, tc, RestartOpt{false, nullptr}, stream);
}

int g2048_ntuple_staged_log_train(g2048_engine *e, const g2048_ntuple_staged_net *net, uint32_t rounds, uint32_t lr_shift,
                                  const g2048_ntuple_log *log, int64_t *delta, const g2048_ntuple_tc *tc, void *stream)
{
    return ntuple_log_train(e, net, rounds, lr_shift, log, delta, tc, RestartOpt{false, nullptr}, stream);
}

int g2048_ntuple_log_train_restart(g2048_engine *e, const g2048_ntuple_net *net, uint32_t rounds, uint32_t lr_shift,
                                   const g2048_ntuple_log *log, int64_t *delta, const g2048_ntuple_tc *tc, const g2048_restart *restart,
                                   void *stream)
{
    return ntuple_log_train(e, net, rounds, lr_shift, log, delta, tc, RestartOpt{true, restart}, stream);
}

int g2048_ntuple_staged_log_train_restart(g2048_engine *e, const g2048_ntuple_staged_net *net, uint32_t rounds, uint32_t lr_shift,
                                          const g2048_ntuple_log *log, int64_t *delta, const g2048_ntuple_tc *tc,
                                          const g2048_restart *restart, void *stream)
{
    return ntuple_log_train(e, net, rounds, lr_shift, log, delta, tc, RestartOpt{true, restart}, stream);
}

// One budgeted step with the caller's actions: g2048_ntuple_play's contract and clock at k_steps == 1, g2048_step's checks of
// the action buffer.  What can be refused without the engine is refused first.
int g2048_play_step(g2048_engine *e, const void *actions, int32_t action_dtype, const g2048_ntuple_play_io *io, void *stream)
{
    if (action_dtype < G2048_ACT_RANDOM || action_dtype > G2048_ACT_I64)
        return fail(G2048_ERR_INVALID, "unknown action_dtype %d", action_dtype);
    if (action_dtype != G2048_ACT_RANDOM && !actions)
        return fail(G2048_ERR_INVALID, "actions is NULL but action_dtype is %d", action_dtype);
    if (action_dtype != G2048_ACT_RANDOM && (reinterpret_cast<uintptr_t>(actions) & (action_size(action_dtype) - 1)))
        return fail(G2048_ERR_INVALID, "misaligned buffer: actions need their element size");
    g2048::NtuplePlayOut o;
    if (int rc = ntuple_play_out(io, &o))
        return rc;
    if (int rc = usable(e))
        return rc;
    if (e->st.rng)
        return fail(G2048_ERR_INVALID, "g2048_play_step needs the spawn stream: this engine is in numpy-RNG mode, whose budgeted "
                                       "form is not offered (play it with g2048_step)");
    G2048_HIP(hipSetDevice(e->device));
    e->t += 1;
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, nullptr, 1);
    a.actions = action_dtype == G2048_ACT_RANDOM ? nullptr : actions;
    a.k_steps = 1;
    G2048_HIP(g2048::launch_play_step(a, action_dtype, o, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_ntuple_evaluate_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_net *net, const g2048_ntuple_io *io,
                                void *stream)
{
    return ntuple_evaluate(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_staged_evaluate_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net,
                                       const g2048_ntuple_io *io, void *stream)
{
    return ntuple_evaluate(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_search(const g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_search_io *io, void *stream)
{
    return ntuple_search(from_engine(e), net, io, nullptr, stream);
}

int g2048_ntuple_staged_search(const g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_search_io *io,
                               void *stream)
{
    return ntuple_search(from_engine(e), net, io, nullptr, stream);
}

int g2048_ntuple_search_active(const g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_search_io *io,
                               const uint32_t *active, void *stream)
{
    if (int rc = ntuple_search_mask(active))
        return rc;
    return ntuple_search(from_engine(e), net, io, active, stream);
}

int g2048_ntuple_staged_search_active(const g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_search_io *io,
                                      const uint32_t *active, void *stream)
{
    if (int rc = ntuple_search_mask(active))
        return rc;
    return ntuple_search(from_engine(e), net, io, active, stream);
}

int g2048_ntuple_deep_search(const g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_deep_io *io, void *stream)
{
    return ntuple_deep_search(from_engine(e), net, io, stream);
}

int g2048_ntuple_deep_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_net *net, const g2048_ntuple_deep_io *io,
                                   void *stream)
{
    return ntuple_deep_search(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_staged_deep_search(const g2048_engine *e, const g2048_ntuple_staged_net *net, const g2048_ntuple_deep_io *io,
                                    void *stream)
{
    return ntuple_deep_search(from_engine(e), net, io, stream);
}

int g2048_ntuple_staged_deep_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net,
                                          const g2048_ntuple_deep_io *io, void *stream)
{
    return ntuple_deep_search(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_adaptive_search(const g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_adaptive_io *io, void *stream)
{
    return ntuple_adaptive_search(from_engine(e), net, io, stream);
}

int g2048_ntuple_adaptive_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_net *net,
                                       const g2048_ntuple_adaptive_io *io, void *stream)
{
    return ntuple_adaptive_search(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_staged_adaptive_search(const g2048_engine *e, const g2048_ntuple_staged_net *net,
                                        const g2048_ntuple_adaptive_io *io, void *stream)
{
    return ntuple_adaptive_search(from_engine(e), net, io, stream);
}

int g2048_ntuple_staged_adaptive_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net,
                                              const g2048_ntuple_adaptive_io *io, void *stream)
{
    return ntuple_adaptive_search(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_reduced_search(const g2048_engine *e, const g2048_ntuple_net *net, const g2048_ntuple_reduced_io *io, void *stream)
{
    return ntuple_adaptive_search(from_engine(e), net, io, stream);
}

int g2048_ntuple_reduced_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_net *net,
                                      const g2048_ntuple_reduced_io *io, void *stream)
{
    return ntuple_adaptive_search(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_staged_reduced_search(const g2048_engine *e, const g2048_ntuple_staged_net *net,
                                       const g2048_ntuple_reduced_io *io, void *stream)
{
    return ntuple_adaptive_search(from_engine(e), net, io, stream);
}

int g2048_ntuple_staged_reduced_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net,
                                             const g2048_ntuple_reduced_io *io, void *stream)
{
    return ntuple_adaptive_search(from_plain(boards, n), net, io, stream);
}

int g2048_ntuple_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_net *net, const g2048_ntuple_search_io *io,
                              void *stream)
{
    return ntuple_search(from_plain(boards, n), net, io, nullptr, stream);
}

int g2048_ntuple_staged_search_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net,
                                     const g2048_ntuple_search_io *io, void *stream)
{
    return ntuple_search(from_plain(boards, n), net, io, nullptr, stream);
}

int g2048_ntuple_values_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_net *net, int64_t *v, void *stream)
{
    return ntuple_values_plain(boards, n, net, v, stream);
}

int g2048_ntuple_staged_values_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net, int64_t *v, void *stream)
{
    return ntuple_values_plain(boards, n, net, v, stream);
}

int g2048_ntuple_stage_plain(const uint8_t *boards, uint64_t n, const g2048_ntuple_staged_net *net, uint8_t *stage, void *stream)
{
    if (int rc = plain_boards(boards, n))
        return rc;
    g2048::NtupleNet nn;
    if (int rc = ntuple_net(net, &nn, false))
        return rc;
    if (!stage)
        return fail(G2048_ERR_INVALID, "stage is NULL");
    G2048_HIP(g2048::launch_ntuple_stage(reinterpret_cast<const uint4 *>(boards), static_cast<uint32_t>(n), nn, stage,
                                         static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_ntuple_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift,
                              const g2048_ntuple_net *net, void *stream)
{
    return ntuple_update_plain(boards, n, delta, lr_shift, net, nullptr, stream);
}

int g2048_ntuple_staged_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift,
                                     const g2048_ntuple_staged_net *net, void *stream)
{
    return ntuple_update_plain(boards, n, delta, lr_shift, net, nullptr, stream);
}

int g2048_ntuple_tc_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases,
                                 const g2048_ntuple_net *net, const g2048_ntuple_tc *tc, void *stream)
{
    const TcArgs t{phases, tc};
    return ntuple_update_plain(boards, n, delta, lr_shift, net, &t, stream);
}

int g2048_ntuple_staged_tc_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases,
                                        const g2048_ntuple_staged_net *net, const g2048_ntuple_tc *tc, void *stream)
{
    const TcArgs t{phases, tc};
    return ntuple_update_plain(boards, n, delta, lr_shift, net, &t, stream);
}

int g2048_ntuple_mean_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases,
                                   const g2048_ntuple_net *net, const g2048_ntuple_mean *mean, void *stream)
{
    const MeanArgs m{phases, mean};
    return ntuple_update_plain(boards, n, delta, lr_shift, net, nullptr, stream, &m);
}

int g2048_ntuple_staged_mean_update_plain(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases,
                                          const g2048_ntuple_staged_net *net, const g2048_ntuple_mean *mean, void *stream)
{
    const MeanArgs m{phases, mean};
    return ntuple_update_plain(boards, n, delta, lr_shift, net, nullptr, stream, &m);
}

int g2048_ntuple_trace_push(const uint8_t *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                            uint64_t n, const g2048_ntuple_trace *tr, uint32_t slot, int64_t *delta, void *stream)
{
    return ntuple_push<g2048::NtupleTrace>(after, after_value, best_next, terminated, n, tr, "tr", "trace", slot, delta, stream);
}

int g2048_ntuple_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, const g2048_ntuple_net *net,
                              const g2048_ntuple_trace *tr, uint32_t slot, void *stream)
{
    return ntuple_trace_update(n, delta, lr_shift, net, nullptr, tr, slot, stream);
}

int g2048_ntuple_staged_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, const g2048_ntuple_staged_net *net,
                                     const g2048_ntuple_trace *tr, uint32_t slot, void *stream)
{
    return ntuple_trace_update(n, delta, lr_shift, net, nullptr, tr, slot, stream);
}

int g2048_ntuple_tc_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const g2048_ntuple_net *net,
                                 const g2048_ntuple_tc *tc, const g2048_ntuple_trace *tr, uint32_t slot, void *stream)
{
    const TcArgs t{phases, tc};
    return ntuple_trace_update(n, delta, lr_shift, net, &t, tr, slot, stream);
}

int g2048_ntuple_staged_tc_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases,
                                        const g2048_ntuple_staged_net *net, const g2048_ntuple_tc *tc, const g2048_ntuple_trace *tr,
                                        uint32_t slot, void *stream)
{
    const TcArgs t{phases, tc};
    return ntuple_trace_update(n, delta, lr_shift, net, &t, tr, slot, stream);
}

int g2048_ntuple_mean_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const g2048_ntuple_net *net,
                                   const g2048_ntuple_mean *mean, const g2048_ntuple_trace *tr, uint32_t slot, void *stream)
{
    const MeanArgs m{phases, mean};
    return ntuple_trace_update(n, delta, lr_shift, net, nullptr, tr, slot, stream, &m);
}

int g2048_ntuple_staged_mean_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases,
                                          const g2048_ntuple_staged_net *net, const g2048_ntuple_mean *mean,
                                          const g2048_ntuple_trace *tr, uint32_t slot, void *stream)
{
    const MeanArgs m{phases, mean};
    return ntuple_trace_update(n, delta, lr_shift, net, nullptr, tr, slot, stream, &m);
}

int g2048_ntuple_delay_push(const uint8_t *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                            uint64_t n, const g2048_ntuple_delay *dl, uint32_t slot, int64_t *delta, void *stream)
{
    return ntuple_push<g2048::NtupleDelay>(after, after_value, best_next, terminated, n, dl, "dl", "delay", slot, delta, stream);
}

int g2048_ntuple_delay_update(uint64_t n, uint32_t lr_shift, uint32_t mode, const g2048_ntuple_net *net, const g2048_ntuple_delay *dl,
                              uint32_t slot, void *stream)
{
    return ntuple_delay_update(n, lr_shift, mode, net, nullptr, dl, slot, stream);
}

int g2048_ntuple_staged_delay_update(uint64_t n, uint32_t lr_shift, uint32_t mode, const g2048_ntuple_staged_net *net,
                                     const g2048_ntuple_delay *dl, uint32_t slot, void *stream)
{
    return ntuple_delay_update(n, lr_shift, mode, net, nullptr, dl, slot, stream);
}

int g2048_ntuple_tc_delay_update(uint64_t n, uint32_t lr_shift, uint32_t phases, uint32_t mode, const g2048_ntuple_net *net,
                                 const g2048_ntuple_tc *tc, const g2048_ntuple_delay *dl, uint32_t slot, void *stream)
{
    const TcArgs t{phases, tc};
    return ntuple_delay_update(n, lr_shift, mode, net, &t, dl, slot, stream);
}

int g2048_ntuple_staged_tc_delay_update(uint64_t n, uint32_t lr_shift, uint32_t phases, uint32_t mode,
                                        const g2048_ntuple_staged_net *net, const g2048_ntuple_tc *tc, const g2048_ntuple_delay *dl,
                                        uint32_t slot, void *stream)
{
    const TcArgs t{phases, tc};
    return ntuple_delay_update(n, lr_shift, mode, net, &t, dl, slot, stream);
}

// g2048_carousel and the records of a call -> the launcher's arguments, or G2048_ERR_INVALID (before any HIP call: works
// without a device)
static int carousel_args(const g2048_carousel *c, uint8_t *records, uint64_t n, uint64_t index_offset, const uint8_t *terminated,
                         g2048::CarouselArgs *a)
{
    if (!c)
        return fail(G2048_ERR_INVALID, "carousel is NULL");
    if (c->n_stages < 2 || c->n_stages > G2048_NTUPLE_MAX_STAGES)
        return fail(G2048_ERR_INVALID, "n_stages=%u: a carousel needs 2 <= n_stages <= %d", c->n_stages, G2048_NTUPLE_MAX_STAGES);
    if (int rc = stage_thresholds(c->n_stages, c->thresholds))
        return rc;
    if (c->capacity < 1 || c->capacity > G2048_CAROUSEL_MAX_CAPACITY)
        return fail(G2048_ERR_INVALID, "capacity=%u: need 1 <= capacity <= %d", c->capacity, G2048_CAROUSEL_MAX_CAPACITY);
    if (!c->pool)
        return fail(G2048_ERR_INVALID, "carousel pool is NULL");
    if (!c->count)
        return fail(G2048_ERR_INVALID, "carousel count is NULL");
    if (!c->seen)
        return fail(G2048_ERR_INVALID, "carousel seen is NULL");
    if (!c->episodes)
        return fail(G2048_ERR_INVALID, "carousel episodes is NULL");
    if (!c->scratch)
        return fail(G2048_ERR_INVALID, "carousel scratch is NULL");
    if (!records)
        return fail(G2048_ERR_INVALID, "records is NULL");
    if (!terminated)
        return fail(G2048_ERR_INVALID, "terminated is NULL");
    if ((reinterpret_cast<uintptr_t>(c->pool) | reinterpret_cast<uintptr_t>(records)) & 15u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: carousel pool and records need 16 bytes");
    if (reinterpret_cast<uintptr_t>(c->count) & 7u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: carousel count needs 8 bytes");
    if ((reinterpret_cast<uintptr_t>(c->episodes) | reinterpret_cast<uintptr_t>(c->scratch)) & 3u)
        return fail(G2048_ERR_INVALID, "misaligned buffer: carousel episodes and scratch need 4 bytes");
    if (n == 0 || n > 0xffffff00ull) // (the cap of g2048_create)
        return fail(G2048_ERR_INVALID, "n=%llu: need 1 <= n <= 2^32 - 256", (unsigned long long)n);
    if (index_offset > 0x100000000ull || index_offset + n > 0x100000000ull)
        return fail(G2048_ERR_INVALID, "index_offset=%llu, n=%llu: need index_offset + n <= 2^32", (unsigned long long)index_offset,
                    (unsigned long long)n);
    *a = g2048::CarouselArgs{};
    a->records = reinterpret_cast<uint4 *>(records);
    a->terminated = terminated;
    a->n = static_cast<uint32_t>(n);
    a->index_offset = static_cast<uint32_t>(index_offset);
    a->n_stages = c->n_stages;
    a->capacity = c->capacity;
    for (uint32_t j = 0; j + 1 < c->n_stages; ++j)
        a->thresholds[j] = c->thresholds[j];
    a->seed_lo = static_cast<uint32_t>(c->seed);
    a->seed_hi = static_cast<uint32_t>(c->seed >> 32);
    a->pool = reinterpret_cast<uint4 *>(c->pool);
    a->count = c->count;
    a->seen = c->seen;
    a->episodes = c->episodes;
    a->scratch = static_cast<uint32_t *>(c->scratch);
    return G2048_OK;
}

uint64_t g2048_carousel_scratch_bytes(uint64_t n) { return n == 0 || n > 0xffffff00ull ? 0 : g2048::kCarouselScratchBytes; }

int g2048_carousel_step(g2048_engine *e, const g2048_carousel *c, const uint8_t *terminated, void *stream)
{
    if (int rc = usable(e))
        return rc;
    g2048::CarouselArgs a;
    if (int rc = carousel_args(c, reinterpret_cast<uint8_t *>(e->st.boards), e->n, e->board_offset, terminated, &a))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_carousel_step(a, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_carousel_step_plain(uint8_t *records, uint64_t n, uint64_t index_offset, const uint8_t *terminated, const g2048_carousel *c,
                              void *stream)
{
    g2048::CarouselArgs a;
    if (int rc = carousel_args(c, records, n, index_offset, terminated, &a))
        return rc;
    G2048_HIP(g2048::launch_carousel_step(a, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_restart_step(g2048_engine *e, const g2048_restart *r, const uint8_t *terminated, void *stream)
{
    if (int rc = usable(e))
        return rc;
    g2048::RestartArgs a;
    if (int rc = restart_args(r, &a))
        return rc;
    if (int rc = restart_records(reinterpret_cast<const uint8_t *>(e->st.boards), e->n, terminated))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_restart_step(e->st.boards, terminated, static_cast<uint32_t>(e->n), a, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_restart_step_plain(uint8_t *records, uint64_t n, const uint8_t *terminated, const g2048_restart *r, void *stream)
{
    g2048::RestartArgs a;
    if (int rc = restart_args(r, &a))
        return rc;
    if (int rc = restart_records(records, n, terminated))
        return rc;
    G2048_HIP(g2048::launch_restart_step(reinterpret_cast<uint4 *>(records), terminated, static_cast<uint32_t>(n), a,
                                         static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_add_tile(g2048_engine *e, uint32_t slot, void *stream)
{
    if (int rc = usable(e))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    e->fresh = 0;
    G2048_HIP(g2048::launch_add_tile(make_args(e, nullptr, 0), slot, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_fill_random_actions(const g2048_engine *e, uint64_t t_first, uint32_t k_steps, uint8_t *out, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_fill_actions(out, static_cast<uint32_t>(e->n), static_cast<uint32_t>(e->board_offset),
                                         static_cast<uint32_t>(e->seed), static_cast<uint32_t>(e->seed >> 32),
                                         t_first, k_steps, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_onehot(const g2048_engine *e, void *out, int32_t obs_dtype, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (obs_dtype < G2048_OBS_U8 || obs_dtype > G2048_OBS_F32)
        return fail(G2048_ERR_INVALID, "unknown obs_dtype %d", obs_dtype);
    if (reinterpret_cast<uintptr_t>(out) & 15u)
        return fail(G2048_ERR_INVALID, "one-hot output must be 16-byte aligned");
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_onehot(e->st.boards, static_cast<uint32_t>(e->n), out, obs_dtype,
                                   static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// A synchronous copy between the engine's device memory and the caller's host buffer (the engine's side is never NULL).
static int copy_sync(const g2048_engine *e, void *dst, const void *src, size_t bytes, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!dst || !src)
        return fail(G2048_ERR_INVALID, "NULL argument");
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, static_cast<hipStream_t>(stream)));
    G2048_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// ------------------------------------------------------------------------- host-resident I/O
static int ensure_host_io(g2048_engine *e)
{
    if (int rc = ensure_words(e)) // (the completion word)
        return rc;
    if (e->host_block)
        return G2048_OK;
    const size_t n = e->n;
    auto up = [](size_t x) { return (x + 63) & ~static_cast<size_t>(63); };
    const size_t off_act = 0, off_rew = up(off_act + 8 * n), off_term = up(off_rew + 4 * n), off_ill = up(off_term + n),
                 off_high = up(off_ill + n), off_boards = up(off_high + n), off_tb = up(off_boards + 16 * n),
                 off_sc = up(off_tb + 16 * n), bytes = up(off_sc + 4 * n);
    if (int rc = e->host_block.alloc(bytes, "the host-resident I/O arrays"))
        return rc;
    auto fill = [&](g2048_host_io &io, char *b) {
        io.actions = reinterpret_cast<int64_t *>(b + off_act);
        io.reward = reinterpret_cast<float *>(b + off_rew);
        io.terminated = reinterpret_cast<uint8_t *>(b + off_term);
        io.illegal = reinterpret_cast<uint8_t *>(b + off_ill);
        io.highest = reinterpret_cast<uint8_t *>(b + off_high);
        io.boards = reinterpret_cast<uint8_t *>(b + off_boards);
        io.terminal_boards = reinterpret_cast<uint8_t *>(b + off_tb);
        io.scores = reinterpret_cast<int32_t *>(b + off_sc);
    };
    fill(e->host_io, static_cast<char *>(e->host_block.host));
    fill(e->host_io_dev, static_cast<char *>(e->host_block.dev));
    return G2048_OK;
}

// A launch whose completion the host will POLL for must really execute: on a capturing stream it would only be
// recorded and the poll would never end.
static int refuse_capture(hipStream_t s, const char *what)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return G2048_OK; // cannot tell (e.g. legacy stream semantics): go on
    }
    if (st != hipStreamCaptureStatusNone)
        return fail(G2048_ERR_INVALID, "%s blocks until the device has finished; it cannot be used on a capturing stream", what);
    return G2048_OK;
}

static double wait_limit_seconds()
{
    static const double limit = [] {
        const char *v = std::getenv("G2048_WAIT_TIMEOUT_S");
        const double x = v ? std::atof(v) : 0.0;
        return x > 0.0 ? x : 120.0;
    }();
    return limit;
}

// Poll the completion word (published by the device with system-scope release; tickets on one stream only grow) until
// it reaches `want`.  Liveness: after ~2 s without the word the stream is queried every ~2 s -- a failed stream ends the
// wait with its error, a stream that has drained without publishing is a bug and says so -- and an overall deadline
// (G2048_WAIT_TIMEOUT_S, default 120 s) returns an error instead of spinning forever on a hung device.
static int wait_done(g2048_engine *e, unsigned long long want, hipStream_t s)
{
    using clock = std::chrono::steady_clock;
    clock::time_point started{}, last_check{};
    bool armed = false;
    const unsigned long long *done = host_word(e, kDoneWord);
    for (uint64_t spins = 0;; ++spins) {
        if (__atomic_load_n(done, __ATOMIC_ACQUIRE) >= want)
            return G2048_OK;
        cpu_relax();
        if ((spins & 0xfffffu) == 0xfffffu) { // every ~million polls
            const clock::time_point now = clock::now();
            if (!armed) {
                armed = true;
                started = last_check = now;
            } else if (now - last_check > std::chrono::seconds(2)) {
                last_check = now;
                const hipError_t q = hipStreamQuery(s);
                if (q == hipSuccess) // everything on the stream has finished: the word must be there
                    return __atomic_load_n(done, __ATOMIC_ACQUIRE) >= want
                               ? G2048_OK
                               : fail(G2048_ERR_HIP, "the device finished without publishing the completion word");
                if (q != hipErrorNotReady)
                    return fail(G2048_ERR_HIP, "stream failed while the host was waiting for the device: %s", hipGetErrorString(q));
                if (std::chrono::duration<double>(now - started).count() > wait_limit_seconds())
                    return fail(G2048_ERR_HIP, "no completion after %.0f s (G2048_WAIT_TIMEOUT_S): the device looks hung",
                                wait_limit_seconds());
            }
        }
    }
}

int g2048_host_io_map(g2048_engine *e, g2048_host_io *out)
{
    if (int rc = usable(e))
        return rc;
    if (!out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    G2048_HIP(hipSetDevice(e->device));
    if (int rc = ensure_host_io(e))
        return rc;
    *out = e->host_io;
    return G2048_OK;
}

int g2048_step_host(g2048_engine *e, int auto_reset, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!e->host_block)
        return fail(G2048_ERR_INVALID, "call g2048_host_io_map first (the actions are read from its buffer)");
    G2048_HIP(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = refuse_capture(s, "g2048_step_host"))
        return rc;
    if (e->strict_actions) { // the actions are HOST memory here: refused before anything is stepped
        const int64_t *acts = e->host_io.actions;
        for (uint64_t i = 0; i < e->n; ++i)
            if (acts[i] < 0 || acts[i] > 3)
                return fail(G2048_ERR_INVALID, "strict actions: action %lld of board %llu is outside 0..3 (game2048_env.py:49 "
                                               "Discrete(4)); nothing was stepped",
                            static_cast<long long>(acts[i]), static_cast<unsigned long long>(e->board_offset + i));
    }
    const g2048_host_io &d = e->host_io_dev;
    g2048_step_io io{};
    io.actions = d.actions;
    io.action_dtype = G2048_ACT_I64;
    io.reward = d.reward;
    io.terminated = d.terminated;
    io.illegal = d.illegal;
    io.highest = d.highest;
    io.terminal_boards = d.terminal_boards;
    io.boards_out = d.boards;
    e->t += 1;
    e->fresh = 0;
    g2048::StepArgs a = make_args(e, &io, auto_reset);
    const unsigned long long want = ++e->done_count;
    if (e->st.rng) { // numpy-RNG mode: step (+ compacted resets), then boards + scores + the completion word
        a.boards_out = nullptr;
        G2048_HIP(g2048::launch_step(a, io.action_dtype, s));
        G2048_HIP(g2048::launch_fetch(e->st.boards, a.n, reinterpret_cast<uint4 *>(d.boards), d.scores, dev_word(e, kDoneWord), want, s));
    } else {
        a.done_seq = dev_word(e, kDoneWord);
        a.done_value = want;
        G2048_HIP(g2048::launch_step(a, io.action_dtype, s));
    }
    return wait_done(e, want, s);
}

int g2048_fetch_host(g2048_engine *e, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!e->host_block)
        return fail(G2048_ERR_INVALID, "call g2048_host_io_map first");
    G2048_HIP(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = refuse_capture(s, "g2048_fetch_host"))
        return rc;
    const unsigned long long want = ++e->done_count;
    G2048_HIP(g2048::launch_fetch(e->st.boards, static_cast<uint32_t>(e->n), reinterpret_cast<uint4 *>(e->host_io_dev.boards),
                                  e->host_io_dev.scores, dev_word(e, kDoneWord), want, s));
    return wait_done(e, want, s);
}

int g2048_stream_signal(g2048_engine *e, void *stream, uint64_t *ticket)
{
    if (int rc = usable(e))
        return rc;
    if (!ticket)
        return fail(G2048_ERR_INVALID, "NULL argument");
    G2048_HIP(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = refuse_capture(s, "g2048_stream_signal"))
        return rc;
    if (int rc = ensure_words(e))
        return rc;
    const unsigned long long want = ++e->done_count;
    G2048_HIP(g2048::launch_signal(dev_word(e, kDoneWord), want, s));
    *ticket = want;
    return G2048_OK;
}

int g2048_stream_wait(g2048_engine *e, uint64_t ticket, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!e->words || ticket == 0 || ticket > e->done_count)
        return fail(G2048_ERR_INVALID, "ticket %llu was not issued by g2048_stream_signal on this engine",
                    (unsigned long long)ticket);
    return wait_done(e, ticket, static_cast<hipStream_t>(stream));
}

// Is p device-accessible memory of this process (hipMalloc / torch tensor)?  Plain host memory is not
// known to the runtime and makes hipPointerGetAttributes fail.
static bool is_device_ptr(const void *p)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError(); // clear the sticky error of the failed query
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// Engine-less entry points (g2048_augment, g2048_canonicalize) launch on the device their buffers live on, whatever
// the caller's current device is, and put the caller's device back when they return.  Every buffer must be reachable
// from that one device: device or managed memory OF that device, or pinned / registered host memory (which has a
// device address everywhere).  Plain pageable host memory is refused.
struct DeviceScope {
    int previous = -1;
    ~DeviceScope()
    {
        if (previous >= 0)
            (void)hipSetDevice(previous);
    }
};

static int enter_device_of(DeviceScope &scope, const void *const *bufs, int n_bufs)
{
    int target = -1;
    for (int k = 0; k < n_bufs; ++k) {
        if (!bufs[k])
            continue;
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, bufs[k]) != hipSuccess) {
            (void)hipGetLastError();
            return fail(G2048_ERR_INVALID, "buffer %p is not memory the device can reach (pageable host memory?)", bufs[k]);
        }
        if (attr.type == hipMemoryTypeHost) {
            if (!attr.devicePointer)
                return fail(G2048_ERR_INVALID, "host buffer %p has no device address (allocate it pinned and mapped)", bufs[k]);
            continue; // reachable from every device
        }
        if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) // e.g. hipMemoryTypeUnregistered
            return fail(G2048_ERR_INVALID, "buffer %p is not memory the device can reach (pageable host memory?)", bufs[k]);
        if (target < 0)
            target = attr.device;
        else if (attr.device != target)
            return fail(G2048_ERR_INVALID, "buffers live on different devices (%d and %d)", target, attr.device);
    }
    int current = 0;
    G2048_HIP(hipGetDevice(&current));
    if (target >= 0 && target != current) {
        G2048_HIP(hipSetDevice(target));
        scope.previous = current;
    }
    return G2048_OK;
}

// The engine keeps RECORDS (cells + packed score deficit); the plain views -- board cells uint8[n][16] and int32[n]
// scores, `width` 16 and 4 bytes per board -- are produced / consumed by small kernels, `launch`ed on the caller's buffer
// when it is device memory (which needs `width`-byte alignment; stream-ordered, no synchronisation) and on the staging
// buffer with a synchronous copy when it is host memory.

// The checks every view transfer starts with; *device: `buf` is device memory.
static int view_entry(const g2048_engine *e, const void *buf, size_t width, const char *reads_last, bool *device)
{
    if (int rc = usable(e))
        return rc;
    if (!buf)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (reads_last)
        if (int rc = need_last_records(e, reads_last))
            return rc;
    G2048_HIP(hipSetDevice(e->device));
    *device = is_device_ptr(buf);
    if (*device && (reinterpret_cast<uintptr_t>(buf) & (width - 1)))
        return fail(G2048_ERR_INVALID, "device %s buffers must be %zu-byte aligned", width == 16 ? "board" : "score", width);
    return G2048_OK;
}

// `reads_last`: the name of an entry point whose view comes from the terminal records, which the engine must keep
static int export_view(const g2048_engine *ce, void *buf, size_t width, const char *reads_last, void *stream,
                       hipError_t (*launch)(const g2048_engine *e, void *view, hipStream_t s))
{
    g2048_engine *e = const_cast<g2048_engine *>(ce);
    bool device = false;
    if (int rc = view_entry(e, buf, width, reads_last, &device))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (device) {
        G2048_HIP(launch(e, buf, s));
        return G2048_OK; // device destination: ready in stream order
    }
    if (int rc = e->scratch.alloc(e->n * 16, "the host staging buffer"))
        return rc;
    G2048_HIP(launch(e, e->scratch.p, s));
    return copy_sync(e, buf, e->scratch.p, e->n * width, stream);
}

// `vet_host`: checks the values of a host buffer before anything is copied (NULL: none)
static int import_view(g2048_engine *e, const void *buf, size_t width, int (*vet_host)(const g2048_engine *e, const void *buf),
                       void *stream, hipError_t (*launch)(const g2048_engine *e, const void *view, hipStream_t s))
{
    bool device = false;
    if (int rc = view_entry(e, buf, width, nullptr, &device))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (device) {
        G2048_HIP(launch(e, buf, s));
        return G2048_OK;
    }
    if (vet_host)
        if (int rc = vet_host(e, buf))
            return rc;
    if (int rc = e->scratch.alloc(e->n * 16, "the host staging buffer"))
        return rc;
    if (int rc = copy_sync(e, e->scratch.p, buf, e->n * width, stream))
        return rc;
    G2048_HIP(launch(e, e->scratch.p, s));
    G2048_HIP(hipStreamSynchronize(s)); // the staging buffer must be free again when this returns
    return G2048_OK;
}

// a record holds a score of 24 bits
static int vet_scores(const g2048_engine *e, const void *buf)
{
    const int32_t *scores = static_cast<const int32_t *>(buf);
    for (uint64_t i = 0; i < e->n; ++i)
        if (scores[i] < 0 || scores[i] > 0x00ffffff)
            return fail(G2048_ERR_INVALID, "score %d of board %llu is outside 0 .. 2^24-1", scores[i], (unsigned long long)i);
    return G2048_OK;
}

int g2048_get_boards(const g2048_engine *e, uint8_t *buf, void *stream)
{
    return export_view(e, buf, 16, nullptr, stream, [](const g2048_engine *en, void *view, hipStream_t s) {
        return g2048::launch_export_boards(en->st.boards, static_cast<uint32_t>(en->n), static_cast<uint4 *>(view), s);
    });
}

int g2048_set_boards(g2048_engine *e, const uint8_t *buf, void *stream)
{
    return import_view(e, buf, 16, nullptr, stream, [](const g2048_engine *en, const void *view, hipStream_t s) {
        return g2048::launch_import_boards(en->st.boards, static_cast<uint32_t>(en->n), static_cast<const uint4 *>(view), s);
    });
}

int g2048_get_scores(const g2048_engine *e, int32_t *buf, void *stream)
{
    return export_view(e, buf, 4, nullptr, stream, [](const g2048_engine *en, void *view, hipStream_t s) {
        return g2048::launch_export_scores(en->st.boards, static_cast<uint32_t>(en->n), static_cast<int32_t *>(view), s);
    });
}

int g2048_set_scores(g2048_engine *e, const int32_t *buf, void *stream)
{
    return import_view(e, buf, 4, vet_scores, stream, [](const g2048_engine *en, const void *view, hipStream_t s) {
        return g2048::launch_import_scores(en->st.boards, static_cast<uint32_t>(en->n), static_cast<const int32_t *>(view),
                                           en->st.ep_counters, s);
    });
}

int g2048_get_last_scores(const g2048_engine *e, int32_t *buf, void *stream)
{
    return export_view(e, buf, 4, "g2048_get_last_scores", stream, [](const g2048_engine *en, void *view, hipStream_t s) {
        return g2048::launch_export_last_scores(en->st, static_cast<uint32_t>(en->n), static_cast<int32_t *>(view), s);
    });
}

void *g2048_records_ptr(const g2048_engine *e) { return e ? e->st.boards : nullptr; }
void *g2048_last_records_ptr(const g2048_engine *e) { return e && e->track_last ? e->st.last_record : nullptr; }

int g2048_episode_stats(const g2048_engine *e, g2048_stats *out, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    G2048_HIP(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    G2048_HIP(g2048::launch_stats(tracked_state(e), static_cast<uint32_t>(e->n), e->stats_partials, e->summary_scratch, e->stats_dev, false, s));
    g2048::StatsOut h{};
    G2048_HIP(hipMemcpyAsync(&h, e->stats_dev, sizeof h, hipMemcpyDeviceToHost, s));
    G2048_HIP(hipStreamSynchronize(s));
    out->episodes = h.episodes;
    out->illegal_ends = h.illegal_ends;
    out->last_count = h.last_count;
    out->last_score_sum = static_cast<int64_t>(h.last_score_sum);
    out->last_score_max = h.last_score_max;
    out->max_exp = h.max_exp;
    for (int k = 0; k < 32; ++k)
        out->highest_hist[k] = h.highest_hist[k];
    out->return_sum = h.return_sum;
    return G2048_OK;
}

static int stats_async(const g2048_engine *e, g2048_stats *device_out, bool returns_only, void *stream)
{
    static_assert(sizeof(g2048_stats) == sizeof(g2048::StatsOut), "g2048_stats and the kernel's StatsOut must share one layout");
    if (int rc = usable(e))
        return rc;
    if (!device_out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (!is_device_ptr(device_out))
        return fail(G2048_ERR_INVALID, "the asynchronous statistics need a DEVICE buffer (use g2048_episode_stats for a host struct)");
    G2048_HIP(hipSetDevice(e->device));
    G2048_HIP(g2048::launch_stats(tracked_state(e), static_cast<uint32_t>(e->n), e->stats_partials, e->summary_scratch,
                                  reinterpret_cast<g2048::StatsOut *>(device_out),
                                  returns_only, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_episode_stats_async(const g2048_engine *e, g2048_stats *device_out, void *stream)
{
    return stats_async(e, device_out, false, stream);
}

int g2048_returns_summary_async(const g2048_engine *e, g2048_stats *device_out, void *stream)
{
    return stats_async(e, device_out, true, stream);
}

// numpy-RNG mode on: the planes' owner and the launchers' flag, st.rng, are set together
static int ensure_numpy_rng(g2048_engine *e)
{
    if (int rc = e->rng.alloc(g2048::numpy_rng_bytes(e->n), "the numpy-RNG planes"))
        return rc;
    e->st.rng = e->rng.as<uint64_t>();
    return G2048_OK;
}

int g2048_set_numpy_rng(g2048_engine *e, const uint64_t *planes, void *stream)
{
    if (int rc = usable(e))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    if (!planes) { // back to the spawn stream: the owner and the flag are cleared together
        e->st.rng = nullptr;
        G2048_HIP(e->rng.reset());
        return G2048_OK;
    }
    if (int rc = ensure_numpy_rng(e))
        return rc;
    return copy_sync(e, e->st.rng, planes, e->n * 40, stream);
}

int g2048_seed_numpy(g2048_engine *e, uint64_t base_seed, void *stream)
{
    if (int rc = g2048_seed(e, base_seed, stream))
        return rc;
    if (int rc = ensure_numpy_rng(e))
        return rc;
    G2048_HIP(g2048::launch_seed_numpy(e->st.rng, static_cast<uint32_t>(e->n), base_seed + e->board_offset,
                                       static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

int g2048_get_numpy_rng(const g2048_engine *e, uint64_t *planes, void *stream)
{
    if (!e || !e->st.rng)
        return fail(G2048_ERR_INVALID, "engine is not in numpy-RNG mode");
    return copy_sync(e, planes, e->st.rng, e->n * 40, stream);
}

int g2048_augment(const uint8_t *boards, const uint8_t *next_boards, const uint8_t *actions, uint64_t n,
                  uint8_t *boards_out, uint8_t *next_out, uint8_t *actions_out, void *stream)
{
    if (!boards || !actions || !boards_out || !actions_out || (next_boards && !next_out))
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (n > 0x1fffffffull)
        return fail(G2048_ERR_INVALID, "n too large");
    if (n == 0)
        return G2048_OK;
    DeviceScope scope;
    const void *bufs[] = {boards, next_boards, actions, boards_out, next_out, actions_out};
    if (int rc = enter_device_of(scope, bufs, 6))
        return rc;
    G2048_HIP(g2048::launch_augment(reinterpret_cast<const uint4 *>(boards), reinterpret_cast<const uint4 *>(next_boards),
                                    actions, static_cast<uint32_t>(n), reinterpret_cast<uint4 *>(boards_out),
                                    reinterpret_cast<uint4 *>(next_out), actions_out, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

uint64_t g2048_state_bytes(const g2048_engine *e)
{
    return e ? sizeof(StateHeader) + e->game_bytes + (e->st.rng ? e->n * 40 : 0) : 0;
}

int g2048_get_state(const g2048_engine *e, void *host_buf, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!host_buf)
        return fail(G2048_ERR_INVALID, "NULL argument");
    StateHeader h{kStateMagic, e->n, e->seed, e->board_offset, e->t, e->fresh, e->max_exp, e->illegal_reward,
                  (e->st.rng ? 1u : 0u) | (e->track_last ? 0u : 2u)}; // flags: 1 = numpy-RNG planes follow, 2 = no terminal records
    std::memcpy(host_buf, &h, sizeof h);
    char *body = static_cast<char *>(host_buf) + sizeof h;
    if (int rc = copy_sync(e, body, e->slab.p, e->kept_bytes, stream))
        return rc;
    std::memset(body + e->kept_bytes, 0, e->game_bytes - e->kept_bytes); // the engine's work memory is not state
    if (e->st.rng)
        return copy_sync(e, body + e->game_bytes, e->st.rng, e->n * 40, stream);
    return G2048_OK;
}

int g2048_set_state(g2048_engine *e, const void *host_buf, uint64_t blob_bytes, void *stream)
{
    if (int rc = usable(e))
        return rc;
    if (!host_buf)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (blob_bytes < sizeof(StateHeader))
        return fail(G2048_ERR_INVALID, "state blob is too short (%llu bytes)", (unsigned long long)blob_bytes);
    StateHeader h;
    std::memcpy(&h, host_buf, sizeof h);
    if (h.magic != kStateMagic || h.n != e->n)
        return fail(G2048_ERR_INVALID, "state blob does not match this engine (magic %llx%s, n %llu vs %llu)",
                    (unsigned long long)h.magic, h.magic == 0x3376383430324700ull ? " = a blob written before ABI 14: its games were played "
                    "under the old spawn rule and cannot be continued under this one" :
                    (h.magic == 0x3476383430324700ull ? " = a blob written by ABI 14: same games, another slab layout -- save it again "
                    "with g2048_get_boards / g2048_get_scores and re-create" : ""),
                    (unsigned long long)h.n, (unsigned long long)e->n);
    const uint64_t want = sizeof(StateHeader) + e->game_bytes + ((h.reserved & 1u) ? e->n * 40 : 0);
    if (blob_bytes != want)
        return fail(G2048_ERR_INVALID, "state blob is %llu bytes, this engine's state is %llu",
                    (unsigned long long)blob_bytes, (unsigned long long)want);
    if (h.max_exp > 31u || h.board_offset + h.n > 0x100000000ull)
        return fail(G2048_ERR_INVALID, "state blob header is corrupt (max_exp %u, board_offset %llu)", h.max_exp,
                    (unsigned long long)h.board_offset);
    e->seed = h.seed;
    e->board_offset = h.board_offset;
    e->t = h.t;
    e->fresh = h.fresh;
    e->max_exp = h.max_exp;
    e->illegal_reward = h.illegal_reward;
    e->track_last = (h.reserved & 2u) ? 0 : 1;
    const char *body = static_cast<const char *>(host_buf) + sizeof h;
    if (int rc = copy_sync(e, e->slab.p, body, e->kept_bytes, stream)) // (what follows in the game region is ignored)
        return rc;
    if (h.reserved & 1u) // the blob carries numpy-RNG planes
        return g2048_set_numpy_rng(e, reinterpret_cast<const uint64_t *>(body + e->game_bytes), stream);
    return g2048_set_numpy_rng(e, nullptr, stream);
}

int g2048_canonicalize(uint8_t *boards, uint8_t *next_boards, uint8_t *actions, uint64_t n, uint8_t *symmetry_out,
                       void *stream)
{
    if (!boards)
        return fail(G2048_ERR_INVALID, "boards is NULL");
    if (n > 0xffffff00ull)
        return fail(G2048_ERR_INVALID, "n too large");
    if ((reinterpret_cast<uintptr_t>(boards) | reinterpret_cast<uintptr_t>(next_boards)) & 15u)
        return fail(G2048_ERR_INVALID, "board buffers must be 16-byte aligned");
    if (n == 0)
        return G2048_OK;
    DeviceScope scope;
    const void *bufs[] = {boards, next_boards, actions, symmetry_out};
    if (int rc = enter_device_of(scope, bufs, 4))
        return rc;
    G2048_HIP(g2048::launch_canonicalize(reinterpret_cast<uint4 *>(boards), reinterpret_cast<uint4 *>(next_boards), actions,
                                         static_cast<uint32_t>(n), symmetry_out, static_cast<hipStream_t>(stream)));
    return G2048_OK;
}

// ------------------------------------------------------------------------------- collective
// The path's only exchange step: the all-gather of episodic returns (scores of last_record) once per rollout.
// RCCL is bound lazily (dlopen) so that the library loads, and everything else works, on a box without
// RCCL or without a GPU; a process that never calls g2048_comm_* never touches it.
} // extern "C"

namespace {

struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

Rccl g_rccl;
std::mutex g_rccl_mutex;

int load_rccl()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.handle)
        return G2048_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *nm : names) {
        h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
        if (h)
            break;
    }
    if (!h)
        return fail(G2048_ERR_HIP, "cannot load RCCL (librccl.so): %s", dlerror());
    Rccl r;
    r.handle = h;
#define G2048_SYM(field, name)                                                                                 \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(h, name));                                             \
    if (!r.field)                                                                                              \
        return fail(G2048_ERR_HIP, "RCCL has no symbol %s", name);
    G2048_SYM(GetUniqueId, "ncclGetUniqueId")
    G2048_SYM(CommInitRank, "ncclCommInitRank")
    G2048_SYM(CommInitAll, "ncclCommInitAll")
    G2048_SYM(CommDestroy, "ncclCommDestroy")
    G2048_SYM(AllGather, "ncclAllGather")
    G2048_SYM(GroupStart, "ncclGroupStart")
    G2048_SYM(GroupEnd, "ncclGroupEnd")
    G2048_SYM(GetErrorString, "ncclGetErrorString")
#undef G2048_SYM
    g_rccl = r;
    return G2048_OK;
}

#define G2048_NCCL(call)                                                                                       \
    do {                                                                                                       \
        ncclResult_t r_ = (call);                                                                              \
        if (r_ != ncclSuccess)                                                                                 \
            return fail(G2048_ERR_HIP, "%s failed: %s", #call, g_rccl.GetErrorString(r_));                      \
    } while (0)

} // namespace

struct g2048_comm {
    ncclComm_t comm = nullptr;
    int world = 0, rank = 0, device = 0;
};

struct g2048_comm_local {
    int n = 0;
    int devices[G2048_COMM_LOCAL_MAX] = {};
    ncclComm_t comms[G2048_COMM_LOCAL_MAX] = {};
};

extern "C" {

int g2048_comm_unique_id(uint8_t id[G2048_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) <= G2048_COMM_ID_BYTES, "ncclUniqueId does not fit G2048_COMM_ID_BYTES");
    if (!id)
        return fail(G2048_ERR_INVALID, "id is NULL");
    if (int rc = load_rccl())
        return rc;
    ncclUniqueId u;
    G2048_NCCL(g_rccl.GetUniqueId(&u));
    std::memset(id, 0, G2048_COMM_ID_BYTES);
    std::memcpy(id, &u, sizeof u);
    return G2048_OK;
}

int g2048_comm_create(int world, int rank, const uint8_t id[G2048_COMM_ID_BYTES], int device, g2048_comm **out)
{
    if (!out || !id)
        return fail(G2048_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world)
        return fail(G2048_ERR_INVALID, "rank %d / world %d out of range", rank, world);
    if (int rc = load_rccl())
        return rc;
    G2048_HIP(hipSetDevice(device));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    g2048_comm *c = new (std::nothrow) g2048_comm;
    if (!c)
        return fail(G2048_ERR_NOMEM, "out of host memory");
    c->world = world;
    c->rank = rank;
    c->device = device;
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(G2048_ERR_HIP, "ncclCommInitRank failed: %s", g_rccl.GetErrorString(r));
    }
    *out = c;
    return G2048_OK;
}

int g2048_comm_destroy(g2048_comm *c)
{
    if (!c)
        return G2048_OK;
    ncclResult_t r = c->comm ? g_rccl.CommDestroy(c->comm) : ncclSuccess;
    delete c;
    if (r != ncclSuccess)
        return fail(G2048_ERR_HIP, "ncclCommDestroy failed: %s", g_rccl.GetErrorString(r));
    return G2048_OK;
}

int g2048_allgather_returns(const g2048_engine *ce, g2048_comm *c, int32_t *out, void *stream)
{
    g2048_engine *e = const_cast<g2048_engine *>(ce);
    if (int rc = usable(e))
        return rc;
    if (!c || !out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (c->device != e->device)
        return fail(G2048_ERR_INVALID, "communicator is on device %d, engine on device %d", c->device, e->device);
    if (int rc = need_last_records(e, "g2048_allgather_returns"))
        return rc;
    G2048_HIP(hipSetDevice(e->device));
    if (int rc = e->returns.alloc(e->n * 4, "the all-gather send buffer"))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the returns are the scores of last_record: materialise int32[n] in the engine's send buffer, then ONE
    // all-gather (equal shards: rank r's n returns land at out[r * n]), all on the caller's stream
    int32_t *send = e->returns.as<int32_t>();
    G2048_HIP(g2048::launch_export_last_scores(e->st, static_cast<uint32_t>(e->n), send, s));
    G2048_NCCL(g_rccl.AllGather(send, out, e->n, ncclInt32, c->comm, s));
    return G2048_OK;
}

int g2048_allgather_summary(const g2048_engine *e, g2048_comm *c, g2048_stats *out, void *stream)
{
    static_assert(sizeof(g2048_stats) % 8 == 0, "g2048_stats is shipped as uint64 words");
    if (int rc = usable(e))
        return rc;
    if (!c || !out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    if (c->device != e->device)
        return fail(G2048_ERR_INVALID, "communicator is on device %d, engine on device %d", c->device, e->device);
    if (!is_device_ptr(out))
        return fail(G2048_ERR_INVALID, "g2048_allgather_summary needs a DEVICE buffer of `world` g2048_stats");
    G2048_HIP(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // this rank's summary goes straight into ITS row of the gathered array (one launch), then ONE in-place all-gather of
    // sizeof(g2048_stats) bytes per rank on the same stream: no send buffer, no stream hop, nothing for the host to wait for
    g2048_stats *mine = out + c->rank;
    G2048_HIP(g2048::launch_stats(tracked_state(e), static_cast<uint32_t>(e->n), e->stats_partials, e->summary_scratch,
                                  reinterpret_cast<g2048::StatsOut *>(mine), true, s));
    G2048_NCCL(g_rccl.AllGather(mine, out, sizeof(g2048_stats) / 8, ncclUint64, c->comm, s));
    return G2048_OK;
}

int g2048_comm_world(const g2048_comm *c) { return c ? c->world : 0; }
int g2048_comm_rank(const g2048_comm *c) { return c ? c->rank : -1; }

int g2048_comm_local_create(const int *devices, int n_devices, g2048_comm_local **out)
{
    if (!devices || !out)
        return fail(G2048_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_devices < 1 || n_devices > G2048_COMM_LOCAL_MAX)
        return fail(G2048_ERR_INVALID, "n_devices %d out of range 1..%d", n_devices, G2048_COMM_LOCAL_MAX);
    for (int a = 0; a < n_devices; ++a)
        for (int b = a + 1; b < n_devices; ++b)
            if (devices[a] == devices[b])
                return fail(G2048_ERR_INVALID, "device %d listed twice: one communicator per device", devices[a]);
    if (int rc = load_rccl())
        return rc;
    g2048_comm_local *c = new (std::nothrow) g2048_comm_local;
    if (!c)
        return fail(G2048_ERR_NOMEM, "out of host memory");
    c->n = n_devices;
    for (int r = 0; r < n_devices; ++r)
        c->devices[r] = devices[r];
    const ncclResult_t res = g_rccl.CommInitAll(c->comms, n_devices, c->devices); // the expensive part: done ONCE
    if (res != ncclSuccess) {
        delete c;
        return fail(G2048_ERR_HIP, "ncclCommInitAll failed: %s", g_rccl.GetErrorString(res));
    }
    *out = c;
    return G2048_OK;
}

int g2048_comm_local_destroy(g2048_comm_local *c)
{
    if (!c)
        return G2048_OK;
    ncclResult_t first = ncclSuccess;
    for (int r = 0; r < c->n; ++r) {
        const ncclResult_t res = c->comms[r] ? g_rccl.CommDestroy(c->comms[r]) : ncclSuccess;
        if (res != ncclSuccess && first == ncclSuccess)
            first = res;
    }
    delete c;
    if (first != ncclSuccess)
        return fail(G2048_ERR_HIP, "ncclCommDestroy failed: %s", g_rccl.GetErrorString(first));
    return G2048_OK;
}

int g2048_allgather_returns_local(g2048_comm_local *c, g2048_engine *const *engines, int32_t *const *outs,
                                  void *const *streams)
{
    if (!c || !engines || !outs)
        return fail(G2048_ERR_INVALID, "NULL argument");
    const int n_engines = c->n;
    for (int r = 0; r < n_engines; ++r) {
        if (!engines[r] || !outs[r])
            return fail(G2048_ERR_INVALID, "engine or output %d is NULL", r);
        if (engines[r]->device != c->devices[r])
            return fail(G2048_ERR_INVALID, "engine %d is on device %d, the communicator's slot %d on device %d", r,
                        engines[r]->device, r, c->devices[r]);
        if (int rc = need_last_records(engines[r], "g2048_allgather_returns_local"))
            return rc;
        if (engines[r]->n != engines[0]->n)
            return fail(G2048_ERR_INVALID, "engines must hold equal shards (engine %d has %llu boards, engine 0 %llu)", r,
                        (unsigned long long)engines[r]->n, (unsigned long long)engines[0]->n);
    }
    for (int r = 0; r < n_engines; ++r) {
        G2048_HIP(hipSetDevice(c->devices[r]));
        if (int rc = engines[r]->returns.alloc(engines[r]->n * 4, "the all-gather send buffer"))
            return rc;
        G2048_HIP(g2048::launch_export_last_scores(engines[r]->st, static_cast<uint32_t>(engines[r]->n), engines[r]->returns.as<int32_t>(),
                                                   static_cast<hipStream_t>(streams ? streams[r] : nullptr)));
    }
    ncclResult_t res = g_rccl.GroupStart();
    for (int r = 0; r < n_engines && res == ncclSuccess; ++r) {
        if (hipSetDevice(c->devices[r]) != hipSuccess) {
            res = ncclUnhandledCudaError;
            break;
        }
        res = g_rccl.AllGather(engines[r]->returns.as<int32_t>(), outs[r], engines[r]->n, ncclInt32, c->comms[r],
                               static_cast<hipStream_t>(streams ? streams[r] : nullptr));
    }
    const ncclResult_t end = g_rccl.GroupEnd();
    if (res == ncclSuccess)
        res = end;
    if (res != ncclSuccess)
        return fail(G2048_ERR_HIP, "RCCL all-gather failed: %s", g_rccl.GetErrorString(res));
    return G2048_OK; // enqueued: outs[r] is complete when streams[r] reaches this point
}

} // extern "C"
