// sqy_capi.cpp -- the C-ABI of libsqeazy_amd.so (include/sqeazy_amd.h) and the stage sequencing on the GPU.
//
// Mirrors src/cpp/src/sqeazy.cpp:16-335 (entry points) and dynamic_pipeline.hpp:560-690 (encode:
// header, head filters, sink, tail filters, header rewrite), with every stage a HIP kernel launch on
// device-resident ping-pong buffers instead of an OpenMP loop over host memory.
#include "../../include/sqeazy_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sqy_batch_window.hpp"
#include "sqy_kernels.h"
#include "sqy_lanes.hpp"
#include "sqy_pipeline.hpp"

namespace {


using sqy::Pipeline;
using sqy::Stage;
using sqy::StageKind;

#define SQY_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            std::fprintf(stderr, "[sqeazy]\t HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

// ---- run-time options ------------------------------------------------------------------------------
// Measurement / test switches.  The environment is read ONCE, when the library is loaded (getenv in the middle of a call races with
// setenv from other host threads); afterwards they change only through SQYAMD_Set_Option (atomics).  None of them changes a byte of
// any result -- except host_l2_bytes, which stands for a value the reference reads off the host CPU and is a parameter of rmestbkrd.
long env_flag(const char* name) { const char* v = std::getenv(name); return v && *v && std::strcmp(v, "0") != 0 ? 1 : 0; }
long env_number(const char* name, long dflt, long lo, long hi)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    char* end = nullptr;
    const long long x = std::strtoll(v, &end, 10);
    if (*end != '\0' || x < lo || x > hi) {
        std::fprintf(stderr, "[sqeazy]\t %s=%s is not a number in [%ld, %ld]: ignored\n", name, v, lo, hi);
        return dflt;
    }
    return (long)x;
}
constexpr long kWarmupMax = 1l << 30;
constexpr long kStageLanesDefault = 2, kParseLanesDefault = 3;      // (measured: DESIGN.md section 5)
constexpr long kBatchBytesMax = (1l << 32) - 1, kBatchGroupBytesDefault = 1l << 30;
constexpr long kBatchJointMaxDefault = 128l << 20;                 // (the batch encode sweep: the largest size swept)
constexpr uint64_t kSlabsGroupBytes = 4ull << 30;                  // slab-set and batch decode: LZ4 output of one group (slabs: inflight <= 0; batch: the option's default and maximum)
struct Options {
    std::atomic<long> transpose_chain;                  // the bit-plane transposes of calls in flight on LIBRARY-OWNED streams run one after the other
    std::atomic<long> transpose_chain_caller_streams;   // .. on streams the callers bring as well (opt-in: couples those streams, see the bitswap1 stage)
    std::atomic<long> block_parallel;                   // block-linked frames: block-parallel encode and decode (0: the one-wavefront walk)
    std::atomic<long> block_parallel_warmup;            // bytes parsed in front of a block to guess its table
    std::atomic<long> block_parallel_stats;             // print the blocks that failed the table check
    std::atomic<long> tail_scan;                        // serial-layout decode: the walk over the tails as a scan
    std::atomic<long> decode_two_waves;                 // chunked-layout decode: two wavefronts per frame (one parses, one copies)
    std::atomic<long> noise_digest;                     // frames in place: the transpose leaves the noise digest, the parse proves noise chunks empty from it
    std::atomic<long> transpose_tiles_per_wave;         // frames in place: tiles one wavefront of the transposer takes (sizes its grid)
    std::atomic<long> stored_tail_index;                // decode, chunked layout: the stored frames at the stream's end are found where they must start, not by the scan
    std::atomic<long> host_l2_bytes;                    // rmestbkrd: the host CPU's L2 size as the reference's compass reads it (detected; tests set it)
    std::atomic<long> decode_frames_subset;             // frame-range decode: only the LZ4 frames the range needs, where the pipeline allows (0: full decode + copy)
    std::atomic<long> decode_box_subset;                // box decode: only the LZ4 frames the box's z-range needs, where the pipeline allows (0: full decode + window copy)
    std::atomic<long> decode_boxes_joint;               // many boxes of one blob: the frames united, one output launch for all boxes (0: the single-box driver box by box)
    std::atomic<long> compare_boxes_subset;             // compare of many boxes of one blob: only the LZ4 frames the boxes' z-ranges need, the comparing range transposer or one compare in the compaction, where sqy::compare_boxes_path allows (0: the blob decoded whole once, one window compare)
    std::atomic<long> project_boxes_walk;               // projection along axis 0 on the transposer path: the z-walking form (registers, plain stores) where every box is on the 32-voxel grid (0: always the atomics -- same images)
    std::atomic<long> project_boxes_subset;             // projection of many boxes of one blob: only the LZ4 frames the boxes' z-ranges need, the projecting range transposer or one projection in the compaction, where sqy::project_boxes_path allows (0: the blob decoded whole once, one projection launch)
    std::atomic<long> bin_boxes_subset;                 // binned read of many boxes of one blob: only the LZ4 frames the boxes' z-ranges need, the binning job-table kernel (a workgroup per block of cells, LDS accumulators) or one per-cell launch in the compaction, where sqy::bin_boxes_path allows (0: the blob decoded whole once, one per-cell launch)
    std::atomic<long> pyramid_boxes_subset;             // pyramid of many boxes of one blob: only the LZ4 frames the boxes' z-ranges need, decoded once for all levels, where sqy::pyramid_boxes_path allows (0: the blob decoded whole once)
    std::atomic<long> pyramid_boxes_fused;              // .. all fused levels from one pass over the planes, the levels above them (and every further level of the copy forms) by ONE pyramid_reduce launch (0: level 0 by Bin_Boxes' launch, every further level by a pyramid_reduce launch from the level below -- same outputs)
    std::atomic<long> histogram_boxes_subset;           // histograms of many boxes of one blob: only the LZ4 frames the boxes' z-ranges need, the counting range transposer or one window histogram in the compaction, where sqy::histogram_boxes_path allows (0: the blob decoded whole once, one window histogram)
    std::atomic<long> histogram_boxes_merge;            // how the histogram kernels add equal neighbours: 2 a piece of sixteen bytes whose bins are all equal in one LDS atomic, 1 equal consecutive voxels of a thread's whole run in one, 0 one per voxel -- same counts
    std::atomic<long> update_box_subset;                // box update of one blob: only the LZ4 frames the box's z-range needs are decoded, patched, parsed again and spliced between the old ones, where sqy::update_box_path allows (0: whole decode, one paste, the single call's encode)
    std::atomic<long> update_boxes_subset;              // update of many boxes of one blob: update_box_subset's stages, each once for all boxes (0: the blob decoded whole once, the pastes layer by layer, the single call's encode)
    std::atomic<long> decode_slabs_joint;               // slab-set decode: the chunked LZ4 blobs of a group indexed and decoded by one launch each (0: blob by blob)
    std::atomic<long> decode_batch_joint;               // batch decode: the joint-eligible blobs of a group indexed, decoded and transposed back by one launch each (0: blob by blob)
    std::atomic<long> decode_batch_group_bytes;         // .. the LZ4 output one group holds at most (a group holds at least one blob)
    std::atomic<long> encode_batch_joint;               // batch encode: the joint-eligible volumes of a group share one launch of every kernel (0: volume by volume)
    std::atomic<long> encode_batch_group_bytes;         // .. the LZ4 input one group holds at most (a group holds at least one volume)
    std::atomic<long> encode_batch_joint_max_bytes;     // .. a volume with more LZ4 input than this is encoded on its own (frames in place)
    std::atomic<long> batch_strided_fused;              // strided views: the transposers gather from / scatter into the view, `lz4` packs into the stream and unpacks from the LZ4 output (0: packed copies everywhere)
    std::atomic<long> batch_window_fused;               // windows: the inverse transposer stores only the window's voxels, `lz4` windows are copied out of the LZ4 output (0: every blob decoded dense, one window copy)
    std::atomic<long> batch_update_fused;               // window updates: `bitswap1->lz4` blobs written as `bitswap1->lz4` keep their planes, the window is patched into them; kept planes and `lz4` blobs are LZ4-decoded straight into their places (0: every blob decoded dense by the batch decode's launches, one paste)
    std::atomic<long> batch_compare_fused;              // window compares: the inverse transposer compares the window's voxels with the view's where it would store them, `lz4` windows are compared in the LZ4 output (0: every blob decoded dense, one compare launch)
    std::atomic<long> stage_lanes;                      // frames-in-place calls on caller streams run on the library's lanes: 0 never, 1 always, 2 where transpose_chain_caller_streams is on
    std::atomic<long> parse_lanes;                      // .. how many parse lanes a device has (1-8)
    // counters (Get reads, Set takes 0 only): calls that ran on the lanes; calls that stayed on their caller's stream because it had a
    // backlog; .. because an idle lane did not answer (a foreign kernel in front of it in its hardware queue)
    std::atomic<long> lane_calls{0}, lane_backlog_fallbacks{0}, lane_blocked_fallbacks{0};
    std::atomic<long> call_stamps{0};                   // host time stamps per encode call (SQYAMD_Call_Stamps); off: a call pays one relaxed load
    std::atomic<long> dedupe_report{0};                 // the duplicate search's keys and decisions of the newest call (SQYAMD_Dedupe_Report); off: one relaxed load
    Options()
        : transpose_chain(env_flag("SQY_NO_TRANSPOSE_CHAIN") ? 0 : 1), transpose_chain_caller_streams(env_flag("SQY_TRANSPOSE_CHAIN_CALLER_STREAMS")),
          block_parallel(env_flag("SQY_NO_BLOCK_PARALLEL") ? 0 : 1), block_parallel_warmup(env_number("SQY_BLOCK_PARALLEL_WARMUP", 65536, 0, kWarmupMax)),
          block_parallel_stats(env_flag("SQY_BLOCK_PARALLEL_STATS")), tail_scan(env_flag("SQY_NO_TAIL_SCAN") ? 0 : 1),
          decode_two_waves(env_flag("SQY_NO_DECODE_TWO_WAVES") ? 0 : 1), noise_digest(env_flag("SQY_NO_NOISE_DIGEST") ? 0 : 1),
          transpose_tiles_per_wave(env_number("SQY_TRANSPOSE_TILES_PER_WAVE", sqy::kBitswap1TilesPerWave, 1, 64)), stored_tail_index(env_flag("SQY_NO_STORED_TAIL_INDEX") ? 0 : 1),
          host_l2_bytes((long)sqy::host_l2_cache_bytes()), decode_frames_subset(env_flag("SQY_NO_DECODE_FRAMES_SUBSET") ? 0 : 1),
          decode_box_subset(env_flag("SQY_NO_DECODE_BOX_SUBSET") ? 0 : 1), decode_boxes_joint(env_flag("SQY_NO_DECODE_BOXES_JOINT") ? 0 : 1),
          compare_boxes_subset(env_flag("SQY_NO_COMPARE_BOXES_SUBSET") ? 0 : 1),
          project_boxes_walk(env_flag("SQY_NO_PROJECT_BOXES_WALK") ? 0 : 1), project_boxes_subset(env_flag("SQY_NO_PROJECT_BOXES_SUBSET") ? 0 : 1),
          bin_boxes_subset(env_flag("SQY_NO_BIN_BOXES_SUBSET") ? 0 : 1), pyramid_boxes_subset(env_flag("SQY_NO_PYRAMID_BOXES_SUBSET") ? 0 : 1),
          pyramid_boxes_fused(env_flag("SQY_NO_PYRAMID_BOXES_FUSED") ? 0 : 1), histogram_boxes_subset(env_flag("SQY_NO_HISTOGRAM_BOXES_SUBSET") ? 0 : 1),
          histogram_boxes_merge(env_flag("SQY_NO_HISTOGRAM_BOXES_MERGE") ? 0 : 2), update_box_subset(env_flag("SQY_NO_UPDATE_BOX_SUBSET") ? 0 : 1),
          update_boxes_subset(env_flag("SQY_NO_UPDATE_BOXES_SUBSET") ? 0 : 1),
          decode_slabs_joint(env_flag("SQY_NO_DECODE_SLABS_JOINT") ? 0 : 1), decode_batch_joint(env_flag("SQY_NO_DECODE_BATCH_JOINT") ? 0 : 1),
          decode_batch_group_bytes(env_number("SQY_DECODE_BATCH_GROUP_BYTES", (long)kSlabsGroupBytes, 1, (long)kSlabsGroupBytes)), encode_batch_joint(env_flag("SQY_NO_ENCODE_BATCH_JOINT") ? 0 : 1),
          encode_batch_group_bytes(env_number("SQY_ENCODE_BATCH_GROUP_BYTES", kBatchGroupBytesDefault, 1, kBatchBytesMax)),
          encode_batch_joint_max_bytes(env_number("SQY_ENCODE_BATCH_JOINT_MAX_BYTES", kBatchJointMaxDefault, 0, kBatchBytesMax)),
          batch_strided_fused(env_flag("SQY_NO_BATCH_STRIDED_FUSED") ? 0 : 1), batch_window_fused(env_flag("SQY_NO_BATCH_WINDOW_FUSED") ? 0 : 1),
          batch_update_fused(env_flag("SQY_NO_BATCH_UPDATE_FUSED") ? 0 : 1), batch_compare_fused(env_flag("SQY_NO_BATCH_COMPARE_FUSED") ? 0 : 1), stage_lanes(env_number("SQY_STAGE_LANES", kStageLanesDefault, 0, 2)),
          parse_lanes(env_number("SQY_PARSE_LANES", kParseLanesDefault, 1, sqy::LanePicker::kMaxLanes)) { sqy::set_bitswap1_tiles_per_wave(transpose_tiles_per_wave.load()); }
    std::atomic<long>* find(const char* name)
    {
        if (!name) return nullptr;
        if (!std::strcmp(name, "transpose_chain")) return &transpose_chain;
        if (!std::strcmp(name, "transpose_chain_caller_streams")) return &transpose_chain_caller_streams;
        if (!std::strcmp(name, "block_parallel")) return &block_parallel;
        if (!std::strcmp(name, "block_parallel_warmup")) return &block_parallel_warmup;
        if (!std::strcmp(name, "block_parallel_stats")) return &block_parallel_stats;
        if (!std::strcmp(name, "tail_scan")) return &tail_scan;
        if (!std::strcmp(name, "decode_two_waves")) return &decode_two_waves;
        if (!std::strcmp(name, "noise_digest")) return &noise_digest;
        if (!std::strcmp(name, "transpose_tiles_per_wave")) return &transpose_tiles_per_wave;
        if (!std::strcmp(name, "stored_tail_index")) return &stored_tail_index;
        if (!std::strcmp(name, "host_l2_bytes")) return &host_l2_bytes;
        if (!std::strcmp(name, "decode_frames_subset")) return &decode_frames_subset;
        if (!std::strcmp(name, "decode_box_subset")) return &decode_box_subset;
        if (!std::strcmp(name, "decode_boxes_joint")) return &decode_boxes_joint;
        if (!std::strcmp(name, "compare_boxes_subset")) return &compare_boxes_subset;
        if (!std::strcmp(name, "project_boxes_subset")) return &project_boxes_subset;
        if (!std::strcmp(name, "project_boxes_walk")) return &project_boxes_walk;
        if (!std::strcmp(name, "bin_boxes_subset")) return &bin_boxes_subset;
        if (!std::strcmp(name, "pyramid_boxes_subset")) return &pyramid_boxes_subset;
        if (!std::strcmp(name, "pyramid_boxes_fused")) return &pyramid_boxes_fused;
        if (!std::strcmp(name, "histogram_boxes_subset")) return &histogram_boxes_subset;
        if (!std::strcmp(name, "histogram_boxes_merge")) return &histogram_boxes_merge;
        if (!std::strcmp(name, "update_box_subset")) return &update_box_subset;
        if (!std::strcmp(name, "update_boxes_subset")) return &update_boxes_subset;
        if (!std::strcmp(name, "decode_slabs_joint")) return &decode_slabs_joint;
        if (!std::strcmp(name, "decode_batch_joint")) return &decode_batch_joint;
        if (!std::strcmp(name, "decode_batch_group_bytes")) return &decode_batch_group_bytes;
        if (!std::strcmp(name, "encode_batch_joint")) return &encode_batch_joint;
        if (!std::strcmp(name, "encode_batch_group_bytes")) return &encode_batch_group_bytes;
        if (!std::strcmp(name, "encode_batch_joint_max_bytes")) return &encode_batch_joint_max_bytes;
        if (!std::strcmp(name, "batch_strided_fused")) return &batch_strided_fused;
        if (!std::strcmp(name, "batch_window_fused")) return &batch_window_fused;
        if (!std::strcmp(name, "batch_update_fused")) return &batch_update_fused;
        if (!std::strcmp(name, "batch_compare_fused")) return &batch_compare_fused;
        if (!std::strcmp(name, "stage_lanes")) return &stage_lanes;
        if (!std::strcmp(name, "parse_lanes")) return &parse_lanes;
        if (!std::strcmp(name, "lane_calls")) return &lane_calls;
        if (!std::strcmp(name, "lane_backlog_fallbacks")) return &lane_backlog_fallbacks;
        if (!std::strcmp(name, "lane_blocked_fallbacks")) return &lane_blocked_fallbacks;
        if (!std::strcmp(name, "call_stamps")) return &call_stamps;
        if (!std::strcmp(name, "dedupe_report")) return &dedupe_report;
        return nullptr;
    }
};
Options g_opt;

// ---- call stamps ---------------------------------------------------------------------------------
// Where the host side of an encode call spends its time (option "call_stamps", read back through SQYAMD_Call_Stamps): the steady
// clock at seven places of the call, the call's place in the order of the transpose lane and the parse lane it took.  Together with
// a kernel trace of the same run this splits a call's cycle into what the device did and what it waited for
// (tools/inflight_timeline.py).  The last kStampRing calls are kept.
struct CallStamps {
    enum { entry, lanes_taken, clear_launched, transpose_launched, parse_queued, sync_returned, returned, kStamps };
    long seq = -1;                      // n-th call on the transpose lane since the counters were reset (-1: the call did not take the lanes)
    long lane = -1;                     // its parse lane
    long thread = 0;                    // the calling thread (a hash of its id: which calls follow each other)
    long ns[kStamps] = {};
    void stamp(int i) { ns[i] = (long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};
constexpr size_t kStampRing = 8192;
std::mutex g_stamps_mu;
std::vector<CallStamps> g_stamps;       // a ring once it holds kStampRing records
size_t g_stamps_next = 0;
// One call's record: stamped at entry, and put into the ring when it goes out of scope -- declared in front of the call's context
// lease, so that the last stamp is taken when the context has gone back to the pool.
struct StampScope {
    CallStamps rec;
    const bool on;
    StampScope() : on(g_opt.call_stamps.load(std::memory_order_relaxed) != 0) 
    {
        if (!on) return;
        rec.stamp(CallStamps::entry);
        rec.thread = (long)(std::hash<std::thread::id>()(std::this_thread::get_id()) & 0x7fffffff);
    }
    CallStamps* get() { return on ? &rec : nullptr; }
    ~StampScope()
    {
        if (!on) return;
        rec.stamp(CallStamps::returned);
        std::lock_guard<std::mutex> lock(g_stamps_mu);
        if (g_stamps.size() < kStampRing) g_stamps.push_back(rec);
        else { g_stamps[g_stamps_next] = rec; g_stamps_next = (g_stamps_next + 1) % kStampRing; }
    }
};

// ---- dedupe report -------------------------------------------------------------------------------
// What the duplicate-chunk search of the newest chunked encode call decided (option "dedupe_report", read back through
// SQYAMD_Dedupe_Report): the key of every full chunk and dup_of of every chunk, as the kernels left them in the call's workspace.
// A missed duplicate does not show in the blob (equal chunks compress to equal frames) and a key is only worth testing against
// when it is the kernels' own: tests/dedupe_collisions.py.
struct DedupeReport {
    std::vector<uint64_t> keys;         // one per FULL chunk
    std::vector<uint32_t> dup_of;       // one per chunk (a ragged last chunk is its own)
};
std::mutex g_dedupe_report_mu;
DedupeReport g_dedupe_report;

// ---- per-kernel timing -------------------------------------------------------------------------
struct ProfEntry { std::string name; double ms = 0; long launches = 0; };
struct PendingEvent { const char* name; hipEvent_t a, b; };
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
std::vector<ProfEntry> g_prof;

// Timing events are pooled (created once, reused by every later call): creating and destroying two events per kernel cost the
// calls of a profiled run tens of microseconds of host time each.
std::mutex g_evpool_mu;
std::vector<hipEvent_t> g_evpool[16];           // per device (an event belongs to the device it was created on)
int ev_dev()
{
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 16) ? d : -1;
}
hipEvent_t ev_take()
{
    const int d = ev_dev();
    if (d >= 0) {
        std::lock_guard<std::mutex> lock(g_evpool_mu);
        if (!g_evpool[d].empty()) { hipEvent_t e = g_evpool[d].back(); g_evpool[d].pop_back(); return e; }
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
void ev_give(hipEvent_t e)
{
    if (!e) return;
    const int d = ev_dev();
    if (d < 0) { hipEventDestroy(e); return; }
    std::lock_guard<std::mutex> lock(g_evpool_mu);
    g_evpool[d].push_back(e);
}

struct ProfScope {
    hipStream_t s;
    PendingEvent ev{};
    std::vector<PendingEvent>* sink;
    bool on;
    ProfScope(const char* name, hipStream_t stream, std::vector<PendingEvent>* pending) : s(stream), sink(pending), on(g_prof_on.load())
    {
        if (!on) return;
        ev.name = name;
        ev.a = ev_take(); ev.b = ev_take();
        if (!ev.a || !ev.b) { ev_give(ev.a); ev_give(ev.b); on = false; return; }
        hipEventRecord(ev.a, s);
    }
    ~ProfScope()
    {
        if (!on) return;
        hipEventRecord(ev.b, s);
        sink->push_back(ev);
    }
};

// one launch (an expression of type hipError_t), timed under `name` when profiling is on; `stream` and `pend` are the call's
#define SQY_TIMED(name, launch)                                                                         \
    do {                                                                                                \
        ProfScope ps_(name, stream, pend);                                                              \
        SQY_HIP(launch);                                                                                \
    } while (0)

void prof_add(const char* name, double ms)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    size_t i = 0;
    for (; i < g_prof.size(); ++i) if (g_prof[i].name == name) break;
    if (i == g_prof.size()) g_prof.push_back(ProfEntry{name, 0, 0});
    g_prof[i].ms += ms;
    g_prof[i].launches += 1;
}

// a launch that is counted, not timed (no events next to a kernel of a few microseconds in front of a call's transpose)
void prof_count(const char* name) { if (g_prof_on.load()) prof_add(name, 0); }

void prof_collect(std::vector<PendingEvent>& pending)
{
    for (PendingEvent& p : pending) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) prof_add(p.name, ms);
        ev_give(p.a);
        ev_give(p.b);
    }
    pending.clear();
}

// ---- HBM workspace (grow-only; one per leased context) ------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    // quiet: an OPTIONAL buffer (the caller has a path that needs none and says which) -- no message from here
    int ensure(size_t bytes, bool quiet = false)
    {
        if (bytes <= cap) return 0;
        if (p) { hipFree(p); p = nullptr; cap = 0; }
        const size_t want = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
        if (hipMalloc(&p, want) != hipSuccess) {
            if (!quiet) std::fprintf(stderr, "[sqeazy]\t unable to allocate %zu bytes of HBM workspace\n", want);
            (void)hipGetLastError();          // (not left behind for the launch checks of a caller that carries on without this buffer)
            p = nullptr;
            return 1;
        }
        cap = want;
        return 0;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};

// pinned host memory (grow-only), for read-backs of more than the context's 4 KiB
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return 0;
        if (p) { hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = (bytes + ((size_t)1 << 16) - 1) & ~(((size_t)1 << 16) - 1);
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            std::fprintf(stderr, "[sqeazy]\t unable to allocate %zu bytes of pinned host memory\n", want);
            (void)hipGetLastError();
            p = nullptr;
            return 1;
        }
        cap = want;
        return 0;
    }
    void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
};

struct Workspace {
    DevBuf ping, pong, lz4_scratch, csize, frame_off, io_src, io_dst, small, plan, dedupe;
    DevBuf spec;              // block-linked frames parsed block-parallel: per block the table it started from and the one it left, the walk lists
    DevBuf diff_side;         // diff3x3x1 in front of a 16-bit bitswap1: the columns the stage can touch (outside the ping/pong rotation)
    DevBuf digest;            // frames in place: the noise digest the transpose leaves for the LZ4 parse (19 KB per 256 KiB chunk)
    DevBuf bkrd;              // rmestbkrd: the four face histograms and their supports
    DevBuf subset;            // frame-range decode: the frame list, the subset's block index, the frame_shuffle map of the range
    DevBuf range_full;        // frame-range decode of a blob the subset path does not take: the whole volume, the range copied out
    DevBuf box_window;        // box decode: the job and tile table of the window copy (one job)
    DevBuf update_box;        // box update, the whole path: the single call's new blob before it is held against the caller's capacity and copied out
    DevBuf boxes_jobs;        // decode of many boxes of one blob: the job and tile table of its one output launch
    DevBuf pyramid_jobs[sqy::kPyramidMaxLevels];      // pyramid of many boxes of one blob: the job and tile tables of its pyramid_reduce launches (the first launch's are in boxes_jobs)
    DevBuf slabs_index;       // slab-set decode: every blob's frame ranking (scratch, block index, counts) of a group
    DevBuf slabs_joint;       // .. the group's joint block index, frame output table, part descriptors and frame_shuffle maps
    DevBuf slabs_out;         // .. the group's LZ4 output (when it does not go straight to the volume)
    HostBuf slabs_host;       // .. the blobs' header prefixes and the ranking's counts, read back
    DevBuf batch_stream;      // batch encode: the LZ4 input of a group's volumes (the bit planes), one stream behind the other
    DevBuf batch_scratch;     // .. a slot of compressed output per entry of the group's joint chunk table
    DevBuf batch_tables;      // .. the tables a group uploads (chunks, volumes, transposer jobs, header text) and what the kernels hand each other
    DevBuf batch_quant;       // .. quantiser->bitswap1->lz4: every volume's histogram, then every encode LUT, then every decode LUT
    HostBuf batch_host;       // .. the records of every volume, the staging area of the upload
    DevBuf batch_pack;        // strided views: the packed copies of a group's views (encode), the dense places of a call's views (decode)
    DevBuf batch_pack_one;    // .. decode: the dense place of a view whose blob is decoded on its own
    DevBuf batch_views[3];    // .. the job and tile tables of the view launches: pack / unpack, the strided transposer, the strided copy
    DevBuf batch_windows[4];  // .. and of the window launches: the window copy, the windowed transposer, the copy out of the LZ4 output, the paste
    DevBuf batch_compares[3]; // window compares: the job and tile tables of the compare launch, the comparing transposer, the compare in the LZ4 output
    DevBuf batch_records;     // .. a record of eight 64-bit words per blob
    DevBuf batch_update;      // window updates: every old blob's place (decoded dense, or its plane stream), on the 256-byte grid
    DevBuf batch_patch_jobs;  // .. the job and tile tables of a group's patch launch
    DevBuf batch_places;      // packed batch encode: the places a group's placement scan leaves for the gather, behind them its gap table
    DevBuf batch_packed;      // .. a slot of max_compressed_length for every volume outside the joint forms, copied to its place at the end
    void* pinned = nullptr;   // 4 KiB of pinned host memory for small read-backs
    void release_buffers()
    {
        ping.release(); pong.release(); lz4_scratch.release(); csize.release(); frame_off.release();
        io_src.release(); io_dst.release(); small.release(); plan.release(); dedupe.release(); diff_side.release(); spec.release(); digest.release(); bkrd.release();
        subset.release(); range_full.release(); box_window.release(); update_box.release(); boxes_jobs.release(); for (DevBuf& b : pyramid_jobs) b.release(); slabs_index.release(); slabs_joint.release(); slabs_out.release(); slabs_host.release();
        batch_stream.release(); batch_scratch.release(); batch_tables.release(); batch_quant.release(); batch_host.release();
        batch_pack.release(); batch_pack_one.release(); for (DevBuf& b : batch_views) b.release(); for (DevBuf& b : batch_windows) b.release();
        for (DevBuf& b : batch_compares) b.release();
        batch_records.release(); batch_update.release(); batch_patch_jobs.release();
        batch_places.release(); batch_packed.release();
    }
};

// A context = one HBM workspace + one private stream.  Concurrent C-ABI calls (the reference is re-entrant:
// every call builds its own pipeline object, src/sqeazy.cpp:123) each lease their own context, so two host
// threads encoding different volumes overlap on the GPU instead of queueing behind a lock.
// Host <-> HBM transfers of the reference-protocol entry points (caller memory is pageable).  A plain hipMemcpy from
// pageable memory runs at 5-6 GB/s; here kLanes host threads each own two pinned staging buffers and a copy stream:
// memcpy user -> pinned slice k while the DMA of slice k-1 is in flight, slices dealt round-robin to the lanes.
struct Stager {
    static constexpr int kLanes = 4;
    static constexpr size_t kSlice = 8u << 20;
    char* pin[kLanes][2] = {};
    hipStream_t st[kLanes] = {};
    hipEvent_t ev[kLanes][2] = {};
    bool ready = false;

    bool init()
    {
        if (ready) return true;
        for (int l = 0; l < kLanes; ++l) {
            if (hipStreamCreateWithFlags(&st[l], hipStreamNonBlocking) != hipSuccess) return false;
            for (int b = 0; b < 2; ++b) {
                if (hipHostMalloc((void**)&pin[l][b], kSlice, hipHostMallocDefault) != hipSuccess) return false;
                if (hipEventCreateWithFlags(&ev[l][b], hipEventDisableTiming) != hipSuccess) return false;
            }
        }
        ready = true;
        return true;
    }
    // to_device: dev <- host;  else host <- dev.  Blocks until the bytes have arrived.  `after` (optional) is a stream
    // whose work must be complete before device memory is read (D2H of freshly computed data).
    bool copy(void* dev, void* host, size_t bytes, bool to_device, int device_id)
    {
        if (bytes == 0) return true;
        if (!init()) return false;
        const size_t nslices = (bytes + kSlice - 1) / kSlice;
        std::atomic<bool> ok(true);
        auto lane_fn = [&](int l) {
            if (hipSetDevice(device_id) != hipSuccess) { ok = false; return; }
            int b = 0;
            size_t pending_off[2] = {0, 0}, pending_len[2] = {0, 0};
            for (size_t k = (size_t)l; k < nslices && ok; k += kLanes, b ^= 1) {
                const size_t off = k * kSlice, len = std::min(kSlice, bytes - off);
                // the buffer's previous transfer must be over before it is reused
                if (hipEventSynchronize(ev[l][b]) != hipSuccess) { ok = false; break; }
                if (to_device) {
                    std::memcpy(pin[l][b], static_cast<char*>(host) + off, len);
                    if (hipMemcpyAsync(static_cast<char*>(dev) + off, pin[l][b], len, hipMemcpyHostToDevice, st[l]) != hipSuccess) { ok = false; break; }
                } else {
                    if (pending_len[b]) std::memcpy(static_cast<char*>(host) + pending_off[b], pin[l][b], pending_len[b]);
                    if (hipMemcpyAsync(pin[l][b], static_cast<char*>(dev) + off, len, hipMemcpyDeviceToHost, st[l]) != hipSuccess) { ok = false; break; }
                    pending_off[b] = off; pending_len[b] = len;
                }
                if (hipEventRecord(ev[l][b], st[l]) != hipSuccess) { ok = false; break; }
            }
            if (hipStreamSynchronize(st[l]) != hipSuccess) ok = false;
            if (!to_device && ok)
                for (int bb = 0; bb < 2; ++bb)
                    if (pending_len[bb]) std::memcpy(static_cast<char*>(host) + pending_off[bb], pin[l][bb], pending_len[bb]);
        };
        const int lanes = (int)std::min<size_t>(kLanes, nslices);
        std::vector<std::thread> th;
        for (int l = 1; l < lanes; ++l) th.emplace_back(lane_fn, l);
        lane_fn(0);
        for (auto& t : th) t.join();
        return ok;
    }
};

struct Context {
    Workspace ws;
    // Streams are created on first use, not with the context: HIP deals streams to a handful of hardware queues in creation
    // order, and a caller that brings its own streams (one per host thread) should not find two of them behind the same queue
    // because this library created streams of its own in between -- their kernels would then never overlap (bench, three
    // callers: 750 instead of 1120 GB/s in about every other process).
    hipStream_t stream = nullptr;       // used when the caller brings no stream (host-pointer entry points)
    hipStream_t side = nullptr;         // decode: stored frames are copied here while the compressed ones are decoded
    hipEvent_t fork = nullptr, join = nullptr;
    hipEvent_t t_done = nullptr;        // recorded behind this call's bit-plane transpose (the transposes of calls in flight run one after the other)
    hipEvent_t lane_t = nullptr;        // a call that takes the lanes: recorded behind its transpose on the transpose lane, its parse lane waits for it
    hipEvent_t lane_p = nullptr;        // .. the liveness marker on its parse lane (lane_t serves as the transpose lane's)
    bool ensure_lane_event()
    {
        if (!lane_p && hipEventCreateWithFlags(&lane_p, hipEventDisableTiming) != hipSuccess) { lane_p = nullptr; return false; }
        if (!lane_t && hipEventCreateWithFlags(&lane_t, hipEventDisableTiming) != hipSuccess) { lane_t = nullptr; return false; }
        return true;
    }
    hipStream_t own_stream()
    {
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) stream = nullptr;
        return stream;
    }
    bool ensure_side()
    {
        if (side && fork && join) return true;
        if (!side && hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { side = nullptr; return false; }
        if (!fork && hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) { fork = nullptr; return false; }
        if (!join && hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess) { join = nullptr; return false; }
        return true;
    }
    std::vector<PendingEvent> pending;
    Stager stager;
    bool busy = false;
};

constexpr int kMaxDev = 16;
constexpr size_t kMaxCtxPerDev = 8;
// the chain of the bit-plane transposes of the calls in flight on one device (see the bitswap1 stage): the event behind the last
// transpose launched, and when that was
std::mutex g_tchain_mu[kMaxDev];
hipEvent_t g_tchain_last[kMaxDev] = {};
std::chrono::steady_clock::time_point g_tchain_when[kMaxDev];
// The lanes of one device (round 7): streams of the library's own on which the frames-in-place calls that callers make on streams of
// THEIRS run.  The runtime deals streams to the few hardware queues a process gets; kernels of two streams behind one queue never
// overlap, so with one caller stream per call in flight it is the callers' number of streams, not the work, that decides what runs
// side by side.  On lanes it is the library's: ONE transpose lane (the clear + bit-plane transpose of every such call, in call order
// -- the serial order the event chain below expresses between streams, without an event) and `parse_lanes` parse lanes (everything
// behind the transpose, on the lane with the fewest calls leased).  Created on first use and kept; plain non-blocking streams.
struct Lanes {
    std::mutex mu;                      // lane creation, the picker, and the launches onto the transpose lane
    hipStream_t transpose = nullptr;
    hipStream_t parse[sqy::LanePicker::kMaxLanes] = {};
    sqy::LanePicker picker;
    bool ensure(int lane)
    {
        if (!transpose && hipStreamCreateWithFlags(&transpose, hipStreamNonBlocking) != hipSuccess) { transpose = nullptr; return false; }
        if (!parse[lane] && hipStreamCreateWithFlags(&parse[lane], hipStreamNonBlocking) != hipSuccess) { parse[lane] = nullptr; return false; }
        return true;
    }
};
Lanes g_lanes[kMaxDev];
// how long a call polls for its caller's stream to arrive before it stays on that stream (see EncodeCall::take_lanes)
constexpr std::chrono::microseconds kLaneArrival(2000);
// how long an idle lane may take to answer a marker before it counts as blocked (an idle queue answers in 10-30 us)
constexpr std::chrono::microseconds kLaneAnswer(250);

// What one call holds of the lanes: its parse lane's lease (given back on every way out) and what it queued where (for the drain).
struct LaneLease {
    Lanes* lanes = nullptr;
    int lane = -1;
    hipStream_t transpose = nullptr, parse = nullptr;
    hipEvent_t t_done = nullptr;        // recorded behind the call's last launch on the transpose lane
    bool complete = false;              // the call has seen everything it queued on the lanes finish (EncodeCall::finish)
    bool taken() const { return lanes != nullptr; }
    // waits for what this call queued on the lanes -- not for other calls' transposes behind it on the transpose lane.  A call that
    // has synchronised with its parse lane behind its last launch has nothing left to wait for, and must not ask the lane again: by
    // then the NEXT call may have queued its kernels there (the picker sends it to the lane of the call that is about to finish), and
    // hipStreamSynchronize would wait for that call's whole parse -- one call in four did, 1.6 ms each.
    // Only the ways out that have not seen the lane finish (errors) wait here.
    void drain()
    {
        if (!lanes || complete) return;
        if (t_done) (void)hipEventSynchronize(t_done);
        else (void)hipStreamSynchronize(transpose);
        (void)hipStreamSynchronize(parse);
    }
    ~LaneLease()
    {
        if (!lanes) return;
        std::lock_guard<std::mutex> lock(lanes->mu);
        lanes->picker.give(lane);
    }
    LaneLease() = default;
    LaneLease(const LaneLease&) = delete;
    LaneLease& operator=(const LaneLease&) = delete;
};

std::mutex g_pool_mu;
std::condition_variable g_pool_cv;
std::vector<std::unique_ptr<Context>> g_pool[kMaxDev];

struct ContextLease {
    Context* ctx = nullptr;
    ContextLease()
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return;
        std::unique_lock<std::mutex> lock(g_pool_mu);
        for (;;) {
            for (auto& c : g_pool[dev]) if (!c->busy) { ctx = c.get(); break; }
            if (ctx) break;
            if (g_pool[dev].size() < kMaxCtxPerDev) {
                std::unique_ptr<Context> c(new Context());
                if (hipHostMalloc(&c->ws.pinned, 4096, hipHostMallocDefault) != hipSuccess) return;
                ctx = c.get();
                g_pool[dev].push_back(std::move(c));
                break;
            }
            g_pool_cv.wait(lock);
        }
        ctx->busy = true;
    }
    ~ContextLease()
    {
        if (!ctx) return;
        {
            std::lock_guard<std::mutex> lock(g_pool_mu);
            ctx->busy = false;
        }
        g_pool_cv.notify_one();
    }
    ContextLease(const ContextLease&) = delete;
    ContextLease& operator=(const ContextLease&) = delete;
};

// Every exit of an encode / decode -- the early error returns included -- leaves the stream idle before the context goes
// back to the pool: kernels and async copies still in flight would otherwise read host vectors that are being destroyed
// and HBM buffers the next call (on another stream) may reuse or free.  Timing events that nobody harvested are dropped.
struct DrainOnExit {
    hipStream_t s;
    std::vector<PendingEvent>* pending;
    hipStream_t side = nullptr;         // the context's side stream (decode)
    LaneLease* lanes = nullptr;         // encode: what the call queued on the library's lanes
    ~DrainOnExit()
    {
        // (a call on the lanes saw its caller's stream complete before it took them and has queued nothing there since)
        if (!lanes || !lanes->taken()) (void)hipStreamSynchronize(s);
        if (lanes) lanes->drain();
        if (side) (void)hipStreamSynchronize(side);
        if (!pending->empty()) {
            if (g_prof_on.load()) prof_collect(*pending);
            else { for (PendingEvent& p : *pending) { ev_give(p.a); ev_give(p.b); } pending->clear(); }
        }
    }
};

// The background filters' shapes, checked before anything is uploaded or launched (both are head filters: the volume's shape).
// rmestbkrd reads rows z = 1 and Z-2 (background_scheme_utils.hpp:86); rmbkrd_neighbor5x5x5 takes a row length from an offset its
// list may not have (sqy::neighbor5_geometry_defined).
bool background_geometry_ok(const Pipeline& pipe, const std::vector<uint64_t>& dims)
{
    for (const Stage& st : pipe.stages) {
        if (st.kind != StageKind::rmestbkrd && st.kind != StageKind::rmbkrd_neighbor5) continue;
        if (dims.size() != 3) {
            std::fprintf(stderr, "[sqeazy]\t %s: shape of rank %zu, the stage takes {Z, Y, X}; refused\n", st.name.c_str(), dims.size());
            return false;
        }
        if (st.kind == StageKind::rmestbkrd && dims[0] < 2) {
            std::fprintf(stderr, "[sqeazy]\t rmestbkrd: %llu frame(s); the reference reads frames 1 and Z-2 out of bounds; refused\n",
                         (unsigned long long)dims[0]);
            return false;
        }
        if (st.kind == StageKind::rmbkrd_neighbor5 && !sqy::neighbor5_geometry_defined(dims[0], dims[1], dims[2])) {
            std::fprintf(stderr, "[sqeazy]\t rmbkrd_neighbor5x5x5: shape %llux%llux%llu takes the reference's row length from an offset it does not "
                                 "have (X < 5, Y < 5, X = Y = 5, or a single centre row); refused\n",
                         (unsigned long long)dims[0], (unsigned long long)dims[1], (unsigned long long)dims[2]);
            return false;
        }
    }
    return true;
}

bool device_present()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// Multiplies the extents of a shape up to the first one that is not positive (then 0) or the first partial product of 2^31 or more (then
// that product).  One encode call takes [1, 2^31) voxels: the reference multiplies the extents into an `int` (dynamic_pipeline.hpp:565).
uint64_t voxel_count(const long* shape, unsigned rank)
{
    uint64_t n = 1;
    for (unsigned i = 0; i < rank; ++i) {
        if (shape[i] <= 0) return 0;
        n *= (uint64_t)shape[i];
        if (n >= ((uint64_t)1 << 31)) break;
    }
    return n;
}

// frame_shuffle's frame_chunk_size (frame_shuffle_scheme_impl.hpp:86-90); negative reads as 0, which both directions refuse
uint64_t frame_chunk_size(const Stage& st)
{
    auto c = st.cfg.find("frame_chunk_size");
    return c != st.cfg.end() ? (uint64_t)std::max(std::atoi(c->second.c_str()), 0) : 1;
}

// ---- encode --------------------------------------------------------------------------------------
// The body of dynamic_pipeline::encode (dynamic_pipeline.hpp:560-616) on device buffers.
// dstoffset == nullptr: the blob starts at d_dst.  Otherwise it may start anywhere inside [d_dst, d_dst + dst_capacity) and
// *dstoffset says where ("frames in place": a 16-bit bitswap1 in front of lz4 writes the plane stream straight into d_dst as
// the bodies of the LZ4 frames it will become; the stored frames that end the payload -- the noise planes, 98 % of the bytes of
// a microscopy stack -- then never move, only the compressed frames in front are gathered up against them).
// Where every `every`-th LZ4 frame of the payload starts (chunked layout): what a caller needs to re-order byte ranges of slab
// blobs into one blob (single-blob mode of the multi-GPU path) without walking the frames itself.
struct FrameQuery {
    int every = 0;              // 0: not asked for
    long* offsets = nullptr;    // out, relative to the blob start: frames 0, every, 2 every, ..; then the blob length
    int max_entries = 0;
    int count = 0;              // out: frames listed (the end entry comes on top)
};

// The frame descriptor of sqeazy's LZ4 frames: the FLG and BD bytes and the header checksum byte (lz4frame.c, LZ4F_headerChecksum)
struct Lz4Descriptor { unsigned char flg, bd; uint32_t hc; };
Lz4Descriptor lz4_descriptor(int block_id)
{
    const unsigned char fd[2] = {0x40, (unsigned char)(block_id << 4)};
    return {fd[0], fd[1], (sqy::xxh32(fd, 2, 0) >> 8) & 0xff};
}

// One encode call: where it runs, the stream between the stages, and what the stages hand each other.
struct EncodeCall {
    Context& cx;
    Workspace* ws;
    std::vector<PendingEvent>* pend;
    hipStream_t stream;                  // where the next launch goes: the stream the call was made on, or one of the library's lanes
    LaneLease* lanes;
    CallStamps* stamps;                  // nullptr: not asked for
    Pipeline pipe;
    std::vector<uint64_t> dims;
    uint64_t len;                        // voxels
    int elem_size;
    void* d_dst;
    uint64_t dst_capacity;
    long* dstoffset;                     // nullptr: the blob starts at d_dst
    FrameQuery* fq;

    // the stream between stages
    const uint8_t* cur;
    int cur_elem;                        // bytes per element
    uint64_t cur_len;                    // elements
    bool use_ping = true;

    // left for lz4 by the stages in front of it
    struct {
        sqy::Lz4DedupeLayout dedupe;            // 16-bit bitswap1: ws->dedupe holds hashes of the 1 KiB pieces of the plane stream (total != 0)
        sqy::Lz4InplacePlan place;              // frames in place: chunk k of the plane stream sits at d_dst + body0 + k * in_stride
        uint32_t* digest = nullptr;             // frames in place: the noise digest (sqy_kernels.h: launch_bitswap1_u16), digest_stride words per chunk
        uint32_t digest_stride = 0;
        sqy::Lz4TableClearPlan clear;           // frames in place: who empties the duplicate search's table and the dense list's counter
        bool dedupe_cleared = false;            // .. a launch that does so is queued (the clear kernel, or the transposer's): lz4 launches no fills
                                                // (set behind that launch's success only, and gone with the call: no context keeps it)
        const uint64_t* frame_map = nullptr;    // frame_shuffle directly in front: frames are read through the map
        uint64_t frame_bytes = 0;
    } prep;
    // left for a 16-bit bitswap1 by diff3x3x1 directly in front of it: only the columns the stage can touch (compact side buffer)
    struct DiffSide { const uint16_t* p = nullptr; uint32_t w = 0, X = 0; } side;
    // left for finish() by lz4
    struct {
        bool on = false;                        // the payload is LZ4 frames
        int block_id = 0;
        uint64_t total = 0, chunk = 0, nchunks = 0, stride = 0;
        const sqy::Lz4Block* blocks = nullptr;  // block-linked frames (nthreads == 1, or chunks of several LZ4 blocks): the block list in HBM
        const uint32_t* dup_of = nullptr;       // chunks that are byte-identical to an earlier chunk share its frame
        uint64_t* tail_info = nullptr;          // frames in place: the run of stored chunks that ends the payload
        bool inplace_done = false;              // frames in place, finished on the device: where the blob is
        uint64_t blob_at = 0, blob_bytes = 0, payload_bytes = 0;
    } lz4;

    EncodeCall(Context& c, hipStream_t s, Pipeline&& p, std::vector<uint64_t>&& d, uint64_t voxels, int elem, const void* src, void* dst,
               uint64_t capacity, long* offset, FrameQuery* frames, LaneLease* lane_lease, CallStamps* call_stamps)
        : cx(c), ws(&c.ws), pend(&c.pending), stream(s), lanes(lane_lease), stamps(call_stamps), pipe(std::move(p)), dims(std::move(d)), len(voxels), elem_size(elem), d_dst(dst),
          dst_capacity(capacity), dstoffset(offset), fq(frames), cur(static_cast<const uint8_t*>(src)), cur_elem(elem), cur_len(voxels) {}

    uint8_t* next_buf(size_t bytes)
    {
        DevBuf& b = use_ping ? ws->ping : ws->pong;
        use_ping = !use_ping;
        return b.ensure(bytes) ? nullptr : static_cast<uint8_t*>(b.p);
    }
    int produced(const uint8_t* out) { cur = out; return 0; }           // the stage's output is the next stage's input
    bool is_tail(size_t si) const { return pipe.sink_index >= 0 && (int)si > pipe.sink_index; }
    // the reference's 3-D schemes refuse other shapes (sqeazy::detail::<scheme>::encode)
    bool not_3d(const char* scheme) const
    {
        if (dims.size() != 3) std::fprintf(stderr, "[sqeazy::detail::%s::encode] received non-3D shape which is currently unsupported!\n", scheme);
        return dims.size() != 3;
    }
    bool followed_by(size_t si, StageKind k) const { return si + 1 < pipe.stages.size() && pipe.stages[si + 1].kind == k; }
    // the shape a 3-D stage sees: the volume's -- or, behind a sink that did not write one byte per voxel, {1, 1, bytes}
    // (dynamic_pipeline.hpp:658-666: the tail chain's "sinked_shape")
    void stage_shape(size_t si, uint64_t& Z, uint64_t& Y, uint64_t& X) const
    {
        const bool flat = is_tail(si) && cur_len * (uint64_t)cur_elem != len;
        Z = flat ? 1 : dims[0]; Y = flat ? 1 : dims[1]; X = flat ? cur_len : dims[2];
    }

    // Frames in place on a stream the caller brought: the rest of the call moves onto the library's lanes (option stage_lanes).
    // The call has to start behind everything queued on the caller's stream S at the time of the call.  A hipStreamWaitEvent on the
    // transpose lane would say so -- and make every transpose queued behind this one wait for S's backlog as well, the coupling of
    // callers' streams that transpose_chain_caller_streams is opt-in for.  So the wait is done HERE, on the calling thread (which
    // blocks until the call is complete anyway): S is polled (hipStreamQuery) until everything on it is complete, then the call
    // takes its place in the lane and needs no edge on the device at all.  Nothing is queued on S for that -- not even an event:
    // S may share its hardware queue with a parse lane, and a marker would sit there behind another call's whole parse (measured:
    // 0.65 instead of 0.60 ms per step).  A stream that has not arrived within kLaneArrival carries a backlog: that call
    // stays on S, as with stage_lanes = 0 (returns 0 with `stream` unchanged).  On success `lock` holds the device's lane mutex --
    // launches onto the transpose lane are in call order, and a timed kernel's two events enclose nothing of another call.
    int take_lanes(std::unique_lock<std::mutex>& lock)
    {
        // stage_lanes = 2 (default): only for callers who said that their streams carry nothing but these calls.  The lanes sit on ALL
        // of the process's hardware queues; a long foreign kernel on any caller stream then shares a queue with one of them and holds
        // up every call that uses that lane (measured: one call in three, or all of them when it is the transpose lane's queue) --
        // below the streams, where no poll sees it.  On its own stream a call meets such a kernel only when the runtime happens to
        // put the two streams behind one queue.
        const long mode = g_opt.stage_lanes.load();
        if (!lanes || mode == 0 || (mode == 2 && !g_opt.transpose_chain_caller_streams.load()) || (stream != nullptr && stream == cx.stream)) return 0;
        int devid = 0;
        if (hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= kMaxDev) return 0;
        if (!cx.ensure_lane_event()) { std::fprintf(stderr, "[sqeazy]\t no HIP event for the lanes\n"); return 1; }
        const auto deadline = std::chrono::steady_clock::now() + kLaneArrival;
        for (;;) {
            const hipError_t e = hipStreamQuery(stream);
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            if (e != hipErrorNotReady) { std::fprintf(stderr, "[sqeazy]\t HIP error %s while waiting for the caller's stream\n", hipGetErrorString(e)); return 1; }
            if (std::chrono::steady_clock::now() > deadline) { g_opt.lane_backlog_fallbacks += 1; return 0; }
            std::this_thread::yield();
        }
        Lanes& L = g_lanes[devid];
        lock = std::unique_lock<std::mutex>(L.mu);
        const int lane = L.picker.take((int)g_opt.parse_lanes.load());
        if (!L.ensure(lane)) {
            L.picker.give(lane);
            std::fprintf(stderr, "[sqeazy]\t no HIP stream for the lanes\n");
            return 1;
        }
        // Liveness.  The lanes share the process's hardware queues with the callers' streams, and a kernel waits for whatever is in
        // front of it in its QUEUE: a long kernel of the caller's own on some other stream holds up a lane without any stream saying
        // so.  When this call is the only one on the lanes (every lease but its own given back: nothing of the library's is in
        // flight there) an idle lane answers a marker at once; one that does not within kLaneAnswer has such a kernel in front, and
        // the call stays on its caller's stream.  With other calls on the lanes a marker would wait for THEIR kernels: not asked.
        if (L.picker.total() == 1) {
            const hipError_t r = hipEventRecord(cx.lane_t, L.transpose);
            if (r != hipSuccess || hipEventRecord(cx.lane_p, L.parse[lane]) != hipSuccess) { L.picker.give(lane); SQY_HIP(hipErrorUnknown); }
            lock.unlock();                                  // (calls that arrive now queue behind the markers)
            const auto answer_by = std::chrono::steady_clock::now() + kLaneAnswer;
            bool alive = false;
            for (;;) {
                const hipError_t et = hipEventQuery(cx.lane_t), ep = et == hipSuccess ? hipEventQuery(cx.lane_p) : et;
                if (et == hipSuccess && ep == hipSuccess) { alive = true; break; }
                (void)hipGetLastError();
                if (std::chrono::steady_clock::now() > answer_by) break;
                std::this_thread::yield();
            }
            lock.lock();
            if (!alive) {
                L.picker.give(lane);
                lock.unlock();
                g_opt.lane_blocked_fallbacks += 1;
                return 0;
            }
        }
        const long seq = g_opt.lane_calls.fetch_add(1);
        if (stamps) { stamps->seq = seq; stamps->lane = lane; stamps->stamp(CallStamps::lanes_taken); }
        lanes->lanes = &L;
        lanes->lane = lane;
        lanes->transpose = L.transpose;
        lanes->parse = L.parse[lane];
        stream = L.transpose;
        return 0;
    }
    // behind the call's last launch on the transpose lane: its parse lane waits for that, and takes the rest of the call
    int leave_transpose_lane(std::unique_lock<std::mutex>& lock)
    {
        SQY_HIP(hipEventRecord(cx.lane_t, stream));
        lanes->t_done = cx.lane_t;
        lock.unlock();
        stream = lanes->parse;
        SQY_HIP(hipStreamWaitEvent(stream, cx.lane_t, 0));
        return 0;
    }

    // The bit-plane transposes of the calls in flight on one device run one after the other (round 4): a stream waits for the
    // transpose of the call in front before it starts its own.  Two HBM-bound kernels side by side each run at half speed
    // and end together; chained, the first call's parse starts a whole transpose earlier (bench, four calls in flight:
    // +3 %; also chaining the duplicate search behind it: -12 %, measured and not kept).  Only a transpose launched within
    // the last few milliseconds is waited for.  The chain is an edge between streams: by default only streams this library
    // owns (the host-pointer entry points, the Slabs workers) are chained -- a stream the CALLER brings may carry work this
    // library knows nothing about (a backlog, a host function that waits for another of the caller's threads), and a hidden
    // wait on it would couple calls that are documented as independent (round-4 advice).  A caller whose streams carry
    // nothing but these calls opts in: SQYAMD_Set_Option("transpose_chain_caller_streams", 1) (bench.py does, and says so).
    // "transpose_chain" = 0 (or SQY_NO_TRANSPOSE_CHAIN=1 when the library is loaded) switches the chain off altogether.
    // (round 7) A call on the lanes needs none of this: its transpose is on the transpose lane, behind the one in front.
    struct TransposeChain {
        int devid = -1;                                     // -1: this call's transpose is not chained
        std::unique_lock<std::mutex> lock;                  // the device's chain, held from the wait to the record
    };
    // in front of the transpose's launch: waits for the transpose in front
    int chain_wait(TransposeChain& tc, bool inplace)
    {
        const bool owned = stream != nullptr && stream == cx.stream;
        int devid = 0;
        if ((lanes && lanes->taken()) || !g_opt.transpose_chain.load() || !(owned || g_opt.transpose_chain_caller_streams.load()) || !inplace ||
            hipGetDevice(&devid) != hipSuccess || devid < 0 || devid >= kMaxDev) return 0;
        if (!cx.t_done && hipEventCreateWithFlags(&cx.t_done, hipEventDisableTiming) != hipSuccess) return 1;
        tc.lock = std::unique_lock<std::mutex>(g_tchain_mu[devid]);
        const auto now = std::chrono::steady_clock::now();
        if (g_tchain_last[devid] && g_tchain_last[devid] != cx.t_done && now - g_tchain_when[devid] < std::chrono::milliseconds(5))
            SQY_HIP(hipStreamWaitEvent(stream, g_tchain_last[devid], 0));
        g_tchain_when[devid] = now;
        tc.devid = devid;
        return 0;
    }
    // behind it: this call's transpose is the one the next call waits for
    int chain_record(TransposeChain& tc)
    {
        if (tc.devid < 0) return 0;
        SQY_HIP(hipEventRecord(cx.t_done, stream));
        g_tchain_last[tc.devid] = cx.t_done;
        tc.lock.unlock();
        return 0;
    }

    // A 16-bit bitswap1 with lz4 right behind it leaves piece hashes for the duplicate-chunk search (bit planes of small values repeat)
    // and, where lz4_inplace_plan says so, writes the plane stream as frames in place.  Planned and allocated here; then the call takes
    // its lanes and clears the search's table in front of the transpose (one small kernel instead of three fill dispatches between the
    // kernels behind it).  Every allocation is in front of take_lanes: the lane mutex is held for launches only.
    int bitswap1_for_lz4(size_t si, std::unique_lock<std::mutex>& lane_lock)
    {
        const sqy::Lz4Params& lz = pipe.stages[si + 1].lz4;
        const sqy::Lz4EncodeLayout lay = sqy::lz4_encode_layout(lz, cur_len * 2, pipe.nthreads);
        const uint64_t words = sqy::bitswap1_piece_hash_words(cur, cur, cur_len);         // (0 unless whole tiles, 16-byte aligned input)
        prep.dedupe = sqy::lz4_dedupe_layout(lay, words);
        if (!prep.dedupe.total) return 0;
        if (ws->dedupe.ensure(prep.dedupe.total)) return 1;
        // room in front for the sqy header (its length depends on the payload size: take the longest)
        const uint64_t hdr_max = sqy::header_pack(elem_size, false, dims, pipe.name(), (uint64_t)INT_MAX).size() + 2;
        prep.place = sqy::lz4_inplace_plan(lay, words, si + 2 == pipe.stages.size(), dstoffset != nullptr,
                                           (unsigned)(reinterpret_cast<uintptr_t>(d_dst) & 15), dst_capacity, hdr_max);
        if (!prep.place.on) return 0;
        if (ws->plan.ensure((lay.nchunks + 1) * sizeof(uint32_t))) return 1;
        const uint32_t dstride = sqy::lz4_noise_digest_words(lz, lay, g_opt.noise_digest.load() != 0, cur_len / 8);      // (round 6)
        if (dstride && !ws->digest.ensure(lay.nchunks * (uint64_t)dstride * sizeof(uint32_t), true)) {
            prep.digest = static_cast<uint32_t*>(ws->digest.p);
            prep.digest_stride = dstride;
        }
        if (take_lanes(lane_lock)) return 1;
        // who empties the search's table: on the lanes the transposer's own launch (bitswap1 hands it prep.clear), else the clear kernel
        prep.clear = sqy::lz4_table_clear_plan(prep.dedupe, true, lanes && lanes->taken());
        if (prep.clear.who == sqy::Lz4TableClearPlan::kernel) {
            SQY_HIP(sqy::launch_lz4_dedupe_clear(ws->dedupe.p, prep.dedupe, static_cast<uint32_t*>(ws->plan.p), stream));
            prof_count("lz4_dedupe_clear");
            prep.dedupe_cleared = true;
        }
        if (stamps) stamps->stamp(CallStamps::clear_launched);            // (on the lanes: the place of the launch that is no longer there)
        return 0;
    }

    int bitswap1(size_t si)
    {
        std::unique_lock<std::mutex> lane_lock;             // (held from take_lanes to leave_transpose_lane, or to the first error return)
        if (cur_elem == 2 && followed_by(si, StageKind::lz4) && bitswap1_for_lz4(si, lane_lock)) return 1;
        const bool inplace = prep.place.on;
        uint8_t* out = inplace ? static_cast<uint8_t*>(d_dst) + prep.place.body0 : next_buf(cur_len * cur_elem);
        if (!out) return 1;
        if (!inplace && (reinterpret_cast<uintptr_t>(out) & 15)) prep.dedupe = sqy::Lz4DedupeLayout();     // (no piece hashes into such a buffer)
        uint32_t* ph = prep.dedupe.total ? static_cast<uint32_t*>(ws->dedupe.p) : nullptr;
        const bool on_lanes = lanes && lanes->taken();
        TransposeChain tc;
        if (chain_wait(tc, inplace)) return 1;
        if (cur_elem == 2) {
            sqy::Bitswap1Clear clr;
            if (inplace && prep.clear.who == sqy::Lz4TableClearPlan::transposer) {
                clr.table = static_cast<uint8_t*>(ws->dedupe.p) + prep.clear.table_at;
                clr.key_bytes = prep.clear.key_bytes;
                clr.bytes = prep.clear.bytes;
                clr.zero_word = static_cast<uint32_t*>(ws->plan.p);
            }
            SQY_TIMED("bitswap1_u16", sqy::launch_bitswap1_u16(reinterpret_cast<const uint16_t*>(cur), reinterpret_cast<uint16_t*>(out), cur_len, stream, ph,
                                                               inplace ? (uint32_t)prep.place.chunk : 0, side.p, side.w, side.X, inplace ? prep.digest : nullptr,
                                                               prep.digest_stride, &clr));
            if (clr.bytes) prep.dedupe_cleared = true;
        } else
            SQY_TIMED("bitswap1_u8", sqy::launch_bitswap1_u8(cur, out, cur_len, stream));
        if (chain_record(tc)) return 1;
        if (stamps) stamps->stamp(CallStamps::transpose_launched);
        if (on_lanes && leave_transpose_lane(lane_lock)) return 1;
        side = DiffSide();                      // (consumed: a later bitswap1 of the pipeline reads its plain input)
        return produced(out);
    }

    // raster_reorder and zcurve_reorder: inside a tile the reference's morton_at_ct<log2(tile)> code is row-major, so the tiled raster kernel
    // is both stages.  (round 5) As a tail filter the stream is the sink's `char` output (sqeazy_pipelines.hpp:64-77 lists the stages for the
    // tail chain): stage_shape.
    int reorder(size_t si, bool zcurve)
    {
        const char* name = zcurve ? "zcurve_reorder" : "raster_reorder";
        if (not_3d(zcurve ? "zcurve" : "reorder")) return 1;
        const Stage& st = pipe.stages[si];
        auto t = st.cfg.find("tile_size");                 // (raster_reorder: always there, from_string fills in the default)
        const uint64_t ts = t != st.cfg.end() ? (uint64_t)std::atoi(t->second.c_str()) : (zcurve ? 2 : 0);
        uint64_t Z, Y, X;
        stage_shape(si, Z, Y, X);
        if (zcurve ? !sqy::zcurve_geometry_defined(Z, Y, X, ts) : !sqy::raster_geometry_defined(Z, Y, X, ts, cur_elem)) {
            std::fprintf(stderr, "[sqeazy]\t %s: the reference's result is undefined for shape %llux%llux%llu at tile_size=%llu (%s); refused\n", name,
                         (unsigned long long)Z, (unsigned long long)Y, (unsigned long long)X, (unsigned long long)ts,
                         zcurve ? "tile sizes other than 2..128 powers of two, or a tile that does not divide a power-of-two shape"
                                : "remainder in some dimensions only, or a tile wider than one 16-byte block");
            return 1;
        }
        uint8_t* out = next_buf(cur_len * cur_elem);
        if (!out) return 1;
        SQY_TIMED(name, sqy::launch_raster_reorder(cur, out, Z, Y, X, ts, cur_elem, false, stream));
        return produced(out);
    }

    // remove_estimated_background_scheme::encode (remove_estimated_background_scheme_impl.hpp:71-110); shape checked by background_geometry_ok
    int rmestbkrd()
    {
        const uint64_t portion = sqy::rmestbkrd_face_portion(dims[1] * dims[2], (uint32_t)g_opt.host_l2_bytes.load());
        if (ws->bkrd.ensure(sqy::rmestbkrd_work_bytes(cur_elem))) return 1;
        uint8_t* out = next_buf(cur_len * cur_elem);
        if (!out) return 1;
        SQY_TIMED("rmestbkrd", sqy::launch_rmestbkrd(cur, out, dims[0], dims[1], dims[2], portion, cur_elem, ws->bkrd.p, stream));
        return produced(out);
    }

    // flatten_to_neighborhood_scheme::encode (flatten_to_neighborhood_scheme_impl.hpp:90-150): the threshold in the voxel type,
    // cut_fraction = fraction * (size<Neighborhood>() - 1) in float; shape checked by background_geometry_ok
    int rmbkrd_neighbor5(size_t si)
    {
        const Stage& st = pipe.stages[si];
        const float cut = st.nb_fraction * (float)(125u - 1u);
        uint8_t* out = next_buf(cur_len * cur_elem);
        if (!out) return 1;
        SQY_TIMED("rmbkrd_neighbor5x5x5", sqy::launch_rmbkrd_neighbor5(cur, out, dims[0], dims[1], dims[2], (uint32_t)st.nb_threshold, cut,
                                                                       sqy::neighbor5_z_end(dims[0], dims[2]), cur_elem, stream));
        return produced(out);
    }

    // pass_through_scheme_impl.hpp:66-79: the sink that only re-types the stream to bytes
    int pass_through() { cur_len *= (uint64_t)cur_elem; cur_elem = 1; return 0; }

    int bitshuffle(size_t si)
    {
        const Stage& st = pipe.stages[si];
        auto b = st.cfg.find("block_size");
        const uint64_t be = sqy::bitshuffle_block_elems(cur_elem, b != st.cfg.end() ? (uint64_t)std::atoi(b->second.c_str()) : 0);
        if (!be) { std::fprintf(stderr, "[sqeazy]\t bitshuffle: block_size must be a multiple of 8\n"); return 1; }
        uint8_t* out = next_buf(cur_len * cur_elem);
        if (!out) return 1;
        SQY_TIMED("bitshuffle", sqy::launch_bitshuffle(cur, out, cur_len, cur_elem, be, false, stream));
        return produced(out);
    }

    // frame_shuffle and tile_shuffle: the sequential binary32 sums of `units` runs of `per_unit` elements of `in`, read back, ordered on the
    // host (order(sums, map)), and the map sent to *d_map (behind the sums in ws->small).  `map` is read by that async copy: the caller keeps
    // it until the stream has been synchronised.
    template <class Order>
    int shuffle_map(const uint8_t* in, uint64_t units, uint64_t per_unit, bool tail, const char* prof, Order order,
                                std::vector<uint64_t>& map, uint64_t** d_map)
    {
        if (ws->small.ensure(std::max<uint64_t>(units * 16, 4096))) return 1;
        float* d_sums = static_cast<float*>(ws->small.p);
        *d_map = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(ws->small.p) + ((units * 4 + 15) & ~(uint64_t)15));
        const uint64_t fm_bytes = sqy::frame_metric_scratch_bytes(units, per_unit, cur_elem);
        if (ws->lz4_scratch.ensure(std::max<uint64_t>(fm_bytes, 16))) return 1;      // free until the sink runs
        SQY_TIMED(prof, sqy::launch_frame_metric(in, units, per_unit, cur_elem, d_sums, stream, ws->lz4_scratch.p, fm_bytes, tail));
        std::vector<float> sums(units);
        map.assign(units, 0);
        SQY_HIP(hipMemcpyAsync(sums.data(), d_sums, units * sizeof(float), hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        order(sums.data(), map.data());
        SQY_HIP(hipMemcpyAsync(*d_map, map.data(), units * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        return 0;
    }

    int tile_shuffle(size_t si)
    {
        if (not_3d("tile_shuffle")) return 1;
        Stage& st = pipe.stages[si];
        auto t = st.cfg.find("tile_size");
        const uint64_t ts = t != st.cfg.end() ? (uint64_t)std::atoi(t->second.c_str()) : 32;
        // (tail filter: tile_shuffle_scheme<char> on the sink's stream -- the tile sums add SIGNED bytes and the metric is a char)
        const bool tail = is_tail(si);
        uint64_t Z, Y, X;
        stage_shape(si, Z, Y, X);
        if (!sqy::tile_shuffle_geometry_defined(Z, Y, X, ts)) {
            std::fprintf(stderr, "[sqeazy]\t tile_shuffle: shape %llux%llux%llu is not a whole multiple of tile_size=%llu; the reference's remainder "
                                 "path (P^2 median over tiles read past their end, thread-timing dependent map) is not reproduced; refused\n",
                         (unsigned long long)Z, (unsigned long long)Y, (unsigned long long)X, (unsigned long long)ts);
            return 1;
        }
        const uint64_t per_tile = ts * ts * ts, ntiles = cur_len / per_tile, tile_bytes = per_tile * (uint64_t)cur_elem;
        // 1. tiles made contiguous (tile-major copy), 2. their sequential binary32 sums, 3. order on the host, 4. tiles appended in that order
        uint8_t* tiled = next_buf(cur_len * cur_elem);
        if (!tiled) return 1;
        SQY_TIMED("tile_gather", sqy::launch_raster_reorder(cur, tiled, Z, Y, X, ts, cur_elem, false, stream));
        std::vector<uint64_t> map;
        uint64_t* d_map = nullptr;
        auto order = [&](const float* sums, uint64_t* m) { sqy::tile_shuffle_order(sums, ntiles, per_tile, cur_elem, m, tail); };
        if (shuffle_map(tiled, ntiles, per_tile, tail, "tile_metric", order, map, &d_map)) return 1;
        uint8_t* out = next_buf(cur_len * cur_elem);
        if (!out) return 1;
        SQY_TIMED("tile_shuffle", sqy::launch_frame_gather(tiled, out, ntiles, tile_bytes, d_map, stream));
        SQY_HIP(hipStreamSynchronize(stream));                     // `map` (host) is read by the async copy of shuffle_map
        st.cfg["reorder_map"] = sqy::to_verbatim(map.data(), ntiles * sizeof(uint64_t));   // tile_shuffle_scheme_impl.hpp:88
        return produced(out);
    }

    int diff3x3x1(size_t si)
    {
        if (dims.size() != 3) {
            // diff_scheme_impl.hpp:84-87 returns the output pointer unmoved -> the chain throws
            // (dynamic_stage_chain.hpp:313-317); no exception may cross this ABI
            std::fprintf(stderr, "[diff_scheme] unable to process input data that is not 3D\n");
            return 1;
        }
        // as a tail filter the stream is the sink's `char` output, {1, 1, bytes} unless that is one byte per voxel: which the stage cannot take
        const bool tail = is_tail(si);
        uint64_t Z, Y, X;
        stage_shape(si, Z, Y, X);
        if ((int64_t)(X - 1) * (int64_t)(Y - 2) <= 1 || Y < 3 || X < 2) {
            std::fprintf(stderr, "[sqeazy]\t diff3x3x1: shape %llux%llux%llu reads out of bounds in the reference; refused\n",
                         (unsigned long long)Z, (unsigned long long)Y, (unsigned long long)X);
            return 1;
        }
        if (cur_elem == 1 && (Z > 127 || Y > 127 || X > 127)) {
            std::fprintf(stderr, "[sqeazy]\t diff3x3x1 on 8-bit voxels: extents > 127 overflow the reference's char coordinates; refused\n");
            return 1;
        }
        const uint32_t sw = (!tail && followed_by(si, StageKind::bitswap1) && (reinterpret_cast<uintptr_t>(cur) & 15) == 0)
                                ? sqy::diff3x3x1_side_width(Z, Y, X, cur_elem) : 0;
        if (sw) {
            // a buffer of its own: `cur` stays where it is, so the transpose's output (the next buffer of the
            // ping/pong rotation) can never be the buffer `cur` lives in
            if (ws->diff_side.ensure(Z * Y * (uint64_t)sw * 2)) return 1;
            uint8_t* sbuf = static_cast<uint8_t*>(ws->diff_side.p);
            SQY_TIMED("diff3x3x1", sqy::launch_diff3x3x1_side(reinterpret_cast<const uint16_t*>(cur), reinterpret_cast<uint16_t*>(sbuf), Z, Y, X, sw, stream));
            side.p = reinterpret_cast<const uint16_t*>(sbuf);
            side.w = sw;
            side.X = (uint32_t)X;
            return 0;                                                   // (`cur` stays the stage's input: the transpose reads both)
        }
        uint8_t* out = next_buf(cur_len * cur_elem);
        if (!out) return 1;
        SQY_TIMED("diff3x3x1", sqy::launch_diff3x3x1(cur, out, Z, Y, X, cur_elem, stream, tail));
        return produced(out);
    }

    int frame_shuffle(size_t si)
    {
        if (not_3d("frame_shuffle")) return 1;
        Stage& st = pipe.stages[si];
        // (tail filter: signed bytes; ONE frame {1, 1, bytes} when the sink did not write one byte per voxel)
        const bool tail = is_tail(si);
        // frame_chunk_size = N: N consecutive frames are one sort unit (frame_shuffle_utils.hpp:105-133, encode_full) -- the stage
        // on Z / N "frames" of N * Y * X voxels.  Z % N != 0 takes the reference's encode_with_remainder (Boost's P^2 median
        // estimate as the metric, :193-260): not reproduced
        const uint64_t fcs = frame_chunk_size(st);
        uint64_t Z0, Y, X;
        stage_shape(si, Z0, Y, X);
        if (fcs == 0 || Z0 % fcs != 0) {
            std::fprintf(stderr, "[sqeazy]\t frame_shuffle: %llu frames are no whole multiple of frame_chunk_size=%llu; the reference's remainder path "
                                 "(a P^2 median estimate as the metric) is not reproduced; refused\n", (unsigned long long)Z0, (unsigned long long)fcs);
            return 1;
        }
        const uint64_t Z = Z0 / fcs, per_frame = Y * X * fcs;
        std::vector<uint64_t> map;
        uint64_t* d_map = nullptr;
        auto order = [&](const float* sums, uint64_t* m) { sqy::frame_shuffle_order(sums, Z, per_frame, m); };
        if (shuffle_map(cur, Z, per_frame, tail, "frame_metric", order, map, &d_map)) return 1;
        // when lz4 follows immediately and its chunks tile the frames, the permuted copy is never materialised:
        // the LZ4 kernels read frame map[f] where the stream has frame f
        const uint64_t frame_bytes = per_frame * (uint64_t)cur_elem;
        bool fused = false;
        if (followed_by(si, StageKind::lz4) && frame_bytes) {
            const sqy::Lz4EncodeLayout lay = sqy::lz4_encode_layout(pipe.stages[si + 1].lz4, cur_len * (uint64_t)cur_elem, pipe.nthreads);
            fused = lay.chunked() && frame_bytes % lay.chunk == 0;        // (block-linked frames read a gathered copy)
        }
        if (fused) {
            prep.frame_map = d_map;
            prep.frame_bytes = frame_bytes;
        } else {
            uint8_t* out = next_buf(cur_len * cur_elem);
            if (!out) return 1;
            SQY_TIMED("frame_gather", sqy::launch_frame_gather(cur, out, Z, frame_bytes, d_map, stream));
            cur = out;
        }
        SQY_HIP(hipStreamSynchronize(stream));                     // `map` (host) is read by the async copy of shuffle_map
        st.cfg["frame_chunk_size"] = std::to_string(fcs);
        st.cfg["reorder_map"] = sqy::to_verbatim(map.data(), Z * sizeof(uint64_t));   // frame_shuffle_scheme_impl.hpp:86-90
        return 0;
    }

    // quantiser_scheme<uint16_t,char>::encode (quantiser_scheme_impl.hpp:176-226); with a bitswap1 right behind it that stage as well
    int quantiser(size_t& si)
    {
        Stage& st = pipe.stages[si];
        if (ws->small.ensure(65536 * sizeof(uint32_t) + 65536)) return 1;
        uint32_t* d_histo = static_cast<uint32_t*>(ws->small.p);
        uint8_t* d_lut = static_cast<uint8_t*>(ws->small.p) + 65536 * sizeof(uint32_t);
        SQY_TIMED("histogram_u16", sqy::launch_histogram_u16(reinterpret_cast<const uint16_t*>(cur), cur_len, d_histo, stream));
        std::vector<uint32_t> histo(65536);
        std::vector<unsigned char> lut_encode(65536);
        uint16_t lut_decode[256];
        SQY_HIP(hipMemcpyAsync(histo.data(), d_histo, 65536 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        sqy::QuantiserWeighting qw;
        {
            auto wf = st.cfg.find("weighting_function");
            if (wf != st.cfg.end() && !sqy::quantiser_parse_weighting(wf->second, &qw)) return 1;    // (refused by supported() already)
        }
        sqy::quantiser_build_luts(histo.data(), 65536, lut_encode.data(), lut_decode, qw);
        SQY_HIP(hipMemcpyAsync(d_lut, lut_encode.data(), 65536, hipMemcpyHostToDevice, stream));
        uint8_t* out = next_buf(cur_len);
        if (!out) return 1;
        // (round 5) bitswap1 right behind the sink: look-up and 8-bit bit-plane transpose in one pass
        if (followed_by(si, StageKind::bitswap1) && (reinterpret_cast<uintptr_t>(cur) & 15) == 0) {
            SQY_TIMED("quantiser_bitswap1_u8", sqy::launch_quantiser_apply_bitswap1_u8(reinterpret_cast<const uint16_t*>(cur), out, cur_len, d_lut, stream));
            si += 1;                                                   // the bitswap1 stage is done as well
        } else {
            SQY_TIMED("quantiser_apply", sqy::launch_quantiser_apply_u16(reinterpret_cast<const uint16_t*>(cur), out, cur_len, d_lut, stream));
        }
        SQY_HIP(hipStreamSynchronize(stream));                     // lut_encode (host) is read by the async copy above
        // quantiser_scheme_impl.hpp:200-204: the decode LUT goes to the file the caller named, else into the header
        auto lp = st.cfg.find("decode_lut_path");
        if (lp != st.cfg.end()) {
            if (!sqy::quantiser_lut_to_file(lp->second, lut_decode, 256)) {
                // (the reference does not notice and returns a blob nobody can decode; here the encode fails)
                std::fprintf(stderr, "[sqeazy]\t quantiser: unable to write the decode LUT to %s\n", lp->second.c_str());
                return 1;
            }
        } else
            st.cfg["decode_lut_string"] = sqy::to_verbatim(lut_decode, sizeof(lut_decode));
        cur = out;
        cur_elem = 1;                                              // sink output is `char`
        return 0;
    }

    int lz4_stage(size_t si)
    {
        const sqy::Lz4Params& lz = pipe.stages[si].lz4;
        lz4.block_id = lz.block_id;
        lz4.total = cur_len * (uint64_t)cur_elem;
        const sqy::Lz4EncodeLayout lay = sqy::lz4_encode_layout(lz, lz4.total, pipe.nthreads);
        lz4.chunk = lay.chunk;
        lz4.nchunks = lay.nchunks;
        if (lay.chunked()) {
            if (lz4_chunked(lay.accel)) return 1;
            if (lz4.inplace_done) return 0;
        } else if (lz4_linked(si, lay.kind == sqy::Lz4LayoutKind::serial, lay.accel)) {
            return 1;
        }
        SQY_TIMED("lz4_frame_scan", sqy::launch_lz4_frame_scan(static_cast<uint32_t*>(ws->csize.p), lz4.nchunks, lz4.total, (uint32_t)lz4.chunk,
                                                               static_cast<uint64_t*>(ws->frame_off.p), stream, lz4.blocks, lz4.dup_of, lz4.tail_info));
        lz4.on = true;
        return 0;
    }

    // chunked layout, one LZ4 block per frame: every chunk is independent.  The duplicate search, the parse and the dense pass behind it --
    // or, frames in place with a header short enough, everything up to the finished blob (lz4_inplace_finish)
    int lz4_chunked(uint32_t accel)
    {
        lz4.stride = (lz4.chunk + 15) & ~(uint64_t)15;
        if (ws->lz4_scratch.ensure(std::max<uint64_t>(lz4.nchunks * lz4.stride, 16))) return 1;
        if (ws->csize.ensure(std::max<uint64_t>(lz4.nchunks, 1) * sizeof(uint32_t))) return 1;
        if (ws->frame_off.ensure((lz4.nchunks + 1 + 4) * sizeof(uint64_t))) return 1;
        if (prep.place.on) lz4.tail_info = static_cast<uint64_t*>(ws->frame_off.p) + lz4.nchunks + 1;
        sqy::Lz4DedupeArgs dedupe_args;              // frames in place: the duplicate decision per chunk is made inside the parse kernel
        bool fused_dedupe = false;
        if (prep.dedupe.total) {                     // (left by the bitswap1 directly in front: lz4 is a pipeline's one sink, Pipeline::supported)
            ProfScope ps("lz4_dedupe", stream, pend);
            // frames in place (acceleration 1): only the key table is built here, the decision per chunk (byte compare, hole fill)
            // is the first thing the chunk's parse wavefront does (lz4_chunk_dedupe).  (holes: which 1 KiB pieces of the plane stream the
            // transpose left unwritten, all zero)
            fused_dedupe = prep.place.on && accel == 1;
            SQY_HIP(sqy::launch_lz4_dedupe(cur, lz4.total, (uint32_t)lz4.chunk, ws->dedupe.p, prep.dedupe, stream, prep.place.in_stride, prep.place.on,
                                           prep.dedupe_cleared, fused_dedupe ? &dedupe_args : nullptr));
            lz4.dup_of = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(ws->dedupe.p) + prep.dedupe.dup_at);
            if (fused_dedupe && prep.digest) { dedupe_args.digest = prep.digest; dedupe_args.digest_stride = prep.digest_stride; }
        }
        if (ws->plan.ensure((lz4.nchunks + 1) * sizeof(uint32_t))) return 1;
        uint32_t* d_redo = static_cast<uint32_t*>(ws->plan.p);       // chunks the first pass leaves to the dense batches
        SQY_TIMED("lz4_chunks", sqy::launch_lz4_chunks(cur, lz4.total, (uint32_t)lz4.chunk, static_cast<uint8_t*>(ws->lz4_scratch.p), lz4.stride,
                                                       static_cast<uint32_t*>(ws->csize.p), lz4.nchunks, stream, prep.frame_map, prep.frame_bytes, d_redo,
                                                       fused_dedupe ? nullptr : lz4.dup_of, prep.place.in_stride, accel, prep.dedupe_cleared,
                                                       fused_dedupe ? &dedupe_args : nullptr));
        std::string hdr_prefix, hdr_suffix;
        if (prep.place.on && !(fq && fq->every > 0)) sqy::header_pack_parts(elem_size, false, dims, pipe.name(), &hdr_prefix, &hdr_suffix);
        if (prep.place.on && !hdr_prefix.empty() && hdr_prefix.size() + hdr_suffix.size() <= sqy::kLz4InplaceHeaderTextMax)
            return lz4_inplace_finish(d_redo, hdr_prefix, hdr_suffix);
        SQY_HIP(hipMemcpyAsync(ws->pinned, d_redo, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        const uint32_t n_redo = *static_cast<uint32_t*>(ws->pinned);
        return n_redo ? lz4_dense(d_redo, n_redo) : 0;
    }

    // the chunks the first pass left to the dense batches (d_redo[0] of them)
    int lz4_dense(uint32_t* d_redo, uint32_t n_redo)
    {
        SQY_TIMED("lz4_chunks_dense", sqy::launch_lz4_chunks_dense(cur, lz4.total, (uint32_t)lz4.chunk, static_cast<uint8_t*>(ws->lz4_scratch.p), lz4.stride,
                                                                   static_cast<uint32_t*>(ws->csize.p), d_redo, n_redo, stream, prep.frame_map, prep.frame_bytes,
                                                                   prep.place.in_stride));
        return 0;
    }

    // Frames in place, ONE host round trip per call (round 4): frame scan + tail marks, the stored chunks in front of the tail put aside,
    // the gather and the sqy header are all queued behind the parse right away and take what they need (where the stored tail begins,
    // the payload size) from device memory; what the host has to know comes back through pinned memory with the one synchronisation.
    // Only when the parse left chunks to the dense pass (streams of short sequences: seldom on microscopy stacks) do these kernels return
    // untouched -- they look at the list's counter -- and run again behind the dense pass (status 2).
    int lz4_inplace_finish(uint32_t* d_redo, const std::string& hdr_prefix, const std::string& hdr_suffix)
    {
        const Lz4Descriptor fd = lz4_descriptor(lz4.block_id);
        uint8_t* outb = static_cast<uint8_t*>(d_dst);
        volatile uint64_t* record = static_cast<volatile uint64_t*>(ws->pinned);
        // (round 6) scan, tail marks, gather and header are ONE kernel (lz4_inplace_tail_fused_kernel: no workgroup waits for
        // another; with calls in flight the five launches it replaces were 0.3 ms of a call's 2.4).  Only when stored chunks
        // sit in front of the stored tail -- their bodies lie where gathered frames go -- does it hand back (status 4) to the
        // separate kernels, which put those chunks aside first.
        const bool fused_tail = lz4.nchunks <= 65536;         // (a workgroup of the fused kernel owns at most 64 chunks)
        // fused: the one kernel; else the frame scan (scan_too) and the separate kernel
        auto tail = [&](const uint32_t* guard, bool fused, bool scan_too) -> int {
            record[0] = 0;
            if (!fused && scan_too)
                SQY_TIMED("lz4_frame_scan", sqy::launch_lz4_frame_scan(static_cast<uint32_t*>(ws->csize.p), lz4.nchunks, lz4.total, (uint32_t)lz4.chunk,
                                                                       static_cast<uint64_t*>(ws->frame_off.p), stream, nullptr, lz4.dup_of, lz4.tail_info, guard,
                                                                       outb + prep.place.body0, prep.place.in_stride, fd.bd, fd.hc));
            auto with_args = [&](auto launch) {
                return launch(outb, prep.place.t0, prep.place.in_stride, lz4.total, (uint32_t)lz4.chunk, lz4.nchunks, static_cast<uint8_t*>(ws->lz4_scratch.p), lz4.stride,
                              static_cast<uint32_t*>(ws->csize.p), static_cast<uint64_t*>(ws->frame_off.p), lz4.dup_of, lz4.tail_info, fd.bd, fd.hc,
                              hdr_prefix.data(), (uint32_t)hdr_prefix.size(), hdr_suffix.data(), (uint32_t)hdr_suffix.size(), (uint32_t)elem_size, guard,
                              const_cast<uint64_t*>(record), stream);
            };
            SQY_TIMED(fused ? "lz4_inplace_tail" : "lz4_frame_gather",
                      fused ? with_args(sqy::launch_lz4_inplace_tail_fused) : with_args(sqy::launch_lz4_inplace_tail));
            return 0;
        };
        if (tail(d_redo, fused_tail, true)) return 1;
        if (stamps) stamps->stamp(CallStamps::parse_queued);
        SQY_HIP(hipStreamSynchronize(stream));
        if (stamps) stamps->stamp(CallStamps::sync_returned);
        if (record[0] == 2) {                                  // chunks left to the dense pass: it runs, then the tail again
            if (lz4_dense(d_redo, (uint32_t)record[6])) return 1;
            if (tail(nullptr, fused_tail, true)) return 1;
            SQY_HIP(hipStreamSynchronize(stream));
        }
        if (record[0] == 4) {                                  // stored chunks in front of the stored tail: put aside first
            if (tail(nullptr, false, false)) return 1;
            SQY_HIP(hipStreamSynchronize(stream));
        }
        if (record[0] != 1) {
            std::fprintf(stderr, "[sqeazy]\t internal error: frames in place did not finish (status %llu)\n", (unsigned long long)record[0]);
            return 1;
        }
        lz4.inplace_done = true;
        lz4.blob_at = record[1]; lz4.blob_bytes = record[2]; lz4.payload_bytes = record[3];
        lz4.on = true;
        return 0;
    }

    // block-linked frames: the serial layout (nthreads == 1) or chunks that span several LZ4 blocks.  The table of a frame is carried
    // from block to block (lz4_utils.hpp:99-173): one wavefront walks each frame -- or every block is parsed at once from a guess of that
    // table that is checked afterwards (lz4_linked_spec)
    int lz4_linked(size_t si, bool serial, uint32_t accel)
    {
        const sqy::Lz4Plan plan = sqy::lz4_plan_blocks(lz4.total, lz4.chunk, pipe.stages[si].lz4.block_bytes(), serial);
        if (!plan.ok || plan.blocks.empty()) {
            std::fprintf(stderr, "[sqeazy]\t lz4: block layout not available on MI355X\n");
            return 1;
        }
        const uint64_t nblocks = plan.blocks.size(), nframes = plan.frame_first.size() - 1;
        const uint64_t blocks_bytes = nblocks * sizeof(sqy::Lz4Block), first_bytes = (nframes + 1) * sizeof(uint32_t);
        static_assert(sizeof(sqy::Lz4Block) == sizeof(sqy::Lz4BlockPlan) && sizeof(sqy::Lz4Block) == 32, "plan entries are read by the kernels as they are");
        if (ws->plan.ensure(blocks_bytes + first_bytes)) return 1;
        sqy::Lz4Block* d_blocks = static_cast<sqy::Lz4Block*>(ws->plan.p);
        uint32_t* d_first = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws->plan.p) + blocks_bytes);
        SQY_HIP(hipMemcpyAsync(d_blocks, plan.blocks.data(), blocks_bytes, hipMemcpyHostToDevice, stream));
        SQY_HIP(hipMemcpyAsync(d_first, plan.frame_first.data(), first_bytes, hipMemcpyHostToDevice, stream));
        lz4.stride = ((uint64_t)plan.max_block + 15) & ~(uint64_t)15;
        if (ws->lz4_scratch.ensure(std::max<uint64_t>(nblocks * lz4.stride, 16))) return 1;
        if (ws->csize.ensure(nblocks * sizeof(uint32_t))) return 1;
        if (ws->frame_off.ensure((nblocks + 1) * sizeof(uint64_t))) return 1;
        // Few long frames (the serial layout above all): block-parallel.  Every block is parsed by its own wavefront from
        // a table rebuilt by parsing the >= 64 KiB in front of it, the tables are checked against what the block in
        // front really left, and what fails the check is parsed again in order (sqy_kernels.h: Lz4SpecArgs).  Twice the
        // parse work on thousands of wavefronts instead of one: worth it when the frame walks would leave the chip empty.
        // measurement / test knob: SQY_NO_BLOCK_PARALLEL (the frame walk of rounds 2-3)
        // (without room for the tables -- 32 KiB per block -- the walk, which needs none)
        const bool spec_wanted = g_opt.block_parallel.load() != 0 && sqy::lz4_spec_wanted(plan);
        const bool spec_room = spec_wanted && !ws->spec.ensure(nblocks * sqy::kLz4SpecTableWords * sizeof(uint32_t) + 3 * nblocks * sizeof(uint32_t), true);
        if (spec_wanted && !spec_room) {
            // (round-4 advice) said once, not per call: the result is the same, the rate is not
            static std::atomic<bool> told{false};
            if (!told.exchange(true))
                std::fprintf(stderr, "[sqeazy]\t lz4: no HBM for the block-parallel parse's tables (%llu MiB): block-linked frames are walked by one "
                                     "wavefront each (same bytes, hundreds of times slower on long frames)\n",
                             (unsigned long long)((nblocks * sqy::kLz4SpecTableWords * sizeof(uint32_t)) >> 20));
        }
        if (spec_room) {
            if (lz4_linked_spec(plan, d_blocks, accel)) return 1;
        } else {
            SQY_TIMED("lz4_linked", sqy::launch_lz4_linked(cur, d_blocks, d_first, nframes, plan.max_block, static_cast<uint8_t*>(ws->lz4_scratch.p),
                                                           lz4.stride, static_cast<uint32_t*>(ws->csize.p), stream, accel));
        }
        SQY_HIP(hipStreamSynchronize(stream));                 // `plan` (host) is read by the async copies above
        lz4.blocks = d_blocks;
        lz4.nchunks = nblocks;                                  // scan and gather work per block from here on
        lz4.chunk = plan.max_block;
        return 0;
    }

    // The block-parallel parse of block-linked frames: every block from a guessed table, then verify / redo rounds until every block
    // started from the table the block in front really left.  Returns with the stream synchronised.
    int lz4_linked_spec(const sqy::Lz4Plan& plan, const sqy::Lz4Block* d_blocks, uint32_t accel)
    {
        const uint64_t nblocks = plan.blocks.size();
        const uint64_t list_bytes = nblocks * sizeof(uint32_t);
        // SQY_BLOCK_PARALLEL_WARMUP = bytes of warm-up in front of a block (default and liblz4's reach: 64 KiB; less makes the guess fail
        // more often -- the result stays exact, the blocks that fail are parsed again)
        std::vector<uint32_t> wfirst, wlast, ok(nblocks);
        sqy::lz4_warmup_windows(plan, (uint64_t)g_opt.block_parallel_warmup.load(), &wfirst, &wlast);
        sqy::Lz4SpecArgs sa;
        sa.tables = static_cast<uint32_t*>(ws->spec.p);
        uint32_t* d_wfirst = sa.tables + nblocks * sqy::kLz4SpecTableWords;
        uint32_t* d_wlast = d_wfirst + nblocks;
        uint32_t* d_ok = d_wlast + nblocks;
        sa.wave_first = d_wfirst; sa.wave_last = d_wlast; sa.mode = 1;
        SQY_HIP(hipMemcpyAsync(d_wfirst, wfirst.data(), list_bytes, hipMemcpyHostToDevice, stream));
        SQY_HIP(hipMemcpyAsync(d_wlast, wlast.data(), list_bytes, hipMemcpyHostToDevice, stream));
        SQY_TIMED("lz4_linked_blocks", sqy::launch_lz4_linked_spec(cur, d_blocks, sa, nblocks, plan.max_block, static_cast<uint8_t*>(ws->lz4_scratch.p),
                                                                   lz4.stride, static_cast<uint32_t*>(ws->csize.p), stream, accel));
        for (uint64_t round = 0;; ++round) {
            SQY_TIMED("lz4_linked_verify", sqy::launch_lz4_linked_verify(d_blocks, nblocks, sa.tables, plan.max_block, d_ok, stream));
            SQY_HIP(hipMemcpyAsync(ok.data(), d_ok, list_bytes, hipMemcpyDeviceToHost, stream));
            SQY_HIP(hipStreamSynchronize(stream));
            // runs of blocks that did not start from the true table: one wavefront each, in order, from the table in front
            // (round-5 advice) a run is parsed by ONE wavefront, block after block: at most kRunMax blocks of it per launch (the
            // rest keep failing the check and are taken by the next rounds, each from the table the last one left) -- the top
            // plane of a quantised stack fails as one run of 511 blocks, seconds of work: sixteen launches of a fraction of a
            // second instead of one kernel that runs for seconds; and the caller is told, once, what layout to ask for.
            constexpr uint64_t kRunMax = 32;
            const sqy::Lz4RedoRuns runs = sqy::lz4_redo_runs(plan, ok, kRunMax, &wfirst, &wlast);
            const uint64_t nruns = runs.nruns, longest_run = runs.longest;
            if (longest_run > 4 * kRunMax) {
                static std::atomic<bool> told{false};
                if (!told.exchange(true))
                    std::fprintf(stderr, "[sqeazy]\t lz4: %llu blocks in a row of this block-linked frame (nthreads = 1) can only be parsed one after "
                                         "the other -- a stream of short sequences, whose table no guess reproduces -- by one wavefront, "
                                         "~10 ms per block.  The chunked layout (nthreads = 0 or > 1: independent frames, same decoder) "
                                         "takes milliseconds for the same data.\n", (unsigned long long)longest_run);
            }
            if (g_opt.block_parallel_stats.load()) {
                uint64_t nbad = 0;
                for (uint64_t r = 0; r < nruns; ++r) nbad += wlast[r] - wfirst[r] + 1;
                std::fprintf(stderr, "[sqeazy]\t lz4 block-parallel: round %llu, %llu of %llu blocks to parse again in %llu runs",
                             (unsigned long long)round, (unsigned long long)nbad, (unsigned long long)nblocks, (unsigned long long)nruns);
                for (uint64_t r = 0; r < nruns && r < 24; ++r) std::fprintf(stderr, "%s%u..%u", r ? ", " : ": blocks ", wfirst[r], wlast[r]);
                std::fprintf(stderr, "\n");
            }
            if (nruns == 0) return 0;
            if (round > nblocks + 8) {
                std::fprintf(stderr, "[sqeazy]\t lz4: the block-parallel parse did not settle\n");
                return 1;
            }
            SQY_HIP(hipMemcpyAsync(d_wfirst, wfirst.data(), nruns * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            SQY_HIP(hipMemcpyAsync(d_wlast, wlast.data(), nruns * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            sa.mode = 2;
            ProfScope ps("lz4_linked_redo", stream, pend);
            SQY_HIP(sqy::launch_lz4_linked_spec(cur, d_blocks, sa, nruns, plan.max_block, static_cast<uint8_t*>(ws->lz4_scratch.p),
                                                lz4.stride, static_cast<uint32_t*>(ws->csize.p), stream, accel));
            SQY_HIP(hipStreamSynchronize(stream));             // (wfirst / wlast are reused by the next round)
        }
    }

    // frames in place, not finished on the device: what the frame scan left about the run of stored chunks that ends the payload
    struct StoredTail { uint64_t j = 0, head_bytes = 0, raw_head = 0; };

    // the payload's size (known already when the device finished the blob)
    int payload_size(uint64_t* payload_bytes, StoredTail* tail)
    {
        *payload_bytes = lz4.payload_bytes;
        if (!lz4.on) {
            *payload_bytes = cur_len * (uint64_t)cur_elem;
        } else if (lz4.nchunks == 0) {
            *payload_bytes = 7 + 4;                        // empty input: frame header + end mark
        } else if (prep.place.on && !lz4.inplace_done) {
            SQY_HIP(hipMemcpyAsync(ws->pinned, lz4.tail_info, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
            SQY_HIP(hipStreamSynchronize(stream));
            const uint64_t* ti = static_cast<const uint64_t*>(ws->pinned);
            tail->j = ti[0]; tail->head_bytes = ti[1]; tail->raw_head = ti[2]; *payload_bytes = ti[3];
        } else if (!lz4.inplace_done) {
            SQY_HIP(hipMemcpyAsync(ws->pinned, static_cast<uint64_t*>(ws->frame_off.p) + lz4.nchunks, sizeof(uint64_t),
                                   hipMemcpyDeviceToHost, stream));
            SQY_HIP(hipStreamSynchronize(stream));
            *payload_bytes = *static_cast<uint64_t*>(ws->pinned);
        }
        if (lz4.on && *payload_bytes > (uint64_t)INT_MAX) {
            // encode_parallel sums the chunk sizes into an `int` and rejects the result (lz4_utils.hpp:264-273)
            std::fprintf(stderr, "[sqeazy]\t lz4: %llu payload bytes overflow the reference's int byte count\n",
                         (unsigned long long)*payload_bytes);
            return 1;
        }
        return 0;
    }

    // where every fq->every-th LZ4 frame starts in the blob
    int frame_offsets(uint64_t hdr_bytes, uint64_t payload_bytes)
    {
        if (!lz4.on || lz4.blocks || !fq->offsets) { std::fprintf(stderr, "[sqeazy]\t frame offsets: the payload is not one LZ4 frame per chunk\n"); return 1; }
        const uint64_t cnt = (lz4.nchunks + (uint64_t)fq->every - 1) / (uint64_t)fq->every;
        if (cnt + 1 > (uint64_t)std::max(fq->max_entries, 0)) { std::fprintf(stderr, "[sqeazy]\t frame offsets: %llu entries do not fit\n", (unsigned long long)(cnt + 1)); return 1; }
        std::vector<uint64_t> fo(cnt + 1, 0);
        if (cnt)
            SQY_HIP(hipMemcpy2DAsync(fo.data(), sizeof(uint64_t), ws->frame_off.p, (size_t)fq->every * sizeof(uint64_t), sizeof(uint64_t), cnt,
                                     hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        for (uint64_t i = 0; i < cnt; ++i) fq->offsets[i] = (long)(fo[i] + hdr_bytes);
        fq->offsets[cnt] = (long)(hdr_bytes + payload_bytes);
        fq->count = (int)cnt;
        return 0;
    }

    // Frames in place, put together from the host (a frame-offset query, or header text too long for lz4_inplace_finish): the run of
    // stored chunks j.. that ends the payload stays where the bit-plane transpose put it; frames 0..j-1 are gathered so that they end
    // where frame j begins, the header goes in front of them.  *blob_at: where the blob then begins
    int assemble_inplace(const std::string& hdr, const StoredTail& tail, uint64_t* blob_at)
    {
        uint8_t* out = static_cast<uint8_t*>(d_dst);
        const Lz4Descriptor fd = lz4_descriptor(lz4.block_id);
        const uint64_t frame_j = prep.place.t0 + tail.j * prep.place.in_stride;
        if (tail.head_bytes + hdr.size() > frame_j) { std::fprintf(stderr, "[sqeazy]\t internal error: frames in place overlap the header\n"); return 1; }
        const uint64_t payload_at = frame_j - tail.head_bytes;
        *blob_at = payload_at - hdr.size();
        uint8_t* body0 = out + prep.place.body0;
        SQY_TIMED("lz4_tail_marks", sqy::launch_lz4_tail_marks(body0, prep.place.in_stride, lz4.total, (uint32_t)lz4.chunk, lz4.nchunks, fd.bd, fd.hc, lz4.tail_info, stream));
        if (tail.raw_head) {
            SQY_TIMED("lz4_stash_raw", sqy::launch_lz4_stash_raw(body0, prep.place.in_stride, lz4.total, (uint32_t)lz4.chunk, static_cast<uint8_t*>(ws->lz4_scratch.p), lz4.stride,
                                                                 static_cast<uint32_t*>(ws->csize.p), lz4.dup_of, tail.j, stream));
        }
        if (tail.j) {
            SQY_TIMED("lz4_frame_gather", sqy::launch_lz4_frame_gather(body0, lz4.total, (uint32_t)lz4.chunk, static_cast<uint8_t*>(ws->lz4_scratch.p), lz4.stride,
                                                                       static_cast<uint32_t*>(ws->csize.p), static_cast<uint64_t*>(ws->frame_off.p), out + payload_at, fd.bd, fd.hc,
                                                                       tail.j, stream, nullptr, 0, nullptr, lz4.dup_of, prep.place.in_stride, tail.raw_head != 0));
        }
        SQY_HIP(hipMemcpyAsync(out + *blob_at, hdr.data(), hdr.size(), hipMemcpyHostToDevice, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        return 0;
    }

    // header and payload from d_dst on
    int assemble_plain(const std::string& hdr, uint64_t payload_bytes)
    {
        uint8_t* out = static_cast<uint8_t*>(d_dst);
        const Lz4Descriptor fd = lz4_descriptor(lz4.block_id);
        SQY_HIP(hipMemcpyAsync(out, hdr.data(), hdr.size(), hipMemcpyHostToDevice, stream));
        if (lz4.on && lz4.nchunks == 0) {
            const unsigned char empty[7 + 4] = {0x04, 0x22, 0x4D, 0x18, fd.flg, fd.bd, (unsigned char)fd.hc, 0, 0, 0, 0};
            SQY_HIP(hipMemcpyAsync(out + hdr.size(), empty, sizeof(empty), hipMemcpyHostToDevice, stream));
        } else if (lz4.on) {
            SQY_TIMED("lz4_frame_gather", sqy::launch_lz4_frame_gather(cur, lz4.total, (uint32_t)lz4.chunk, static_cast<uint8_t*>(ws->lz4_scratch.p), lz4.stride,
                                                                       static_cast<uint32_t*>(ws->csize.p), static_cast<uint64_t*>(ws->frame_off.p),
                                                                       out + hdr.size(), fd.bd, fd.hc, lz4.nchunks, stream, prep.frame_map, prep.frame_bytes, lz4.blocks, lz4.dup_of));
        } else {
            SQY_TIMED("payload_copy", hipMemcpyAsync(out + hdr.size(), cur, payload_bytes, hipMemcpyDeviceToDevice, stream));
        }
        SQY_HIP(hipStreamSynchronize(stream));
        return 0;
    }

    // option dedupe_report: the search's keys and decisions, copied out of the workspace behind the call's last synchronisation
    int report_dedupe()
    {
        if (!lz4.dup_of || !prep.dedupe.total || lz4.blocks) return 0;       // (no search in this call: the record kept stays)
        DedupeReport rep;
        rep.keys.resize(lz4.total / lz4.chunk);
        rep.dup_of.resize(lz4.nchunks);
        if (!rep.keys.empty())
            SQY_HIP(hipMemcpyAsync(rep.keys.data(), static_cast<const uint8_t*>(ws->dedupe.p) + prep.dedupe.work_at, rep.keys.size() * sizeof(uint64_t),
                                   hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipMemcpyAsync(rep.dup_of.data(), lz4.dup_of, rep.dup_of.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        std::lock_guard<std::mutex> lock(g_dedupe_report_mu);
        g_dedupe_report = std::move(rep);
        return 0;
    }

    // the blob is complete (the stream synchronised): it lies at d_dst + at
    int done(uint64_t at, uint64_t bytes, long* dstlength)
    {
        if (g_opt.dedupe_report.load(std::memory_order_relaxed) != 0 && report_dedupe()) return 1;
        if (lanes) lanes->complete = true;
        if (g_prof_on.load()) prof_collect(*pend);
        if (dstoffset) *dstoffset = (long)at;
        *dstlength = (long)bytes;
        return 0;
    }

    // The payload's size, the sqy header (written after encoding, as the reference rewrites it: dynamic_pipeline.hpp:599-612), the frame
    // offsets asked for, and the blob put together in d_dst
    int finish(long* dstlength)
    {
        uint64_t payload_bytes = 0, blob_at = 0;
        StoredTail tail;
        if (payload_size(&payload_bytes, &tail)) return 1;
        if (lz4.inplace_done) return done(lz4.blob_at, lz4.blob_bytes, dstlength);
        const std::string hdr = sqy::header_pack(elem_size, false, dims, pipe.name(), payload_bytes);
        if (fq && fq->every > 0 && frame_offsets(hdr.size(), payload_bytes)) return 1;
        const uint64_t blob_bytes = hdr.size() + payload_bytes;
        if (blob_bytes > dst_capacity) {
            std::fprintf(stderr, "[sqeazy]\t destination buffer too small (%llu > %llu bytes)\n", (unsigned long long)blob_bytes,
                         (unsigned long long)dst_capacity);
            return 1;
        }
        if (prep.place.on ? assemble_inplace(hdr, tail, &blob_at) : assemble_plain(hdr, payload_bytes)) return 1;
        return done(blob_at, blob_bytes, dstlength);
    }
};

// A pipeline this library encodes; the reason goes to stderr where the reference would have taken the pipeline
bool pipeline_admitted(const std::string& pipeline, int elem_size)
{
    std::string why;
    if (Pipeline::supported(pipeline, elem_size, &why)) return true;
    if (Pipeline::reference_accepts(pipeline)) std::fprintf(stderr, "[sqeazy]\t pipeline %s: %s\n", pipeline.c_str(), why.c_str());
    return false;
}

// What every encode call checks before it touches the device: the pipeline, the volume's size against the reference's int counts, the
// background filters' geometry.  0: *pipe, *dims and *len are the call's
// (in two halves: a batch admits its pipeline once and every volume's shape)
int admit_pipeline(const std::string& pipeline, int elem_size, int nthreads, Pipeline* pipe)
{
    if (!pipeline_admitted(pipeline, elem_size)) return 1;
    *pipe = Pipeline::from_string(pipeline, elem_size);
    if (pipe->stages.empty()) {
        std::fprintf(stderr, "[sqeazy]\t received %spipeline of size 0, cannot encode buffer\n", pipe->name().c_str());
        return 1;
    }
    pipe->set_n_threads(nthreads);
    return 0;
}
int admit_shape(const Pipeline* pipe, const long* shape, unsigned rank, std::vector<uint64_t>* dims, uint64_t* len)
{
    *len = voxel_count(shape, rank);
    if (*len == 0) { std::fprintf(stderr, "[sqeazy]\t non-positive extent in shape\n"); return 1; }
    if (*len >= ((uint64_t)1 << 31)) {
        std::fprintf(stderr, "[sqeazy]\t %llu+ voxels in one call overflow the reference's int voxel count; encode z-slabs\n", (unsigned long long)*len);
        return 1;
    }
    dims->assign(shape, shape + rank);
    return background_geometry_ok(*pipe, *dims) ? 0 : 1;
}
int admit_encode(const std::string& pipeline, const long* shape, unsigned rank, int elem_size, int nthreads, Pipeline* pipe, std::vector<uint64_t>* dims,
                 uint64_t* len)
{
    return admit_pipeline(pipeline, elem_size, nthreads, pipe) || admit_shape(pipe, shape, rank, dims, len) ? 1 : 0;
}

int encode_on_device(Context& cx, const char* pipeline_c, const void* d_src, const long* shape, unsigned rank, int elem_size,
                     void* d_dst, uint64_t dst_capacity, long* dstlength, int nthreads, hipStream_t stream, long* dstoffset = nullptr,
                     FrameQuery* fq = nullptr, CallStamps* stamps = nullptr)
{
    if (!pipeline_c || !d_src || !shape || !d_dst || !dstlength) return 1;
    if (dstoffset) *dstoffset = 0;
    Pipeline pipe;
    std::vector<uint64_t> dims;
    uint64_t len = 0;
    if (admit_encode(pipeline_c, shape, rank, elem_size, nthreads, &pipe, &dims, &len)) return 1;

    LaneLease lanes;                    // (given back after the drain)
    DrainOnExit drain{stream, &cx.pending, cx.side, &lanes};
    EncodeCall c(cx, stream, std::move(pipe), std::move(dims), len, elem_size, d_src, d_dst, dst_capacity, dstoffset, fq, &lanes, stamps);
    for (size_t si = 0; si < c.pipe.stages.size(); ++si) {
        int rc = 0;
        switch (c.pipe.stages[si].kind) {
            case StageKind::bitswap1:          rc = c.bitswap1(si); break;
            case StageKind::raster_reorder:    rc = c.reorder(si, false); break;
            case StageKind::zcurve_reorder:    rc = c.reorder(si, true); break;
            case StageKind::rmestbkrd:         rc = c.rmestbkrd(); break;
            case StageKind::rmbkrd_neighbor5:  rc = c.rmbkrd_neighbor5(si); break;
            case StageKind::bitshuffle:        rc = c.bitshuffle(si); break;
            case StageKind::tile_shuffle:      rc = c.tile_shuffle(si); break;
            case StageKind::diff3x3x1:         rc = c.diff3x3x1(si); break;
            case StageKind::frame_shuffle:     rc = c.frame_shuffle(si); break;
            case StageKind::quantiser:         rc = c.quantiser(si); break;        // (may do the bitswap1 behind it as well)
            case StageKind::lz4:               rc = c.lz4_stage(si); break;
            case StageKind::pass_through:      rc = c.pass_through(); break;
            default:
                std::fprintf(stderr, "[sqeazy]\t stage %s is not implemented on MI355X\n", c.pipe.stages[si].name.c_str());
                return 1;
        }
        if (rc) return rc;
    }
    return c.finish(dstlength);
}

// dst_capacity < 0: the caller followed the reference protocol and allocated SQY_Pipeline_Max_Compressed_Length bytes
int encode_from_host(const char* pipeline, const char* src, long* shape, unsigned rank, int elem_size, char* dst,
                     long* dstlength, int nthreads, long dst_capacity = -1)
{
    if (!pipeline || !src || !shape || !dst || !dstlength) return 1;
    if (!pipeline_admitted(pipeline, elem_size)) return 1;   // sqeazy.cpp:81-82,118-119: invalid pipeline -> 1 before touching any buffer
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Workspace* ws = &lease.ctx->ws;
    hipStream_t stream = lease.ctx->own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    Pipeline pipe;
    std::vector<uint64_t> dims;
    uint64_t len = 0;
    if (admit_encode(pipeline, shape, rank, elem_size, nthreads, &pipe, &dims, &len)) return 1;      // (in front of the staging buffers)
    const uint64_t raw = len * (uint64_t)elem_size;
    // What the caller was told to allocate: SQY_Pipeline_Max_Compressed_Length_* evaluates the bound on a fresh
    // pipeline (n_threads = 1, sqeazy.cpp:144-231).  The reference itself writes past that for pipelines whose
    // header grows while encoding (frame_shuffle's reorder_map on stacks of many small frames); here the
    // documented "error 1 - destination buffer is not large enough" (inc/sqeazy.h:105) is returned instead.
    const uint64_t bound = dst_capacity >= 0 ? (uint64_t)dst_capacity : Pipeline::from_string(pipeline, elem_size).max_encoded_size(raw, elem_size);
    if (ws->io_src.ensure(std::max<uint64_t>(raw, 16)) || ws->io_dst.ensure(std::max<uint64_t>(bound, 16))) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    if (!lease.ctx->stager.copy(ws->io_src.p, const_cast<char*>(src), raw, true, dev_id)) { std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n"); return 1; }
    long out_len = 0, out_at = 0;
    const int rc = encode_on_device(*lease.ctx, pipeline, ws->io_src.p, shape, rank, elem_size, ws->io_dst.p, bound, &out_len, nthreads, stream, &out_at);
    if (rc) return rc;                  // (returns with the blob complete: the stream has been synchronised)
    if (!lease.ctx->stager.copy(static_cast<char*>(ws->io_dst.p) + out_at, dst, (size_t)out_len, false, dev_id)) { std::fprintf(stderr, "[sqeazy]\t device to host transfer failed\n"); return 1; }
    *dstlength = out_len;
    return 0;
}

// ---- decode --------------------------------------------------------------------------------------
// dynamic_pipeline::decode (dynamic_pipeline.hpp:740-846): tail filters^-1, sink^-1, head filters^-1 in reverse.
// the quantiser's decode LUT (256 x u16): from the file the configuration names, else base64 out of the header.  say: with the messages
bool quantiser_lut_on_host(const sqy::Stage& st, std::vector<unsigned char>* lut, bool say = true)
{
    auto lp = st.cfg.find("decode_lut_path");
    if (lp != st.cfg.end()) {
        // quantiser_scheme_impl.hpp:83-85: a path in the configuration wins over a LUT string
        lut->resize(512);
        if (!sqy::quantiser_lut_from_file(lp->second, reinterpret_cast<uint16_t*>(lut->data()), 256)) {
            if (say) std::fprintf(stderr, "lut from %s cannot be loaded, decoding skipped\n", lp->second.c_str());       // quantiser_utils.hpp:559-562
            return false;
        }
    } else {
        auto it = st.cfg.find("decode_lut_string");
        if (it == st.cfg.end() || !sqy::from_verbatim(it->second, lut)) { if (say) std::fprintf(stderr, "[sqeazy]\t quantiser: no decode_lut_string in the header\n"); return false; }
    }
    if (lut->size() != 512) { if (say) std::fprintf(stderr, "[sqeazy]\t quantiser: malformed decode LUT\n"); return false; }
    return true;
}

// .. into ws->small; synchronous: the host copy does not outlive the call
int quantiser_lut_to_device(const sqy::Stage& st, Workspace* ws)
{
    std::vector<unsigned char> lut;
    if (!quantiser_lut_on_host(st, &lut)) return 1;
    if (ws->small.ensure(4096)) return 1;
    SQY_HIP(hipMemcpy(ws->small.p, lut.data(), 512, hipMemcpyHostToDevice));
    return 0;
}

// The header of a blob is untrusted input: rank 1..16, every extent positive and below 2^31, fewer than 2^31 voxels (what one
// encode call can have produced), header and payload inside the blob.  *raw_bytes = decoded size.
bool header_shape_ok(const sqy::HeaderInfo& h, uint64_t srclen, uint64_t* raw_bytes)
{
    if (h.shape.empty() || h.shape.size() > 16) { std::fprintf(stderr, "[sqeazy]\t decode: header with rank %zu\n", h.shape.size()); return false; }
    uint64_t n = 1;
    for (uint64_t d : h.shape) {
        if (d == 0 || d >= ((uint64_t)1 << 31)) { std::fprintf(stderr, "[sqeazy]\t decode: header with an extent of %llu\n", (unsigned long long)d); return false; }
        n *= d;
        if (n >= ((uint64_t)1 << 31)) { std::fprintf(stderr, "[sqeazy]\t decode: header claims 2^31 or more voxels\n"); return false; }
    }
    const int elem = h.elem_size();
    if (elem != 1 && elem != 2) { std::fprintf(stderr, "[sqeazy]\t decode: blob holds %s voxels\n", h.type.c_str()); return false; }
    if (h.size > srclen || h.payload_bytes > srclen - h.size) { std::fprintf(stderr, "[sqeazy]\t decode: blob truncated\n"); return false; }
    *raw_bytes = n * (uint64_t)elem;
    return true;
}

// The last synchronisation of a decode: the LZ4 decoder's error flag (nullptr: no LZ4 decode ran) comes back with it, *raised says what it holds
int lz4_verdict(Context& cx, const uint32_t* flag, hipStream_t stream, bool* raised)
{
    if (flag) SQY_HIP(hipMemcpyAsync(cx.ws.pinned, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    if (g_prof_on.load()) prof_collect(cx.pending);
    *raised = flag && *static_cast<const uint32_t*>(cx.ws.pinned);
    return 0;
}

// Where the frames and blocks of an LZ4 payload are (lz4_frame_rank / lz4_frame_index), in ws->lz4_scratch and ws->csize
struct Lz4Index : sqy::Lz4DecodeGeometry {
    uint8_t* blk = nullptr;
    uint32_t* frame_first = nullptr;
    uint32_t* counts = nullptr;                  // [0..3] index result, [4] decode error flag
    uint32_t hc[8] = {0, 0, 100, 0, 0, 0, 0, 0}; // the index result read back: [0] frames, [1] blocks, [2] error code (100: not covered)
};
// frame_shuffle's inverse folded into the LZ4 decode: frames go to remap[f] * bytes (zero: the places no map entry names are zeroed first)
struct Lz4Remap { const uint64_t* map = nullptr; uint64_t bytes = 0; bool zero = false; };

// One decode call: the blob's header, the stream between the inverses, and what they hand each other.
struct DecodeCall {
    Context& cx;
    Workspace* ws;
    std::vector<PendingEvent>* pend;
    hipStream_t stream;
    void* d_dst;
    const sqy::HeaderInfo& h;
    Pipeline pipe;
    uint64_t n;                          // voxels
    // element size and count of the stream in front of every stage on the ENCODER's side: what its inverse produces
    // (the quantiser maps every voxel to one byte; pass_through re-types the voxels: elem times as many one-byte elements)
    std::vector<int> elem_before;
    std::vector<uint64_t> count_before;
    // the background filters decode as a copy (remove_estimated_background_scheme_impl.hpp:125-150, flatten_to_neighborhood_scheme_impl.hpp
    // :152-178): behind `lead` of them at the pipeline's front, stage `lead`'s inverse produces the volume
    size_t lead = 0;

    // the stream between the inverses
    const uint8_t* cur;
    uint64_t cur_bytes;
    bool use_ping = true;
    bool diff_in_place = false;            // the bit-plane inverse wrote into the volume itself; the diff3x3x1 inverse works there
    const uint32_t* lz4_flag = nullptr;    // the LZ4 decoder's error flag, read when the call ends
    int lz4_flag_stage = 0;
    // frame_shuffle's inverse: the reorder map out of the header (alive until the call's last synchronisation), and the places no map
    // entry names (maps that are no permutation)
    std::vector<unsigned char> fs_map;
    std::vector<uint64_t> fs_unnamed;

    DecodeCall(Context& c, hipStream_t s, void* dst, const sqy::HeaderInfo& hi, Pipeline&& p, uint64_t voxels, const uint8_t* payload)
        : cx(c), ws(&c.ws), pend(&c.pending), stream(s), d_dst(dst), h(hi), pipe(std::move(p)), n(voxels), elem_before(pipe.stages.size()), count_before(pipe.stages.size()), cur(payload), cur_bytes(hi.payload_bytes)
    {
        int e = h.elem_size();
        uint64_t cnt = n;
        for (size_t i = 0; i < pipe.stages.size(); ++i) {
            elem_before[i] = e;
            count_before[i] = cnt;
            if (pipe.stages[i].kind == StageKind::quantiser) e = 1;
            if (pipe.stages[i].kind == StageKind::pass_through) { cnt *= (uint64_t)e; e = 1; }
        }
        while (lead < pipe.stages.size() && (pipe.stages[lead].kind == StageKind::rmestbkrd || pipe.stages[lead].kind == StageKind::rmbkrd_neighbor5)) ++lead;
    }

    // composite return codes of dynamic_pipeline::detail_decode (dynamic_pipeline.hpp:795-846): a failing tail filter
    // returns its code, a failing sink code + 10, a failing head filter code + 100
    int stage_error(size_t si) const { return is_tail(si) ? 1 : (int)si == pipe.sink_index ? 1 + 10 : 1 + 100; }
    int produced(const uint8_t* out, uint64_t bytes) { cur = out; cur_bytes = bytes; return 0; }   // the next inverse's input
    bool is_tail(size_t si) const { return pipe.sink_index >= 0 && (int)si > pipe.sink_index; }
    bool preceded_by(size_t si, StageKind k) const { return si >= 1 && pipe.stages[si - 1].kind == k; }
    uint64_t in_bytes(size_t si) const { return count_before[si] * (uint64_t)elem_before[si]; }   // bytes the inverse has to produce
    uint8_t* work_buf(uint64_t bytes)                                  // the next buffer of the ping/pong rotation
    {
        DevBuf& b = use_ping ? ws->ping : ws->pong;
        use_ping = !use_ping;
        return b.ensure(std::max<uint64_t>(bytes, 16)) ? nullptr : static_cast<uint8_t*>(b.p);
    }
    // the first stage's inverse produces the volume
    uint8_t* out_buf(size_t stage_index, uint64_t bytes) { return stage_index <= lead ? static_cast<uint8_t*>(d_dst) : work_buf(bytes); }
    // the shape a 3-D stage saw on the encoder's side (h.shape.size() == 3 checked by the caller): the volume's, or {1, 1, bytes} behind
    // a sink that did not write one byte per voxel (dynamic_pipeline.hpp:658-666)
    void stage_shape(size_t si, uint64_t& Z, uint64_t& Y, uint64_t& X) const
    {
        const bool flat = is_tail(si) && count_before[si] != n;
        Z = flat ? 1 : h.shape[0]; Y = flat ? 1 : h.shape[1]; X = flat ? count_before[si] : h.shape[2];
    }

    // zeros where nobody writes: the places the map does not name (round 6: not the whole volume -- the C4 stack's map leaves a few of its
    // 1024 places out, and clearing 1 GiB for them was 0.25 of the decode's 0.85 ms)
    int zero_unnamed_places(uint8_t* out, uint64_t place_bytes, uint64_t bytes)
    {
        // (a memset's launch costs about what 25 MB of it cost the memory)
        if (fs_unnamed.size() * (place_bytes + (25ull << 20)) >= bytes) { SQY_HIP(hipMemsetAsync(out, 0, bytes, stream)); return 0; }
        for (uint64_t v : fs_unnamed) SQY_HIP(hipMemsetAsync(out + v * place_bytes, 0, place_bytes, stream));
        return 0;
    }

    // frame_shuffle's inverse: the reorder map out of the header, checked and sent to the device (ws->small).  Used by the stage itself and
    // by the LZ4 stage behind it, which decodes its frames straight to their places when it can (round 5).
    int frame_shuffle_prepare(size_t fi, uint64_t& Z, uint64_t& frame_bytes_dec, bool& permutation)
    {
        if (const int rc = frame_shuffle_map(fi, Z, frame_bytes_dec, permutation)) return rc;
        if (ws->small.ensure(std::max<uint64_t>(Z * 8, 4096))) return 1;
        SQY_HIP(hipMemcpyAsync(ws->small.p, fs_map.data(), Z * 8, hipMemcpyHostToDevice, stream));
        SQY_HIP(hipStreamSynchronize(stream));                                   // (pageable source: gone from the host's side before anything can return)
        return 0;
    }
    // .. its host part: fs_map (the device's copy, struck slots ~0) and fs_unnamed
    int frame_shuffle_map(size_t fi, uint64_t& Z, uint64_t& frame_bytes_dec, bool& permutation)
    {
        const Stage& fs = pipe.stages[fi];
        if (h.shape.size() != 3) return 1;
        auto it = fs.cfg.find("reorder_map");
        // (as a tail filter behind a sink that did not write one byte per voxel the stream is ONE frame: {1, 1, bytes})
        const uint64_t fcs = frame_chunk_size(fs);
        uint64_t Z0, Y, X;
        stage_shape(fi, Z0, Y, X);
        if (fcs == 0 || Z0 % fcs != 0) { std::fprintf(stderr, "[sqeazy]\t frame_shuffle: frame_chunk_size does not divide the frames\n"); return 1; }
        Z = Z0 / fcs;
        frame_bytes_dec = Y * X * (uint64_t)elem_before[fi] * fcs;
        if (it == fs.cfg.end() || !sqy::from_verbatim(it->second, &fs_map)) { std::fprintf(stderr, "[sqeazy]\t frame_shuffle: no reorder_map in the header\n"); return 1; }
        if (!sqy::frame_shuffle_decode_map(&fs_map, Z, &fs_unnamed, &permutation)) {
            std::fprintf(stderr, fs_map.size() != Z * 8 ? "[sqeazy]\t frame_shuffle: malformed reorder_map\n" : "[sqeazy]\t frame_shuffle: reorder_map out of range\n");
            return 1;
        }
        return 0;
    }
    // frame_shuffle right in front of the LZ4 stage si (on the encoder's side), both on the same `total` bytes of a 3-D volume
    bool shuffle_in_front(size_t si, uint64_t total) const
    {
        return preceded_by(si, StageKind::frame_shuffle) && in_bytes(si - 1) == total && h.shape.size() == 3;
    }
    // .. and the chunked layout with every chunk inside one of the shuffle's Z places of fb bytes: *fold, the LZ4 frames can be decoded
    // straight to where the shuffle's inverse would move them (fs_map; upload: in ws->small as well)
    int shuffle_fold(size_t si, uint64_t total, const sqy::Lz4DecodeGeometry& g, uint64_t nframes, bool upload, uint64_t& Z, uint64_t& fb, bool& permutation, bool* fold)
    {
        *fold = false;
        if (!(shuffle_in_front(si, total) && sqy::lz4_chunks_whole(nframes, g.nchunks, total, g.chunk))) return 0;
        if (const int rc = upload ? frame_shuffle_prepare(si - 1, Z, fb, permutation) : frame_shuffle_map(si - 1, Z, fb, permutation)) return rc;
        *fold = sqy::lz4_folds_into_shuffle(nframes, g.nchunks, total, g.chunk, Z, fb);
        return 0;
    }

    // The LZ4 frames' inverse: the frame index, then the frames decoded -- with frame_shuffle in front straight to the places its inverse
    // would move them to, which then is done as well
    int lz4(size_t& si)
    {
        const uint64_t total = in_bytes(si);
        Lz4Index ix;
        if (const int rc = lz4_index(si, total, ix)) return rc;
        Lz4Remap rm;
        if (const int rc = lz4_remap(si, total, ix, rm)) return rc;
        uint8_t* out = out_buf(rm.map ? si - 1 : si, total);
        if (!out) return 1;
        if (rm.zero) { if (const int rc = zero_unnamed_places(out, rm.bytes, total)) return rc; }   // (frames nobody names come out as zeros, as behind the stage's own inverse)
        bool decoded = false;
        if (lz4_linked_parallel(ix, out, total, &decoded)) return 1;
        if (!decoded && lz4_frames(si, ix, out, total, rm)) return 1;
        if (rm.map) si -= 1;                                       // the frame_shuffle stage is done as well
        return produced(out, total);
    }

    int lz4_index(size_t si, uint64_t total, Lz4Index& ix)
    {
        const Stage& st = pipe.stages[si];
        static_cast<sqy::Lz4DecodeGeometry&>(ix) = sqy::lz4_decode_geometry(st.lz4, total);
        const uint64_t max_blocks = ix.max_blocks;
        // block list, frame starts, and a table of frame-start candidates (16 B x >= 8 slots per expected frame)
        const uint64_t idx_bytes = (max_blocks * 16 + (max_blocks + 2) * 4 + 64 + 15) & ~15ull;
        const uint64_t cand_bytes = sqy::lz4_frame_rank_scratch_bytes(ix.nchunks);
        if (ws->lz4_scratch.ensure(idx_bytes + cand_bytes)) return 1;
        ix.blk = static_cast<uint8_t*>(ws->lz4_scratch.p);
        ix.frame_first = reinterpret_cast<uint32_t*>(ix.blk + max_blocks * 16);
        void* cand = ix.blk + idx_bytes;
        if (ws->csize.ensure(64)) return 1;
        ix.counts = static_cast<uint32_t*>(ws->csize.p);
        SQY_HIP(hipMemsetAsync(ix.counts, 0, 64, stream));
        if (ix.nchunks > 1) {
            // chunked layout expected: rank the frame list in parallel.  The frames at the stream's end that are stored blocks of
            // the chunk size are found where they must start, not by the scan (hc[6] of them); should the ranking give up with
            // such a tail, the whole stream is scanned before the walk below is tried.
            for (int with_tail = g_opt.stored_tail_index.load() ? 1 : 0; with_tail >= 0; --with_tail) {
                SQY_TIMED("lz4_frame_rank", sqy::launch_lz4_frame_rank(cur, cur_bytes, ix.blk, ix.frame_first, max_blocks, ix.counts, ix.nchunks, cand, stream,
                                                                       with_tail ? ix.chunk : 0, with_tail ? total - (ix.nchunks - 1) * ix.chunk : 0));
                SQY_HIP(hipMemcpyAsync(ix.hc, ix.counts, sizeof(ix.hc), hipMemcpyDeviceToHost, stream));
                SQY_HIP(hipStreamSynchronize(stream));
                if (ix.hc[2] != 100 || ix.hc[6] == 0) break;
                SQY_HIP(hipMemsetAsync(ix.counts, 0, 64, stream));
            }
        }
        if (ix.hc[2] == 100) {
            // one frame, the serial block-linked layout, or anything the parallel ranking does not cover
            SQY_TIMED("lz4_frame_index", sqy::launch_lz4_frame_index(cur, cur_bytes, ix.blk, ix.frame_first, max_blocks, ix.counts, stream));
            SQY_HIP(hipMemcpyAsync(ix.hc, ix.counts, sizeof(ix.hc), hipMemcpyDeviceToHost, stream));
            SQY_HIP(hipStreamSynchronize(stream));
        }
        if (ix.hc[2]) { std::fprintf(stderr, "[sqy::lz4] corrupt LZ4 frame stream (code %u)\n", ix.hc[2]); return stage_error(si); }
        const uint32_t nframes = ix.hc[0];
        if (nframes > 1 && nframes != ix.nchunks) {
            std::fprintf(stderr, "[sqy::lz4] %u frames where %llu chunks were expected\n", nframes, (unsigned long long)ix.nchunks);
            return stage_error(si);
        }
        if (nframes == 0 && total > 0) {
            std::fprintf(stderr, "[sqy::lz4] no LZ4 frame in the payload, %llu bytes expected\n", (unsigned long long)total);
            return stage_error(si);
        }
        return 0;
    }

    // frame_shuffle right in front (on the encoder's side), the chunked layout, every chunk inside one of its frames: the frames
    // are decoded straight to where the shuffle's inverse would move them (round 5: one pass over the volume less -- the C4
    // config's decode 1.49 -> 1.1 ms)
    int lz4_remap(size_t si, uint64_t total, const Lz4Index& ix, Lz4Remap& rm)
    {
        uint64_t Z = 0, fb = 0;
        bool permutation = true, fold = false;
        if (const int rc = shuffle_fold(si, total, ix, ix.hc[0], true, Z, fb, permutation, &fold)) return rc;
        // (round-5 advice) a map that names a place twice -- frames of equal metric on the encoder's side, or a crafted blob --:
        // several LZ4 frames must not decode into one place at once (the ring kernels read matches that reach behind their
        // ring back from there).  The device's copy of such a map has every frame but the last one named for a place struck
        // (frame_shuffle_prepare): struck frames are not decoded, the places nobody names are zeroed first.
        if (fold) {
            rm.map = static_cast<const uint64_t*>(ws->small.p);
            rm.bytes = fb;
            rm.zero = !permutation;
        }
        return 0;
    }

    // ONE block-linked frame (nthreads = 1 on the encoder's side): every block at once with the history as an unknown, the
    // references resolved afterwards (sqy_kernels.hip: lz4_blocks_decode_sym_kernel).  A stream that is not a frame of
    // full blocks, or is damaged, raises the flag: *decoded stays false, and the one-wavefront walk (lz4_frames) decides, as in rounds 2-3.
    int lz4_linked_parallel(const Lz4Index& ix, uint8_t* out, uint64_t total, bool* decoded)
    {
        const bool par_wanted = ix.hc[0] == 1 && g_opt.block_parallel.load() && sqy::lz4_linked_decode_parallel_possible(ix.hc[1], total, ix.block_bytes);
        const bool par_room = par_wanted && !ws->spec.ensure(((total * sizeof(uint16_t) + 255) & ~(uint64_t)255) + sqy::lz4_linked_decode_scan_scratch_bytes(ix.hc[1]), true);
        if (par_wanted && !par_room) {
            // (round-4 advice) the references need 2 bytes per decoded byte; without them the walk decodes the frame -- said once
            static std::atomic<bool> told{false};
            if (!told.exchange(true))
                std::fprintf(stderr, "[sqeazy]\t lz4: no HBM for the block-parallel decode's references (%llu MiB): the block-linked frame is decoded "
                                     "by one wavefront (same bytes, hundreds of times slower)\n", (unsigned long long)((total * sizeof(uint16_t)) >> 20));
        }
        if (!par_room) return 0;                                   // (no room for the references: the walk needs none)
        hipError_t le;
        {
            ProfScope ps("lz4_linked_decode", stream, pend);
            uint8_t* scan = static_cast<uint8_t*>(ws->spec.p) + ((total * sizeof(uint16_t) + 255) & ~(uint64_t)255);
            le = sqy::launch_lz4_linked_decode_parallel(cur, ix.blk, ix.hc[1], out, static_cast<uint16_t*>(ws->spec.p), total, ix.block_bytes,
                                                        ix.counts + 4, stream, g_opt.tail_scan.load() ? scan : nullptr);
        }
        if (le != hipSuccess) (void)hipGetLastError();                    // (e.g. no 128 KiB of LDS for the tails: the walk)
        uint32_t bad = 0;
        SQY_HIP(hipMemcpyAsync(&bad, ix.counts + 4, sizeof(bad), hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        *decoded = le == hipSuccess && bad == 0;
        if (!*decoded) SQY_HIP(hipMemsetAsync(ix.counts + 4, 0, sizeof(uint32_t), stream));
        return 0;
    }

    // every frame by its own wavefront(s), the stored ones copied on the side stream
    int lz4_frames(size_t si, const Lz4Index& ix, uint8_t* out, uint64_t total, const Lz4Remap& rm)
    {
        const uint32_t nframes = ix.hc[0];
        {
            const bool side_ok = cx.ensure_side();           // (without it the copy simply follows on the same stream)
            SQY_TIMED("lz4_frames_decode", sqy::launch_lz4_frames_decode(cur, ix.blk, ix.frame_first, nframes, out, total, ix.chunk, ix.block_bytes, ix.hc[3], ix.counts + 4, stream,
                                                                         side_ok ? cx.side : nullptr, cx.fork, cx.join, rm.map, rm.bytes,
                                                                         g_opt.decode_two_waves.load() && ix.hc[1] == nframes));
        }
        // (the decoder's verdict is read at the END of the call, with the call's last synchronisation: the stages in between are
        // plain data movement and stay inside their buffers whatever the bytes are -- one host round trip less per decode)
        lz4_flag = ix.counts + 4;
        lz4_flag_stage = (int)si;
        return 0;
    }

    int bitswap1(size_t& si)
    {
        const int e_in = elem_before[si];
        const uint64_t n_in = count_before[si];
        // quantiser right in front (on the encoder's side): the inverse transpose and the quantiser's look-up in one pass
        if (e_in == 1 && preceded_by(si, StageKind::quantiser) && count_before[si - 1] == n_in && elem_before[si - 1] == 2) {
            if (quantiser_lut_to_device(pipe.stages[si - 1], ws)) return 1;
            uint8_t* out16 = out_buf(si - 1, n_in * 2);
            if (!out16) return 1;
            if (sqy::bitswap1_u8_decode_lut_possible(cur, out16, n_in)) {
                SQY_TIMED("bitswap1_quantiser_decode", sqy::launch_bitswap1_u8_decode_lut(cur, reinterpret_cast<uint16_t*>(out16), n_in,
                                                                                          static_cast<const uint16_t*>(ws->small.p), stream));
                si -= 1;                                           // the quantiser stage is done as well
                return produced(out16, n_in * 2);
            }
            // (odd sizes: the two stages one after the other; out16 is the output buffer of quantiser())
            if (si - 1 > lead) use_ping = !use_ping;               // hand the buffer back to the quantiser stage
        }
        // diff3x3x1 as the pipeline's first stage (16-bit, the usual geometry): its inverse can only change the leading columns of
        // a row, so the planes are transposed straight into the volume and the inverse works there (round 4; before: into a
        // work buffer, from which the inverse copied every untouched column -- 0.75 ms of a 2 GiB slab's 1.1)
        uint8_t* out = nullptr;
        if (si == 1 && pipe.stages[0].kind == StageKind::diff3x3x1 && e_in == 2 && h.shape.size() == 3 && n_in == n &&
            (reinterpret_cast<uintptr_t>(d_dst) & 15) == 0 && sqy::diff3x3x1_decode_chain_columns(h.shape[0], h.shape[1], h.shape[2], 2)) {
            out = static_cast<uint8_t*>(d_dst);
            diff_in_place = true;
        } else
            out = out_buf(si, in_bytes(si));
        if (!out) return 1;
        SQY_TIMED("bitswap1_decode", sqy::launch_bitswap1_decode(cur, out, n_in, e_in, stream));
        return produced(out, in_bytes(si));
    }

    // raster_reorder and zcurve_reorder (one kernel, see the encoder's side)
    int reorder(size_t si, bool zcurve)
    {
        if (h.shape.size() != 3) return zcurve ? stage_error(si) : 1;
        const Stage& st = pipe.stages[si];
        auto t = st.cfg.find("tile_size");
        const uint64_t ts = t != st.cfg.end() ? (uint64_t)std::atoi(t->second.c_str()) : (zcurve ? 2 : 0);
        uint64_t Z, Y, X;
        stage_shape(si, Z, Y, X);                                  // (tail filter: the sink's char stream)
        if (zcurve ? !sqy::zcurve_geometry_defined(Z, Y, X, ts) : !sqy::raster_geometry_defined(Z, Y, X, ts, elem_before[si])) {
            std::fprintf(stderr, "[sqeazy]\t %s: tile_size %llu does not fit the shape\n", zcurve ? "zcurve_reorder" : "raster_reorder", (unsigned long long)ts);
            return stage_error(si);
        }
        uint8_t* out = out_buf(si, in_bytes(si));
        if (!out) return 1;
        SQY_TIMED(zcurve ? "zcurve_reorder_decode" : "raster_reorder_decode", sqy::launch_raster_reorder(cur, out, Z, Y, X, ts, elem_before[si], true, stream));
        return produced(out, in_bytes(si));
    }

    int bitshuffle(size_t si)
    {
        const Stage& st = pipe.stages[si];
        const int e_here = is_tail(si) ? 1 : elem_before[si];     // tail filters work on the sink's bytes
        auto b = st.cfg.find("block_size");
        const uint64_t be = sqy::bitshuffle_block_elems(e_here, b != st.cfg.end() ? (uint64_t)std::atoi(b->second.c_str()) : 0);
        if (!be) return stage_error(si);
        uint8_t* out = out_buf(si, in_bytes(si));
        if (!out) return 1;
        SQY_TIMED("bitshuffle_decode", sqy::launch_bitshuffle(cur, out, in_bytes(si) / (uint64_t)e_here, e_here, be, true, stream));
        return produced(out, in_bytes(si));
    }

    int tile_shuffle(size_t si)
    {
        if (h.shape.size() != 3) return stage_error(si);
        const Stage& st = pipe.stages[si];
        auto t = st.cfg.find("tile_size");
        const uint64_t ts = t != st.cfg.end() ? (uint64_t)std::atoi(t->second.c_str()) : 32;
        uint64_t Z, Y, X;
        stage_shape(si, Z, Y, X);
        if (!sqy::tile_shuffle_geometry_defined(Z, Y, X, ts)) {
            std::fprintf(stderr, "[sqeazy]\t tile_shuffle: tile_size %llu does not divide the shape\n", (unsigned long long)ts);
            return stage_error(si);
        }
        auto it = st.cfg.find("reorder_map");
        const uint64_t stage_in_bytes = in_bytes(si);
        const uint64_t per_tile = ts * ts * ts, ntiles = count_before[si] / per_tile, tile_bytes = per_tile * (uint64_t)elem_before[si];
        std::vector<unsigned char> mapb;
        if (it == st.cfg.end() || !sqy::from_verbatim(it->second, &mapb)) { std::fprintf(stderr, "[sqeazy]\t tile_shuffle: no reorder_map in the header\n"); return stage_error(si); }
        if (mapb.size() != ntiles * 8) { std::fprintf(stderr, "[sqeazy]\t tile_shuffle: malformed reorder_map\n"); return stage_error(si); }
        // tile_shuffle_utils.hpp:473-482: encoded tile i goes to slot map[i], a later i wins, unnamed slots stay zero:
        // as a gather, slot t takes the LAST i that names it
        std::vector<uint64_t> src_of(ntiles, ~0ull);
        for (uint64_t i = 0; i < ntiles; ++i) {
            uint64_t v; std::memcpy(&v, mapb.data() + 8 * i, 8);
            if (v >= ntiles) { std::fprintf(stderr, "[sqeazy]\t tile_shuffle: reorder_map out of range\n"); return stage_error(si); }
            src_of[v] = i;
        }
        if (ws->small.ensure(std::max<uint64_t>(ntiles * 8, 4096))) return 1;
        SQY_HIP(hipMemcpyAsync(ws->small.p, src_of.data(), ntiles * 8, hipMemcpyHostToDevice, stream));
        uint8_t* tb = work_buf(stage_in_bytes);                         // tile-major intermediate
        if (!tb) return 1;
        SQY_TIMED("tile_unshuffle", sqy::launch_frame_gather(cur, tb, ntiles, tile_bytes, static_cast<const uint64_t*>(ws->small.p), stream));
        SQY_HIP(hipStreamSynchronize(stream));                          // src_of (host) is read by the async copy above
        uint8_t* out = out_buf(si, stage_in_bytes);
        if (!out) return 1;
        SQY_TIMED("tile_scatter", sqy::launch_raster_reorder(tb, out, Z, Y, X, ts, elem_before[si], true, stream));
        return produced(out, stage_in_bytes);
    }

    int diff3x3x1(size_t si)
    {
        if (h.shape.size() != 3) return 1;
        // as a tail filter (behind the sink) the stream is `char` and has the volume's shape only when the sink wrote one
        // byte per voxel (dynamic_pipeline.hpp:658-666); anything else the encoder refused
        const bool tail = is_tail(si);
        if (tail && (count_before[si] != n || elem_before[si] != 1)) return stage_error(si);
        uint8_t* out = out_buf(si, in_bytes(si));
        if (!out) return 1;
        void* left_tmp = nullptr;
        if (si == 0 && diff_in_place && cur == out) {              // the bit-plane inverse wrote the volume's own memory (bitswap1)
            left_tmp = work_buf(in_bytes(si));
            if (!left_tmp) return 1;
        }
        ProfScope ps("diff3x3x1_decode", stream, pend);
        const bool side_ok = cx.ensure_side();
        SQY_HIP(sqy::launch_diff3x3x1_decode(cur, out, h.shape[0], h.shape[1], h.shape[2], elem_before[si], ws->lz4_scratch.p, stream, tail,
                                             side_ok ? cx.side : nullptr, cx.fork, cx.join, left_tmp));
        return produced(out, in_bytes(si));
    }

    int quantiser(size_t si)
    {
        if (quantiser_lut_to_device(pipe.stages[si], ws)) return 1;
        uint8_t* out = out_buf(si, in_bytes(si));
        if (!out) return 1;
        SQY_TIMED("quantiser_decode", sqy::launch_quantiser_decode(cur, reinterpret_cast<uint16_t*>(out), n, static_cast<const uint16_t*>(ws->small.p), stream));
        SQY_HIP(hipStreamSynchronize(stream));
        return produced(out, in_bytes(si));
    }

    int frame_shuffle(size_t si)
    {
        uint64_t Z = 0, frame_bytes_dec = 0;
        bool permutation = true;
        if (const int rc = frame_shuffle_prepare(si, Z, frame_bytes_dec, permutation)) return rc;
        uint8_t* out = out_buf(si, in_bytes(si));
        if (!out) return 1;
        // Frames with equal metrics share ONE source frame in the encoder (std::find, frame_shuffle_utils.hpp:158-161): the map then
        // names a frame twice and others not at all.  The reference's decode leaves the frames nobody names as the output
        // buffer had them (frame_shuffle_utils.hpp:337-344); here they come out as zeros, not as whatever the
        // workspace held.
        if (!permutation) { if (const int rc = zero_unnamed_places(out, frame_bytes_dec, in_bytes(si))) return rc; }
        SQY_TIMED("frame_scatter", sqy::launch_frame_scatter(cur, out, Z, frame_bytes_dec, static_cast<const uint64_t*>(ws->small.p), stream));
        return produced(out, in_bytes(si));
    }

    // the call's last synchronisation, and with it the LZ4 decoder's verdict
    int finish()
    {
        bool raised = false;
        if (const int rc = lz4_verdict(cx, lz4_flag, stream, &raised)) return rc;
        if (!raised) return 0;
        std::fprintf(stderr, "[sqy::lz4] corrupt LZ4 block, or a frame that does not decode to its share of the volume\n");
        return stage_error((size_t)lz4_flag_stage);
    }

    // ---- frame-range decode (SQYAMD_Decode_Frames_*, SQYAMD_Decode_Box_*) ----
    // The LZ4 frames that frames [z0, z0 + nz) of the volume need, decoded into range_buf.  Taken for the chunked layout of
    // [heads ->] lz4 | bitswap1->lz4 | quantiser->bitswap1->lz4 | frame_shuffle->lz4  (the background heads decode as a copy);
    // *taken = false for anything else, with nothing written (the caller decodes the whole blob).  The decoder's verdict is left in
    // lz4_flag, as by lz4_frames.  What follows is the caller's: frames_range_out (the frames, dense, into d_dst) or box_range_out (a box of
    // them into a view).  direct_ok: a shuffle range on place boundaries may be decoded straight into d_dst (range_buf == d_dst then)
    std::vector<unsigned char> sub_host;   // the tables uploaded to ws->subset (alive until the call's last synchronisation)
    sqy::RangeForm range_form = sqy::RangeForm::plain;
    sqy::FrameRangePlan range_plan;        // (direct: only where direct_ok)
    uint8_t* range_buf = nullptr;

    int frames_subset(uint64_t z0, uint64_t nz, bool direct_ok, bool* taken)
    {
        if (const int rc = frames_subset(std::vector<std::pair<uint64_t, uint64_t>>{{z0, nz}}, direct_ok, taken)) return rc;
        range_plan = sqy::frame_range_plan_of(ranges_plan, 0);
        range_plan.direct = range_plan.direct && direct_ok;
        return 0;
    }

    // the same for a set of ranges (z0, nz) (SQYAMD_Decode_Boxes_*): one table upload, one LZ4 launch over the united frames into one
    // buffer; ranges_plan says where each range lies in there.  direct_ok: one range only
    sqy::FrameRangesPlan ranges_plan;
    Lz4Index range_ix;                      // the frame index the subset was taken from (valid where *taken)
    int frames_subset(const std::vector<std::pair<uint64_t, uint64_t>>& ranges, bool direct_ok, bool* taken)
    {
        *taken = false;
        const size_t ns = pipe.stages.size();
        if (ns == 0 || pipe.stages[ns - 1].kind != StageKind::lz4 || lead >= ns) return 0;
        const size_t li = ns - 1, nfront = li - lead;
        auto kind = [&](size_t i) { return pipe.stages[i].kind; };
        typedef sqy::RangeForm Form;
        Form form;
        if (nfront == 0) form = Form::plain;
        else if (nfront == 1 && kind(lead) == StageKind::bitswap1) form = Form::planes;
        else if (nfront == 1 && kind(lead) == StageKind::frame_shuffle) form = Form::shuffle;
        else if (nfront == 2 && kind(lead) == StageKind::quantiser && kind(lead + 1) == StageKind::bitswap1) form = Form::planes_lut;
        else return 0;
        const int e = h.elem_size();
        const uint64_t total = in_bytes(li);
        // the stream in front of lz4 holds the voxels in their order (planes_lut: one quantised byte per voxel)
        if (total != n * (uint64_t)(form == Form::planes_lut ? 1 : e)) return 0;
        if (form == Form::planes && (elem_before[lead] != e || count_before[lead] != n)) return 0;
        if (form == Form::planes_lut && (e != 2 || elem_before[lead + 1] != 1 || count_before[lead + 1] != n)) return 0;
        if (form == Form::shuffle && !shuffle_in_front(li, total)) return 0;
        Lz4Index ix;
        if (const int rc = lz4_index(li, total, ix)) return rc;
        const uint32_t nframes = ix.hc[0];
        if (nframes < 2 || nframes != ix.nchunks) return 0;          // one frame, or the serial layout: the history runs from the start
        const uint64_t chunk = ix.chunk;
        uint64_t P = 0, fbp = 0;                                       // shuffle: P places of fbp bytes
        if (form == Form::shuffle) {
            bool permutation = true, fold = false;
            if (const int rc = shuffle_fold(li, total, ix, nframes, true, P, fbp, permutation, &fold)) return rc;
            if (!fold) return 0;
        }
        // the LZ4 frames the range needs and where its bytes lie behind their decode
        ranges_plan = sqy::frame_ranges_plan(form, n, e, h.shape[0], ranges, chunk, total, nframes, fs_map, fbp, P);
        range_form = form;
        const sqy::FrameRangesPlan& p = ranges_plan;
        if (!p.ok) return 0;
        const bool direct = direct_ok && ranges.size() == 1 && p.boxes[0].direct;

        // the tables: ids | subset frame starts | remap | subset block index
        const uint64_t nsel = p.ids.size(), mpf = (chunk + ix.block_bytes - 1) / ix.block_bytes;
        const uint64_t o_ff = (nsel * 4 + 15) & ~15ull, o_map = o_ff + (((nsel + 1) * 4 + 15) & ~15ull), o_blk = o_map + ((p.remap.size() * 8 + 15) & ~15ull);
        if (ws->subset.ensure(std::max<uint64_t>(o_blk + nsel * mpf * 16, 16))) return 1;
        sub_host.assign(o_blk, 0);
        if (nsel) std::memcpy(sub_host.data(), p.ids.data(), nsel * 4);
        if (!p.remap.empty()) std::memcpy(sub_host.data() + o_map, p.remap.data(), p.remap.size() * 8);
        uint8_t* d_sub = static_cast<uint8_t*>(ws->subset.p);
        if (o_blk) SQY_HIP(hipMemcpyAsync(d_sub, sub_host.data(), o_blk, hipMemcpyHostToDevice, stream));

        *taken = true;
        range_ix = ix;
        // shuffle with the range on place boundaries (frame_chunk_size 1): straight into d_dst; else through the workspace
        uint8_t* sbuf = direct ? static_cast<uint8_t*>(d_dst) : work_buf(p.out_bytes);       // where the subset decodes to
        if (!sbuf) return 1;
        // places of the range that no slot names come out as zeros (frame_shuffle's inverse)
        for (const auto& run : p.zero_runs) SQY_HIP(hipMemsetAsync(sbuf + run.first * fbp, 0, (run.second - run.first) * fbp, stream));
        if (nsel) {
            SQY_TIMED("lz4_frames_subset_decode",
                      sqy::launch_lz4_frames_subset_decode(cur, ix.blk, ix.frame_first, nframes, reinterpret_cast<const uint32_t*>(d_sub), (uint32_t)nsel,
                                                           (uint32_t)mpf, d_sub + o_blk, reinterpret_cast<uint32_t*>(d_sub + o_ff), sbuf, p.out_bytes, chunk,
                                                           ix.block_bytes, ix.hc[3], ix.counts + 4, stream,
                                                           form == Form::shuffle ? reinterpret_cast<const uint64_t*>(d_sub + o_map) : nullptr, fbp,
                                                           g_opt.decode_two_waves.load() && ix.hc[1] == nframes));
            lz4_flag = ix.counts + 4;
            lz4_flag_stage = (int)li;
        }
        range_buf = sbuf;
        return 0;
    }

    // the planes of range_plan for the range transposers, the quantiser's decode table on the device where the form has one
    int range_planes(sqy::Bitswap1Range* r, const uint16_t** lut)
    {
        const sqy::FrameRangePlan& p = range_plan;
        *r = sqy::Bitswap1Range{};
        std::copy(p.plane, p.plane + 16, r->plane);
        r->tail = p.tail; r->w0 = p.w0; r->w1 = p.w1; r->v0 = p.v0; r->v1 = p.v1; r->L = p.L;
        return range_lut(lut);
    }
    int range_lut(const uint16_t** lut)
    {
        *lut = nullptr;
        if (range_form == sqy::RangeForm::planes_lut) {
            if (quantiser_lut_to_device(pipe.stages[lead], ws)) return 1;
            *lut = static_cast<const uint16_t*>(ws->small.p);
        }
        return 0;
    }

    // SQYAMD_Decode_Frames_*' last launch behind frames_subset: the nz frames of fb bytes, dense, into d_dst
    int frames_range_out(uint64_t nz, uint64_t fb)
    {
        typedef sqy::RangeForm Form;
        const sqy::FrameRangePlan& p = range_plan;
        if (range_form == Form::plain || (range_form == Form::shuffle && !p.direct)) {
            SQY_TIMED("frames_range_copy", hipMemcpyAsync(d_dst, range_buf + p.range_at, nz * fb, hipMemcpyDeviceToDevice, stream));
        } else if (range_form != Form::shuffle) {
            sqy::Bitswap1Range r;
            const uint16_t* lut = nullptr;
            if (range_planes(&r, &lut)) return 1;
            SQY_TIMED(lut ? "bitswap1_quantiser_decode_range" : "bitswap1_decode_range",
                      sqy::launch_bitswap1_decode_range(range_buf, d_dst, r, p.we, lut, stream));
        }
        return 0;
    }
};

// the header of a blob in device memory: a prefix of the blob fetched, grown until the delimiter is inside
int fetch_header(const uint8_t* d_src, uint64_t srclen, hipStream_t stream, sqy::HeaderInfo& h)
{
    std::vector<char> head;
    for (uint64_t want = 1 << 16;; want *= 16) {
        const uint64_t take = std::min<uint64_t>(want, srclen);
        head.resize(take);
        SQY_HIP(hipMemcpyAsync(head.data(), d_src, take, hipMemcpyDeviceToHost, stream));
        SQY_HIP(hipStreamSynchronize(stream));
        h = sqy::header_unpack(head.data(), head.data() + take);
        if (h.valid || take == srclen) break;
    }
    if (!h.valid) { std::fprintf(stderr, "[sqeazy]\t unable to find a sqy header in the blob\n"); return 1; }
    return 0;
}

// The inverses of stages [0, from) in reverse order, from c.cur on (from = the stage count: the whole pipeline; the slab-set decode starts
// behind an LZ4 stage that has already run).  The result is c.cur; the caller moves it to d_dst when it is not there.
int decode_stages(DecodeCall& c, size_t from)
{
    for (size_t si = from; si-- > 0;) {
        int rc = 0;
        switch (c.pipe.stages[si].kind) {
            case StageKind::lz4:               rc = c.lz4(si); break;              // (may do the frame_shuffle in front as well)
            case StageKind::bitswap1:          rc = c.bitswap1(si); break;         // (may do the quantiser in front as well)
            case StageKind::raster_reorder:    rc = c.reorder(si, false); break;
            case StageKind::zcurve_reorder:    rc = c.reorder(si, true); break;
            case StageKind::bitshuffle:        rc = c.bitshuffle(si); break;
            case StageKind::tile_shuffle:      rc = c.tile_shuffle(si); break;
            case StageKind::diff3x3x1:         rc = c.diff3x3x1(si); break;
            case StageKind::quantiser:         rc = c.quantiser(si); break;
            case StageKind::frame_shuffle:     rc = c.frame_shuffle(si); break;
            case StageKind::pass_through:      break;                              // pass_through_scheme_impl.hpp:81-95: bytes are the voxels
            case StageKind::rmestbkrd:
            case StageKind::rmbkrd_neighbor5:  break;                              // a copy: `cur` is the filtered volume (written out at the end)
            default:                           return 1;
        }
        if (rc) return rc;
    }
    return 0;
}

// Admission of an untrusted blob by its header: the voxel type the entry point was called for (who: how the message names the blob), a
// pipeline this library implements, and header_shape_ok (every extent positive, fewer than 2^31 voxels, no wrap-around anywhere)
bool admit_blob(const sqy::HeaderInfo& h, uint64_t srclen, int want_elem, uint64_t* raw_bytes, const char* who = "blob")
{
    if (h.elem_size() != want_elem) { std::fprintf(stderr, "[sqeazy]\t %s holds %s voxels\n", who, h.type.c_str()); return false; }
    std::string why;
    if (!Pipeline::supported(h.pipename, want_elem, &why)) {
        std::fprintf(stderr, "[sqeazy]\t%s cannot be build with this version of sqeazy (%s)\n", h.pipename.c_str(), why.c_str());
        return false;
    }
    return header_shape_ok(h, srclen, raw_bytes);
}

int decode_on_device(Context& cx, const void* d_src_v, uint64_t srclen, void* d_dst, uint64_t dst_capacity, int want_elem, hipStream_t stream)
{
    if (!d_src_v || !d_dst) return 1;
    const uint8_t* d_src = static_cast<const uint8_t*>(d_src_v);
    DrainOnExit drain{stream, &cx.pending, cx.side};
    sqy::HeaderInfo h;
    if (fetch_header(d_src, srclen, stream, h)) return 1;
    uint64_t raw_bytes = 0;
    if (!admit_blob(h, srclen, want_elem, &raw_bytes)) return 1;
    if (raw_bytes > dst_capacity) {
        std::fprintf(stderr, "[sqeazy]\t decode: buffer too small or blob truncated\n");
        return 1;
    }

    DecodeCall c(cx, stream, d_dst, h, Pipeline::from_string(h.pipename), raw_bytes / (uint64_t)want_elem, d_src + h.size);
    if (const int rc = decode_stages(c, c.pipe.stages.size())) return rc;
    if (c.cur != d_dst) SQY_HIP(hipMemcpyAsync(d_dst, c.cur, raw_bytes, hipMemcpyDeviceToDevice, stream));
    return c.finish();
}

// Frames [z0, z0 + nz) of the blob (the index along shape[0]) into d_dst: the subset path (DecodeCall::frames_subset) where it applies and
// the option allows, else the whole blob decoded into the workspace and the range copied out.  Same checks as decode_on_device, plus
// the range and the capacity for it -- all before anything is written.
int decode_frames_on_device(Context& cx, const void* d_src_v, uint64_t srclen, long z0, long nz, void* d_dst, uint64_t dst_capacity, int want_elem,
                            hipStream_t stream)
{
    if (!d_src_v || !d_dst) return 1;
    const uint8_t* d_src = static_cast<const uint8_t*>(d_src_v);
    std::vector<PendingEvent>* pend = &cx.pending;
    DrainOnExit drain{stream, &cx.pending, cx.side};
    sqy::HeaderInfo h;
    if (fetch_header(d_src, srclen, stream, h)) return 1;
    uint64_t raw_bytes = 0;
    if (!admit_blob(h, srclen, want_elem, &raw_bytes)) return 1;
    const uint64_t Z = h.shape[0], fb = raw_bytes / Z;
    if (z0 < 0 || nz <= 0 || (uint64_t)z0 + (uint64_t)nz > Z) {
        std::fprintf(stderr, "[sqeazy]\t decode frames: range [%ld, %ld + %ld) outside the blob's %llu frames\n", z0, z0, nz, (unsigned long long)Z);
        return 1;
    }
    const uint64_t range_bytes = (uint64_t)nz * fb;
    if (range_bytes > dst_capacity) { std::fprintf(stderr, "[sqeazy]\t decode frames: buffer too small\n"); return 1; }

    if (g_opt.decode_frames_subset.load()) {
        DecodeCall c(cx, stream, d_dst, h, Pipeline::from_string(h.pipename), raw_bytes / (uint64_t)want_elem, d_src + h.size);
        bool taken = false;
        if (const int rc = c.frames_subset((uint64_t)z0, (uint64_t)nz, true, &taken)) return rc;
        if (taken) {
            if (const int rc = c.frames_range_out((uint64_t)nz, fb)) return rc;
            return c.finish();
        }
    }
    // every other blob: the whole volume, then the range
    if (cx.ws.range_full.ensure(std::max<uint64_t>(raw_bytes, 16))) return 1;
    if (const int rc = decode_on_device(cx, d_src_v, srclen, cx.ws.range_full.p, raw_bytes, want_elem, stream)) return rc;
    SQY_TIMED("frames_range_copy", hipMemcpyAsync(d_dst, static_cast<const uint8_t*>(cx.ws.range_full.p) + (uint64_t)z0 * fb, range_bytes,
                                                  hipMemcpyDeviceToDevice, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    if (g_prof_on.load()) prof_collect(cx.pending);
    return 0;
}

// A device-memory decode on host pointers: src_bytes of src staged in the leased context's io_src, call(context, d_src, d_dst, stream), then
// dst_bytes of its io_dst back to dst.  The callers have checked the (untrusted) headers: nothing is allocated before that.
template <class F>
int decode_staged(const char* src, uint64_t src_bytes, char* dst, uint64_t dst_bytes, F&& call)
{
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Workspace* ws = &lease.ctx->ws;
    hipStream_t stream = lease.ctx->own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    if (ws->io_src.ensure(std::max<uint64_t>(src_bytes, 16)) || ws->io_dst.ensure(std::max<uint64_t>(dst_bytes, 16))) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    if (!lease.ctx->stager.copy(ws->io_src.p, const_cast<char*>(src), (size_t)src_bytes, true, dev_id)) { std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n"); return 1; }
    if (const int rc = call(*lease.ctx, ws->io_src.p, ws->io_dst.p, stream)) return rc;
    if (!lease.ctx->stager.copy(ws->io_dst.p, dst, dst_bytes, false, dev_id)) { std::fprintf(stderr, "[sqeazy]\t device to host transfer failed\n"); return 1; }
    return 0;
}

// The header front of the host variants that name a part of ONE blob (frames, a box, boxes), before anything is staged: the header found,
// its shape sound (header_shape_ok; *raw: the volume's bytes) and its voxels the entry point's
bool host_header_ok(const char* src, long srclength, int elem_size, sqy::HeaderInfo* h, uint64_t* raw)
{
    *h = sqy::header_unpack(src, src + srclength);
    if (!h->valid) { std::fprintf(stderr, "[sqeazy]\t unable to find a sqy header in the blob\n"); return false; }
    if (!header_shape_ok(*h, (uint64_t)srclength, raw)) return false;
    if (h->elem_size() != elem_size) { std::fprintf(stderr, "[sqeazy]\t blob holds %s voxels\n", h->type.c_str()); return false; }
    return true;
}

// host-pointer frame-range decode: only the range comes back
int decode_frames_from_host(const char* src, long srclength, long z0, long nz, char* dst, long dst_capacity, int elem_size)
{
    if (!src || !dst || srclength <= 0) return 1;
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw)) return 1;
    const uint64_t Z = h.shape[0], fb = raw / Z;
    if (z0 < 0 || nz <= 0 || (uint64_t)z0 + (uint64_t)nz > Z || (uint64_t)nz * fb > (uint64_t)std::max(dst_capacity, 0l)) {
        std::fprintf(stderr, "[sqeazy]\t decode frames: range [%ld, %ld + %ld) outside the blob's %llu frames, or buffer too small\n", z0, z0, nz,
                     (unsigned long long)Z);
        return 1;
    }
    const uint64_t range_bytes = (uint64_t)nz * fb;
    return decode_staged(src, (uint64_t)srclength, dst, range_bytes, [&](Context& cx, void* d_src, void* d_dst, hipStream_t stream) {
        return decode_frames_on_device(cx, d_src, (uint64_t)srclength, z0, nz, d_dst, range_bytes, elem_size, stream);
    });
}

int decode_from_host(const char* src, long srclength, char* dst, int elem_size)
{
    if (!src || !dst || srclength <= 0) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(src, src + srclength);
    if (!h.valid) { std::fprintf(stderr, "[sqeazy]\t unable to find a sqy header in the blob\n"); return 1; }
    uint64_t raw = 0;
    if (!header_shape_ok(h, (uint64_t)srclength, &raw)) return 1;
    return decode_staged(src, (uint64_t)srclength, dst, raw, [&](Context& cx, void* d_src, void* d_dst, hipStream_t stream) -> int {
        if (const int rc = decode_on_device(cx, d_src, (uint64_t)srclength, d_dst, raw, elem_size, stream)) return rc;
        SQY_HIP(hipStreamSynchronize(stream));
        return 0;
    });
}

// ---- strided views (SQYAMD_PipelineEncode_BatchStrided_*, SQYAMD_Decode_BatchStrided_*) ---------------------------------------------------
// A view is admitted on the host (sqy::admit_view: the stride rules, folded) before the device is touched.  A dense view is the Batch
// entry points' volume.  For the others, layer one: packed copies -- one batch_pack launch per encode group into Workspace::batch_pack in
// front of the Batch drivers, one batch_unpack launch per decode call behind them.  Layer two (the option batch_strided_fused): the
// bitswap1 transposers gather from and scatter into the view, `lz4` packs into the stream and unpacks from the LZ4 output.
static_assert(sizeof(sqy::BatchViewJob) == sqy::kBatchViewJobBytes, "the view job's layout");

// The jobs of one view launch and their tile table (tiles of sqy::kBatchTileVoxels voxels).  `host` is the upload's source (pageable): it
// must outlive the copy, so a launch that has been queued is waited for before its tables go -- on every way out of the scope that owns
// it, the error returns included (behind a call's own synchronisation the wait finds the stream idle)
struct ViewLaunch {
    enum Kind { pack, unpack, bitswap1, bitswap1_decode, copy_to_view };
    std::vector<sqy::BatchViewJob> jobs;
    std::vector<uint32_t> first_tile;
    uint32_t ntiles = 0;
    std::vector<unsigned char> host;
    hipStream_t queued_on = nullptr;
    bool queued = false;
    ViewLaunch() = default;
    ViewLaunch(const ViewLaunch&) = delete;
    ViewLaunch& operator=(const ViewLaunch&) = delete;
    ~ViewLaunch() { wait(); }
    void wait() { if (queued) (void)hipStreamSynchronize(queued_on); queued = false; }
    void clear() { wait(); jobs.clear(); first_tile.clear(); ntiles = 0; host.clear(); }
    void add(const void* view, const void* dense, const sqy::BatchView& v)
    {
        jobs.push_back(sqy::BatchViewJob{const_cast<void*>(view), const_cast<void*>(dense), v.Z, v.Y, v.X, v.sz, v.sy});
        first_tile.push_back(ntiles);
        ntiles += sqy::batch_bitswap1_tiles(v.Z * v.Y * v.X);
    }
};
// the tables to Workspace::batch_views[slot], the launch behind them under its profile name; no jobs: nothing
int launch_views(Context& cx, hipStream_t stream, ViewLaunch& l, ViewLaunch::Kind kind, int slot, int elem_size)
{
    if (l.jobs.empty()) return 0;
    std::vector<PendingEvent>* pend = &cx.pending;
    const size_t nj = l.jobs.size(), jobs_bytes = nj * sizeof(sqy::BatchViewJob), tiles_at = (jobs_bytes + 15) & ~(size_t)15;
    l.first_tile.push_back(l.ntiles);
    l.host.assign(tiles_at + (nj + 1) * 4, 0);
    std::memcpy(l.host.data(), l.jobs.data(), jobs_bytes);
    std::memcpy(l.host.data() + tiles_at, l.first_tile.data(), (nj + 1) * 4);
    DevBuf& buf = cx.ws.batch_views[slot];
    if (buf.ensure(l.host.size())) return 1;
    l.queued_on = stream;
    l.queued = true;
    SQY_HIP(hipMemcpyAsync(buf.p, l.host.data(), l.host.size(), hipMemcpyHostToDevice, stream));
    const sqy::BatchViewJob* d_jobs = static_cast<const sqy::BatchViewJob*>(buf.p);
    const uint32_t* d_tiles = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(buf.p) + tiles_at);
    switch (kind) {
    case ViewLaunch::pack: SQY_TIMED("batch_pack", sqy::launch_batch_view_copy(d_jobs, d_tiles, (uint32_t)nj, l.ntiles, elem_size, false, stream)); break;
    case ViewLaunch::unpack: SQY_TIMED("batch_unpack", sqy::launch_batch_view_copy(d_jobs, d_tiles, (uint32_t)nj, l.ntiles, elem_size, true, stream)); break;
    case ViewLaunch::bitswap1: SQY_TIMED("batch_bitswap1_strided", sqy::launch_bitswap1_batch_strided(d_jobs, d_tiles, (uint32_t)nj, l.ntiles, elem_size, stream)); break;
    case ViewLaunch::bitswap1_decode:
        SQY_TIMED("batch_bitswap1_decode_strided", sqy::launch_bitswap1_decode_batch_strided(d_jobs, d_tiles, (uint32_t)nj, l.ntiles, elem_size, stream));
        break;
    case ViewLaunch::copy_to_view:      // (batch decode, plain `lz4` blobs: the copy out of the LZ4 output is the unpack)
        SQY_TIMED("batch_copy_strided", sqy::launch_batch_view_copy(d_jobs, d_tiles, (uint32_t)nj, l.ntiles, elem_size, true, stream));
        break;
    }
    return 0;
}
// The caller's view table on the host, before the device is touched: views[i] admitted from row i of shapes and strides (strides nullptr:
// every view dense), ptrs[i] aligned to the voxel size.  1 with a message: a view that breaks a rule
int admit_views(const char* who, const void* const* ptrs, const long* shapes, const long* strides, unsigned rank, int n, int elem_size, std::vector<sqy::BatchView>* views)
{
    if (rank == 0 || rank > 3) { std::fprintf(stderr, "[sqeazy]\t %s: views have 1 to 3 dimensions, not %u\n", who, rank); return 1; }
    views->resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!ptrs[i]) return 1;
        if (reinterpret_cast<uintptr_t>(ptrs[i]) % (uintptr_t)elem_size) { std::fprintf(stderr, "[sqeazy]\t %s: view %d not aligned to the voxel size\n", who, i); return 1; }
        if (!sqy::admit_view(shapes + (size_t)i * rank, strides ? strides + (size_t)i * rank : nullptr, rank, &(*views)[(size_t)i])) {
            std::fprintf(stderr, "[sqeazy]\t %s: view %d: the innermost stride must be 1, every stride positive and no smaller than the extent times the stride of the next dimension\n", who, i);
            return 1;
        }
    }
    return 0;
}

// ---- windows (SQYAMD_Decode_BatchWindow_*) ----------------------------------------------------------------------------------------------------
// A window is admitted on the host (sqy::admit_window) against its blob's header before anything is written.  Layer one: the blob is
// decoded dense into a place of Workspace::batch_pack, ONE batch_window_copy launch at the end of the call copies every window out.
// Layer two (the option batch_window_fused): on the joint path the `bitswap1->lz4` blobs' inverse transposer stores only the window's
// voxels, the `lz4` blobs' windows are copied straight out of the LZ4 output.
static_assert(sizeof(sqy::BatchWindowJob) == sqy::kBatchWindowJobBytes, "the window job's layout");

// a window's view as the caller gave it, padded to three dimensions and NOT folded (admit_view folds; the window's rows must stay rows)
struct WindowView { uint64_t sz, sy; };
WindowView window_view(const sqy::BatchWindow& w, const long* strides, unsigned rank)
{
    uint64_t s[3] = {w.Y * w.X, w.X, 1};
    if (strides) {
        for (unsigned k = 0; k < rank; ++k) s[3 - rank + k] = (uint64_t)strides[k];
        for (int k = 2 - (int)rank; k >= 0; --k) s[k] = (k == 1 ? w.X : w.Y) * s[k + 1];      // (extent 1 there: never stepped over)
    }
    return WindowView{s[0], s[1]};
}

// ViewLaunch for jobs in the window launches' layout (sqy::batch_window_layout); the same rule for `host`
template <class Job>
struct TiledJobs {
    std::vector<Job> jobs;
    std::vector<uint32_t> first_tile;
    uint32_t ntiles = 0;
    std::vector<unsigned char> host;
    hipStream_t queued_on = nullptr;
    bool queued = false;
    TiledJobs() = default;
    TiledJobs(const TiledJobs&) = delete;
    TiledJobs& operator=(const TiledJobs&) = delete;
    ~TiledJobs() { wait(); }
    void wait() { if (queued) (void)hipStreamSynchronize(queued_on); queued = false; }
    void clear() { wait(); jobs.clear(); first_tile.clear(); ntiles = 0; host.clear(); }
    // a job that owns the next `tiles` workgroups of the launch
    void push(const Job& j, uint32_t tiles) { jobs.push_back(j); first_tile.push_back(ntiles); ntiles += tiles; }
    // the tables to buf: the jobs at its start, *d_tiles the prefix sums behind them
    int upload(hipStream_t stream, DevBuf& buf, const uint32_t** d_tiles)
    {
        const size_t nj = jobs.size();
        const sqy::BatchWindowLayout lay = sqy::batch_window_layout(nj, sizeof(Job));
        first_tile.push_back(ntiles);
        host.assign(lay.total, 0);
        std::memcpy(host.data(), jobs.data(), nj * sizeof(Job));
        std::memcpy(host.data() + lay.tiles_at, first_tile.data(), (nj + 1) * 4);
        if (buf.ensure(host.size())) return 1;
        queued_on = stream;
        queued = true;
        SQY_HIP(hipMemcpyAsync(buf.p, host.data(), host.size(), hipMemcpyHostToDevice, stream));
        *d_tiles = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(buf.p) + lay.tiles_at);
        return 0;
    }
};
// A window job's workgroups.  blob_tiles: the job is a windowed transposer's -- the blob's tiles that reach into the window's frames, from
// tile0 on --, else a copy's or a compare's: the window's own tiles
struct WindowTiles { uint64_t tile0; uint32_t count; };
WindowTiles window_tiles(const sqy::BatchWindow& w, const WindowView& v, bool blob_tiles)
{
    if (!blob_tiles) return WindowTiles{0, sqy::batch_bitswap1_tiles(w.Z * w.Y * w.X)};
    const sqy::WindowGeometry g = sqy::window_geometry(w, v.sz, v.sy);
    return WindowTiles{sqy::window_first_tile(g, sqy::kBatchTileVoxels), (uint32_t)sqy::window_tile_count(g, sqy::kBatchTileVoxels)};
}
struct WindowLaunch : TiledJobs<sqy::BatchWindowJob> {
    // paste (SQYAMD_Update_BatchWindow_*): the copy the other way round, the job's `dense` is written
    enum Kind { copy, bitswap1_decode, copy_from_lz4, paste };
    // blob_tiles: window_tiles
    void add(const void* view, const void* dense, const sqy::BatchWindow& w, const WindowView& v, bool blob_tiles)
    {
        const WindowTiles t = window_tiles(w, v, blob_tiles);
        push(sqy::BatchWindowJob{const_cast<void*>(view), dense, w.Z, w.Y, w.X, v.sz, v.sy, w.bZ, w.bY, w.bX, w.oz, w.oy, w.ox, t.tile0}, t.count);
    }
};
// the tables to Workspace::batch_windows[kind], the launch behind them under its profile name; no jobs: nothing
int launch_windows(Context& cx, hipStream_t stream, WindowLaunch& l, WindowLaunch::Kind kind, int elem_size)
{
    if (l.jobs.empty()) return 0;
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t nj = (uint32_t)l.jobs.size();
    DevBuf& buf = cx.ws.batch_windows[(int)kind];
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, buf, &d_tiles)) return 1;
    const sqy::BatchWindowJob* d_jobs = static_cast<const sqy::BatchWindowJob*>(buf.p);
    switch (kind) {
    case WindowLaunch::copy: SQY_TIMED("batch_window_copy", sqy::launch_batch_window_copy(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream)); break;
    case WindowLaunch::bitswap1_decode:
        SQY_TIMED("batch_bitswap1_decode_window", sqy::launch_bitswap1_decode_batch_window(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream));
        break;
    case WindowLaunch::copy_from_lz4: SQY_TIMED("batch_copy_window", sqy::launch_batch_window_copy(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream)); break;
    case WindowLaunch::paste: SQY_TIMED("batch_window_paste", sqy::launch_batch_window_paste(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream)); break;
    }
    return 0;
}

// ---- a box of one large blob (SQYAMD_Decode_Box_*) ------------------------------------------------------------------------------
// The frame-range decode's pruning joined with the windows' clip: sqy::decode_box_path says what runs.  On the subset paths the LZ4 frames
// the box's z-range needs are decoded into the workspace (DecodeCall::frames_subset, as for SQYAMD_Decode_Frames_*), then ONE launch
// stores the box's voxels into the view; every other blob is decoded whole into Workspace::range_full and one window copy cuts the box out.

// one window copy under the name "box_window_copy": the box w of the dense volume at `dense` into the view (l: alive until the stream has
// been waited for)
int launch_box_copy(Context& cx, hipStream_t stream, WindowLaunch& l, void* view, const void* dense, const sqy::BatchWindow& w, const WindowView& v, int elem_size)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    l.add(view, dense, w, v, false);
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.box_window, &d_tiles)) return 1;
    SQY_TIMED("box_window_copy", sqy::launch_batch_window_copy(static_cast<const sqy::BatchWindowJob*>(cx.ws.box_window.p), d_tiles, 1, l.ntiles, elem_size, stream));
    return 0;
}

// SQYAMD_Decode_Box_*'s last launch behind DecodeCall::frames_subset: the box w of the frames in c.range_buf into the view at c.d_dst
int box_range_out(DecodeCall& c, WindowLaunch& l, const sqy::BatchWindow& w, const WindowView& v, unsigned rank)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangePlan& p = c.range_plan;
    const int e = c.h.elem_size();
    if (sqy::decode_box_path(true, c.range_form, true) == sqy::BoxPath::subset_transposer) {
        sqy::Bitswap1Range r;
        const uint16_t* lut = nullptr;
        if (c.range_planes(&r, &lut)) return 1;
        const sqy::BatchWindowJob box{c.d_dst, c.range_buf, w.Z, w.Y, w.X, v.sz, v.sy, w.bZ, w.bY, w.bX, w.oz, w.oy, w.ox, 0};
        SQY_TIMED(lut ? "bitswap1_quantiser_decode_box" : "bitswap1_decode_box", sqy::launch_bitswap1_decode_range_window(c.range_buf, r, box, p.we, lut, stream));
        return 0;
    }
    // plain, shuffle: the range in the workspace is a blob of the box's frames, the box begins at its first one
    return launch_box_copy(c.cx, stream, l, c.d_dst, c.range_buf + p.range_at, sqy::window_in_own_frames(w, rank), v, e);
}

// The box [origin, origin + extent) of the blob into the view at d_dst.  Same checks as decode_on_device, plus the window against the
// header (the view has been admitted by the caller) -- all before anything is written.
int decode_box_on_device(Context& cx, const void* d_src_v, uint64_t srclen, const long* origin, const long* extent, const long* strides, unsigned rank, void* d_dst,
                         int want_elem, hipStream_t stream)
{
    const uint8_t* d_src = static_cast<const uint8_t*>(d_src_v);
    DrainOnExit drain{stream, &cx.pending, cx.side};
    sqy::HeaderInfo h;
    if (fetch_header(d_src, srclen, stream, h)) return 1;
    uint64_t raw_bytes = 0;
    if (!admit_blob(h, srclen, want_elem, &raw_bytes)) return 1;
    sqy::BatchWindow w;
    if (!sqy::admit_window(h.shape, origin, extent, rank, &w)) {
        std::fprintf(stderr, "[sqeazy]\t decode box: the box does not lie inside the blob's shape, or has another rank\n");
        return 1;
    }
    const WindowView v = window_view(w, strides, rank);
    WindowLaunch l;                                                     // (waits for the stream before its tables go)
    if (g_opt.decode_box_subset.load()) {
        DecodeCall c(cx, stream, d_dst, h, Pipeline::from_string(h.pipename), raw_bytes / (uint64_t)want_elem, d_src + h.size);
        bool taken = false;
        if (const int rc = c.frames_subset((uint64_t)origin[0], (uint64_t)extent[0], false, &taken)) return rc;
        if (taken) {
            if (const int rc = box_range_out(c, l, w, v, rank)) return rc;
            return c.finish();
        }
    }
    // sqy::BoxPath::whole_copy: the whole volume, then the box
    if (cx.ws.range_full.ensure(std::max<uint64_t>(raw_bytes, 16))) return 1;
    if (const int rc = decode_on_device(cx, d_src_v, srclen, cx.ws.range_full.p, raw_bytes, want_elem, stream)) return rc;
    if (const int rc = launch_box_copy(cx, stream, l, d_dst, cx.ws.range_full.p, w, v, want_elem)) return rc;
    SQY_HIP(hipStreamSynchronize(stream));
    if (g_prof_on.load()) prof_collect(cx.pending);
    return 0;
}

// what SQYAMD_Decode_Box_* checks without a header, before a device is looked for
bool box_arguments_ok(const void* src, long srclength, const long* origin, const void* dst, const long* extent, unsigned rank)
{
    if (!src || !dst || !origin || !extent || srclength <= 0 || rank == 0 || rank > 3) return false;
    for (unsigned k = 0; k < rank; ++k) if (origin[k] < 0) return false;
    return true;
}

int decode_box_device(const void* d_src, long srclength, const long* origin, void* d_dst, const long* dst_shape, const long* dst_strides, unsigned rank, int elem_size,
                      void* hip_stream)
{
    if (!box_arguments_ok(d_src, srclength, origin, d_dst, dst_shape, rank)) { std::fprintf(stderr, "[sqeazy]\t decode box: bad arguments\n"); return 1; }
    std::vector<sqy::BatchView> views;
    const void* const ptrs[1] = {d_dst};
    if (admit_views("decode box", ptrs, dst_shape, dst_strides, rank, 1, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_box_on_device(*lease.ctx, d_src, (uint64_t)srclength, origin, dst_shape, dst_strides, rank, d_dst, elem_size, static_cast<hipStream_t>(hip_stream));
}

// host pointers: the header and the box are checked here, before anything is staged; the box comes back dense
int decode_box_from_host(const char* src, long srclength, const long* origin, const long* extent, unsigned rank, char* dst, long dst_capacity, int elem_size)
{
    if (!box_arguments_ok(src, srclength, origin, dst, extent, rank)) { std::fprintf(stderr, "[sqeazy]\t decode box: bad arguments\n"); return 1; }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw)) return 1;
    sqy::BatchWindow w;
    if (!sqy::admit_window(h.shape, origin, extent, rank, &w) || w.Z * w.Y * w.X * (uint64_t)elem_size > (uint64_t)std::max(dst_capacity, 0l)) {
        std::fprintf(stderr, "[sqeazy]\t decode box: the box does not lie inside the blob's shape, or buffer too small\n");
        return 1;
    }
    const uint64_t box_bytes = w.Z * w.Y * w.X * (uint64_t)elem_size;
    return decode_staged(src, (uint64_t)srclength, dst, box_bytes, [&](Context& cx, void* d_src, void* d_dst, hipStream_t stream) {
        return decode_box_on_device(cx, d_src, (uint64_t)srclength, origin, extent, nullptr, rank, d_dst, elem_size, stream);
    });
}

// ---- boxes of one large blob: what every SQYAMD_*_Boxes_* driver shares -------------------------------------------------------
// A family is an admission per box (sqy::admit_window, admit_projection, ..) and an output: ONE launch behind DecodeCall::frames_subset on
// the boxes' z-ranges united -- ONE header fetch, frame index and pruned LZ4 launch for all boxes --, and the same output out of the whole
// volume, decoded ONCE into Workspace::range_full, for every other blob.  BoxesCall holds that flow; the families below say what is theirs.

// the refusal of box i in the words of the family `who`
bool box_refused(const char* who, size_t i, const char* why) { std::fprintf(stderr, "[sqeazy]\t %s: box %zu %s\n", who, i, why); return false; }

// f(i, origin, extent) for every box of the tables, until one says false
template <class F>
bool every_box(size_t count, const long* origins, const long* extents, unsigned rank, F&& f)
{
    for (size_t i = 0; i < count; ++i)
        if (!f(i, origins + i * rank, extents + i * rank)) return false;
    return true;
}

// what a family's *_arguments_ok checks of the boxes without a header, before a device is looked for: admit(i, shape, origin, extent) -- the
// family's sqy::admit_* -- of every box against the smallest shape that holds it
template <class F>
bool every_box_in_its_own_shape(long count, const long* origins, const long* extents, unsigned rank, F&& admit)
{
    return every_box((size_t)count, origins, extents, rank, [&](size_t i, const long* o, const long* e) { return admit(i, sqy::smallest_holding_shape(o, e, rank), o, e); });
}

// the largest voxel of the entry point's type (the sum bounds of the admissions)
uint64_t voxel_max(int elem_size) { return elem_size == 2 ? 65535u : 255u; }

// the common prefix of the range transposers' jobs (sqy::Bitswap1BoxJob, ..CompareJob, ..ProjectJob, ..BinJob, ..PyramidJob): the window w
// with the sink's two pitches, the box's range b of the united frames and its first thread; we: the bytes of a stored voxel
template <class Job>
void fill_range_job(Job& j, const sqy::BatchWindow& w, uint64_t sz, uint64_t sy, const sqy::FrameRangesBox& b, int we)
{
    j.g = sqy::window_geometry(w, sz, sy);
    j.r = sqy::bitswap1_range_of<sqy::Bitswap1Range>(b);
    j.t0 = sqy::range_first_thread(b.w0, 128u / (8u * (uint32_t)we));
}
// the workgroups of such a job where they share the range's words
uint32_t range_job_groups_of(const sqy::FrameRangesBox& b, int we) { return (uint32_t)sqy::range_job_groups(b.w0, b.w1, 128u / (8u * (uint32_t)we)); }

struct BoxesCall {
    Context& cx;
    const char* who;                        // the family in the messages: "decode boxes", ..
    const void* d_src_v;
    uint64_t srclen;
    int want_elem;
    hipStream_t stream;
    DrainOnExit drain;
    sqy::HeaderInfo h;
    uint64_t raw_bytes = 0;
    std::vector<sqy::BatchWindow> ws;                       // box i in the blob
    std::vector<std::pair<uint64_t, uint64_t>> ranges;      // .. and its frames
    // what the one output launch may hold, whichever it is: the family's own sum and a bound of the range transposer's groups
    uint64_t groups = 0, range_groups = 0;
    bool verdict = false;                   // run() got as far as the decode's verdict: its return is the decode's (SQYAMD_Compare_Boxes_*'s rows)

    BoxesCall(Context& cx_, const char* who_, const void* d_src, uint64_t srclen_, int want_elem_, hipStream_t stream_)
        : cx(cx_), who(who_), d_src_v(d_src), srclen(srclen_), want_elem(want_elem_), stream(stream_), drain{stream_, &cx_.pending, cx_.side} {}

    // decode_on_device's checks of the blob, then per_box(i, origin, extent, &ws[i], &own) for every box: the family's admission, which
    // says its refusal itself (box_refused) and leaves in `own` the box's share of the family's launch
    template <class F>
    int admit(size_t count, const long* origins, const long* extents, unsigned rank, F&& per_box)
    {
        if (fetch_header(static_cast<const uint8_t*>(d_src_v), srclen, stream, h)) return 1;
        if (!admit_blob(h, srclen, want_elem, &raw_bytes)) return 1;
        ws.resize(count);
        ranges.resize(count);
        const uint64_t frame_voxels = raw_bytes / (uint64_t)want_elem / h.shape[0];
        return every_box(count, origins, extents, rank, [&](size_t i, const long* o, const long* e) {
            uint64_t own = 0;
            if (!per_box(i, o, e, &ws[i], &own)) return false;
            ranges[i] = {(uint64_t)o[0], (uint64_t)e[0]};
            groups += own;
            range_groups += (uint64_t)e[0] * frame_voxels / sqy::kBatchTileVoxels + 2;      // (at least range_job_groups of the box's words)
            return true;
        }) ? 0 : 1;
    }
    bool launch_holds(uint64_t n) const
    {
        if (n > 0x7fffffffull) std::fprintf(stderr, "[sqeazy]\t %s: too many workgroups for one launch\n", who);
        return n <= 0x7fffffffull;
    }
    bool one_launch_holds() const { return launch_holds(std::max(groups, range_groups)); }

    // All checks are behind: nothing has been written so far.  With the family's option on and a blob DecodeCall::frames_subset takes,
    // range_launch(c) behind the pruned LZ4 decode (d_dst: DecodeCall's destination); else the whole volume, then whole_launch(volume)
    template <class R, class W>
    int run(bool subset_option, void* d_dst, R&& range_launch, W&& whole_launch)
    {
        if (subset_option) {
            DecodeCall c(cx, stream, d_dst, h, Pipeline::from_string(h.pipename), raw_bytes / (uint64_t)want_elem, static_cast<const uint8_t*>(d_src_v) + h.size);
            bool taken = false;
            if (const int rc = c.frames_subset(ranges, false, &taken)) return rc;
            if (taken) {
                if (c.ranges_plan.boxes.size() != ws.size()) return 1;
                if (const int rc = range_launch(c)) return rc;
                verdict = true;
                return c.finish();
            }
        }
        // sqy::BoxPath::whole_copy: the whole volume ONCE, then all boxes in the family's dense launch
        if (cx.ws.range_full.ensure(std::max<uint64_t>(raw_bytes, 16))) return 1;
        if (const int rc = decode_on_device(cx, d_src_v, srclen, cx.ws.range_full.p, raw_bytes, want_elem, stream)) { verdict = true; return rc; }
        if (whole_launch(cx.ws.range_full.p)) return 1;
        SQY_HIP(hipStreamSynchronize(stream));
        if (g_prof_on.load()) prof_collect(cx.pending);
        verdict = true;
        return 0;
    }
};

// SQYAMD_Decode_Boxes_*'s and SQYAMD_Compare_Boxes_*'s admission: sqy::admit_window, the view (strides + i rank, or dense), the copy's tiles
int admit_box_windows(BoxesCall& b, size_t count, const long* origins, const long* extents, const long* strides, unsigned rank, std::vector<WindowView>* vs)
{
    vs->resize(count);
    const int refused = b.admit(count, origins, extents, rank, [&](size_t i, const long* o, const long* e, sqy::BatchWindow* w, uint64_t* tiles) {
        if (!sqy::admit_window(b.h.shape, o, e, rank, w)) return box_refused(b.who, i, "does not lie inside the blob's shape, or has another rank");
        (*vs)[i] = window_view(*w, strides ? strides + i * rank : nullptr, rank);
        *tiles = sqy::batch_bitswap1_tiles(w->Z * w->Y * w->X);
        return true;
    });
    return refused || !b.one_launch_holds() ? 1 : 0;
}

// ---- the host variants of the box families: host_header_ok in front, then the boxes against the header, then ------------------------------
// the outputs of `bytes` each dense and back to back in the caller's buffer: sqy::output_offsets, said where the buffer is too small
bool host_outputs_fit(const char* who, const std::vector<uint64_t>& bytes, long capacity, std::vector<uint64_t>* at)
{
    if (sqy::output_offsets(bytes, capacity, at)) return true;
    std::fprintf(stderr, "[sqeazy]\t %s: buffer too small\n", who);
    return false;
}
// decode_staged with the outputs' places in the staged buffer: call(context, d_src, ptrs, stream), ptrs[i] = its start + at[i]
template <class F>
int boxes_staged(const char* src, long srclength, char* out, const std::vector<uint64_t>& at, F&& call)
{
    return decode_staged(src, (uint64_t)srclength, out, at.back(), [&](Context& cx, void* d_src, void* d_dst, hipStream_t stream) {
        std::vector<void*> ptrs(at.size() - 1);
        for (size_t i = 0; i < ptrs.size(); ++i) ptrs[i] = static_cast<uint8_t*>(d_dst) + at[i];
        return call(cx, d_src, ptrs.data(), stream);
    });
}

// ---- many boxes of one large blob (SQYAMD_Decode_Boxes_*) ------------------------------------------------------------------------
// BoxesCall with stores into the boxes' views; sqy::decode_boxes_path says what runs.  Its own: the box_by_box route, and DecodeCall's
// destination is the first view.
static_assert(sizeof(sqy::Bitswap1BoxJob) % 16 == 0, "the box job's layout");

// one window copy under the name "boxes_window_copy", a job per box
int launch_boxes_copy(Context& cx, hipStream_t stream, WindowLaunch& l, int elem_size)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.boxes_jobs, &d_tiles)) return 1;
    SQY_TIMED("boxes_window_copy", sqy::launch_batch_window_copy(static_cast<const sqy::BatchWindowJob*>(cx.ws.boxes_jobs.p), d_tiles, (uint32_t)l.jobs.size(), l.ntiles,
                                                                  elem_size, stream));
    return 0;
}

// the boxes' last launch behind DecodeCall::frames_subset: box i (ws[i], its view vs[i] at dsts[i]) out of the united frames in c.range_buf
int boxes_range_out(DecodeCall& c, WindowLaunch& l, TiledJobs<sqy::Bitswap1BoxJob>& tj, const std::vector<sqy::BatchWindow>& ws, const std::vector<WindowView>& vs,
                    void* const* dsts, unsigned rank)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const size_t count = ws.size();
    if (sqy::decode_boxes_path(true, c.range_form, true, true) == sqy::BoxesPath::subset_transposer) {
        const uint16_t* lut = nullptr;
        if (c.range_lut(&lut)) return 1;
        for (size_t i = 0; i < count; ++i) {
            sqy::Bitswap1BoxJob j{};
            j.view = dsts[i];
            fill_range_job(j, ws[i], vs[i].sz, vs[i].sy, p.boxes[i], p.we);
            if (!sqy::bitswap1_box_job_ok(j)) return 1;
            tj.push(j, range_job_groups_of(p.boxes[i], p.we));
        }
        const uint32_t* d_tiles = nullptr;
        if (tj.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
        SQY_TIMED(lut ? "bitswap1_quantiser_decode_boxes" : "bitswap1_decode_boxes",
                  sqy::launch_bitswap1_decode_range_windows(c.range_buf, static_cast<const sqy::Bitswap1BoxJob*>(c.cx.ws.boxes_jobs.p), d_tiles, (uint32_t)count, tj.ntiles,
                                                            p.we, lut, stream));
        return 0;
    }
    // plain, shuffle: box i's range in the workspace is a blob of its frames, the box begins at its first one
    for (size_t i = 0; i < count; ++i) l.add(dsts[i], c.range_buf + p.boxes[i].range_at, sqy::window_in_own_frames(ws[i], rank), vs[i], false);
    return launch_boxes_copy(c.cx, stream, l, c.h.elem_size());
}

// Box i = [origins + i rank, .. + extents + i rank) of the blob into the view at d_dsts[i] (strides + i rank, or dense).  The checks of
// decode_box_on_device for every box, and the launches' sizes -- all before anything is written.
int decode_boxes_on_device(Context& cx, const void* d_src_v, uint64_t srclen, size_t count, const long* origins, void* const* d_dsts, const long* extents,
                           const long* strides, unsigned rank, int want_elem, hipStream_t stream)
{
    BoxesCall b(cx, "decode boxes", d_src_v, srclen, want_elem, stream);
    std::vector<WindowView> vs;
    if (admit_box_windows(b, count, origins, extents, strides, rank, &vs)) return 1;
    if (sqy::decode_boxes_path(false, sqy::RangeForm::plain, false, g_opt.decode_boxes_joint.load() != 0) == sqy::BoxesPath::box_by_box) {
        for (size_t i = 0; i < count; ++i)
            if (const int rc = decode_box_on_device(cx, d_src_v, srclen, origins + i * rank, extents + i * rank, strides ? strides + i * rank : nullptr, rank, d_dsts[i],
                                                    want_elem, stream))
                return rc;
        return 0;
    }
    WindowLaunch l;                                                     // (both wait for the stream before their tables go)
    TiledJobs<sqy::Bitswap1BoxJob> tj;
    return b.run(g_opt.decode_box_subset.load() != 0, d_dsts[0], [&](DecodeCall& c) { return boxes_range_out(c, l, tj, b.ws, vs, d_dsts, rank); },
                 [&](const void* volume) {
                     for (size_t i = 0; i < count; ++i) l.add(d_dsts[i], volume, b.ws[i], vs[i], false);
                     return launch_boxes_copy(cx, stream, l, want_elem);
                 });
}

// what SQYAMD_Decode_Boxes_* checks without a header, before a device is looked for: box_arguments_ok for every box
bool boxes_arguments_ok(const void* src, long srclength, long count, const long* origins, const void* const* dsts, const long* extents, unsigned rank)
{
    if (!src || srclength <= 0 || count < 1 || count > INT_MAX || !origins || !extents || rank == 0 || rank > 3) return false;
    for (long i = 0; i < count; ++i)
        if (!box_arguments_ok(src, srclength, origins + (size_t)i * rank, dsts ? dsts[i] : src, extents + (size_t)i * rank, rank)) return false;
    return true;
}

int decode_boxes_device(const void* d_src, long srclength, long count, const long* origins, void* const* d_dsts, const long* dst_shapes, const long* dst_strides,
                        unsigned rank, int elem_size, void* hip_stream)
{
    if (!d_dsts || !boxes_arguments_ok(d_src, srclength, count, origins, d_dsts, dst_shapes, rank)) { std::fprintf(stderr, "[sqeazy]\t decode boxes: bad arguments\n"); return 1; }
    std::vector<sqy::BatchView> views;
    if (admit_views("decode boxes", d_dsts, dst_shapes, dst_strides, rank, (int)count, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_boxes_on_device(*lease.ctx, d_src, (uint64_t)srclength, (size_t)count, origins, d_dsts, dst_shapes, dst_strides, rank, elem_size,
                                  static_cast<hipStream_t>(hip_stream));
}

// the bytes of every box of a host variant that takes or gives the boxes' voxels dense: sqy::admit_window against the header
bool host_box_bytes(const char* who, const sqy::HeaderInfo& h, long count, const long* origins, const long* extents, unsigned rank, int elem_size, std::vector<uint64_t>* bytes)
{
    bytes->resize((size_t)count);
    return every_box((size_t)count, origins, extents, rank, [&](size_t i, const long* o, const long* e) {
        sqy::BatchWindow w;
        if (!sqy::admit_window(h.shape, o, e, rank, &w)) return box_refused(who, i, "does not lie inside the blob's shape");
        (*bytes)[i] = w.Z * w.Y * w.X * (uint64_t)elem_size;
        return true;
    });
}

// host pointers: the header and every box are checked here, before anything is staged; the boxes come back dense, back to back in box order
int decode_boxes_from_host(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, char* dst, long dst_capacity, int elem_size)
{
    if (!dst || !boxes_arguments_ok(src, srclength, count, origins, nullptr, extents, rank)) { std::fprintf(stderr, "[sqeazy]\t decode boxes: bad arguments\n"); return 1; }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    std::vector<uint64_t> bytes, at;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw) || !host_box_bytes("decode boxes", h, count, origins, extents, rank, elem_size, &bytes) ||
        !host_outputs_fit("decode boxes", bytes, dst_capacity, &at))
        return 1;
    return boxes_staged(src, srclength, dst, at, [&](Context& cx, void* d_src, void* const* ptrs, hipStream_t stream) {
        return decode_boxes_on_device(cx, d_src, (uint64_t)srclength, (size_t)count, origins, ptrs, extents, nullptr, rank, elem_size, stream);
    });
}

// ---- the compare of a window with its view (SQYAMD_Compare_BatchWindow_*) ----
// The windowed decode's driver with loads where its stores were: the same groups, plan and window jobs, each job with its record (eight
// 64-bit words in Workspace::batch_records).  Layer one: the blob decoded dense into a place of Workspace::batch_pack, ONE
// batch_window_compare launch at the end of the call.  Layer two (the option batch_compare_fused): on the joint path the `bitswap1->lz4`
// blobs' inverse transposer compares instead of storing, the `lz4` blobs' windows are compared in the LZ4 output.
static_assert(sizeof(sqy::BatchCompareJob) == sqy::kBatchCompareJobBytes, "the compare job's layout");
struct CompareLaunch : TiledJobs<sqy::BatchCompareJob> {
    enum Kind { compare, bitswap1_decode, compare_in_lz4 };
    // blob_tiles: as WindowLaunch::add
    void add(const void* view, const void* dense, const sqy::BatchWindow& w, const WindowView& v, bool blob_tiles, unsigned long long* record)
    {
        const WindowTiles t = window_tiles(w, v, blob_tiles);
        push(sqy::BatchCompareJob{view, dense, w.Z, w.Y, w.X, v.sz, v.sy, w.bZ, w.bY, w.bX, w.oz, w.oy, w.ox, t.tile0, record, 0}, t.count);
    }
};
// the tables to Workspace::batch_compares[kind], the launch behind them under its profile name; no jobs: nothing
int launch_compares(Context& cx, hipStream_t stream, CompareLaunch& l, CompareLaunch::Kind kind, int elem_size)
{
    if (l.jobs.empty()) return 0;
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t nj = (uint32_t)l.jobs.size();
    DevBuf& buf = cx.ws.batch_compares[(int)kind];
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, buf, &d_tiles)) return 1;
    const sqy::BatchCompareJob* d_jobs = static_cast<const sqy::BatchCompareJob*>(buf.p);
    switch (kind) {
    case CompareLaunch::compare: SQY_TIMED("batch_window_compare", sqy::launch_batch_window_compare(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream)); break;
    case CompareLaunch::bitswap1_decode:
        SQY_TIMED("batch_bitswap1_decode_window_compare", sqy::launch_bitswap1_decode_batch_window_compare(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream));
        break;
    case CompareLaunch::compare_in_lz4: SQY_TIMED("batch_compare_window", sqy::launch_batch_window_compare(d_jobs, d_tiles, nj, l.ntiles, elem_size, stream)); break;
    }
    return 0;
}

// the patch launch of a window update's encode group (layer two): old plane stream + the window's view -> the group's stream
static_assert(sizeof(sqy::BatchPatchJob) == sqy::kBatchPatchJobBytes, "the patch job's layout");
struct PatchLaunch : TiledJobs<sqy::BatchPatchJob> {
    void add(const void* view, const void* old_stream, void* new_stream, const sqy::BatchWindow& w, const WindowView& v)
    {
        push(sqy::BatchPatchJob{view, old_stream, new_stream, w.Z, w.Y, w.X, v.sz, v.sy, w.bZ, w.bY, w.bX, w.oz, w.oy, w.ox}, sqy::batch_bitswap1_tiles(w.bZ * w.bY * w.bX));
    }
};
int launch_patches(Context& cx, hipStream_t stream, PatchLaunch& l, int elem_size)
{
    if (l.jobs.empty()) return 0;
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.batch_patch_jobs, &d_tiles)) return 1;
    SQY_TIMED("batch_bitswap1_patch", sqy::launch_bitswap1_batch_patch(static_cast<const sqy::BatchPatchJob*>(cx.ws.batch_patch_jobs.p), d_tiles, (uint32_t)l.jobs.size(), l.ntiles,
                                                                       elem_size, stream));
    return 0;
}

// ---- z-slab blob sets (SQYAMD_Decode_Slabs_*) and batches (SQYAMD_Decode_Batch_*): a group on the joint path -----------------
// Blobs in the chunked LZ4 layout are decoded in groups.  What both callers share, one function per step: the frame ranking of every blob
// of a group in one launch per kernel and one read-back (group_rank), one joint block index and one LZ4 decode launch for all of them
// (group_lz4_decode), a blob's remaining inverses from the group's LZ4 output into its place (group_remaining_stages), one verdict
// read-back (group_verdict).  The caller (decode_slabs_group, decode_batch_group) says where the LZ4 output goes, what follows the decode
// and under which names the launches are profiled.  Every other blob -- and every blob of a group whose decode raised the error flag --
// goes through decode_on_device, one at a time.  The tables' layouts: sqy::decode_rank_layout, decode_joint_layout (sqy_pipeline.cpp).
constexpr uint64_t kSlabsHeadPrefix = 1ull << 16;       // bytes of every blob fetched for its header at first

struct SlabBlob : sqy::Lz4DecodeGeometry {              // (of the LZ4 stage's input, on the joint path)
    const uint8_t* src = nullptr;
    uint64_t len = 0;
    sqy::HeaderInfo h;
    uint64_t raw = 0, dst_off = 0;
    // the joint path: the LZ4 stage's input to the decoder (total bytes, chunks), where its output goes
    std::unique_ptr<DecodeCall> call;
    size_t li = 0;
    uint64_t total = 0, out_base = 0, map_off = 0, fs_bytes = 0;
    bool remap = false;
    int rc = 0;
    std::vector<unsigned char> lut;                     // a batch's `quantiser->bitswap1->lz4` blob on the joint path: its decode table
};

uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

struct GroupNames { const char *frame_index, *lz4_decode; };                // the profile names of a group's two shared launches
constexpr GroupNames kSlabsNames{"slabs_frame_index", "slabs_lz4_decode"}, kBatchNames{"batch_frame_index", "batch_lz4_decode"};

// A group on its way through the steps
struct JointGroup {
    Context& cx;
    const uint8_t* d_src;
    std::vector<SlabBlob>& blobs;
    hipStream_t stream;
    GroupNames names;
    // group_rank: who stays (slab order) and each one's block index, the maps of those with SlabBlob::remap; their frames in all, the compressed
    // ones, the most of one blob; the error flag
    std::vector<size_t> mem;
    std::vector<const void*> blk_of;
    std::vector<unsigned char> maps;
    uint64_t nframes = 0, ncompressed = 0, max_frames = 0;
    uint32_t* flag = nullptr;
    std::vector<unsigned char> up;          // group_lz4_decode: the pageable source of its upload, alive until group_verdict's synchronisation
    uint8_t* out = nullptr;                 // the caller: where the LZ4 output goes -- blob b's at out + blobs[b].out_base, out_bytes in all
    uint64_t out_bytes = 0;
};

// The frame ranking of blobs g[0..m) and its read-back.  Who stays (G.mem): ranked without complaint, one frame per chunk -- with them
// whether their frame_shuffle folds into the decode (SlabBlob::remap, fs_bytes; G.maps).  Anything else -- code 100, an error, a stored tail
// the ranking gave up on -- is appended to `single`, where the single-blob index gets the last word; so is everybody when the frames are
// more than the joint index counts.
int group_rank(JointGroup& G, const std::vector<size_t>& g, std::vector<size_t>& single)
{
    Workspace* ws = &G.cx.ws;
    std::vector<PendingEvent>* pend = &G.cx.pending;
    hipStream_t stream = G.stream;
    const uint32_t m = (uint32_t)g.size();
    std::vector<sqy::DecodeRankBlob> sizes(m);
    for (uint32_t k = 0; k < m; ++k) sizes[k] = sqy::DecodeRankBlob{sqy::lz4_frame_rank_scratch_bytes(G.blobs[g[k]].nchunks), G.blobs[g[k]].max_blocks};
    const sqy::DecodeRankLayout L = sqy::decode_rank_layout(sizes, sqy::lz4_frame_rank_batch_desc_bytes(m));
    if (ws->slabs_index.ensure(L.total)) return 1;
    uint8_t* di = static_cast<uint8_t*>(ws->slabs_index.p);
    uint32_t* counts = reinterpret_cast<uint32_t*>(di + L.counts_at);
    G.flag = reinterpret_cast<uint32_t*>(di + L.flag_at);
    const bool tail = g_opt.stored_tail_index.load() != 0;                 // (the stored tail looked for where it must start, as lz4_index does)
    std::vector<sqy::Lz4RankJob> jobs(m);
    for (uint32_t k = 0; k < m; ++k) {
        const SlabBlob& b = G.blobs[g[k]];
        sqy::Lz4RankJob& j = jobs[k];
        j.in = b.call->cur; j.n = b.call->cur_bytes;
        j.scratch = di + L.blobs[k].scratch_at; j.blk = di + L.blobs[k].blk_at;
        j.frame_first = reinterpret_cast<uint32_t*>(di + L.blobs[k].frame_first_at);
        j.max_blocks = b.max_blocks; j.expected_frames = b.nchunks; j.counts = counts + 16 * k;
        j.chunk = tail ? b.chunk : 0; j.last = tail ? b.total - (b.nchunks - 1) * b.chunk : 0;
    }
    std::vector<unsigned char> hdesc(sqy::lz4_frame_rank_batch_desc_bytes(m));
    SQY_HIP(hipMemsetAsync(G.flag, 0, 64, stream));
    SQY_TIMED(G.names.frame_index, sqy::launch_lz4_frame_rank_batch(jobs.data(), m, di + L.desc_at, hdesc.data(), stream));
    if (ws->slabs_host.ensure((size_t)m * 64)) return 1;
    const uint32_t* hc_all = static_cast<const uint32_t*>(ws->slabs_host.p);
    SQY_HIP(hipMemcpyAsync(ws->slabs_host.p, counts, (size_t)m * 64, hipMemcpyDeviceToHost, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t* hc = hc_all + 16 * k;
        SlabBlob& s = G.blobs[g[k]];
        if (hc[2] != 0 || hc[0] != s.nchunks) { single.push_back(g[k]); continue; }
        G.mem.push_back(g[k]);
        G.blk_of.push_back(jobs[k].blk);
        G.nframes += s.nchunks; G.ncompressed += hc[3]; G.max_frames = std::max(G.max_frames, s.nchunks);
        s.remap = false;
        uint64_t Z = 0, fb = 0;
        bool permutation = true;
        if (s.call->shuffle_fold(s.li, s.total, s, s.nchunks, false, Z, fb, permutation, &s.remap) == 0 && s.remap) {
            s.fs_bytes = fb;
            s.map_off = G.maps.size();
            G.maps.insert(G.maps.end(), s.call->fs_map.begin(), s.call->fs_map.begin() + Z * 8);
        }
    }
    if (G.nframes > 0x7fffffffull) { single.insert(single.end(), G.mem.begin(), G.mem.end()); G.mem.clear(); }
    return 0;
}

// The joint index -- a part per blob and the maps from the host, the rest built by the launch -- and the one LZ4 decode launch into G.out
int group_lz4_decode(JointGroup& G, const sqy::DecodeJointLayout& L)
{
    std::vector<PendingEvent>* pend = &G.cx.pending;
    hipStream_t stream = G.stream;
    if (G.cx.ws.slabs_joint.ensure(L.total)) return 1;
    uint8_t* dj = static_cast<uint8_t*>(G.cx.ws.slabs_joint.p);
    const uint32_t np = (uint32_t)G.mem.size();
    G.up.assign(L.upload_bytes, 0);
    for (uint32_t k = 0, jbase = 0; k < np; ++k) {
        const SlabBlob& s = G.blobs[G.mem[k]];
        sqy::Lz4JointPart pt{};
        pt.blk = G.blk_of[k]; pt.in_off = (uint64_t)(s.call->cur - G.d_src);
        pt.out_base = s.out_base; pt.chunk = s.chunk; pt.total = s.total;
        pt.remap = s.remap ? reinterpret_cast<const uint64_t*>(dj + L.maps_at + s.map_off) : nullptr;
        pt.remap_bytes = s.remap ? s.fs_bytes : 0;
        pt.jbase = jbase; pt.nframes = (uint32_t)s.nchunks;
        std::memcpy(G.up.data() + L.parts_at + k * sizeof(pt), &pt, sizeof(pt));
        jbase += pt.nframes;
    }
    if (!G.maps.empty()) std::memcpy(G.up.data() + L.maps_at, G.maps.data(), G.maps.size());
    SQY_HIP(hipMemcpyAsync(dj, G.up.data(), G.up.size(), hipMemcpyHostToDevice, stream));
    for (size_t b : G.mem) {                                            // frames nobody names come out as zeros (frame_shuffle's inverse)
        SlabBlob& s = G.blobs[b];
        if (s.remap && !s.call->fs_unnamed.empty())
            if (const int rc = s.call->zero_unnamed_places(G.out + s.out_base, s.fs_bytes, s.total)) return rc;
    }
    const bool side_ok = G.cx.ensure_side();
    SQY_TIMED(G.names.lz4_decode,
              sqy::launch_lz4_frames_joint_decode(G.d_src, reinterpret_cast<const sqy::Lz4JointPart*>(dj + L.parts_at), np, (uint32_t)G.max_frames, dj + L.jblk_at,
                                                  reinterpret_cast<uint32_t*>(dj + L.jff_at), reinterpret_cast<uint64_t*>(dj + L.jout_at), (uint32_t)G.nframes,
                                                  G.out, G.out_bytes, G.blobs[G.mem[0]].block_bytes, (uint32_t)std::min<uint64_t>(G.ncompressed, 0xffffffffull), G.flag,
                                                  stream, side_ok ? G.cx.side : nullptr, G.cx.fork, G.cx.join, g_opt.decode_two_waves.load() != 0));
    return 0;
}

// The remaining inverses of the blobs `who`, blob by blob, from the group's LZ4 output into their places
int group_remaining_stages(JointGroup& G, const std::vector<size_t>& who)
{
    bool first = true;
    for (size_t b : who) {
        SlabBlob& s = G.blobs[b];
        DecodeCall& c = *s.call;
        // (the quantiser's table goes to ws->small by a synchronous copy: the blob before must be done with it)
        if (!first) for (const Stage& st : c.pipe.stages) if (st.kind == StageKind::quantiser) { SQY_HIP(hipStreamSynchronize(G.stream)); break; }
        first = false;
        c.cur = G.out + s.out_base;
        c.cur_bytes = s.total;
        if (const int rc = decode_stages(c, s.remap ? s.li - 1 : s.li)) { s.rc = rc; continue; }
        if (c.cur != c.d_dst) SQY_HIP(hipMemcpyAsync(c.d_dst, c.cur, s.raw, hipMemcpyDeviceToDevice, G.stream));
    }
    return 0;
}

// The decoder's verdict, one read-back for the group.  The flag raised -- a damaged frame somewhere in the group --: every blob of it again
// on its own (appended to `single`), which gives each one its exact code
int group_verdict(JointGroup& G, std::vector<size_t>& single)
{
    bool raised = false;
    if (const int rc = lz4_verdict(G.cx, G.flag, G.stream, &raised)) return rc;
    if (raised) for (size_t b : G.mem) { G.blobs[b].rc = 0; single.push_back(b); }
    return 0;
}

// The joint path for slabs g[0..m) of a slab set (slab order).  Blobs it cannot take are appended to `single`; the flag raised: all of g go
// there.  The LZ4 output goes straight into each blob's place in the volume when the LZ4 stage's inverse produces the volume for every
// blob of the group (lz4, frame_shuffle->lz4, behind the background heads) and the places are 16-byte aligned, else to the workspace,
// packed here; every blob's remaining inverses (bitswap1, diff3x3x1, ..) follow the decode.
int decode_slabs_group(Context& cx, const uint8_t* d_src, std::vector<SlabBlob>& blobs, const std::vector<size_t>& g, uint8_t* d_dst,
                       uint64_t volume_bytes, hipStream_t stream, std::vector<size_t>& single)
{
    JointGroup G{cx, d_src, blobs, stream, kSlabsNames};
    if (const int rc = group_rank(G, g, single)) return rc;
    if (G.mem.empty()) return 0;
    bool direct = true;
    for (size_t b : G.mem) {
        const SlabBlob& s = blobs[b];
        const size_t first_after = s.remap ? s.li - 1 : s.li;           // the stage whose inverse the LZ4 decode completes
        if (first_after > s.call->lead || ((reinterpret_cast<uintptr_t>(d_dst) + s.dst_off) & 15) != 0) direct = false;
    }
    if (direct) {
        for (size_t b : G.mem) blobs[b].out_base = blobs[b].dst_off;
        G.out = d_dst;
        G.out_bytes = volume_bytes;
    } else {
        for (size_t b : G.mem) { blobs[b].out_base = G.out_bytes; G.out_bytes = align_up(G.out_bytes + blobs[b].total, 256); }
        if (cx.ws.slabs_out.ensure(std::max<uint64_t>(G.out_bytes, 16))) return 1;
        G.out = static_cast<uint8_t*>(cx.ws.slabs_out.p);
    }
    if (const int rc = group_lz4_decode(G, sqy::decode_joint_layout(G.mem.size(), G.maps.size(), G.nframes))) return rc;
    if (const int rc = group_remaining_stages(G, G.mem)) return rc;
    return group_verdict(G, single);
}

// What follows the LZ4 decode in a batch group (pg: its plan, sqy::decode_batch_plan's).  The tables of the launches -- job lists, tile and
// strip tables, the quantised blobs' LUTs -- in one upload (`tables`: host memory for it, alive until the verdict's synchronisation), then
// the `bitswap1->lz4` blobs: ONE inverse-transpose launch from the workspace into their destinations -- and into the workspace for the
// `diff3x3x1->bitswap1->lz4` blobs --; the `lz4` blobs: ONE copy launch; the `quantiser->bitswap1->lz4` blobs: ONE launch of the transposer
// with the look-up; the 16-bit diff3x3x1 blobs in the chain geometry: ONE launch per chain step (launch_diff3x3x1_decode_batch_copy, _step)
// A batch of views (sv != nullptr): the planes and plain blobs whose destination is a view that takes the voxels directly leave the dense
// launches' tables for sv->scatter and sv->copy (alive as `tables` is) -- one batch_bitswap1_decode_strided, one batch_copy_strided launch
struct StridedDecode {
    const std::vector<sqy::BatchView>* views = nullptr;
    std::vector<uint8_t> direct;            // per blob: 1 = the joint path's last launch writes into the view, 2 = .. the window's voxels into it
    ViewLaunch scatter, copy;
    // windows (SQYAMD_Decode_BatchWindow_*): blob b's window and its unfolded view, for direct[b] == 2 -- one batch_bitswap1_decode_window,
    // one batch_copy_window launch
    const std::vector<sqy::BatchWindow>* wins = nullptr;
    std::vector<WindowView> wviews;
    WindowLaunch wscatter, wcopy;
    // compares (SQYAMD_Compare_BatchWindow_*, records != nullptr): blob b's record at records + 8 b; the windows of direct[b] == 2 are
    // compared, not stored -- one batch_bitswap1_decode_window_compare, one batch_compare_window launch
    unsigned long long* records = nullptr;
    CompareLaunch cscatter, ccopy;
};
int batch_group_tail(JointGroup& G, const sqy::DecodeJointLayout& L, const sqy::DecodeBatchGroup& pg, const std::vector<sqy::DecodeBatchBlob>& plan_in, int elem_size,
                     std::vector<unsigned char>& tables, StridedDecode* sv = nullptr)
{
    std::vector<PendingEvent>* pend = &G.cx.pending;
    hipStream_t stream = G.stream;
    tables.assign(L.jobs_bytes, 0);
    auto host = [&](uint64_t at) { return tables.data() + (at - L.jobs_upload_at); };
    const sqy::DecodeBatchDiff& df = pg.diff;
    std::vector<uint64_t> res_of(G.blobs.size(), 0);                    // a diff blob's residual volume in the workspace
    for (size_t j = 0; j < df.jobs.size(); ++j) res_of[df.jobs[j]] = df.res_at[j];
    const sqy::DecodeBatchTiles* tt[3] = {&pg.planes, &pg.plain, &pg.quantised};
    const sqy::DecodeJointLayout::Family* ff[3] = {&L.planes, &L.plain, &L.quantised};
    size_t dense_jobs[3] = {0, 0, 0};                                   // what stays in the dense launches' tables
    uint32_t dense_tiles[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        const size_t nj = tt[k]->jobs.size();
        std::vector<uint32_t> first_tile;
        for (size_t j = 0; j < nj; ++j) {
            const uint32_t b = tt[k]->jobs[j];
            const SlabBlob& s = G.blobs[b];
            if (sv && sv->direct[b] == 1 && plan_in[b].form != sqy::DecodeBatchForm::diff_planes) {
                (k == 0 ? sv->scatter : sv->copy).add(s.call->d_dst, G.out + s.out_base, (*sv->views)[b]);
                continue;
            }
            if (sv && sv->direct[b] == 2 && sv->records && plan_in[b].form != sqy::DecodeBatchForm::diff_planes) {
                (k == 0 ? sv->cscatter : sv->ccopy).add(s.call->d_dst, G.out + s.out_base, (*sv->wins)[b], sv->wviews[b], k == 0, sv->records + sqy::kCompareFields * b);
                continue;
            }
            if (sv && sv->direct[b] == 2 && plan_in[b].form != sqy::DecodeBatchForm::diff_planes) {
                (k == 0 ? sv->wscatter : sv->wcopy).add(s.call->d_dst, G.out + s.out_base, (*sv->wins)[b], sv->wviews[b], k == 0);
                continue;
            }
            void* to = plan_in[b].form == sqy::DecodeBatchForm::diff_planes ? static_cast<void*>(G.out + res_of[b]) : s.call->d_dst;
            const sqy::Bitswap1Job job{G.out + s.out_base, to, plan_in[b].len};
            std::memcpy(host(ff[k]->jobs_at) + dense_jobs[k] * sizeof(job), &job, sizeof(job));
            if (tt[k] == &pg.quantised) std::memcpy(host(ff[k]->extra_at) + dense_jobs[k] * 512, s.lut.data(), 512);
            first_tile.push_back(dense_tiles[k]);
            dense_tiles[k] += tt[k]->first_tile[j + 1] - tt[k]->first_tile[j];
            ++dense_jobs[k];
        }
        first_tile.push_back(dense_tiles[k]);
        std::memcpy(host(ff[k]->tiles_at), first_tile.data(), first_tile.size() * 4);
    }
    const uint32_t nd = (uint32_t)df.jobs.size();
    for (uint32_t j = 0; j < nd; ++j) {
        const sqy::DecodeBatchBlob& p = plan_in[df.jobs[j]];
        const sqy::DiffBatchJob job{G.out + df.res_at[j], G.blobs[df.jobs[j]].call->d_dst, p.Z, p.Y, p.X, p.chain_columns};
        std::memcpy(host(L.diff.jobs_at) + j * sizeof(job), &job, sizeof(job));
    }
    std::memcpy(host(L.diff.tiles_at), df.first_strip.data(), ((size_t)nd + 1) * 4);
    std::memcpy(host(L.diff.extra_at), df.first_tile.data(), ((size_t)nd + 1) * 4);
    uint8_t* dj = static_cast<uint8_t*>(G.cx.ws.slabs_joint.p);
    if (L.jobs_bytes) SQY_HIP(hipMemcpyAsync(dj + L.jobs_upload_at, tables.data(), L.jobs_bytes, hipMemcpyHostToDevice, stream));
    auto jobs = [&](const sqy::DecodeJointLayout::Family& f) { return reinterpret_cast<const sqy::Bitswap1Job*>(dj + f.jobs_at); };
    auto words = [&](uint64_t at) { return reinterpret_cast<const uint32_t*>(dj + at); };
    if (dense_tiles[0])
        SQY_TIMED("batch_bitswap1_decode", sqy::launch_bitswap1_decode_batch(jobs(L.planes), words(L.planes.tiles_at), (uint32_t)dense_jobs[0], dense_tiles[0], elem_size, stream));
    if (dense_tiles[1]) SQY_TIMED("batch_copy", sqy::launch_batch_copy(jobs(L.plain), words(L.plain.tiles_at), (uint32_t)dense_jobs[1], dense_tiles[1], stream));
    if (dense_tiles[2])
        SQY_TIMED("batch_quantiser_decode", sqy::launch_bitswap1_quantiser_decode_batch(jobs(L.quantised), words(L.quantised.tiles_at), reinterpret_cast<const uint16_t*>(dj + L.quantised.extra_at),
                                                                                         (uint32_t)dense_jobs[2], dense_tiles[2], stream));
    if (sv && (launch_views(G.cx, stream, sv->scatter, ViewLaunch::bitswap1_decode, 1, elem_size) || launch_views(G.cx, stream, sv->copy, ViewLaunch::copy_to_view, 2, elem_size)))
        return 1;
    if (sv && (launch_windows(G.cx, stream, sv->wscatter, WindowLaunch::bitswap1_decode, elem_size) || launch_windows(G.cx, stream, sv->wcopy, WindowLaunch::copy_from_lz4, elem_size)))
        return 1;
    if (sv && (launch_compares(G.cx, stream, sv->cscatter, CompareLaunch::bitswap1_decode, elem_size) || launch_compares(G.cx, stream, sv->ccopy, CompareLaunch::compare_in_lz4, elem_size)))
        return 1;
    if (nd) {
        // (every launch timed on its own: the profile counts the launches, 1 + steps whatever the number of blobs)
        const sqy::DiffBatchJob* d_diff = reinterpret_cast<const sqy::DiffBatchJob*>(dj + L.diff.jobs_at);
        SQY_TIMED("batch_diff3x3x1_decode", sqy::launch_diff3x3x1_decode_batch_copy(d_diff, words(L.diff.extra_at), nd, df.ntiles, stream));
        for (uint32_t step = 0; step < df.steps; ++step)
            SQY_TIMED("batch_diff3x3x1_decode", sqy::launch_diff3x3x1_decode_batch_step(d_diff, words(L.diff.tiles_at), nd, df.nstrips, step, df.max_columns, stream));
    }
    return 0;
}

// a window update's decode (SQYAMD_Update_BatchWindow_*, ud != nullptr): the headers have been fetched and checked (*ud->fetched, moved
// from); a `bitswap1->lz4` blob b with (*ud->keep_planes)[b] is planned as DecodeBatchForm::plain -- its LZ4 output, the plane stream, is
// what its destination gets -- and ud->patched[b] says whether it came out that way (sqy::update_blob_patched)
// into_place[b]: blob b's LZ4 output is what its place holds; a group of such blobs only is decoded straight into the places (all in ONE
// buffer: `places`, place_at[b] of places_bytes), with no launch behind the LZ4 decode (sqy::update_group_into_places)
struct UpdateDecode {
    const std::vector<uint8_t>* keep_planes;
    std::vector<uint8_t> patched;
    std::vector<SlabBlob>* fetched;
    bool fused_on;
    uint8_t* places;
    const std::vector<uint64_t>* place_at;
    uint64_t places_bytes;
    std::vector<uint8_t> into_place;
};

// The joint path for group gi of a batch's plan (made from plan_in under the bound group_bytes).  Blobs it cannot take are appended to
// `single`; the flag raised: all of the group go there.  Every destination is an allocation of its own, so the LZ4 output always goes to
// the workspace, where the plan says (out_at); the pipelines without a batched launch run their remaining inverses as in a slab set.
int decode_batch_group(Context& cx, const uint8_t* d_src, std::vector<SlabBlob>& blobs, const std::vector<sqy::DecodeBatchBlob>& plan_in, uint64_t group_bytes,
                       const sqy::DecodeBatchPlan& plan, size_t gi, int elem_size, hipStream_t stream, std::vector<size_t>& single, StridedDecode* sv = nullptr,
                       const UpdateDecode* ud = nullptr)
{
    if (sv) { sv->scatter.clear(); sv->copy.clear(); sv->wscatter.clear(); sv->wcopy.clear(); sv->cscatter.clear(); sv->ccopy.clear(); }     // (the group before has been synchronised)
    const sqy::DecodeBatchGroup* pg = &plan.groups[gi];
    const std::vector<size_t> g(pg->blobs.begin(), pg->blobs.end());
    for (size_t k = 0; k < g.size(); ++k) blobs[g[k]].out_base = pg->out_at[k];
    JointGroup G{cx, d_src, blobs, stream, kBatchNames};
    if (const int rc = group_rank(G, g, single)) return rc;
    if (G.mem.empty()) return 0;
    // the plan made again without the blobs the ranking refused: they keep their place in the workspace and have no job in any table
    sqy::DecodeBatchPlan again;
    if (G.mem.size() != g.size()) {
        std::vector<uint8_t> dropped(blobs.size(), 0);
        for (size_t b : g) dropped[b] = 1;
        for (size_t b : G.mem) dropped[b] = 0;
        again = sqy::decode_batch_plan(plan_in, group_bytes, &dropped);
        pg = &again.groups[gi];
    }
    // a window update's group whose LZ4 outputs all are what their places hold: straight into the places, nothing behind the LZ4 decode
    const bool into_places = ud && sqy::update_group_into_places(std::vector<uint32_t>(G.mem.begin(), G.mem.end()), ud->into_place);
    if (into_places) {
        for (size_t b : G.mem) blobs[b].out_base = (*ud->place_at)[b];
        G.out_bytes = ud->places_bytes;
        G.out = ud->places;
    } else {
        G.out_bytes = pg->out_bytes;
        if (cx.ws.slabs_out.ensure(std::max<uint64_t>(G.out_bytes, 16))) return 1;
        G.out = static_cast<uint8_t*>(cx.ws.slabs_out.p);
    }
    const sqy::DecodeJointLayout L = sqy::decode_joint_layout(G.mem.size(), G.maps.size(), G.nframes, pg);
    if (const int rc = group_lz4_decode(G, L)) return rc;
    std::vector<unsigned char> tables;
    if (!into_places)
        if (const int rc = batch_group_tail(G, L, *pg, plan_in, elem_size, tables, sv)) return rc;
    std::vector<size_t> rest;                                           // everything else: blob by blob, as in a slab set
    for (size_t b : G.mem) if (plan_in[b].form == sqy::DecodeBatchForm::stages) rest.push_back(b);
    if (const int rc = group_remaining_stages(G, rest)) return rc;
    return group_verdict(G, single);
}

// An entry of a caller's blob table: an offset from 0 on, a byte or more, a destination where the entry point (`who` in the message) takes them
bool blob_entry_ok(const char* who, int i, long offset, long length, bool has_dst = true)
{
    if (offset >= 0 && length > 0 && has_dst) return true;
    std::fprintf(stderr, "[sqeazy]\t %s: blob %d at %ld, %ld bytes%s\n", who, i, offset, length, has_dst ? "" : ", no destination");
    return false;
}

// The headers of a blob set (blobs[i].src, .len given): every blob's prefix with one synchronisation (a header longer than that: fetched on
// its own), each admitted for the entry point's voxel type and then shown to check(i) (false: refused) -- all before anything is written.
// who: how the messages name the entry point.
template <class F>
int fetch_blob_headers(Context& cx, std::vector<SlabBlob>& blobs, int want_elem, hipStream_t stream, const char* who, F&& check)
{
    const int n = (int)blobs.size();
    if (cx.ws.slabs_host.ensure((size_t)n * kSlabsHeadPrefix)) return 1;
    char* hp = static_cast<char*>(cx.ws.slabs_host.p);
    for (int i = 0; i < n; ++i)
        SQY_HIP(hipMemcpyAsync(hp + (uint64_t)i * kSlabsHeadPrefix, blobs[i].src, std::min(kSlabsHeadPrefix, blobs[i].len), hipMemcpyDeviceToHost, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i) {
        SlabBlob& b = blobs[i];
        const uint64_t take = std::min(kSlabsHeadPrefix, b.len);
        b.h = sqy::header_unpack(hp + (uint64_t)i * kSlabsHeadPrefix, hp + (uint64_t)i * kSlabsHeadPrefix + take);
        if (!b.h.valid && take < b.len && fetch_header(b.src, b.len, stream, b.h)) return 1;
        if (!b.h.valid) { std::fprintf(stderr, "[sqeazy]\t %s: no sqy header in blob %d\n", who, i); return 1; }
        if (!admit_blob(b.h, b.len, want_elem, &b.raw, (std::string(who) + ": blob " + std::to_string(i)).c_str())) return 1;
        if (!check(i)) return 1;
    }
    return 0;
}

// Whether blob b may take the joint path, with its DecodeCall (destination dst) made: the last stage lz4 and chunks of one LZ4 block.  More
// than one chunk for a slab set (the ranking then tells the chunked layout from the serial one); a batch also takes ONE chunk -- a
// single-chunk stream is the same bytes in both layouts.
bool joint_candidate(Context& cx, SlabBlob& b, void* dst, int want_elem, hipStream_t stream, uint64_t min_chunks)
{
    b.call.reset(new DecodeCall(cx, stream, dst, b.h, Pipeline::from_string(b.h.pipename), b.raw / (uint64_t)want_elem, b.src + b.h.size));
    DecodeCall& c = *b.call;
    const size_t ns = c.pipe.stages.size();
    if (ns == 0 || c.pipe.stages[ns - 1].kind != StageKind::lz4) return false;
    b.li = ns - 1;
    b.total = c.in_bytes(b.li);
    static_cast<sqy::Lz4DecodeGeometry&>(b) = sqy::lz4_decode_geometry(c.pipe.stages[b.li].lz4, b.total);
    return b.nchunks >= min_chunks && b.chunk <= b.block_bytes;
}

int decode_slabs_on_device(Context& cx, const void* d_src_v, const long* offsets, const long* lengths, int nslabs, void* d_dst_v, uint64_t dst_capacity,
                           long* frames, int inflight, int want_elem, hipStream_t stream)
{
    if (!d_src_v || !d_dst_v || !offsets || !lengths || nslabs <= 0) { std::fprintf(stderr, "[sqeazy]\t decode slabs: bad arguments\n"); return 1; }
    const uint8_t* d_src = static_cast<const uint8_t*>(d_src_v);
    uint8_t* d_dst = static_cast<uint8_t*>(d_dst_v);
    DrainOnExit drain{stream, &cx.pending, cx.side};
    std::vector<SlabBlob> blobs((size_t)nslabs);
    for (int i = 0; i < nslabs; ++i) {
        if (!blob_entry_ok("decode slabs", i, offsets[i], lengths[i])) return 1;
        blobs[i].src = d_src + offsets[i];
        blobs[i].len = (uint64_t)lengths[i];
    }
    // 1. the headers: every blob's prefix with one synchronisation (a header longer than that: fetched on its own), checked before anything
    // is written
    uint64_t volume = 0;
    if (fetch_blob_headers(cx, blobs, want_elem, stream, "decode slabs", [&](int i) {
            SlabBlob& b = blobs[i];
            const sqy::HeaderInfo& h0 = blobs[0].h;
            if (b.h.shape.size() != h0.shape.size() || !std::equal(b.h.shape.begin() + 1, b.h.shape.end(), h0.shape.begin() + 1)) {
                std::fprintf(stderr, "[sqeazy]\t decode slabs: blob %d's shape does not continue blob 0's\n", i);
                return false;
            }
            b.dst_off = volume;
            volume += b.raw;
            return true;
        })) return 1;
    if (volume > dst_capacity) { std::fprintf(stderr, "[sqeazy]\t decode slabs: %llu bytes do not fit the buffer\n", (unsigned long long)volume); return 1; }
    if (frames) for (int i = 0; i < nslabs; ++i) frames[i] = (long)blobs[i].h.shape[0];

    // 2. who takes the joint path: the last stage lz4, more than one chunk (the ranking then tells the chunked layout from the serial one)
    std::vector<size_t> joint, single;
    for (int i = 0; i < nslabs; ++i) {
        SlabBlob& b = blobs[i];
        const bool ok = g_opt.decode_slabs_joint.load() != 0 && joint_candidate(cx, b, d_dst + b.dst_off, want_elem, stream, 2);
        (ok ? joint : single).push_back((size_t)i);
    }
    // 3. groups: LZ4 output up to kSlabsGroupBytes (at least one blob), at most `inflight` blobs, one block size (sqy_pipeline.cpp)
    std::vector<sqy::SlabJointBlob> sizes;
    for (size_t b : joint) sizes.push_back(sqy::SlabJointBlob{blobs[b].total, blobs[b].block_bytes});
    for (std::vector<size_t>& g : sqy::decode_slab_groups(sizes, kSlabsGroupBytes, inflight)) {
        for (size_t& j : g) j = joint[j];
        if (const int rc = decode_slabs_group(cx, d_src, blobs, g, d_dst, volume, stream, single)) return rc;
    }
    // 4. the others, one at a time
    for (size_t b : single)
        blobs[b].rc = decode_on_device(cx, blobs[b].src, blobs[b].len, d_dst + blobs[b].dst_off, blobs[b].raw, want_elem, stream);
    for (const SlabBlob& b : blobs) if (b.rc) return b.rc;
    return 0;
}

// host-pointer slab-set decode: the span of the blobs goes to the device, the volume comes back
int decode_slabs_from_host(const char* src, const long* offsets, const long* lengths, int nslabs, char* dst, long dst_capacity, long* frames,
                           int elem_size)
{
    if (!src || !dst || !offsets || !lengths || nslabs <= 0) { std::fprintf(stderr, "[sqeazy]\t decode slabs: bad arguments\n"); return 1; }
    uint64_t span = 0, volume = 0;
    for (int i = 0; i < nslabs; ++i) {                                   // untrusted input: before anything is allocated or uploaded
        if (!blob_entry_ok("decode slabs", i, offsets[i], lengths[i])) return 1;
        const sqy::HeaderInfo h = sqy::header_unpack(src + offsets[i], src + offsets[i] + lengths[i]);
        if (!h.valid) { std::fprintf(stderr, "[sqeazy]\t decode slabs: no sqy header in blob %d\n", i); return 1; }
        uint64_t raw = 0;
        if (!header_shape_ok(h, (uint64_t)lengths[i], &raw)) return 1;
        volume += raw;
        span = std::max<uint64_t>(span, (uint64_t)offsets[i] + (uint64_t)lengths[i]);
    }
    if (volume > (uint64_t)std::max(dst_capacity, 0l)) { std::fprintf(stderr, "[sqeazy]\t decode slabs: %llu bytes do not fit the buffer\n", (unsigned long long)volume); return 1; }
    return decode_staged(src, span, dst, volume, [&](Context& cx, void* d_src, void* d_dst, hipStream_t stream) {
        return decode_slabs_on_device(cx, d_src, offsets, lengths, nslabs, d_dst, volume, frames, 0, elem_size, stream);
    });
}

// ---- batch decode (SQYAMD_Decode_Batch_*) -------------------------------------------------------------------------------------
// Independent blobs -- any shape, any pipeline, each destination an allocation of its own --, the way back from a batch encode.  The
// joint-eligible ones (the last stage lz4, chunks of one LZ4 block; ONE chunk will do) go through decode_batch_group in the groups
// sqy::decode_batch_plan deals them to: per group one frame ranking, one read-back of its counts, one joint index and LZ4 decode into the
// workspace, batch_group_tail's launches, one verdict read-back.  Every other blob, and what a group hands back, goes through
// decode_on_device in blob order.
struct BatchDecodeArgs { const long* offsets; const long* lengths; int nblobs; void* const* dsts; const long* capacities; long* decoded; };

// the arguments alone, before any device is looked for; decoded_bytes zeroed where it can be
int admit_decode_batch(const void* src, const BatchDecodeArgs& a)
{
    if (a.decoded && a.nblobs > 0) for (int i = 0; i < a.nblobs; ++i) a.decoded[i] = 0;
    if (!src || !a.offsets || !a.lengths || !a.dsts || !a.capacities || a.nblobs <= 0) { std::fprintf(stderr, "[sqeazy]\t decode batch: bad arguments\n"); return 1; }
    for (int i = 0; i < a.nblobs; ++i)
        if (!blob_entry_ok("decode batch", i, a.offsets[i], a.lengths[i], a.dsts[i] != nullptr)) return 1;
    return 0;
}

// what a blob's header has to say before anything is written: it fits its destination, which is aligned to the voxel size
bool batch_blob_fits(int i, uint64_t raw, const void* dst, long capacity, int elem_size)
{
    if (raw > (uint64_t)std::max(capacity, 0l)) { std::fprintf(stderr, "[sqeazy]\t decode batch: blob %d's %llu bytes do not fit its buffer\n", i, (unsigned long long)raw); return false; }
    if (reinterpret_cast<uintptr_t>(dst) % (uintptr_t)elem_size) { std::fprintf(stderr, "[sqeazy]\t decode batch: destination %d not aligned to the voxel size\n", i); return false; }
    return true;
}

// The joint forms behind a filter stage, of 16-bit blobs (p.form stays `stages` for everything else):
//   quantiser->bitswap1->lz4: the LZ4 output is the 8-bit plane stream of the n quantised voxels; the decode table as the single call reads
//   it (a table that cannot be had: `stages`, where that call says so)
//   diff3x3x1->bitswap1->lz4, diff3x3x1->lz4: the geometry of launch_diff3x3x1_decode's chain of several frames per launch, a destination
//   on the 16-byte grid
void batch_stage_form(SlabBlob& b, const void* dst, int want_elem, sqy::DecodeBatchBlob& p)
{
    const DecodeCall& c = *b.call;
    const std::vector<Stage>& st = c.pipe.stages;
    if (want_elem != 2 || st.size() < 2 || st.size() > 3 || c.count_before[st.size() - 1] != c.n) return;
    if (st.size() == 3 && st[1].kind != StageKind::bitswap1) return;
    if (st[0].kind == StageKind::quantiser) {
        if (st.size() != 3 || c.elem_before[0] != 2 || c.elem_before[1] != 1 || b.total != c.n || !quantiser_lut_on_host(st[0], &b.lut, false)) return;
        p.form = sqy::DecodeBatchForm::quantised;
        p.len = c.n;
    } else if (st[0].kind == StageKind::diff3x3x1) {
        if (c.elem_before[st.size() - 1] != 2 || b.total != b.raw || b.h.shape.size() != 3 || (reinterpret_cast<uintptr_t>(dst) & 15) != 0) return;
        const uint64_t w = sqy::diff3x3x1_decode_chain_columns(b.h.shape[0], b.h.shape[1], b.h.shape[2], 2);
        if (!w || !sqy::diff3x3x1_decode_frames_fit(w)) return;
        p.form = st.size() == 3 ? sqy::DecodeBatchForm::diff_planes : sqy::DecodeBatchForm::diff_plain;
        p.len = c.n;
        p.Z = (uint32_t)b.h.shape[0]; p.Y = (uint32_t)b.h.shape[1]; p.X = (uint32_t)b.h.shape[2];
        p.chain_columns = (uint32_t)w;
    }
}

// views (SQYAMD_Decode_BatchStrided_*): blob i's header shape must be row i of shapes (rank dimensions); a.dsts[i] is view i
// windows (SQYAMD_Decode_BatchWindow_*, wa != nullptr): row i of shapes is the extent of a window of blob i that begins at row i of
// wa->origins; a blob whose window is all of it is a view as above, and a call of such blobs only takes every path it takes there
// compares (SQYAMD_Compare_BatchWindow_*, wa->compare != nullptr): a.dsts[i] is only read; every blob is a window, the whole ones too.  What
// the driver leaves for its caller when it has handled every blob (done): each blob's code and its window's voxels
struct CompareOut { unsigned long long* d_records; std::vector<int> rc; std::vector<uint64_t> voxels; bool done = false; };
struct WindowArgs { const long* origins; const long* strides; CompareOut* compare = nullptr; };
int decode_batch_on_device(Context& cx, const void* d_src_v, const BatchDecodeArgs& a, int want_elem, hipStream_t stream,
                           const std::vector<sqy::BatchView>* views = nullptr, const long* shapes = nullptr, unsigned rank = 0, const WindowArgs* wa = nullptr,
                           UpdateDecode* ud = nullptr)
{
    const uint8_t* d_src = static_cast<const uint8_t*>(d_src_v);
    StridedDecode sv;
    sv.views = views;
    ViewLaunch unpacks;                                                 // (in front of the drain: alive until it has synchronised)
    WindowLaunch wcopies;
    CompareLaunch ccopies;
    CompareOut* const cmp = wa ? wa->compare : nullptr;
    sv.records = cmp ? cmp->d_records : nullptr;
    std::vector<sqy::BatchWindow> wins(wa ? (size_t)a.nblobs : 0);
    DrainOnExit drain{stream, &cx.pending, cx.side};
    const size_t n = (size_t)a.nblobs;
    std::vector<SlabBlob> blobs(n);
    for (size_t i = 0; i < n; ++i) {
        blobs[i].src = d_src + a.offsets[i];
        blobs[i].len = (uint64_t)a.lengths[i];
    }
    if (ud) blobs = std::move(*ud->fetched);
    // 1. the headers, checked before anything is written
    if (!ud && fetch_blob_headers(cx, blobs, want_elem, stream, "decode batch", [&](int i) {
            if (wa) {                                                   // (the view was admitted for the window's extent, aligned to the voxel size)
                if (sqy::admit_window(blobs[i].h.shape, wa->origins ? wa->origins + (size_t)i * rank : nullptr, shapes + (size_t)i * rank, rank, &wins[(size_t)i])) return true;
                std::fprintf(stderr, "[sqeazy]\t decode batch: blob %d's window does not lie inside its shape\n", i);
                return false;
            }
            if (views) {
                const std::vector<uint64_t>& hs = blobs[i].h.shape;
                bool same = hs.size() == rank;
                for (unsigned k = 0; same && k < rank; ++k) same = hs[k] == (uint64_t)shapes[(size_t)i * rank + k];
                if (!same) { std::fprintf(stderr, "[sqeazy]\t decode batch: blob %d's shape is not its view's\n", i); return false; }
            }
            return batch_blob_fits(i, blobs[i].raw, a.dsts[i], a.capacities[i], want_elem);
        }))
        return 1;
    // the blobs whose window is a part of them; none: a call of views
    std::vector<uint8_t> windowed(n, 0);
    bool any_window = false;
    for (size_t i = 0; i < wins.size(); ++i) if (cmp || !wins[i].whole) { windowed[i] = 1; any_window = true; }
    if (cmp) {                                                          // the records: zeros, VIEW_MIN all ones -- on the stream, behind the admission
        std::vector<PendingEvent>* pend = &cx.pending;
        SQY_TIMED("batch_compare_init", sqy::launch_batch_compare_init(cmp->d_records, (uint32_t)n, stream));
    }
    if (a.decoded)
        for (size_t i = 0; i < n; ++i) a.decoded[i] = windowed[i] ? (long)(wins[i].Z * wins[i].Y * wins[i].X * (uint64_t)want_elem) : (long)blobs[i].raw;
    const bool joint_on = g_opt.decode_batch_joint.load() != 0;
    // where blob i's voxels go as a dense volume: its destination -- or, for a view that is no dense allocation, a place in
    // Workspace::batch_pack, unpacked by ONE launch at the end of the call; unless (batch_strided_fused) its pipeline is one whose last
    // launch on the joint path can write into the view: `bitswap1->lz4`, `lz4`
    std::vector<void*> dst_of(a.dsts, a.dsts + n);
    bool strided = false;
    if (views) {
        const bool fused = joint_on && g_opt.batch_strided_fused.load() != 0, wfused = joint_on && (cmp ? g_opt.batch_compare_fused.load() : g_opt.batch_window_fused.load()) != 0;
        sv.direct.assign(n, 0);
        if (any_window) {
            sv.wins = &wins;
            sv.wviews.resize(n);
            for (size_t i = 0; i < n; ++i) sv.wviews[i] = window_view(wins[i], wa->strides ? wa->strides + i * rank : nullptr, rank);
        }
        std::vector<uint64_t> place(n, 0);
        uint64_t bytes = 0;
        for (size_t i = 0; i < n; ++i) {
            if (!windowed[i] && (*views)[i].dense) continue;
            strided = true;
            const std::vector<Stage> st = Pipeline::from_string(blobs[i].h.pipename).stages;
            if ((windowed[i] ? wfused : fused) && !st.empty() && st.back().kind == StageKind::lz4 && (st.size() == 1 || (st.size() == 2 && st[0].kind == StageKind::bitswap1)))
                sv.direct[i] = windowed[i] ? 2 : 1;
            else { place[i] = bytes; bytes += align_up(blobs[i].raw, 256); }
        }
        if (bytes && cx.ws.batch_pack.ensure(bytes)) return 1;
        for (size_t i = 0; i < n; ++i)
            if ((windowed[i] || !(*views)[i].dense) && !sv.direct[i]) {
                dst_of[i] = static_cast<uint8_t*>(cx.ws.batch_pack.p) + place[i];
                if (cmp) ccopies.add(a.dsts[i], dst_of[i], wins[i], sv.wviews[i], false, cmp->d_records + sqy::kCompareFields * i);
                else if (windowed[i]) wcopies.add(a.dsts[i], dst_of[i], wins[i], sv.wviews[i], false);
                else unpacks.add(a.dsts[i], dst_of[i], (*views)[i]);
            }
    }
    StridedDecode* const svp = strided ? &sv : nullptr;

    // 2. who takes the joint path and in which group (the plan: host-only, sqy_pipeline.cpp)
    std::vector<sqy::DecodeBatchBlob> plan_in(n);
    std::vector<size_t> single;
    for (size_t i = 0; i < n && joint_on; ++i) {
        SlabBlob& b = blobs[i];
        sqy::DecodeBatchBlob& p = plan_in[i];
        p.eligible = joint_candidate(cx, b, dst_of[i], want_elem, stream, 1);
        if (!p.eligible) continue;
        const DecodeCall& c = *b.call;
        const std::vector<Stage>& st = c.pipe.stages;
        p.total = b.total;
        p.block_bytes = b.block_bytes;
        if (st.size() == 1) { p.form = sqy::DecodeBatchForm::plain; p.len = b.total; }
        else if (st.size() == 2 && st[0].kind == StageKind::bitswap1 && c.elem_before[0] == want_elem && c.count_before[0] == c.n && b.total == b.raw) {
            p.form = sqy::DecodeBatchForm::planes;
            p.len = c.n;
        } else
            batch_stage_form(b, dst_of[i], want_elem, p);
        if (ud) {
            if ((ud->patched[i] = sqy::update_blob_patched((*ud->keep_planes)[i] != 0, p.form, true))) { p.form = sqy::DecodeBatchForm::plain; p.len = b.total; }
            ud->into_place[i] = sqy::update_lz4_into_place(ud->fused_on, p.form);
        }
        // (a view that was to take its voxels directly and has no such form after all: on its own, below)
        if (svp && sv.direct[i] && p.form != sqy::DecodeBatchForm::planes && p.form != sqy::DecodeBatchForm::plain) p.eligible = false;
    }
    const uint64_t group_bytes = (uint64_t)g_opt.decode_batch_group_bytes.load();
    const sqy::DecodeBatchPlan plan = sqy::decode_batch_plan(plan_in, group_bytes);
    for (size_t i = 0; i < n; ++i) if (plan.group_of[i] < 0) single.push_back(i);
    for (size_t gi = 0; gi < plan.groups.size(); ++gi)
        if (const int rc = decode_batch_group(cx, d_src, blobs, plan_in, group_bytes, plan, gi, want_elem, stream, single, svp, ud)) return rc;
    // 3. the others, one at a time, in blob order
    std::sort(single.begin(), single.end());
    for (size_t b : single) {
        if (ud) ud->patched[b] = sqy::update_blob_patched((*ud->keep_planes)[b] != 0, sqy::DecodeBatchForm::planes, false);    // (decoded dense after all)
        if (!svp || !sv.direct[b]) {
            blobs[b].rc = decode_on_device(cx, blobs[b].src, blobs[b].len, dst_of[b], blobs[b].raw, want_elem, stream);
            continue;
        }
        // a view without a place in the workspace: decoded into one of its own, unpacked
        if (cx.ws.batch_pack_one.ensure(blobs[b].raw)) return 1;
        blobs[b].rc = decode_on_device(cx, blobs[b].src, blobs[b].len, cx.ws.batch_pack_one.p, blobs[b].raw, want_elem, stream);
        if (blobs[b].rc) continue;
        ViewLaunch one;
        WindowLaunch wone;
        CompareLaunch cone;
        if (cmp) {                                                      // (a group that was given up may have added into the record: made ready again)
            std::vector<PendingEvent>* pend = &cx.pending;
            SQY_TIMED("batch_compare_init", sqy::launch_batch_compare_init(cmp->d_records + sqy::kCompareFields * b, 1, stream));
            cone.add(a.dsts[b], cx.ws.batch_pack_one.p, wins[b], sv.wviews[b], false, cmp->d_records + sqy::kCompareFields * b);
        } else if (windowed[b]) wone.add(a.dsts[b], cx.ws.batch_pack_one.p, wins[b], sv.wviews[b], false);
        else one.add(a.dsts[b], cx.ws.batch_pack_one.p, (*views)[b]);
        if (launch_views(cx, stream, one, ViewLaunch::unpack, 0, want_elem) || launch_windows(cx, stream, wone, WindowLaunch::copy, want_elem) ||
            launch_compares(cx, stream, cone, CompareLaunch::compare, want_elem))
            return 1;
        SQY_HIP(hipStreamSynchronize(stream));                          // (the launch's tables are this scope's)
    }
    // 4. the views with a place in the workspace: ONE unpack launch; the windows with one: ONE window copy
    if (svp && (launch_views(cx, stream, unpacks, ViewLaunch::unpack, 0, want_elem) || launch_windows(cx, stream, wcopies, WindowLaunch::copy, want_elem) ||
                launch_compares(cx, stream, ccopies, CompareLaunch::compare, want_elem)))
        return 1;
    if (cmp) {
        for (size_t i = 0; i < n; ++i) { cmp->rc[i] = blobs[i].rc; cmp->voxels[i] = wins[i].Z * wins[i].Y * wins[i].X; }
        cmp->done = true;
    }
    for (const SlabBlob& b : blobs) if (b.rc) return b.rc;
    return 0;
}

// SQYAMD_Decode_BatchStrided_*: the arguments and every view on the host, then the batch driver with the views
int decode_batch_strided_device(const void* d_src, const long* offsets, const long* lengths, int nblobs, void* const* d_dsts, const long* dst_shapes,
                                const long* dst_strides, unsigned rank, long* decoded, int elem_size, void* hip_stream)
{
    if (decoded && nblobs > 0) for (int i = 0; i < nblobs; ++i) decoded[i] = 0;
    if (!d_src || !offsets || !lengths || !d_dsts || !dst_shapes || nblobs <= 0) { std::fprintf(stderr, "[sqeazy]\t decode batch: bad arguments\n"); return 1; }
    std::vector<sqy::BatchView> views;
    if (admit_views("decode batch", d_dsts, dst_shapes, dst_strides, rank, nblobs, elem_size, &views)) return 1;
    std::vector<long> caps((size_t)nblobs);
    for (int i = 0; i < nblobs; ++i) {
        const sqy::BatchView& v = views[(size_t)i];
        const uint64_t bytes = v.Z * v.Y * v.X * (uint64_t)elem_size;
        if (bytes > (uint64_t)LONG_MAX) return 1;
        caps[(size_t)i] = (long)bytes;
    }
    const BatchDecodeArgs a{offsets, lengths, nblobs, d_dsts, caps.data(), decoded};
    if (admit_decode_batch(d_src, a)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_batch_on_device(*lease.ctx, d_src, a, elem_size, static_cast<hipStream_t>(hip_stream), &views, dst_shapes, rank);
}

// SQYAMD_Decode_BatchWindow_*: the arguments and every view (of the window's extent) on the host, then the batch driver with the views and
// the windows' origins -- it admits each window against its blob's header before anything is written
int decode_batch_window_device(const void* d_src, const long* offsets, const long* lengths, int nblobs, const long* src_origins, void* const* d_dsts,
                               const long* dst_shapes, const long* dst_strides, unsigned rank, long* decoded, int elem_size, void* hip_stream)
{
    if (decoded && nblobs > 0) for (int i = 0; i < nblobs; ++i) decoded[i] = 0;
    if (!d_src || !offsets || !lengths || !d_dsts || !dst_shapes || nblobs <= 0) { std::fprintf(stderr, "[sqeazy]\t decode batch: bad arguments\n"); return 1; }
    std::vector<sqy::BatchView> views;
    if (admit_views("decode batch", d_dsts, dst_shapes, dst_strides, rank, nblobs, elem_size, &views)) return 1;
    const std::vector<long> caps((size_t)nblobs, LONG_MAX);             // (a window's bytes are its view's: nothing to fit)
    const BatchDecodeArgs a{offsets, lengths, nblobs, d_dsts, caps.data(), decoded};
    if (admit_decode_batch(d_src, a)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    const WindowArgs wa{src_origins, dst_strides};
    return decode_batch_on_device(*lease.ctx, d_src, a, elem_size, static_cast<hipStream_t>(hip_stream), &views, dst_shapes, rank, &wa);
}

// SQYAMD_Compare_BatchWindow_*: decode_batch_window_device's admission (and the origins' sign, which needs no header), the batch driver
// with a record per blob, ONE copy of the records behind its last launch.  stats: nblobs rows of sqy::kCompareFields words, zeroed on
// every failure; the row of a damaged blob all ones
int compare_batch_window_device(const void* d_src, const long* offsets, const long* lengths, int nblobs, const long* src_origins, const void* const* d_views,
                                const long* view_shapes, const long* view_strides, unsigned rank, unsigned long long* stats, int elem_size, void* hip_stream)
{
    const size_t words = nblobs > 0 ? (size_t)nblobs * sqy::kCompareFields : 0;
    if (stats) std::fill(stats, stats + words, 0ull);
    if (!d_src || !offsets || !lengths || !d_views || !view_shapes || !stats || nblobs <= 0) { std::fprintf(stderr, "[sqeazy]\t compare batch: bad arguments\n"); return 1; }
    std::vector<sqy::BatchView> views;
    if (admit_views("compare batch", d_views, view_shapes, view_strides, rank, nblobs, elem_size, &views)) return 1;
    for (size_t k = 0; src_origins && k < (size_t)nblobs * rank; ++k)
        if (src_origins[k] < 0) { std::fprintf(stderr, "[sqeazy]\t compare batch: window %zu begins in front of its blob\n", k / rank); return 1; }
    const std::vector<long> caps((size_t)nblobs, LONG_MAX);             // (a window's bytes are its view's: nothing to fit)
    const BatchDecodeArgs a{offsets, lengths, nblobs, const_cast<void* const*>(d_views), caps.data(), nullptr};      // (read only: WindowArgs::compare)
    if (admit_decode_batch(d_src, a)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Context& cx = *lease.ctx;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (cx.ws.batch_records.ensure(words * 8)) return 1;
    unsigned long long* d_records = static_cast<unsigned long long*>(cx.ws.batch_records.p);
    CompareOut out{d_records, std::vector<int>((size_t)nblobs, 0), std::vector<uint64_t>((size_t)nblobs, 0)};
    const WindowArgs wa{src_origins, view_strides, &out};
    const int rc = decode_batch_on_device(cx, d_src, a, elem_size, stream, &views, view_shapes, rank, &wa);
    if (!out.done) return rc ? rc : 1;
    std::vector<unsigned long long> host(words);
    SQY_HIP(hipMemcpyAsync(host.data(), d_records, words * 8, hipMemcpyDeviceToHost, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < (size_t)nblobs; ++i) {
        unsigned long long* row = stats + i * sqy::kCompareFields;
        if (out.rc[i]) { std::fill(row, row + sqy::kCompareFields, ~0ull); continue; }
        std::copy(host.begin() + i * sqy::kCompareFields, host.begin() + (i + 1) * sqy::kCompareFields, row);
        row[0] = out.voxels[i];
    }
    return rc;
}

// ---- many boxes of one large blob compared with resident voxels (SQYAMD_Compare_Boxes_*) -----------------------------------
// BoxesCall with loads where Decode_Boxes stores: a record of eight 64-bit words per box in Workspace::batch_records made ready on the
// stream in front of the ONE output launch that adds into the records, ONE copy of them behind it; sqy::compare_boxes_path says what
// runs.  The views are only read and nothing outside the workspace is written.
static_assert(sizeof(sqy::Bitswap1BoxCompareJob) == sqy::kBitswap1BoxCompareJobBytes && sizeof(sqy::Bitswap1BoxCompareJob) % 16 == 0, "the comparing box job's layout");

// one window compare under `name`, a job per box: box i (ws[i]) of the dense volume at denses[i] against its view
int launch_boxes_compare(Context& cx, hipStream_t stream, CompareLaunch& l, const char* name, int elem_size)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.boxes_jobs, &d_tiles)) return 1;
    SQY_TIMED(name, sqy::launch_batch_window_compare(static_cast<const sqy::BatchCompareJob*>(cx.ws.boxes_jobs.p), d_tiles, (uint32_t)l.jobs.size(), l.ntiles, elem_size, stream));
    return 0;
}

// the compare's one launch behind DecodeCall::frames_subset: box i (ws[i], its view vs[i] at views[i]) of the united frames in c.range_buf
// into the record at d_records + 8 i
int boxes_range_compare(DecodeCall& c, CompareLaunch& l, TiledJobs<sqy::Bitswap1BoxCompareJob>& tj, const std::vector<sqy::BatchWindow>& ws, const std::vector<WindowView>& vs,
                        const void* const* views, unsigned rank, unsigned long long* d_records)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const size_t count = ws.size();
    if (sqy::compare_boxes_path(true, c.range_form, true) == sqy::BoxPath::subset_transposer) {
        const uint16_t* lut = nullptr;
        if (c.range_lut(&lut)) return 1;
        for (size_t i = 0; i < count; ++i) {
            sqy::Bitswap1BoxCompareJob j{};
            j.view = views[i];
            fill_range_job(j, ws[i], vs[i].sz, vs[i].sy, p.boxes[i], p.we);
            j.record = d_records + sqy::kCompareFields * i;
            if (!sqy::bitswap1_box_compare_job_ok(j)) return 1;
            tj.push(j, range_job_groups_of(p.boxes[i], p.we));
        }
        const uint32_t* d_tiles = nullptr;
        if (tj.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
        SQY_TIMED(lut ? "bitswap1_quantiser_compare_boxes" : "bitswap1_compare_boxes",
                  sqy::launch_bitswap1_decode_range_windows_compare(c.range_buf, static_cast<const sqy::Bitswap1BoxCompareJob*>(c.cx.ws.boxes_jobs.p), d_tiles, (uint32_t)count,
                                                                    tj.ntiles, p.we, lut, stream));
        return 0;
    }
    // plain, shuffle: boxes_range_out's geometry
    for (size_t i = 0; i < count; ++i)
        l.add(views[i], c.range_buf + p.boxes[i].range_at, sqy::window_in_own_frames(ws[i], rank), vs[i], false, d_records + sqy::kCompareFields * i);
    return launch_boxes_compare(c.cx, stream, l, "boxes_window_compare", c.h.elem_size());
}

// Box i = [origins + i rank, .. + extents + i rank) of the blob against the view at d_views[i] (strides + i rank, or dense).  The checks
// of decode_boxes_on_device -- all before anything runs on the device.  stats: count rows, zeroed by the caller; every row all ones where
// the decode fails behind the admission (a damaged frame that some box needs)
int compare_boxes_on_device(Context& cx, const void* d_src_v, uint64_t srclen, size_t count, const long* origins, const void* const* d_views, const long* extents,
                            const long* strides, unsigned rank, int want_elem, hipStream_t stream, unsigned long long* stats)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    BoxesCall b(cx, "compare boxes", d_src_v, srclen, want_elem, stream);
    std::vector<WindowView> vs;
    if (admit_box_windows(b, count, origins, extents, strides, rank, &vs)) return 1;
    const size_t words = count * sqy::kCompareFields;
    if (cx.ws.batch_records.ensure(words * 8)) return 1;
    unsigned long long* d_records = static_cast<unsigned long long*>(cx.ws.batch_records.p);
    std::vector<unsigned long long> host(words);
    CompareLaunch l;                                                    // (both wait for the stream before their tables go)
    TiledJobs<sqy::Bitswap1BoxCompareJob> tj;
    // the records made ready in front of `compare`, their copy to the host behind it -- in front of the call's last synchronisation
    auto records_around = [&](auto&& compare) -> int {
        SQY_TIMED("batch_compare_init", sqy::launch_batch_compare_init(d_records, (uint32_t)count, stream));
        if (const int rc = compare()) return rc;
        SQY_HIP(hipMemcpyAsync(host.data(), d_records, words * 8, hipMemcpyDeviceToHost, stream));
        return 0;
    };
    const int rc = b.run(g_opt.compare_boxes_subset.load() != 0, nullptr,
                         [&](DecodeCall& c) { return records_around([&] { return boxes_range_compare(c, l, tj, b.ws, vs, d_views, rank, d_records); }); },
                         [&](const void* volume) {
                             return records_around([&] {
                                 for (size_t i = 0; i < count; ++i) l.add(d_views[i], volume, b.ws[i], vs[i], false, d_records + sqy::kCompareFields * i);
                                 return launch_boxes_compare(cx, stream, l, "boxes_window_compare", want_elem);
                             });
                         });
    if (!b.verdict) return rc;
    // the rows behind the call's last synchronisation: the records with VOXELS filled in, or all ones where the decode failed
    for (size_t i = 0; i < count; ++i) {
        unsigned long long* row = stats + i * sqy::kCompareFields;
        if (rc) { std::fill(row, row + sqy::kCompareFields, ~0ull); continue; }
        std::copy(host.begin() + i * sqy::kCompareFields, host.begin() + (i + 1) * sqy::kCompareFields, row);
        row[0] = b.ws[i].Z * b.ws[i].Y * b.ws[i].X;
    }
    return rc;
}

// SQYAMD_Compare_Boxes_*_Device: decode_boxes_device's checks with the views read-only; stats zeroed on every refusal
int compare_boxes_device(const void* d_src, long srclength, long count, const long* origins, const void* const* d_views, const long* view_shapes, const long* view_strides,
                         unsigned rank, unsigned long long* stats, int elem_size, void* hip_stream)
{
    if (stats && count > 0 && count <= INT_MAX) std::fill(stats, stats + (size_t)count * sqy::kCompareFields, 0ull);
    if (!stats || !d_views || !boxes_arguments_ok(d_src, srclength, count, origins, d_views, view_shapes, rank)) {
        std::fprintf(stderr, "[sqeazy]\t compare boxes: bad arguments\n");
        return 1;
    }
    std::vector<sqy::BatchView> views;
    if (admit_views("compare boxes", d_views, view_shapes, view_strides, rank, (int)count, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return compare_boxes_on_device(*lease.ctx, d_src, (uint64_t)srclength, (size_t)count, origins, d_views, view_shapes, view_strides, rank, elem_size,
                                   static_cast<hipStream_t>(hip_stream), stats);
}

// host pointers: the header and every box are checked here, before anything is staged; views: the boxes' voxels dense, back to back in
// box order, exactly views_bytes of them.  The blob and the views are staged once each: two inputs, so the staging is its own
int compare_boxes_from_host(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views, long views_bytes,
                            unsigned long long* stats, int elem_size)
{
    if (stats && count > 0 && count <= INT_MAX) std::fill(stats, stats + (size_t)count * sqy::kCompareFields, 0ull);
    if (!stats || !views || !boxes_arguments_ok(src, srclength, count, origins, nullptr, extents, rank)) { std::fprintf(stderr, "[sqeazy]\t compare boxes: bad arguments\n"); return 1; }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    std::vector<uint64_t> bytes, at;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw) || !host_box_bytes("compare boxes", h, count, origins, extents, rank, elem_size, &bytes)) return 1;
    if (!sqy::output_offsets(bytes, views_bytes, &at) || at.back() != (uint64_t)views_bytes) {
        std::fprintf(stderr, "[sqeazy]\t compare boxes: the views hold another number of bytes than the boxes\n");
        return 1;
    }
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Context& cx = *lease.ctx;
    hipStream_t stream = cx.own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    if (cx.ws.io_src.ensure(std::max<uint64_t>((uint64_t)srclength, 16)) || cx.ws.io_dst.ensure(std::max<uint64_t>(at.back(), 16))) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    if (!cx.stager.copy(cx.ws.io_src.p, const_cast<char*>(src), (size_t)srclength, true, dev_id) ||
        !cx.stager.copy(cx.ws.io_dst.p, const_cast<char*>(views), (size_t)at.back(), true, dev_id)) {
        std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n");
        return 1;
    }
    std::vector<const void*> ptrs((size_t)count);
    for (long i = 0; i < count; ++i) ptrs[(size_t)i] = static_cast<const uint8_t*>(cx.ws.io_dst.p) + at[(size_t)i];
    return compare_boxes_on_device(cx, cx.ws.io_src.p, (uint64_t)srclength, (size_t)count, origins, ptrs.data(), extents, nullptr, rank, elem_size, stream, stats);
}

// ---- many boxes of one large blob projected along an axis (SQYAMD_Project_Boxes_*) -----------------------------------------
// BoxesCall with a combine into images of rank - 1 as its sink; sqy::project_boxes_path says what runs and sqy::admit_projection what is
// admitted.  Its own: the neutral-element launch in front of the atomics, and the walk form without either.  Nothing but the images'
// elements is written outside the workspace.
static_assert(sizeof(sqy::Bitswap1BoxProjectJob) == sqy::kBitswap1BoxProjectJobBytes && sizeof(sqy::BoxProjectJob) == sqy::kBoxProjectJobBytes, "the projecting jobs' layout");

// the thread-per-element projection's jobs: box i (w, its projection q) of the dense volume at `dense` into the image at `out`
struct ProjectLaunch : TiledJobs<sqy::BoxProjectJob> {
    void add(void* out, const void* dense, const sqy::BatchWindow& w, const sqy::Projection& q, int op)
    {
        push(sqy::BoxProjectJob{dense, out, (w.oz * w.bY + w.oy) * w.bX + w.ox, q.E0, q.E1, q.p0, q.su, q.sv, q.sa, q.n, (uint32_t)op, 0, 0},
             (uint32_t)((q.E0 * q.E1 + 255) / 256));
    }
};
int launch_boxes_project(Context& cx, hipStream_t stream, ProjectLaunch& l, int elem_size)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.boxes_jobs, &d_tiles)) return 1;
    SQY_TIMED("boxes_window_project", sqy::launch_boxes_window_project(static_cast<const sqy::BoxProjectJob*>(cx.ws.boxes_jobs.p), d_tiles, (uint32_t)l.jobs.size(), l.ntiles,
                                                                        elem_size, stream));
    return 0;
}

// the projection's launches behind DecodeCall::frames_subset: box i (ws[i], qs[i]) of the united frames in c.range_buf into outs[i]
int boxes_range_project(DecodeCall& c, ProjectLaunch& l, TiledJobs<sqy::Bitswap1BoxProjectJob>& tj, const std::vector<sqy::BatchWindow>& ws,
                        const std::vector<sqy::Projection>& qs, void* const* outs, unsigned rank, int op)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const size_t count = ws.size();
    if (sqy::project_boxes_path(true, c.range_form, true) == sqy::BoxPath::subset_transposer) {
        const uint16_t* lut = nullptr;
        if (c.range_lut(&lut)) return 1;
        for (size_t i = 0; i < count; ++i) {
            const sqy::Projection& q = qs[i];
            sqy::Bitswap1BoxProjectJob j{};
            j.out = outs[i];
            fill_range_job(j, ws[i], q.sz, q.sy, p.boxes[i], p.we);
            j.op = (uint32_t)op; j.axis = q.axis3;
            j.E0 = q.E0; j.E1 = q.E1; j.p0 = q.p0;
            if (!sqy::bitswap1_box_project_job_ok(j)) return 1;
            tj.jobs.push_back(j);
        }
        // the form: axis 0 with every job on the 32-voxel grid walks z in registers and stores once; else the atomics.  The
        // jobs' workgroups depend on it: counted behind the decision
        bool walk = g_opt.project_boxes_walk.load() != 0 && reinterpret_cast<uintptr_t>(c.range_buf) % 4u == 0;
        uint64_t walk_groups = 0;
        for (size_t i = 0; walk && i < count; ++i) {
            walk = sqy::bitswap1_box_project_walk_ok(tj.jobs[i], p.we);
            walk_groups += sqy::project_walk_groups(tj.jobs[i].g);
        }
        walk = walk && walk_groups <= 0x7fffffffull;
        for (size_t i = 0; i < count; ++i) {
            tj.first_tile.push_back(tj.ntiles);
            tj.ntiles += walk ? (uint32_t)sqy::project_walk_groups(tj.jobs[i].g) : range_job_groups_of(p.boxes[i], p.we);
        }
        const uint32_t* d_tiles = nullptr;
        if (tj.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
        const sqy::Bitswap1BoxProjectJob* d_jobs = static_cast<const sqy::Bitswap1BoxProjectJob*>(c.cx.ws.boxes_jobs.p);
        if (walk) {
            SQY_TIMED(lut ? "bitswap1_quantiser_project_boxes" : "bitswap1_project_boxes",
                      sqy::launch_bitswap1_decode_range_windows_project_walk(c.range_buf, d_jobs, d_tiles, (uint32_t)count, tj.ntiles, p.we, lut, stream));
            return 0;
        }
        SQY_TIMED("boxes_project_init", sqy::launch_boxes_project_init(d_jobs, d_tiles, (uint32_t)count, tj.ntiles, stream));
        SQY_TIMED(lut ? "bitswap1_quantiser_project_boxes" : "bitswap1_project_boxes",
                  sqy::launch_bitswap1_decode_range_windows_project(c.range_buf, d_jobs, d_tiles, (uint32_t)count, tj.ntiles, p.we, lut, stream));
        return 0;
    }
    // plain, shuffle: boxes_range_out's geometry
    for (size_t i = 0; i < count; ++i) l.add(outs[i], c.range_buf + p.boxes[i].range_at, sqy::window_in_own_frames(ws[i], rank), qs[i], op);
    return launch_boxes_project(c.cx, stream, l, c.h.elem_size());
}

// Box i = [origins + i rank, .. + extents + i rank) of the blob projected along `axis` into the image at d_outs[i] (out_strides +
// i (rank - 1), or dense).  sqy::admit_projection for every box and the launches' sizes -- all before anything is written
int project_boxes_on_device(Context& cx, const void* d_src_v, uint64_t srclen, size_t count, const long* origins, const long* extents, unsigned rank, int axis, int op,
                            void* const* d_outs, const long* out_strides, int want_elem, hipStream_t stream)
{
    BoxesCall b(cx, "project boxes", d_src_v, srclen, want_elem, stream);
    std::vector<sqy::Projection> qs(count);
    const int refused = b.admit(count, origins, extents, rank, [&](size_t i, const long* o, const long* e, sqy::BatchWindow* w, uint64_t* element_groups) {
        if (!sqy::admit_projection(b.h.shape, o, e, rank, axis, op, voxel_max(want_elem), d_outs[i], out_strides ? out_strides + i * (rank - 1) : nullptr, w, &qs[i]))
            return box_refused(b.who, i, "does not lie inside the blob's shape or has another rank, or its sum might not fit 32 bits");
        *element_groups = (qs[i].E0 * qs[i].E1 + 255) / 256;
        return true;
    });
    if (refused || !b.one_launch_holds()) return 1;
    ProjectLaunch l;                                                    // (both wait for the stream before their tables go)
    TiledJobs<sqy::Bitswap1BoxProjectJob> tj;
    return b.run(g_opt.project_boxes_subset.load() != 0, nullptr, [&](DecodeCall& c) { return boxes_range_project(c, l, tj, b.ws, qs, d_outs, rank, op); },
                 [&](const void* volume) {
                     for (size_t i = 0; i < count; ++i) l.add(d_outs[i], volume, b.ws[i], qs[i], op);
                     return launch_boxes_project(cx, stream, l, want_elem);
                 });
}

// what SQYAMD_Project_Boxes_* checks without a header, before a device is looked for: boxes_arguments_ok, and sqy::admit_projection of
// every box in its own shape -- the axis, the op, the image's pointer and pitches, the sum bound
bool project_arguments_ok(const void* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op, void* const* outs,
                          const long* out_strides, int elem_size)
{
    if (!boxes_arguments_ok(src, srclength, count, origins, outs, extents, rank)) return false;
    return every_box_in_its_own_shape(count, origins, extents, rank, [&](size_t i, const std::vector<uint64_t>& shape, const long* o, const long* e) {
        sqy::BatchWindow w;
        sqy::Projection q;
        const void* out = outs ? outs[i] : static_cast<const void*>(&q);                                   // (host variant: the images are the library's)
        return sqy::admit_projection(shape, o, e, rank, axis, op, voxel_max(elem_size), out, outs && out_strides ? out_strides + i * (rank - 1) : nullptr, &w, &q);
    });
}

int project_boxes_device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op, void* const* d_outs,
                         const long* out_strides, int elem_size, void* hip_stream)
{
    if (!d_outs || !project_arguments_ok(d_src, srclength, count, origins, extents, rank, axis, op, d_outs, out_strides, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t project boxes: bad arguments\n");
        return 1;
    }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return project_boxes_on_device(*lease.ctx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, axis, op, d_outs, out_strides, elem_size,
                                   static_cast<hipStream_t>(hip_stream));
}

// host pointers: the header and every box are checked here, before anything is staged; the images come back dense, back to back in box
// order, 32-bit elements
int project_boxes_from_host(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op, char* out,
                            long out_capacity, int elem_size)
{
    if (!out || !project_arguments_ok(src, srclength, count, origins, extents, rank, axis, op, nullptr, nullptr, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t project boxes: bad arguments\n");
        return 1;
    }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw)) return 1;
    std::vector<uint64_t> bytes((size_t)count), at;
    const bool admitted = every_box((size_t)count, origins, extents, rank, [&](size_t i, const long* o, const long* e) {
        sqy::BatchWindow w;
        sqy::Projection q;
        if (!sqy::admit_projection(h.shape, o, e, rank, axis, op, voxel_max(elem_size), &q, nullptr, &w, &q))
            return box_refused("project boxes", i, "does not lie inside the blob's shape, or its sum might not fit 32 bits");
        bytes[i] = q.E0 * q.E1 * 4u;
        return true;
    });
    if (!admitted || !host_outputs_fit("project boxes", bytes, out_capacity, &at)) return 1;
    return boxes_staged(src, srclength, out, at, [&](Context& cx, void* d_src, void* const* ptrs, hipStream_t stream) {
        return project_boxes_on_device(cx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, axis, op, ptrs, nullptr, elem_size, stream);
    });
}

// ---- many boxes of one large blob read at a coarser resolution (SQYAMD_Bin_Boxes_*) -----------------------------------------
// BoxesCall with cells as its sink; sqy::bin_boxes_path says what runs, sqy::admit_binning what is admitted and sqy::bin_boxes_plan how
// the bit-plane kernel's workgroups share a box's cells.  Its own: the launches' sizes are the cells' and the plan's blocks, checked box
// by box.  No neutral-element launch, no global atomics.  Nothing but the outputs' cells is written outside the workspace.
static_assert(sizeof(sqy::Bitswap1BoxBinJob) == sqy::kBitswap1BoxBinJobBytes && sizeof(sqy::BoxBinJob) == sqy::kBoxBinJobBytes, "the binning jobs' layout");

// the thread-per-cell launch's jobs: box i (w, its binning q) of the dense volume at `dense` into the output at `out`
struct BinLaunch : TiledJobs<sqy::BoxBinJob> {
    void add(void* out, const void* dense, const sqy::BatchWindow& w, const sqy::Binning& q, int op)
    {
        push(sqy::BoxBinJob{dense, out, (w.oz * w.bY + w.oy) * w.bX + w.ox, w.bY * w.bX, w.bX, {w.Z, w.Y, w.X}, {q.bins[0], q.bins[1], q.bins[2]},
                            {q.C[0], q.C[1], q.C[2]}, q.pz, q.py, (uint32_t)op, 0, 0},
             (uint32_t)((q.C[0] * q.C[1] * q.C[2] + 255) / 256));
    }
};
int launch_boxes_bin(Context& cx, hipStream_t stream, BinLaunch& l, int elem_size)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.boxes_jobs, &d_tiles)) return 1;
    SQY_TIMED("boxes_window_bin", sqy::launch_boxes_window_bin(static_cast<const sqy::BoxBinJob*>(cx.ws.boxes_jobs.p), d_tiles, (uint32_t)l.jobs.size(), l.ntiles, elem_size, stream));
    return 0;
}

// the binning's launch behind DecodeCall::frames_subset: box i (ws[i], qs[i]) of the united frames in c.range_buf into outs[i]
int boxes_range_bin(DecodeCall& c, BinLaunch& l, TiledJobs<sqy::Bitswap1BoxBinJob>& tj, const std::vector<sqy::BatchWindow>& ws, const std::vector<sqy::Binning>& qs,
                    void* const* outs, unsigned rank, int op)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const size_t count = ws.size();
    if (sqy::bin_boxes_path(true, c.range_form, true) == sqy::BoxPath::subset_transposer) {
        const uint16_t* lut = nullptr;
        if (c.range_lut(&lut)) return 1;
        for (size_t i = 0; i < count; ++i) {
            const sqy::Binning& q = qs[i];
            sqy::Bitswap1BoxBinJob j{};
            j.out = outs[i];
            fill_range_job(j, ws[i], q.pz, q.py, p.boxes[i], p.we);
            std::copy(q.bins, q.bins + 3, j.bins);
            j.plan = sqy::bin_boxes_plan(q.C, q.bins, ws[i].X);
            j.op = (uint32_t)op;
            j.zreg = sqy::bitswap1_box_bin_zreg_ok(j) ? 1u : 0u;
            if (!sqy::bitswap1_box_bin_job_ok(j) || (uint64_t)tj.ntiles + j.plan.blocks > 0x7fffffffull) return 1;
            tj.push(j, (uint32_t)j.plan.blocks);
        }
        const uint32_t* d_tiles = nullptr;
        if (tj.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
        SQY_TIMED(lut ? "bitswap1_quantiser_bin_boxes" : "bitswap1_bin_boxes",
                  sqy::launch_bitswap1_decode_range_windows_bin(c.range_buf, static_cast<const sqy::Bitswap1BoxBinJob*>(c.cx.ws.boxes_jobs.p), d_tiles, (uint32_t)count, tj.ntiles,
                                                                p.we, lut, stream));
        return 0;
    }
    // plain, shuffle: boxes_range_out's geometry
    for (size_t i = 0; i < count; ++i) l.add(outs[i], c.range_buf + p.boxes[i].range_at, sqy::window_in_own_frames(ws[i], rank), qs[i], op);
    return launch_boxes_bin(c.cx, stream, l, c.h.elem_size());
}

// Box i = [origins + i rank, .. + extents + i rank) of the blob binned into the output at d_outs[i] (out_strides + i rank, or dense).
// sqy::admit_binning for every box and the launches' sizes -- all before anything is written
int bin_boxes_on_device(Context& cx, const void* d_src_v, uint64_t srclen, size_t count, const long* origins, const long* extents, unsigned rank, const long* bins, int op,
                        void* const* d_outs, const long* out_strides, int want_elem, hipStream_t stream)
{
    BoxesCall b(cx, "bin boxes", d_src_v, srclen, want_elem, stream);
    std::vector<sqy::Binning> qs(count);
    uint64_t cell_groups = 0, blocks = 0;                    // what the one output launch may hold, whichever it is
    const int refused = b.admit(count, origins, extents, rank, [&](size_t i, const long* o, const long* e, sqy::BatchWindow* w, uint64_t*) {
        if (!sqy::admit_binning(b.h.shape, o, e, rank, bins, op, voxel_max(want_elem), d_outs[i], out_strides ? out_strides + i * rank : nullptr, w, &qs[i]))
            return box_refused(b.who, i, "does not lie inside the blob's shape or has another rank, or a cell's sum might not fit 32 bits");
        cell_groups += (qs[i].C[0] * qs[i].C[1] * qs[i].C[2] + 255) / 256;           // (the cells are no more than the blob's voxels: no wrap)
        blocks += sqy::bin_boxes_plan(qs[i].C, qs[i].bins, w->X).blocks;
        return b.launch_holds(std::max(cell_groups, blocks));             // (checked box by box: the sums stay far below 2^64)
    });
    if (refused) return 1;
    BinLaunch l;                                                        // (both wait for the stream before their tables go)
    TiledJobs<sqy::Bitswap1BoxBinJob> tj;
    return b.run(g_opt.bin_boxes_subset.load() != 0, nullptr, [&](DecodeCall& c) { return boxes_range_bin(c, l, tj, b.ws, qs, d_outs, rank, op); },
                 [&](const void* volume) {
                     for (size_t i = 0; i < count; ++i) l.add(d_outs[i], volume, b.ws[i], qs[i], op);
                     return launch_boxes_bin(cx, stream, l, want_elem);
                 });
}

// what SQYAMD_Bin_Boxes_* checks without a header, before a device is looked for: boxes_arguments_ok, and sqy::admit_binning of every box
// in its own shape -- the bins, the op, the output's pointer and pitches, the sum bound
bool bin_arguments_ok(const void* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, void* const* outs,
                      const long* out_strides, int elem_size)
{
    if (!bins || !boxes_arguments_ok(src, srclength, count, origins, outs, extents, rank)) return false;
    return every_box_in_its_own_shape(count, origins, extents, rank, [&](size_t i, const std::vector<uint64_t>& shape, const long* o, const long* e) {
        sqy::BatchWindow w;
        sqy::Binning q;
        const void* out = outs ? outs[i] : static_cast<const void*>(&q);                                   // (host variant: the outputs are the library's)
        return sqy::admit_binning(shape, o, e, rank, bins, op, voxel_max(elem_size), out, outs && out_strides ? out_strides + i * rank : nullptr, &w, &q);
    });
}

int bin_boxes_device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, void* const* d_outs,
                     const long* out_strides, int elem_size, void* hip_stream)
{
    if (!d_outs || !bin_arguments_ok(d_src, srclength, count, origins, extents, rank, bins, op, d_outs, out_strides, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t bin boxes: bad arguments\n");
        return 1;
    }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return bin_boxes_on_device(*lease.ctx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, bins, op, d_outs, out_strides, elem_size,
                               static_cast<hipStream_t>(hip_stream));
}

// host pointers: the header and every box are checked here, before anything is staged; the outputs come back dense, back to back in box
// order, 32-bit elements
int bin_boxes_from_host(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, char* out,
                        long out_capacity, int elem_size)
{
    if (!out || !bin_arguments_ok(src, srclength, count, origins, extents, rank, bins, op, nullptr, nullptr, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t bin boxes: bad arguments\n");
        return 1;
    }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw)) return 1;
    std::vector<uint64_t> bytes((size_t)count), at;
    const bool admitted = every_box((size_t)count, origins, extents, rank, [&](size_t i, const long* o, const long* e) {
        sqy::BatchWindow w;
        sqy::Binning q;
        if (!sqy::admit_binning(h.shape, o, e, rank, bins, op, voxel_max(elem_size), &q, nullptr, &w, &q))
            return box_refused("bin boxes", i, "does not lie inside the blob's shape, or a cell's sum might not fit 32 bits");
        bytes[i] = q.C[0] * q.C[1] * q.C[2] * 4u;
        return true;
    });
    if (!admitted || !host_outputs_fit("bin boxes", bytes, out_capacity, &at)) return 1;
    return boxes_staged(src, srclength, out, at, [&](Context& cx, void* d_src, void* const* ptrs, hipStream_t stream) {
        return bin_boxes_on_device(cx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, bins, op, ptrs, nullptr, elem_size, stream);
    });
}

// ---- a whole resolution pyramid of many boxes of one large blob (SQYAMD_Pyramid_Boxes_*) ------------------------------------
// BoxesCall with a table of cell grids per box as its sink, the united frames decoded ONCE for all levels; sqy::pyramid_boxes_path says
// what runs, sqy::admit_pyramid what is admitted -- the launches' sizes with it (sqy::PyramidSizes) -- and sqy::pyramid_boxes_plan which
// levels the bit-plane kernel fuses and how its workgroups share a box's cells.  Its own: the pyramid_reduce launches behind level 0 or
// behind the fused levels.  No neutral-element launch, no global atomics.  Nothing but the outputs' cells is written outside the workspace.
static_assert(sizeof(sqy::Bitswap1BoxPyramidJob) == sqy::kBitswap1BoxPyramidJobBytes && sizeof(sqy::PyramidReduceJob) == sqy::kPyramidReduceJobBytes,
              "the pyramid jobs' layout");

// a pyramid_reduce launch's jobs: level `to` of a box out of its stored level `from`
struct ReduceLaunch : TiledJobs<sqy::PyramidReduceJob> {
    void add(const sqy::Pyramid& y, void* const* outs, uint32_t from, uint32_t to, int op)
    {
        const sqy::Binning& s = y.q[from];
        const sqy::Binning& d = y.q[to];
        sqy::PyramidReduceJob j{};
        j.src = outs[from];
        j.out = outs[to];
        for (int k = 0; k < 3; ++k) {
            j.Cs[k] = s.C[k];
            j.C[k] = d.C[k];
            j.r[k] = std::min(y.raw[to][k] / y.raw[from][k], s.C[k]);     // (the rows nest: a whole ratio; clamped, the same cells)
        }
        j.spz = s.pz; j.spy = s.py; j.pz = d.pz; j.py = d.py;
        j.op = (uint32_t)op;
        push(j, (uint32_t)((d.C[0] * d.C[1] * d.C[2] + 255) / 256));
    }
};
int launch_pyramid_reduce_jobs(Context& cx, hipStream_t stream, ReduceLaunch& l, DevBuf& buf)
{
    if (l.jobs.empty()) return 0;
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, buf, &d_tiles)) return 1;
    SQY_TIMED("pyramid_reduce", sqy::launch_pyramid_reduce(static_cast<const sqy::PyramidReduceJob*>(buf.p), d_tiles, (uint32_t)l.jobs.size(), l.ntiles, stream));
    return 0;
}

// everything behind level 0 where no kernel fuses it: with `fused` ONE launch that takes every further level straight from level 0, else
// a launch per level from the level below
int pyramid_tail_from_level0(Context& cx, hipStream_t stream, ReduceLaunch (&rl)[sqy::kPyramidMaxLevels], const std::vector<sqy::Pyramid>& ys, void* const* outs, long levels,
                             int op, bool fused)
{
    for (long l = 1; l < levels; ++l) {
        ReduceLaunch& r = rl[fused ? 0 : l - 1];
        for (size_t i = 0; i < ys.size(); ++i) r.add(ys[i], outs + i * (size_t)levels, fused ? 0u : (uint32_t)(l - 1), (uint32_t)l, op);
    }
    for (long l = 0; l + 1 < levels; ++l)
        if (launch_pyramid_reduce_jobs(cx, stream, rl[l], cx.ws.pyramid_jobs[l])) return 1;
    return 0;
}

// the launches behind DecodeCall::frames_subset: box i (ws[i], ys[i]) of the united frames in c.range_buf into its outputs outs + i levels
int boxes_range_pyramid(DecodeCall& c, BinLaunch& l, TiledJobs<sqy::Bitswap1BoxBinJob>& tj, TiledJobs<sqy::Bitswap1BoxPyramidJob>& pj,
                        ReduceLaunch (&rl)[sqy::kPyramidMaxLevels], const std::vector<sqy::BatchWindow>& ws, const std::vector<sqy::Pyramid>& ys, void* const* outs,
                        unsigned rank, long levels, int op, bool fused)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const size_t count = ws.size();
    const sqy::PyramidPath path = sqy::pyramid_boxes_path(true, c.range_form, true, fused);
    if (path.path != sqy::BoxPath::subset_transposer || !path.fused) {
        // level 0 is Bin_Boxes' launch of the path, the rest pyramid_reduce's
        std::vector<void*> level0(count);
        std::vector<sqy::Binning> q0(count);
        for (size_t i = 0; i < count; ++i) { level0[i] = outs[i * (size_t)levels]; q0[i] = ys[i].q[0]; }
        if (const int rc = boxes_range_bin(c, l, tj, ws, q0, level0.data(), rank, op)) return rc;
        return pyramid_tail_from_level0(c.cx, stream, rl, ys, outs, levels, op, path.fused);
    }
    const uint16_t* lut = nullptr;
    if (c.range_lut(&lut)) return 1;
    for (size_t i = 0; i < count; ++i) {
        const sqy::BatchWindow& w = ws[i];
        const sqy::Pyramid& y = ys[i];
        sqy::Bitswap1BoxPyramidJob j{};
        for (long k = 0; k < levels; ++k) { j.out[k] = outs[i * (size_t)levels + (size_t)k]; j.pz[k] = y.q[k].pz; j.py[k] = y.q[k].py; }
        fill_range_job(j, w, y.q[0].pz, y.q[0].py, p.boxes[i], p.we);
        std::copy(y.q[0].bins, y.q[0].bins + 3, j.bins);
        const uint64_t E[3] = {w.Z, w.Y, w.X};
        j.plan = sqy::pyramid_boxes_plan(y, E);
        j.op = (uint32_t)op;
        j.zreg = (w.bY * w.bX) % 32 == 0 ? 1u : 0u;
        if (!sqy::bitswap1_box_pyramid_job_ok(j) || (uint64_t)pj.ntiles + j.plan.blocks > 0x7fffffffull) return 1;
        pj.push(j, (uint32_t)j.plan.blocks);
        for (uint32_t k = j.plan.T + 1; k < (uint32_t)levels; ++k) rl[0].add(y, outs + i * (size_t)levels, j.plan.T, k, op);      // the levels above T: from the stored level T
    }
    const uint32_t* d_tiles = nullptr;
    if (pj.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
    SQY_TIMED(lut ? "bitswap1_quantiser_pyramid_boxes" : "bitswap1_pyramid_boxes",
              sqy::launch_bitswap1_decode_range_windows_pyramid(c.range_buf, static_cast<const sqy::Bitswap1BoxPyramidJob*>(c.cx.ws.boxes_jobs.p), d_tiles, (uint32_t)count,
                                                                pj.ntiles, p.we, lut, stream));
    return launch_pyramid_reduce_jobs(c.cx, stream, rl[0], c.cx.ws.pyramid_jobs[0]);
}

// Level l of box i = [origins + i rank, .. + extents + i rank) into d_outs[i levels + l] (out_strides + (i levels + l) rank, or dense).
// sqy::admit_pyramid for every box, the launches' sizes with it -- all before anything is written
int pyramid_boxes_on_device(Context& cx, const void* d_src_v, uint64_t srclen, size_t count, const long* origins, const long* extents, unsigned rank, long levels,
                            const long* bins, int op, void* const* d_outs, const long* out_strides, int want_elem, hipStream_t stream)
{
    BoxesCall b(cx, "pyramid boxes", d_src_v, srclen, want_elem, stream);
    std::vector<sqy::Pyramid> ys(count);
    sqy::PyramidSizes sizes;
    const int refused = b.admit(count, origins, extents, rank, [&](size_t i, const long* o, const long* e, sqy::BatchWindow* w, uint64_t*) {
        return sqy::admit_pyramid(b.h.shape, o, e, rank, levels, bins, op, voxel_max(want_elem), d_outs + i * (size_t)levels,
                                  out_strides ? out_strides + i * (size_t)levels * rank : nullptr, w, &ys[i], &sizes) ||
               box_refused(b.who, i, "does not lie inside the blob's shape or has another rank, a cell's sum might not fit 32 bits, or the call takes too many workgroups "
                                     "for one launch");
    });
    if (refused) return 1;
    const bool fused = g_opt.pyramid_boxes_fused.load() != 0;
    BinLaunch l;                                                        // (all wait for the stream before their tables go)
    TiledJobs<sqy::Bitswap1BoxBinJob> tj;
    TiledJobs<sqy::Bitswap1BoxPyramidJob> pj;
    ReduceLaunch rl[sqy::kPyramidMaxLevels];
    return b.run(g_opt.pyramid_boxes_subset.load() != 0, nullptr,
                 [&](DecodeCall& c) { return boxes_range_pyramid(c, l, tj, pj, rl, b.ws, ys, d_outs, rank, levels, op, fused); },
                 [&](const void* volume) {      // level 0 of all boxes in one launch, the rest pyramid_reduce's
                     for (size_t i = 0; i < count; ++i) l.add(d_outs[i * (size_t)levels], volume, b.ws[i], ys[i].q[0], op);
                     return launch_boxes_bin(cx, stream, l, want_elem) || pyramid_tail_from_level0(cx, stream, rl, ys, d_outs, levels, op, fused);
                 });
}

// what SQYAMD_Pyramid_Boxes_* checks without a header, before a device is looked for: boxes_arguments_ok, and sqy::admit_pyramid of every
// box in its own shape -- the levels, the nesting, the op, every output's pointer and pitches, the sum bound
bool pyramid_arguments_ok(const void* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, int op,
                          void* const* outs, const long* out_strides, int elem_size)
{
    if (!bins || levels < 1 || levels > (long)sqy::kPyramidMaxLevels || !boxes_arguments_ok(src, srclength, count, origins, nullptr, extents, rank)) return false;
    return every_box_in_its_own_shape(count, origins, extents, rank, [&](size_t i, const std::vector<uint64_t>& shape, const long* o, const long* e) {
        sqy::BatchWindow w;
        sqy::Pyramid y;
        const void* own[sqy::kPyramidMaxLevels];                                                           // (host variant: the outputs are the library's)
        for (long l = 0; l < levels; ++l) own[l] = outs ? outs[i * (size_t)levels + (size_t)l] : static_cast<const void*>(&w);
        return sqy::admit_pyramid(shape, o, e, rank, levels, bins, op, voxel_max(elem_size), own, outs && out_strides ? out_strides + i * (size_t)levels * rank : nullptr, &w, &y);
    });
}

int pyramid_boxes_device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, int op,
                         void* const* d_outs, const long* out_strides, int elem_size, void* hip_stream)
{
    if (!d_outs || !pyramid_arguments_ok(d_src, srclength, count, origins, extents, rank, levels, bins, op, d_outs, out_strides, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t pyramid boxes: bad arguments\n");
        return 1;
    }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return pyramid_boxes_on_device(*lease.ctx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, levels, bins, op, d_outs, out_strides, elem_size,
                                   static_cast<hipStream_t>(hip_stream));
}

// host pointers: the header and every box are checked here, before anything is staged; the outputs come back dense and back to back, box
// by box and levels ascending within a box, 32-bit elements
int pyramid_boxes_from_host(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, int op,
                            char* out, long out_capacity, int elem_size)
{
    if (!out || !pyramid_arguments_ok(src, srclength, count, origins, extents, rank, levels, bins, op, nullptr, nullptr, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t pyramid boxes: bad arguments\n");
        return 1;
    }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw)) return 1;
    std::vector<uint64_t> bytes((size_t)count * (size_t)levels), at;
    const bool admitted = every_box((size_t)count, origins, extents, rank, [&](size_t i, const long* o, const long* e) {
        sqy::BatchWindow w;
        sqy::Pyramid y;
        const void* own[sqy::kPyramidMaxLevels];
        for (long l = 0; l < levels; ++l) own[l] = &w;
        if (!sqy::admit_pyramid(h.shape, o, e, rank, levels, bins, op, voxel_max(elem_size), own, nullptr, &w, &y))
            return box_refused("pyramid boxes", i, "does not lie inside the blob's shape, or a cell's sum might not fit 32 bits");
        for (long l = 0; l < levels; ++l) bytes[i * (size_t)levels + (size_t)l] = y.q[l].C[0] * y.q[l].C[1] * y.q[l].C[2] * 4u;
        return true;
    });
    if (!admitted || !host_outputs_fit("pyramid boxes", bytes, out_capacity, &at)) return 1;
    return boxes_staged(src, srclength, out, at, [&](Context& cx, void* d_src, void* const* ptrs, hipStream_t stream) {
        return pyramid_boxes_on_device(cx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, levels, bins, op, ptrs, nullptr, elem_size, stream);
    });
}

// ---- the intensity histograms of many boxes of one large blob (SQYAMD_Histogram_Boxes_*) ------------------------------------
// BoxesCall with a count as its sink; sqy::histogram_boxes_path says what runs and sqy::admit_histogram what is admitted.  Its own: ONE
// launch that zeroes every histogram over the counting launch's own tables in front of it, and no view -- a job's pitches are the box's.
// Nothing but the histograms' counters is written outside the workspace.

// zeroes and one window histogram under the name "boxes_window_histogram", a job per box (its `view` the histogram)
int launch_boxes_histogram(Context& cx, hipStream_t stream, WindowLaunch& l, int elem_size, int shift)
{
    std::vector<PendingEvent>* pend = &cx.pending;
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, cx.ws.boxes_jobs, &d_tiles)) return 1;
    const sqy::BatchWindowJob* d_jobs = static_cast<const sqy::BatchWindowJob*>(cx.ws.boxes_jobs.p);
    SQY_TIMED("boxes_histogram_init", sqy::launch_boxes_histogram_init(d_jobs, d_tiles, (uint32_t)l.jobs.size(), l.ntiles, sqy::histogram_bins(elem_size, shift), stream));
    SQY_TIMED("boxes_window_histogram", sqy::launch_boxes_window_histogram(d_jobs, d_tiles, (uint32_t)l.jobs.size(), l.ntiles, elem_size, (uint32_t)shift,
                                                                            (int)g_opt.histogram_boxes_merge.load(), stream));
    return 0;
}
// the pitches of a box that is counted, not stored by place
WindowView counted_view(const sqy::BatchWindow& w) { return WindowView{w.Y * w.X, w.X}; }

// the histograms' launches behind DecodeCall::frames_subset: box i (ws[i]) of the united frames in c.range_buf into hists[i]
int boxes_range_histogram(DecodeCall& c, WindowLaunch& l, TiledJobs<sqy::Bitswap1BoxJob>& tj, const std::vector<sqy::BatchWindow>& ws, void* const* hists, unsigned rank,
                          int shift, int want_elem)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const size_t count = ws.size();
    if (sqy::histogram_boxes_path(true, c.range_form, true) == sqy::BoxPath::subset_transposer) {
        const uint16_t* lut = nullptr;
        if (c.range_lut(&lut)) return 1;
        if (sqy::histogram_bins(lut ? 2 : p.we, shift) != sqy::histogram_bins(want_elem, shift)) return 1;      // (the counted voxel is the entry point's)
        for (size_t i = 0; i < count; ++i) {
            sqy::Bitswap1BoxJob j{};
            j.view = hists[i];
            fill_range_job(j, ws[i], counted_view(ws[i]).sz, counted_view(ws[i]).sy, p.boxes[i], p.we);      // (the pitches are not used)
            if (!sqy::bitswap1_box_job_ok(j)) return 1;
            tj.push(j, range_job_groups_of(p.boxes[i], p.we));
        }
        const uint32_t* d_tiles = nullptr;
        if (tj.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
        const sqy::Bitswap1BoxJob* d_jobs = static_cast<const sqy::Bitswap1BoxJob*>(c.cx.ws.boxes_jobs.p);
        SQY_TIMED("boxes_histogram_init", sqy::launch_boxes_histogram_init(d_jobs, d_tiles, (uint32_t)count, tj.ntiles, sqy::histogram_bins(want_elem, shift), stream));
        SQY_TIMED(lut ? "bitswap1_quantiser_histogram_boxes" : "bitswap1_histogram_boxes",
                  sqy::launch_bitswap1_decode_range_windows_histogram(c.range_buf, d_jobs, d_tiles, (uint32_t)count, tj.ntiles, p.we, lut, (uint32_t)shift,
                                                                      (int)g_opt.histogram_boxes_merge.load(), stream));
        return 0;
    }
    // plain, shuffle: boxes_range_out's geometry
    for (size_t i = 0; i < count; ++i) l.add(hists[i], c.range_buf + p.boxes[i].range_at, sqy::window_in_own_frames(ws[i], rank), counted_view(ws[i]), false);
    return launch_boxes_histogram(c.cx, stream, l, c.h.elem_size(), shift);
}

// Box i = [origins + i rank, .. + extents + i rank) of the blob counted into the histogram at d_hists[i].  sqy::admit_histogram for
// every box and the launches' sizes -- all before anything is written
int histogram_boxes_on_device(Context& cx, const void* d_src_v, uint64_t srclen, size_t count, const long* origins, const long* extents, unsigned rank, int shift,
                              void* const* d_hists, int want_elem, hipStream_t stream)
{
    BoxesCall b(cx, "histogram boxes", d_src_v, srclen, want_elem, stream);
    const int refused = b.admit(count, origins, extents, rank, [&](size_t i, const long* o, const long* e, sqy::BatchWindow* w, uint64_t* copy_tiles) {
        if (!sqy::admit_histogram(b.h.shape, o, e, rank, shift, want_elem, d_hists[i], w)) return box_refused(b.who, i, "does not lie inside the blob's shape, or has another rank");
        *copy_tiles = sqy::batch_bitswap1_tiles(w->Z * w->Y * w->X);
        return true;
    });
    if (refused || !b.one_launch_holds()) return 1;
    WindowLaunch l;                                                     // (both wait for the stream before their tables go)
    TiledJobs<sqy::Bitswap1BoxJob> tj;
    return b.run(g_opt.histogram_boxes_subset.load() != 0, nullptr, [&](DecodeCall& c) { return boxes_range_histogram(c, l, tj, b.ws, d_hists, rank, shift, want_elem); },
                 [&](const void* volume) {
                     for (size_t i = 0; i < count; ++i) l.add(d_hists[i], volume, b.ws[i], counted_view(b.ws[i]), false);
                     return launch_boxes_histogram(cx, stream, l, want_elem, shift);
                 });
}

// what SQYAMD_Histogram_Boxes_* checks without a header, before a device is looked for: boxes_arguments_ok, and sqy::admit_histogram of
// every box in its own shape -- the shift, the histogram's pointer
bool histogram_arguments_ok(const void* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, void* const* hists,
                            int elem_size)
{
    if (!boxes_arguments_ok(src, srclength, count, origins, hists, extents, rank)) return false;
    return every_box_in_its_own_shape(count, origins, extents, rank, [&](size_t i, const std::vector<uint64_t>& shape, const long* o, const long* e) {
        sqy::BatchWindow w;
        const void* out = hists ? hists[i] : static_cast<const void*>(&w);                                 // (host variant: the histograms are the library's)
        return sqy::admit_histogram(shape, o, e, rank, shift, elem_size, out, &w);
    });
}

int histogram_boxes_device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, void* const* d_hists,
                           int elem_size, void* hip_stream)
{
    if (!d_hists || !histogram_arguments_ok(d_src, srclength, count, origins, extents, rank, shift, d_hists, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t histogram boxes: bad arguments\n");
        return 1;
    }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return histogram_boxes_on_device(*lease.ctx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, shift, d_hists, elem_size,
                                     static_cast<hipStream_t>(hip_stream));
}

// host pointers: the buffer, then the header and every box are checked here, before anything is staged; the histograms come back dense,
// back to back in box order, nbins 32-bit counters each
int histogram_boxes_from_host(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, char* out,
                              long out_capacity, int elem_size)
{
    if (!out || !histogram_arguments_ok(src, srclength, count, origins, extents, rank, shift, nullptr, elem_size)) {
        std::fprintf(stderr, "[sqeazy]\t histogram boxes: bad arguments\n");
        return 1;
    }
    std::vector<uint64_t> at;                                           // (count fits an int: no wrap)
    if (!host_outputs_fit("histogram boxes", std::vector<uint64_t>((size_t)count, (uint64_t)sqy::histogram_bins(elem_size, shift) * 4u), out_capacity, &at)) return 1;
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw)) return 1;
    const bool admitted = every_box((size_t)count, origins, extents, rank, [&](size_t i, const long* o, const long* e) {
        sqy::BatchWindow w;
        return sqy::admit_histogram(h.shape, o, e, rank, shift, elem_size, &w, &w) || box_refused("histogram boxes", i, "does not lie inside the blob's shape");
    });
    if (!admitted) return 1;
    return boxes_staged(src, srclength, out, at, [&](Context& cx, void* d_src, void* const* ptrs, hipStream_t stream) {
        return histogram_boxes_on_device(cx, d_src, (uint64_t)srclength, (size_t)count, origins, extents, rank, shift, ptrs, elem_size, stream);
    });
}

int decode_batch_device(const void* d_src, const BatchDecodeArgs& a, int elem_size, void* hip_stream)
{
    if (admit_decode_batch(d_src, a)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_batch_on_device(*lease.ctx, d_src, a, elem_size, static_cast<hipStream_t>(hip_stream));
}

// the host-pointer variant (not tuned): the span of the blobs staged up, one call of the device driver, every volume brought back
int decode_batch_from_host(const char* src, const BatchDecodeArgs& a, int elem_size)
{
    if (admit_decode_batch(src, a)) return 1;
    const size_t n = (size_t)a.nblobs;
    std::vector<uint64_t> raw(n), at(n);
    uint64_t span = 0, out_bytes = 0;
    for (size_t i = 0; i < n; ++i) {                                      // untrusted input: before anything is allocated or uploaded
        const sqy::HeaderInfo h = sqy::header_unpack(src + a.offsets[i], src + a.offsets[i] + a.lengths[i]);
        if (!h.valid) { std::fprintf(stderr, "[sqeazy]\t decode batch: no sqy header in blob %d\n", (int)i); return 1; }
        if (!admit_blob(h, (uint64_t)a.lengths[i], elem_size, &raw[i], ("decode batch: blob " + std::to_string(i)).c_str())) return 1;
        if (raw[i] > (uint64_t)std::max(a.capacities[i], 0l)) { std::fprintf(stderr, "[sqeazy]\t decode batch: blob %d's %llu bytes do not fit its buffer\n", (int)i, (unsigned long long)raw[i]); return 1; }
        span = std::max<uint64_t>(span, (uint64_t)a.offsets[i] + (uint64_t)a.lengths[i]);
        at[i] = out_bytes;
        out_bytes += align_up(raw[i], 256);
    }
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Workspace* ws = &lease.ctx->ws;
    hipStream_t stream = lease.ctx->own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    if (ws->io_src.ensure(std::max<uint64_t>(span, 16)) || ws->io_dst.ensure(std::max<uint64_t>(out_bytes, 16))) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    if (!lease.ctx->stager.copy(ws->io_src.p, const_cast<char*>(src), (size_t)span, true, dev_id)) { std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n"); return 1; }
    std::vector<void*> d_dsts(n);
    std::vector<long> caps(n);
    for (size_t i = 0; i < n; ++i) { d_dsts[i] = static_cast<char*>(ws->io_dst.p) + at[i]; caps[i] = (long)raw[i]; }
    const BatchDecodeArgs d{a.offsets, a.lengths, a.nblobs, d_dsts.data(), caps.data(), a.decoded};
    const int rc = decode_batch_on_device(*lease.ctx, ws->io_src.p, d, elem_size, stream);
    SQY_HIP(hipStreamSynchronize(stream));
    // (a damaged blob's code comes back behind the good ones, which are in place: they go home as well)
    for (size_t i = 0; i < n; ++i)
        if (!lease.ctx->stager.copy(d_dsts[i], static_cast<char*>(a.dsts[i]), (size_t)raw[i], false, dev_id)) { std::fprintf(stderr, "[sqeazy]\t device to host transfer failed\n"); return 1; }
    return rc;
}

// The body of the device-memory encode entry points: the blob at d_dst (_Device), or where *dstoffset says (at: _DeviceAt), with the
// offsets of the frames fq asks for (_DeviceAt_Frames: *count of them)
int encode_device(const char* pipeline, const void* d_src, const long* shape, unsigned rank, int elem_size, void* d_dst, long dst_capacity,
                  long* dstoffset, long* dstlength, int nthreads, void* hip_stream, bool at, FrameQuery* fq = nullptr, int* count = nullptr)
{
    if ((at && !dstoffset) || (fq && (fq->every <= 0 || !fq->offsets || !count))) return 1;
    StampScope stamps;                  // (in front of the lease: its last stamp is taken when the context has gone back)
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    const int rc = encode_on_device(*lease.ctx, pipeline, d_src, shape, rank, elem_size, d_dst, (uint64_t)std::max(dst_capacity, 0l), dstlength,
                                    nthreads, static_cast<hipStream_t>(hip_stream), dstoffset, fq, stamps.get());
    if (fq) *count = fq->count;
    return rc;
}

// ---- batch encode (SQYAMD_PipelineEncode_Batch_*) -------------------------------------------------
// Many volumes, one blob each, blob i inside slot i of d_dst.  The volumes the planner calls joint-eligible (sqy::encode_batch_form: the
// pipelines lz4, bitswap1->lz4 and quantiser->bitswap1->lz4 with the default weighting and the LUT in the header; sqy::lz4_batch_plan:
// the chunked layout, acceleration 1) go through the kernels group by group -- one launch per kernel for all volumes of a group, two
// host round trips per group (the dense pass's count and, quantised, the decode LUTs for the headers; the records) --, every other
// volume through encode_on_device.
static_assert(sizeof(sqy::Lz4BatchChunkPlan) == sizeof(sqy::Lz4BatchChunk) && sizeof(sqy::Lz4BatchChunk) == 24, "the joint chunk table's layout");
// what the host-only layouts of the batch and slab-set tables (sqy_pipeline.hpp) take the kernels' structs to be
static_assert(sizeof(sqy::Bitswap1Job) == sqy::kBitswap1JobBytes && sizeof(sqy::DiffBatchJob) == sqy::kDiffBatchJobBytes && sizeof(sqy::Lz4JointPart) == sqy::kLz4JointPartBytes &&
              sizeof(sqy::Lz4BatchChunk) == sqy::kLz4BatchChunkBytes && sizeof(sqy::Lz4BatchVolume) == sqy::kLz4BatchVolumeBytes, "the table layouts' element sizes");

// What a batch call checks before it touches the device or writes anything: every argument, the pipeline once, every volume's shape
struct BatchAdmit {
    Pipeline pipe;
    std::vector<std::vector<uint64_t>> dims;
    std::vector<uint64_t> len;              // voxels
};
int admit_batch(const char* pipeline, const void* const* srcs, const long* shapes, unsigned rank, int elem_size, int nvolumes, const void* dst,
                long slot_capacity, long* offsets, long* lengths, int nthreads, BatchAdmit* a)
{
    if (!offsets || !lengths) return 1;
    for (int i = 0; i < nvolumes; ++i) { offsets[i] = 0; lengths[i] = 0; }
    if (!pipeline || !srcs || !shapes || !dst || rank == 0 || nvolumes <= 0 || slot_capacity <= 0) return 1;
    if (admit_pipeline(pipeline, elem_size, nthreads, &a->pipe)) return 1;
    a->dims.resize((size_t)nvolumes);
    a->len.resize((size_t)nvolumes);
    for (int i = 0; i < nvolumes; ++i) {
        if (!srcs[i]) return 1;
        if (admit_shape(&a->pipe, shapes + (size_t)i * rank, rank, &a->dims[(size_t)i], &a->len[(size_t)i])) return 1;
    }
    return 0;
}

// one group of the plan through the kernels; rc 1 with a message when a blob does not fit its slot (nothing of that volume is written).
// staging: pinned, sqy::encode_batch_layout's staging_bytes for the group at its worst-case text
// views (nullptr: every volume dense) with how[vol], sqy ViewRead: how a volume that is no dense allocation is read
// patched (SQYAMD_Update_BatchWindow_*): d_srcs[vol] is the volume's OLD plane stream; the group's patch launch makes the new one from it
// and the window's view, in the transposer job's stead as `gathered` does
enum ViewRead : uint8_t { in_place = 0, gathered, packed_to_stream, packed, patched };
struct UpdateEncode { const std::vector<uint8_t>* is_patched; const void* const* views; const std::vector<sqy::BatchWindow>* wins; const std::vector<WindowView>* wviews; };
// the packed layout (SQYAMD_PipelineEncode_BatchPacked_*) for one group: it begins at `base` of d_dst (a multiple of align), gaps[j]
// (pinned, a word per volume of the group) is what the volumes outside the group take in front of its volume j, no blob may end behind
// `capacity`.  The group leaves every volume's blob length in lens[vol] and whether it was written in placed[vol]; offsets and lengths
// are the caller's to fill.  nullptr: the slot layout
struct PackedGroup { uint64_t align, base, capacity; const uint64_t* gaps; uint64_t* lens; uint8_t* placed; };
int encode_batch_group(Context& cx, const BatchAdmit& a, const sqy::Lz4BatchGroup& g, sqy::EncodeBatchForm form, int elem_size, const void* const* d_srcs,
                       uint8_t* d_dst, uint64_t slot_capacity, long* offsets, long* lengths, uint64_t* records, uint8_t* staging, hipStream_t stream,
                       const std::vector<sqy::BatchView>* views = nullptr, const std::vector<uint8_t>* how = nullptr, const PackedGroup* pk = nullptr,
                       const UpdateEncode* up = nullptr)
{
    Workspace* ws = &cx.ws;
    std::vector<PendingEvent>* pend = &cx.pending;
    const size_t nv = g.vols.size(), nc = g.chunks.size();
    const bool quantised = form == sqy::EncodeBatchForm::quantiser_bitswap1_lz4, transpose = quantised || form == sqy::EncodeBatchForm::bitswap1_lz4;
    // the header text: known now, or only behind round trip 1 (quantised: every volume's name carries its decode LUT)
    std::vector<std::string> text(nv);
    uint64_t text_bytes = 0;
    auto pack_text = [&](size_t j, const std::string& pipename) {
        std::string prefix, suffix;
        sqy::header_pack_parts(elem_size, false, a.dims[g.vols[j]], pipename, &prefix, &suffix);
        if (prefix.size() + suffix.size() > sqy::kBatchHeaderTextMax) {
            std::fprintf(stderr, "[sqeazy]\t volume %u: header text too long for the batch path\n", g.vols[j]);
            return 1;
        }
        text[j] = prefix + '\0' + suffix;                // (split again below: the prefix holds no NUL)
        text_bytes += prefix.size() + suffix.size();
        return 0;
    };
    if (!quantised) {
        const std::string pipename = a.pipe.name();
        for (size_t j = 0; j < nv; ++j) if (pack_text(j, pipename)) return 1;
    }
    // the tables (sqy::encode_batch_layout): what the host uploads -- the volumes and the header text in a copy of their own behind round
    // trip 1 when the text is known only then --, and behind it what the kernels hand each other
    const sqy::EncodeBatchLayout L = sqy::encode_batch_layout(nc, nv, quantised, quantised ? nv * sqy::kBatchHeaderTextMax : text_bytes);
    if (ws->batch_tables.ensure(L.tables) || ws->batch_scratch.ensure(std::max<uint64_t>(nc * g.scratch_stride, 16))) return 1;
    if (pk && ws->batch_places.ensure(2 * nv * sizeof(uint64_t))) return 1;
    uint64_t* const d_place = pk ? static_cast<uint64_t*>(ws->batch_places.p) : nullptr;
    uint64_t* const d_gap = pk && std::any_of(pk->gaps, pk->gaps + nv, [](uint64_t x) { return x != 0; }) ? d_place + nv : nullptr;   // (no gap: no upload)
    // the views of the group that are no dense allocations: the packed copies' places in Workspace::batch_pack (16-byte aligned)
    auto read_of = [&](uint32_t vol) { return how ? (ViewRead)(*how)[vol] : in_place; };
    std::vector<uint64_t> place(nv, 0);
    uint64_t pack_bytes = 0;
    bool to_stream = false;
    for (size_t j = 0; j < nv; ++j) {
        if (read_of(g.vols[j]) == packed) { place[j] = pack_bytes; pack_bytes += (a.len[g.vols[j]] * (uint64_t)elem_size + 15) & ~(uint64_t)15; }
        to_stream = to_stream || read_of(g.vols[j]) == packed_to_stream;
    }
    if (pack_bytes && ws->batch_pack.ensure(pack_bytes)) return 1;
    if ((transpose || to_stream) && ws->batch_stream.ensure(std::max<uint64_t>(g.stream_bytes, 16))) return 1;
    if (quantised && ws->batch_quant.ensure(nv * sqy::kQuantiserBatchTableBytes)) return 1;
    uint8_t* const d_tab = static_cast<uint8_t*>(ws->batch_tables.p);
    uint8_t* const d_stream = transpose ? static_cast<uint8_t*>(ws->batch_stream.p) : nullptr;
    ViewLaunch packs, gathers;
    PatchLaunch patches;

    sqy::Lz4BatchChunk* h_table = reinterpret_cast<sqy::Lz4BatchChunk*>(staging + L.table_at);
    uint32_t* h_volof = reinterpret_cast<uint32_t*>(staging + L.volof_at);
    sqy::Lz4BatchVolume* h_vols = reinterpret_cast<sqy::Lz4BatchVolume*>(staging + L.vols_at);
    sqy::Bitswap1Job* h_jobs = reinterpret_cast<sqy::Bitswap1Job*>(staging + L.jobs_at);
    uint32_t* h_tiles = reinterpret_cast<uint32_t*>(staging + L.tiles_at);
    char* h_text = reinterpret_cast<char*>(staging + L.text_at);
    uint64_t text_used = 0;
    uint32_t ntiles = 0;
    // the volume table and the header text, once every volume's text is there
    auto fill_volumes = [&]() {
        for (size_t j = 0; j < nv; ++j) {
            const uint32_t vol = g.vols[j];
            const size_t cut = text[j].find('\0');
            const uint32_t prefix_len = (uint32_t)cut, suffix_len = (uint32_t)(text[j].size() - cut - 1);
            std::memcpy(h_text + text_used, text[j].data(), prefix_len);
            std::memcpy(h_text + text_used + prefix_len, text[j].data() + cut + 1, suffix_len);
            // (packed: the place comes from the placement scan, which also holds the blob against the capacity)
            h_vols[j] = sqy::Lz4BatchVolume{pk ? 0 : (uint64_t)vol * slot_capacity, pk ? ~(uint64_t)0 : slot_capacity, g.first_chunk[j], g.first_chunk[j + 1] - g.first_chunk[j],
                                            (uint32_t)text_used, prefix_len, suffix_len, (uint32_t)elem_size, vol, 0};
            text_used += prefix_len + suffix_len;
        }
    };
    if (!quantised) fill_volumes();
    size_t njobs = 0;                                                   // the jobs of the dense transposer: every volume but the gathered views
    for (size_t j = 0; j < nv; ++j) {
        const uint32_t vol = g.vols[j];
        const ViewRead read = read_of(vol);
        // where the volume's voxels are dense: its own allocation, its packed copy -- or (plain lz4, packed_to_stream) its stream
        const void* src = d_srcs[vol];
        if (read == packed) {
            src = static_cast<uint8_t*>(ws->batch_pack.p) + place[j];
            packs.add(d_srcs[vol], src, (*views)[vol]);
        } else if (read == packed_to_stream) {
            src = static_cast<uint8_t*>(ws->batch_stream.p) + g.stream_at[j];
            packs.add(d_srcs[vol], src, (*views)[vol]);
        }
        if (read == gathered)
            gathers.add(d_srcs[vol], d_stream + g.stream_at[j], (*views)[vol]);
        else if (read == patched)
            patches.add(up->views[vol], d_srcs[vol], d_stream + g.stream_at[j], (*up->wins)[vol], (*up->wviews)[vol]);
        else {
            h_jobs[njobs] = sqy::Bitswap1Job{src, d_stream ? d_stream + g.stream_at[j] : nullptr, a.len[vol]};
            h_tiles[njobs++] = ntiles;
            ntiles += sqy::batch_bitswap1_tiles(a.len[vol]);
        }
        for (uint32_t e = g.first_chunk[j]; e < g.first_chunk[j + 1]; ++e) {
            const sqy::Lz4BatchChunkPlan& c = g.chunks[e];
            // (plain lz4: the stream IS the volume -- the entry's offset counts from address 0)
            const uint64_t off = transpose ? c.off : (uint64_t)reinterpret_cast<uintptr_t>(src) + (c.off - g.stream_at[j]);
            h_table[e] = sqy::Lz4BatchChunk{off, c.n, c.vol, c.slot, 0};
            h_volof[e] = (uint32_t)j;
        }
    }
    h_tiles[njobs] = ntiles;
    SQY_HIP(hipMemcpyAsync(d_tab, staging, quantised ? L.vols_at : L.upload, hipMemcpyHostToDevice, stream));
    if (d_gap) SQY_HIP(hipMemcpyAsync(d_gap, pk->gaps, nv * sizeof(uint64_t), hipMemcpyHostToDevice, stream));

    const sqy::Lz4BatchChunk* d_table = reinterpret_cast<const sqy::Lz4BatchChunk*>(d_tab + L.table_at);
    const sqy::Lz4BatchVolume* d_vols = reinterpret_cast<const sqy::Lz4BatchVolume*>(d_tab + L.vols_at);
    uint32_t* d_csize = reinterpret_cast<uint32_t*>(d_tab + L.csize_at);
    uint32_t* d_redo = reinterpret_cast<uint32_t*>(d_tab + L.redo_at);
    uint64_t* d_foff = reinterpret_cast<uint64_t*>(d_tab + L.foff_at);
    uint64_t* d_vinfo = reinterpret_cast<uint64_t*>(d_tab + L.vinfo_at);
    uint8_t* d_scratch = static_cast<uint8_t*>(ws->batch_scratch.p);
    const sqy::Bitswap1Job* d_jobs = reinterpret_cast<const sqy::Bitswap1Job*>(d_tab + L.jobs_at);
    const uint32_t* d_tiles = reinterpret_cast<const uint32_t*>(d_tab + L.tiles_at);
    // (quantised) the group's histograms | encode LUTs | decode LUTs, volume j's at index j of each
    uint32_t* const d_histos = static_cast<uint32_t*>(ws->batch_quant.p);
    uint8_t* const d_luts = quantised ? static_cast<uint8_t*>(ws->batch_quant.p) + nv * sqy::kQuantiserBatchHistoBytes : nullptr;
    uint16_t* const d_decode = quantised ? reinterpret_cast<uint16_t*>(d_luts + nv * sqy::kQuantiserBatchLutBytes) : nullptr;
    uint16_t* const h_decode = reinterpret_cast<uint16_t*>(staging + L.decode_at);     // (pinned, behind the staging area of the upload)
    if (launch_views(cx, stream, packs, ViewLaunch::pack, 0, elem_size)) return 1;
    if (quantised) {
        SQY_TIMED("batch_quantiser_histogram", sqy::launch_batch_quantiser_histogram(d_jobs, d_tiles, (uint32_t)nv, ntiles, d_histos, stream));
        SQY_TIMED("batch_quantiser_lut", sqy::launch_batch_quantiser_lut(d_histos, (uint32_t)nv, d_luts, d_decode, stream));
        SQY_TIMED("batch_quantiser_bitswap1", sqy::launch_batch_quantiser_bitswap1(d_jobs, d_tiles, (uint32_t)nv, ntiles, d_luts, stream));
    } else if (transpose) {
        if (njobs) SQY_TIMED("batch_bitswap1", sqy::launch_bitswap1_batch(d_jobs, d_tiles, (uint32_t)njobs, ntiles, elem_size, stream));
        if (launch_views(cx, stream, gathers, ViewLaunch::bitswap1, 1, elem_size) || launch_patches(cx, stream, patches, elem_size)) return 1;
    }
    SQY_TIMED("batch_lz4_chunks", sqy::launch_lz4_chunks_table(d_stream, d_table, (uint32_t)nc, d_scratch, g.scratch_stride, d_csize, d_redo, stream));
    // round trip 1: how many entries the first pass left to the dense batches -- and, quantised, the decode LUTs the headers carry
    if (quantised) SQY_HIP(hipMemcpyAsync(h_decode, d_decode, nv * sqy::kQuantiserBatchDecodeBytes, hipMemcpyDeviceToHost, stream));
    SQY_HIP(hipMemcpyAsync(ws->pinned, d_redo, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    const uint32_t n_redo = *static_cast<uint32_t*>(ws->pinned);
    if (quantised) {
        // every volume's own pipeline name (quantiser_scheme_impl.hpp:200-204: the decode LUT goes into the header), its header text, the upload
        Pipeline named = a.pipe;
        for (size_t j = 0; j < nv; ++j) {
            named.stages[0].cfg["decode_lut_string"] = sqy::to_verbatim(h_decode + j * 256, sqy::kQuantiserBatchDecodeBytes);
            if (pack_text(j, named.name())) return 1;
        }
        fill_volumes();
        SQY_HIP(hipMemcpyAsync(d_tab + L.vols_at, staging + L.vols_at, sqy::encode_batch_layout(nc, nv, quantised, text_bytes).upload - L.vols_at, hipMemcpyHostToDevice, stream));
    }
    if (n_redo)
        SQY_TIMED("batch_lz4_chunks_dense", sqy::launch_lz4_chunks_table_dense(d_stream, d_table, d_scratch, g.scratch_stride, d_csize, d_redo, n_redo, stream));
    SQY_TIMED("batch_lz4_frame_scan", sqy::launch_lz4_batch_scan(d_table, d_vols, (uint32_t)nv, d_csize, d_foff, d_vinfo, stream));
    if (pk) SQY_TIMED("batch_lz4_place", sqy::launch_lz4_batch_place(d_vinfo, d_gap, (uint32_t)nv, pk->align, pk->base, pk->capacity, d_place, stream));
    const Lz4Descriptor fd = lz4_descriptor(a.pipe.stages.back().lz4.block_id);
    SQY_TIMED("batch_lz4_frame_gather", sqy::launch_lz4_batch_gather(d_stream, d_table, (uint32_t)nc, g.max_chunk, d_vols,
                                                                     reinterpret_cast<const uint32_t*>(d_tab + L.volof_at), d_scratch, g.scratch_stride, d_csize,
                                                                     d_foff, d_vinfo, reinterpret_cast<const char*>(d_tab + L.text_at), d_dst, fd.bd, fd.hc, records, stream,
                                                                     d_place));
    // round trip 2: the records
    SQY_HIP(hipStreamSynchronize(stream));
    int rc = 0;
    for (size_t j = 0; j < nv; ++j) {
        const uint32_t vol = g.vols[j];
        const volatile uint64_t* r = records + 3 * (uint64_t)vol;
        if (pk && (r[0] == sqy::kBatchDone || r[0] == sqy::kBatchNoRoom)) {     // (no room: the call goes on, for the capacity a retry needs)
            pk->lens[vol] = r[1];
            pk->placed[vol] = r[0] == sqy::kBatchDone;
            continue;
        }
        if (r[0] == sqy::kBatchDone) { offsets[vol] = (long)((uint64_t)vol * slot_capacity); lengths[vol] = (long)r[1]; continue; }
        if (r[0] == sqy::kBatchNoRoom)
            std::fprintf(stderr, "[sqeazy]\t volume %u: destination slot too small (%llu payload bytes and the header > %llu bytes)\n", vol,
                         (unsigned long long)r[2], (unsigned long long)slot_capacity);
        else if (r[0] == sqy::kBatchPayloadTooLong)
            std::fprintf(stderr, "[sqeazy]\t lz4: %llu payload bytes overflow the reference's int byte count\n", (unsigned long long)r[2]);
        else
            std::fprintf(stderr, "[sqeazy]\t internal error: volume %u of the batch was not finished (status %llu)\n", vol, (unsigned long long)r[0]);
        rc = 1;
    }
    return rc;
}

// the groups of a batch under the options in force (pack_bytes: lz4_batch_plan_views'; empty: none)
sqy::Lz4BatchPlan encode_batch_plan(const BatchAdmit& a, sqy::EncodeBatchForm form, int elem_size, const std::vector<uint64_t>& pack_bytes)
{
    std::vector<uint64_t> totals(a.len.size());
    for (size_t i = 0; i < a.len.size(); ++i) totals[i] = sqy::encode_batch_stream_bytes(form, a.len[i], elem_size);
    return sqy::lz4_batch_plan_views(a.pipe.stages.back().lz4, totals, pack_bytes, a.pipe.nthreads, (uint64_t)g_opt.encode_batch_group_bytes.load(),
                                     (uint64_t)g_opt.encode_batch_joint_max_bytes.load(), sqy::encode_batch_extra_bytes(form));
}

// dense_to (SQYAMD_PipelineEncode_BatchPacked_*; nullptr: the slot layout): the blobs back to back in d_dst by sqy::packed_places' rule --
// slot_capacity is then the capacity of all of d_dst, and *total what the blobs take (or, rc 1 and the blobs do not fit, what they would take)
struct PackedArgs { uint64_t align; long* total; };
int encode_batch_on_device(Context& cx, const char* pipeline, const BatchAdmit& a, const void* const* d_srcs, const long* shapes, unsigned rank, int elem_size,
                           int nvolumes, void* d_dst, uint64_t slot_capacity, long* offsets, long* lengths, int nthreads, hipStream_t stream,
                           const std::vector<sqy::BatchView>* views = nullptr, const PackedArgs* dense_to = nullptr, const UpdateEncode* up = nullptr)
{
    for (int i = 0; i < nvolumes; ++i)
        if (reinterpret_cast<uintptr_t>(d_srcs[i]) % (uintptr_t)elem_size) { std::fprintf(stderr, "[sqeazy]\t volume %d: source not aligned to the voxel size\n", i); return 1; }
    const sqy::EncodeBatchForm form = g_opt.encode_batch_joint.load() ? sqy::encode_batch_form(a.pipe, elem_size) : sqy::EncodeBatchForm::none;
    sqy::Lz4BatchPlan plan;
    plan.group_of.assign((size_t)nvolumes, -1);
    // the views that are no dense allocations: gathered by the transposer, packed into the stream (plain lz4), or packed into the
    // group's workspace -- whose bytes count against the group bound
    std::vector<uint8_t> how((size_t)nvolumes, in_place);
    std::vector<uint64_t> pack_bytes((size_t)nvolumes, 0);
    bool strided = false;
    if (views) {
        const bool fused = g_opt.batch_strided_fused.load() != 0;
        for (size_t i = 0; i < (size_t)nvolumes; ++i) {
            if ((*views)[i].dense) continue;
            strided = true;
            how[i] = fused && form == sqy::EncodeBatchForm::bitswap1_lz4 ? gathered : fused && form == sqy::EncodeBatchForm::lz4 ? packed_to_stream : packed;
            if (how[i] == packed) pack_bytes[i] = (a.len[i] * (uint64_t)elem_size + 15) & ~(uint64_t)15;
        }
    }
    if (up)
        for (size_t i = 0; i < (size_t)nvolumes; ++i)
            if ((*up->is_patched)[i]) { how[i] = patched; strided = true; }
    if (form != sqy::EncodeBatchForm::none) plan = encode_batch_plan(a, form, elem_size, strided ? pack_bytes : std::vector<uint64_t>());
    for (size_t i = 0; i < (size_t)nvolumes; ++i)
        if (how[i] == patched && (form != sqy::EncodeBatchForm::bitswap1_lz4 || plan.group_of[i] < 0)) {
            std::fprintf(stderr, "[sqeazy]\t internal error: volume %zu kept its planes and has no group to patch them\n", i);
            return 1;
        }
    const size_t n = (size_t)nvolumes;
    int rc = 0;
    // the packed layout's state: every blob's length, whether a group wrote it, and for a volume outside the joint forms where its blob
    // waits in Workspace::batch_packed
    std::vector<uint64_t> lens, waits_at;
    std::vector<uint8_t> placed;
    uint64_t* gaps = nullptr;                                           // (pinned, behind the staging area: the group at hand's)
    // the groups, in order; the packed layout hands each where it begins and what lies between its members
    auto run_groups = [&]() -> int {
        if (plan.groups.empty()) return 0;
        DrainOnExit drain{stream, &cx.pending};
        // pinned: a record per volume of the batch (3 words), behind them the staging area of the group that needs the largest one
        const bool quantised = form == sqy::EncodeBatchForm::quantiser_bitswap1_lz4;
        uint64_t staging = 0, most_vols = 0;
        for (const sqy::Lz4BatchGroup& g : plan.groups) {
            staging = std::max(staging, sqy::encode_batch_layout(g.chunks.size(), g.vols.size(), quantised, g.vols.size() * sqy::kBatchHeaderTextMax).staging_bytes);
            most_vols = std::max<uint64_t>(most_vols, g.vols.size());
        }
        staging = (staging + 15) & ~(uint64_t)15;
        const uint64_t records_bytes = ((uint64_t)nvolumes * 24 + 63) & ~(uint64_t)63;
        if (cx.ws.batch_host.ensure(records_bytes + staging + (dense_to ? most_vols * sizeof(uint64_t) : 0))) return 1;
        uint64_t* records = static_cast<uint64_t*>(cx.ws.batch_host.p);
        std::memset(records, 0, records_bytes);
        gaps = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(cx.ws.batch_host.p) + records_bytes + staging);
        int grc = 0;
        for (const sqy::Lz4BatchGroup& g : plan.groups) {
            PackedGroup pk{};
            if (dense_to) {
                // every volume in front of the group is known by now: the others, and the groups before it (the plan deals volumes in order)
                const uint32_t v0 = g.vols[0];
                const sqy::PackedPlaces before = sqy::packed_places(std::vector<uint64_t>(lens.begin(), lens.begin() + v0), std::vector<uint64_t>(), dense_to->align, 0, slot_capacity);
                if (!before.ok) return 1;
                pk = PackedGroup{dense_to->align, v0 ? align_up(before.end, dense_to->align) : 0, slot_capacity, gaps, lens.data(), placed.data()};
                for (size_t j = 0; j < g.vols.size(); ++j) {
                    gaps[j] = 0;
                    for (uint32_t k = j ? g.vols[j - 1] + 1 : v0; k < g.vols[j]; ++k) gaps[j] += align_up(lens[k], dense_to->align);
                }
            }
            if (encode_batch_group(cx, a, g, form, elem_size, d_srcs, static_cast<uint8_t*>(d_dst), slot_capacity, offsets, lengths, records,
                                   static_cast<uint8_t*>(cx.ws.batch_host.p) + records_bytes, stream, strided ? views : nullptr, strided ? &how : nullptr,
                                   dense_to ? &pk : nullptr, up)) {
                grc = 1;
                if (dense_to) break;                                      // (the groups behind it would not know where they begin)
            }
        }
        if (g_prof_on.load()) prof_collect(cx.pending);
        return grc;
    };
    // every other volume: the single-call path into `cap` bytes at dst (the blob where the call leaves it: *at, *len)
    auto run_single = [&](int i, uint8_t* dst, uint64_t cap, long* at, long* len) -> int {
        const void* src = d_srcs[i];
        if (how[(size_t)i] != in_place) {                               // a view outside the joint forms: from its packed copy
            if (cx.ws.batch_pack.ensure(a.len[(size_t)i] * (uint64_t)elem_size)) return 1;
            src = cx.ws.batch_pack.p;
            ViewLaunch one;
            one.add(d_srcs[i], src, (*views)[(size_t)i]);
            DrainOnExit drain{stream, &cx.pending};                     // (the launch's tables are this scope's)
            if (launch_views(cx, stream, one, ViewLaunch::pack, 0, elem_size)) return 1;
        }
        return encode_on_device(cx, pipeline, src, shapes + (size_t)i * rank, rank, elem_size, dst, cap, len, nthreads, stream, at);
    };
    if (!dense_to) {
        rc = run_groups();
        // .. into its slot, in volume order
        for (int i = 0; i < nvolumes && rc == 0; ++i) {
            if (plan.group_of[(size_t)i] >= 0) continue;
            long at = 0, len = 0;
            rc = run_single(i, static_cast<uint8_t*>(d_dst) + (uint64_t)i * slot_capacity, slot_capacity, &at, &len);
            if (rc == 0) { offsets[i] = (long)((uint64_t)i * slot_capacity) + at; lengths[i] = len; }
        }
        if (rc) for (int i = 0; i < nvolumes; ++i) { offsets[i] = 0; lengths[i] = 0; }
        return rc;
    }
    // The packed layout.  A volume outside the joint forms uses its whole slot and leaves the blob anywhere in it, so these go first, each
    // into a workspace slot of its own: the host then knows their sizes, the groups get them as gaps, and the blobs are copied to their
    // places at the end.  (offsets, lengths and *total are zero here: admit_batch_packed)
    lens.assign(n, 0);
    waits_at.assign(n, 0);
    placed.assign(n, 0);
    uint64_t waiting = 0;
    std::vector<uint64_t> slot_at(n, 0), slot_cap(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (plan.group_of[i] >= 0) continue;
        slot_at[i] = waiting;
        slot_cap[i] = a.pipe.max_encoded_size(a.len[i] * (uint64_t)elem_size, elem_size);
        waiting += align_up(slot_cap[i], 256);
    }
    if (waiting && cx.ws.batch_packed.ensure(waiting)) return 1;
    for (int i = 0; i < nvolumes; ++i) {
        if (plan.group_of[(size_t)i] >= 0) continue;
        long at = 0, len = 0;
        if (run_single(i, static_cast<uint8_t*>(cx.ws.batch_packed.p) + slot_at[(size_t)i], slot_cap[(size_t)i], &at, &len)) return 1;
        waits_at[(size_t)i] = slot_at[(size_t)i] + (uint64_t)at;
        lens[(size_t)i] = (uint64_t)len;
    }
    if (run_groups()) return 1;
    const sqy::PackedPlaces places = sqy::packed_places(lens, std::vector<uint64_t>(), dense_to->align, 0, slot_capacity);
    if (!places.ok) { std::fprintf(stderr, "[sqeazy]\t encode batch: the packed blobs pass 2^63 bytes\n"); return 1; }
    if (places.first_unfit < n) {
        std::fprintf(stderr, "[sqeazy]\t encode batch: the packed blobs take %llu bytes, the destination holds %llu (volume %zu is the first that does not fit)\n",
                     (unsigned long long)places.end, (unsigned long long)slot_capacity, places.first_unfit);
        *dense_to->total = (long)places.end;
        return 1;
    }
    for (size_t i = 0; i < n; ++i)
        if (plan.group_of[i] >= 0 && !placed[i]) { std::fprintf(stderr, "[sqeazy]\t internal error: volume %zu of the batch was not placed\n", i); return 1; }
    for (size_t i = 0; i < n; ++i)
        if (plan.group_of[i] < 0)
            SQY_HIP(hipMemcpyAsync(static_cast<uint8_t*>(d_dst) + places.at[i], static_cast<uint8_t*>(cx.ws.batch_packed.p) + waits_at[i], lens[i], hipMemcpyDeviceToDevice, stream));
    if (waiting) SQY_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < n; ++i) { offsets[i] = (long)places.at[i]; lengths[i] = (long)lens[i]; }
    *dense_to->total = (long)places.end;
    return 0;
}

int encode_batch_device(const char* pipeline, const void* const* d_srcs, const long* shapes, unsigned rank, int elem_size, int nvolumes, void* d_dst,
                        long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    BatchAdmit a;
    if (admit_batch(pipeline, d_srcs, shapes, rank, elem_size, nvolumes, d_dst, slot_capacity, offsets, lengths, nthreads, &a)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return encode_batch_on_device(*lease.ctx, pipeline, a, d_srcs, shapes, rank, elem_size, nvolumes, d_dst, (uint64_t)slot_capacity, offsets, lengths, nthreads,
                                  static_cast<hipStream_t>(hip_stream));
}

// SQYAMD_PipelineEncode_BatchStrided_*: the Batch call's checks, then every view on the host; strides == nullptr: the Batch call
int encode_batch_strided_device(const char* pipeline, const void* const* d_srcs, const long* shapes, const long* strides, unsigned rank, int elem_size, int nvolumes,
                                void* d_dst, long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    BatchAdmit a;
    if (admit_batch(pipeline, d_srcs, shapes, rank, elem_size, nvolumes, d_dst, slot_capacity, offsets, lengths, nthreads, &a)) return 1;
    std::vector<sqy::BatchView> views;
    if (admit_views("encode batch", d_srcs, shapes, strides, rank, nvolumes, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return encode_batch_on_device(*lease.ctx, pipeline, a, d_srcs, shapes, rank, elem_size, nvolumes, d_dst, (uint64_t)slot_capacity, offsets, lengths, nthreads,
                                  static_cast<hipStream_t>(hip_stream), strides ? &views : nullptr);
}

// ---- window update (SQYAMD_Update_BatchWindow_*) ------------------------------------------------------------------------------
// New blob i = the single call's blob for (old blob i decoded, its window's voxels replaced by view i's), into slot i.  The batch decode
// driver puts every old blob into its place of Workspace::batch_update (sqy::update_batch_plan), ONE paste launch writes the windows into
// the places that hold voxels, the batch encode driver reads the places as its sources.  The places that hold planes (layer two,
// sqy::update_blob_patched) are read by the encode groups' patch launches together with the views.  Nothing is written to d_dst before
// every old blob has been decoded: a damaged one leaves it untouched.
int update_batch_on_device(Context& cx, const char* pipeline, BatchAdmit& a, const void* d_src, const long* src_offsets, const long* src_lengths, int nblobs,
                           const long* origins, const void* const* d_wins, const long* win_shapes, const long* win_strides, unsigned rank, int elem_size, void* d_dst,
                           uint64_t slot_capacity, long* offsets, long* lengths, int nthreads, hipStream_t stream)
{
    const size_t n = (size_t)nblobs;
    std::vector<SlabBlob> blobs(n);
    for (size_t i = 0; i < n; ++i) {
        blobs[i].src = static_cast<const uint8_t*>(d_src) + src_offsets[i];
        blobs[i].len = (uint64_t)src_lengths[i];
    }
    // 1. the headers: the voxel type, the window inside the shape, the shape under the new pipeline -- before anything is written
    std::vector<sqy::BatchWindow> wins(n);
    std::vector<long> shapes(n * rank);
    a.dims.resize(n);
    a.len.resize(n);
    {
        DrainOnExit drain{stream, &cx.pending, cx.side};
        if (fetch_blob_headers(cx, blobs, elem_size, stream, "update batch", [&](int i) {
                if (!sqy::admit_window(blobs[i].h.shape, origins ? origins + (size_t)i * rank : nullptr, win_shapes + (size_t)i * rank, rank, &wins[(size_t)i])) {
                    std::fprintf(stderr, "[sqeazy]\t update batch: blob %d's window does not lie inside its shape\n", i);
                    return false;
                }
                for (unsigned k = 0; k < rank; ++k) shapes[(size_t)i * rank + k] = (long)blobs[i].h.shape[k];
                return admit_shape(&a.pipe, shapes.data() + (size_t)i * rank, rank, &a.dims[(size_t)i], &a.len[(size_t)i]) == 0;
            }))
            return 1;
    }
    // 2. the plan (host-only, sqy_pipeline.cpp): which blobs keep their planes, every blob's place
    const bool fused_on = g_opt.batch_update_fused.load() != 0 && g_opt.decode_batch_joint.load() != 0 && g_opt.encode_batch_joint.load() != 0;
    const sqy::EncodeBatchForm form = g_opt.encode_batch_joint.load() ? sqy::encode_batch_form(a.pipe, elem_size) : sqy::EncodeBatchForm::none;
    std::vector<int32_t> group_of(n, -1);
    if (form != sqy::EncodeBatchForm::none) group_of = encode_batch_plan(a, form, elem_size, std::vector<uint64_t>()).group_of;
    std::vector<uint64_t> raw(n);
    for (size_t i = 0; i < n; ++i) raw[i] = blobs[i].raw;
    const sqy::UpdateBatchPlan plan = sqy::update_batch_plan(raw, form, group_of, fused_on);
    if (cx.ws.batch_update.ensure(std::max<uint64_t>(plan.bytes, 16))) return 1;
    std::vector<void*> places(n);
    std::vector<long> caps(n);
    for (size_t i = 0; i < n; ++i) { places[i] = static_cast<uint8_t*>(cx.ws.batch_update.p) + plan.place_at[i]; caps[i] = (long)raw[i]; }
    // 3. the old blobs, through the batch decode driver
    UpdateDecode ud{&plan.keep_planes, std::vector<uint8_t>(n, 0), &blobs, fused_on, static_cast<uint8_t*>(cx.ws.batch_update.p), &plan.place_at, plan.bytes,
                    std::vector<uint8_t>(n, 0)};
    const BatchDecodeArgs d{src_offsets, src_lengths, nblobs, places.data(), caps.data(), nullptr};
    if (const int rc = decode_batch_on_device(cx, d_src, d, elem_size, stream, nullptr, nullptr, 0, nullptr, &ud)) return rc;
    // 4. the windows into the places that hold voxels: ONE launch
    std::vector<WindowView> wviews(n);
    WindowLaunch pastes;
    for (size_t i = 0; i < n; ++i) {
        wviews[i] = window_view(wins[i], win_strides ? win_strides + i * rank : nullptr, rank);
        if (!ud.patched[i]) pastes.add(d_wins[i], places[i], wins[i], wviews[i], false);
    }
    {
        DrainOnExit drain{stream, &cx.pending, cx.side};
        if (launch_windows(cx, stream, pastes, WindowLaunch::paste, elem_size)) return 1;
        pastes.wait();
    }
    // 5. the new blobs, through the batch encode driver
    const UpdateEncode ue{&ud.patched, d_wins, &wins, &wviews};
    return encode_batch_on_device(cx, pipeline, a, places.data(), shapes.data(), rank, elem_size, nblobs, d_dst, slot_capacity, offsets, lengths, nthreads, stream, nullptr,
                                  nullptr, &ue);
}

// what needs no header, before a device is looked for; then the driver
int update_batch_window_device(const char* pipeline, const void* d_src, const long* src_offsets, const long* src_lengths, int nblobs, const long* origins,
                               const void* const* d_wins, const long* win_shapes, const long* win_strides, unsigned rank, int elem_size, void* d_dst, long slot_capacity,
                               long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    if (!offsets || !lengths) return 1;
    for (int i = 0; i < nblobs; ++i) { offsets[i] = 0; lengths[i] = 0; }
    if (!pipeline || !d_src || !src_offsets || !src_lengths || !d_wins || !win_shapes || !d_dst || nblobs <= 0 || slot_capacity <= 0) {
        std::fprintf(stderr, "[sqeazy]\t update batch: bad arguments\n");
        return 1;
    }
    BatchAdmit a;
    if (admit_pipeline(pipeline, elem_size, nthreads, &a.pipe)) return 1;
    for (int i = 0; i < nblobs; ++i)
        if (!blob_entry_ok("update batch", i, src_offsets[i], src_lengths[i], d_wins[i] != nullptr)) return 1;
    std::vector<sqy::BatchView> views;
    if (admit_views("update batch", d_wins, win_shapes, win_strides, rank, nblobs, elem_size, &views)) return 1;
    for (size_t k = 0; origins && k < (size_t)nblobs * rank; ++k)
        if (origins[k] < 0) { std::fprintf(stderr, "[sqeazy]\t update batch: window %zu begins in front of its blob\n", k / rank); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return update_batch_on_device(*lease.ctx, pipeline, a, d_src, src_offsets, src_lengths, nblobs, origins, d_wins, win_shapes, win_strides, rank, elem_size, d_dst,
                                  (uint64_t)slot_capacity, offsets, lengths, nthreads, static_cast<hipStream_t>(hip_stream));
}

// ---- a box written into one large blob (SQYAMD_Update_Box_*) --------------------------------------------------------------------
// New blob = the single call's blob for (old blob decoded, the box's voxels replaced by the view's).  sqy::update_box_path says what runs.
// subset_patch: the LZ4 frames the box's z-range needs are decoded into the workspace (DecodeCall::frames_subset, as for
// SQYAMD_Decode_Box_*), the box is patched into that compaction where it lies, its chunks are parsed again by the batch encode's parse,
// and two launches splice the new frames between the old ones, which are copied from the old blob as they stand.  whole: the blob decoded
// into Workspace::range_full, one paste launch, the single call's encode.  Nothing is written to d_dst before the old frames that are
// needed have been decoded and found sound.
struct UpdateBoxCall {
    Context& cx;
    hipStream_t stream;
    const char* pipeline_text;
    const Pipeline& pipe;                    // `pipeline`, parsed, its thread count set
    const uint8_t* d_src;
    uint64_t srclen;
    const sqy::HeaderInfo& h;
    uint64_t raw_bytes;
    const sqy::BatchWindow& w;
    const WindowView& v;
    uint64_t z0, nz;                         // the box's range along the header's first dimension
    unsigned rank;
    const void* d_view;
    int elem;
    void* d_dst;
    uint64_t capacity;
    long* dstlength;
    int nthreads;
};

// the tables of the subset path's parse and splice in Workspace::batch_tables, 16-byte aligned each.  What the host writes: table_at: an
// Lz4BatchChunk per selected chunk | slot_at: a word per frame of the blob | text_at: the header's prefix and suffix -- `upload` bytes.
// Behind them what the kernels hand each other: csize_at, redo_at (nsel + 1 words), foff_at (nframes + 1 offsets), info_at (2 words)
struct SpliceTables {
    uint64_t table_at = 0, slot_at = 0, text_at = 0, upload = 0, csize_at = 0, redo_at = 0, foff_at = 0, info_at = 0, total = 0;
    std::vector<unsigned char> host;
    hipStream_t queued_on = nullptr;
    bool queued = false;
    SpliceTables(uint64_t nsel, uint64_t nframes, uint64_t text_bytes)
    {
        auto up = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
        slot_at = up(nsel * sizeof(sqy::Lz4BatchChunk));
        text_at = slot_at + up(nframes * 4);
        upload = csize_at = text_at + up(text_bytes);
        redo_at = csize_at + up(nsel * 4);
        foff_at = redo_at + up((nsel + 1) * 4);
        info_at = foff_at + up((nframes + 1) * 8);
        total = info_at + 16;
        host.assign(upload, 0);
    }
    SpliceTables(const SpliceTables&) = delete;
    SpliceTables& operator=(const SpliceTables&) = delete;
    ~SpliceTables() { if (queued) (void)hipStreamSynchronize(queued_on); }
};

// subset path, stage 2: the box into the compaction at c.range_buf, in place
int update_box_patch(DecodeCall& c, const UpdateBoxCall& u, WindowLaunch& l)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangePlan& p = c.range_plan;
    if (c.range_form == sqy::RangeForm::planes) {
        sqy::Bitswap1Range r;
        const uint16_t* lut = nullptr;
        if (c.range_planes(&r, &lut)) return 1;
        const sqy::BatchWindowJob box{const_cast<void*>(u.d_view), nullptr, u.w.Z, u.w.Y, u.w.X, u.v.sz, u.v.sy, u.w.bZ, u.w.bY, u.w.bX, u.w.oz, u.w.oy, u.w.ox, 0};
        if (!sqy::bitswap1_range_patch_ok(r, box, p.we)) { std::fprintf(stderr, "[sqeazy]\t internal error: the frame range does not hold the box\n"); return 1; }
        SQY_TIMED("bitswap1_range_patch", sqy::launch_bitswap1_range_patch(c.range_buf, r, box, p.we, stream));
        return 0;
    }
    // plain: the range in the workspace is a blob of the box's frames, the box begins at its first one (box_range_out's rule)
    l.add(u.d_view, c.range_buf + p.range_at, sqy::window_in_own_frames(u.w, u.rank), u.v, false);
    const uint32_t* d_tiles = nullptr;
    if (l.upload(stream, c.cx.ws.box_window, &d_tiles)) return 1;
    SQY_TIMED("box_window_paste", sqy::launch_batch_window_paste(static_cast<const sqy::BatchWindowJob*>(c.cx.ws.box_window.p), d_tiles, 1, l.ntiles, u.elem, stream));
    return 0;
}

// subset path, stage 3: the selected chunks parsed again (the batch encode's parse over a table of them); the host round trip between
// its two passes brings the LZ4 decoder's verdict on the old frames with it -- a damaged one ends the call here, d_dst untouched
int update_box_parse(DecodeCall& c, SpliceTables& T, uint64_t chunk, uint64_t stride)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    Workspace* ws = c.ws;
    const sqy::FrameRangePlan& p = c.range_plan;
    const uint32_t nsel = (uint32_t)p.ids.size();
    const uint64_t total = c.in_bytes(c.pipe.stages.size() - 1);
    sqy::Lz4BatchChunk* h_table = reinterpret_cast<sqy::Lz4BatchChunk*>(T.host.data() + T.table_at);
    for (uint32_t k = 0; k < nsel; ++k) {
        const uint64_t f = p.ids[k];
        h_table[k] = sqy::Lz4BatchChunk{p.coff[f], (uint32_t)std::min<uint64_t>(chunk, total - f * chunk), 0, k, 0};
    }
    if (ws->batch_tables.ensure(T.total) || ws->batch_scratch.ensure(std::max<uint64_t>((uint64_t)nsel * stride, 16))) return 1;
    uint8_t* d_tab = static_cast<uint8_t*>(ws->batch_tables.p);
    T.queued_on = stream;
    T.queued = true;
    SQY_HIP(hipMemcpyAsync(d_tab, T.host.data(), T.upload, hipMemcpyHostToDevice, stream));
    const sqy::Lz4BatchChunk* d_table = reinterpret_cast<const sqy::Lz4BatchChunk*>(d_tab + T.table_at);
    uint32_t* d_csize = reinterpret_cast<uint32_t*>(d_tab + T.csize_at);
    uint32_t* d_redo = reinterpret_cast<uint32_t*>(d_tab + T.redo_at);
    uint8_t* d_scratch = static_cast<uint8_t*>(ws->batch_scratch.p);
    SQY_TIMED("lz4_chunks_table", sqy::launch_lz4_chunks_table(c.range_buf, d_table, nsel, d_scratch, stride, d_csize, d_redo, stream));
    uint32_t* h_redo = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ws->pinned) + 16);
    SQY_HIP(hipMemcpyAsync(h_redo, d_redo, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (const int rc = c.finish()) return rc;                           // (synchronises; the verdict)
    const uint32_t n_redo = *h_redo;
    if (n_redo) SQY_TIMED("lz4_chunks_table_dense", sqy::launch_lz4_chunks_table_dense(c.range_buf, d_table, d_scratch, stride, d_csize, d_redo, n_redo, stream));
    return 0;
}

// subset path, stages 4 and 5: the splice into d_dst, and the one read-back of its record
int update_box_splice(DecodeCall& c, const UpdateBoxCall& u, const SpliceTables& T, const sqy::Lz4SpliceJob& job, uint64_t stride)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    Workspace* ws = c.ws;
    uint8_t* d_tab = static_cast<uint8_t*>(ws->batch_tables.p);
    uint64_t* d_foff = reinterpret_cast<uint64_t*>(d_tab + T.foff_at);
    uint64_t* d_info = reinterpret_cast<uint64_t*>(d_tab + T.info_at);
    volatile uint64_t* record = reinterpret_cast<volatile uint64_t*>(static_cast<uint8_t*>(ws->pinned) + 64);
    record[0] = 0; record[1] = 0; record[2] = 0;
    const Lz4Descriptor fd = lz4_descriptor(u.pipe.stages.back().lz4.block_id);
    SQY_TIMED("lz4_splice_scan", sqy::launch_lz4_splice_scan(job, u.capacity, d_foff, d_info, stream));
    SQY_TIMED("lz4_splice_gather", sqy::launch_lz4_splice_gather(job, c.cur, c.range_buf, static_cast<const uint8_t*>(ws->batch_scratch.p), stride, d_foff, d_info,
                                                                 reinterpret_cast<const char*>(d_tab + T.text_at), static_cast<uint8_t*>(u.d_dst), fd.bd, fd.hc,
                                                                 const_cast<uint64_t*>(record), stream));
    SQY_HIP(hipStreamSynchronize(stream));
    if (g_prof_on.load()) prof_collect(*pend);
    if (record[0] == sqy::kSpliceDone) { *u.dstlength = (long)record[1]; return 0; }
    if (record[0] == sqy::kSpliceNoRoom) {
        std::fprintf(stderr, "[sqeazy]\t update box: destination buffer too small (%llu > %llu bytes)\n", (unsigned long long)record[1], (unsigned long long)u.capacity);
        *u.dstlength = (long)record[1];
    } else if (record[0] == sqy::kSplicePayloadTooLong)
        std::fprintf(stderr, "[sqeazy]\t lz4: %llu payload bytes overflow the reference's int byte count\n", (unsigned long long)record[2]);
    else
        std::fprintf(stderr, "[sqeazy]\t update box: the old blob's frame index does not fit its payload (status %llu)\n", (unsigned long long)record[0]);
    return 1;
}

// every other blob: whole decode, one paste, the single call's encode -- into the workspace first, so that a blob that does not fit leaves
// d_dst untouched and its exact length known
// (boxes: SQYAMD_Update_Boxes_*' table, pasted layer by layer; nullptr: the one box of u)
struct UpdateBoxesTable;
int update_boxes_whole_paste(const UpdateBoxCall& u, const UpdateBoxesTable& t);
int update_box_whole(const UpdateBoxCall& u, const UpdateBoxesTable* boxes = nullptr)
{
    Context& cx = u.cx;
    hipStream_t stream = u.stream;
    if (cx.ws.range_full.ensure(std::max<uint64_t>(u.raw_bytes, 16))) return 1;
    if (const int rc = decode_on_device(cx, u.d_src, u.srclen, cx.ws.range_full.p, u.raw_bytes, u.elem, stream)) return rc;
    if (boxes) {
        if (const int rc = update_boxes_whole_paste(u, *boxes)) return rc;
    } else {
        DrainOnExit drain{stream, &cx.pending, cx.side};
        WindowLaunch paste;
        paste.add(u.d_view, cx.ws.range_full.p, u.w, u.v, false);
        if (launch_windows(cx, stream, paste, WindowLaunch::paste, u.elem)) return 1;
        paste.wait();
    }
    Pipeline fresh = Pipeline::from_string(u.pipeline_text, u.elem);
    const uint64_t bound = std::max(fresh.max_encoded_size(u.raw_bytes, u.elem), u.pipe.max_encoded_size(u.raw_bytes, u.elem));
    if (cx.ws.update_box.ensure(std::max<uint64_t>(bound, 16))) return 1;
    std::vector<long> shape(u.h.shape.begin(), u.h.shape.end());
    long len = 0, at = 0;
    if (const int rc = encode_on_device(cx, u.pipeline_text, cx.ws.range_full.p, shape.data(), u.rank, u.elem, cx.ws.update_box.p, bound, &len, u.nthreads, stream, &at)) return rc;
    if ((uint64_t)len > u.capacity) {
        std::fprintf(stderr, "[sqeazy]\t update box: destination buffer too small (%ld > %llu bytes)\n", len, (unsigned long long)u.capacity);
        *u.dstlength = len;
        return 1;
    }
    SQY_HIP(hipMemcpyAsync(u.d_dst, static_cast<const uint8_t*>(cx.ws.update_box.p) + at, (size_t)len, hipMemcpyDeviceToDevice, stream));
    SQY_HIP(hipStreamSynchronize(stream));
    *u.dstlength = len;
    return 0;
}

// the subset path where sqy::update_box_path allows it; *taken = false: nothing was written, the caller takes the whole path
// ranges: the frames to decode (the box's z-range; SQYAMD_Update_Boxes_*: its segments); patch: stage 2, the box or boxes into the
// compaction; option_on: the caller's option
int update_box_subset(const UpdateBoxCall& u, bool option_on, const std::vector<std::pair<uint64_t, uint64_t>>& ranges, const std::function<int(DecodeCall&)>& patch,
                      bool* taken)
{
    *taken = false;
    Context& cx = u.cx;
    hipStream_t stream = u.stream;
    const uint64_t n = u.raw_bytes / (uint64_t)u.elem;
    sqy::UpdateBoxFacts facts;
    facts.option_on = option_on;
    Pipeline held = Pipeline::from_string(u.h.pipename, u.elem);
    facts.same_stages = sqy::pipelines_same_stages(u.pipe, held);
    facts.form_ok = sqy::update_box_form_ok(u.pipe);
    if (!facts.option_on || !facts.same_stages || !facts.form_ok) return 0;
    facts.layout = sqy::lz4_encode_layout(u.pipe.stages.back().lz4, u.raw_bytes, u.pipe.nthreads);
    // (before the old blob is touched: what its index must show for the path to hold)
    facts.subset_taken = true; facts.frames = facts.blocks = facts.layout.nchunks; facts.frame_chunk = facts.layout.chunk;
    if (sqy::update_box_path(facts) != sqy::UpdateBoxPath::subset_patch) return 0;

    DrainOnExit drain{stream, &cx.pending, cx.side};
    DecodeCall c(cx, stream, nullptr, u.h, std::move(held), n, u.d_src + u.h.size);
    // 1. the frame index and the frames of the ranges, each a whole chunk of the compaction (range_plan: the first range's, and the
    // frames and offsets of all of them)
    bool subset = false;
    if (const int rc = c.frames_subset(ranges, false, &subset)) return rc;
    if (subset) c.range_plan = sqy::frame_range_plan_of(c.ranges_plan, 0);
    c.range_plan.direct = false;
    facts.subset_taken = subset && (c.range_form == sqy::RangeForm::plain || c.range_form == sqy::RangeForm::planes);
    facts.frames = c.range_ix.hc[0]; facts.blocks = c.range_ix.hc[1]; facts.frame_chunk = c.range_ix.chunk;
    if (sqy::update_box_path(facts) != sqy::UpdateBoxPath::subset_patch) return 0;      // (a subset decode already launched is drained; the whole path decides)
    const sqy::FrameRangePlan& p = c.range_plan;
    const uint64_t chunk = facts.layout.chunk, nframes = facts.frames, nsel = p.ids.size();
    const uint64_t stride = (chunk + 15) & ~(uint64_t)15;
    std::string prefix, suffix;
    sqy::header_pack_parts(u.elem, false, u.h.shape, u.pipe.name(), &prefix, &suffix);
    SpliceTables T(nsel, nframes, prefix.size() + suffix.size());
    std::vector<uint32_t> slot_of(nframes, sqy::kSpliceOldFrame);
    for (uint64_t k = 0; k < nsel; ++k) slot_of[p.ids[k]] = (uint32_t)k;
    if (nsel == 0 || chunk > 0x7fffffffull || !sqy::lz4_splice_ok(slot_of, nsel)) { std::fprintf(stderr, "[sqeazy]\t internal error: update box: no frame table\n"); return 1; }
    std::memcpy(T.host.data() + T.slot_at, slot_of.data(), nframes * 4);
    std::memcpy(T.host.data() + T.text_at, prefix.data(), prefix.size());
    std::memcpy(T.host.data() + T.text_at + prefix.size(), suffix.data(), suffix.size());
    *taken = true;
    // 2. the box into the compaction
    if (const int rc = patch(c)) return rc;
    // 3. the selected chunks parsed again; the old frames' verdict
    if (const int rc = update_box_parse(c, T, chunk, stride)) return rc;
    // 4., 5. the splice and its record
    const uint8_t* d_tab = static_cast<const uint8_t*>(cx.ws.batch_tables.p);
    const sqy::Lz4SpliceJob job{c.range_ix.blk, reinterpret_cast<const uint32_t*>(d_tab + T.slot_at), reinterpret_cast<const sqy::Lz4BatchChunk*>(d_tab + T.table_at),
                                reinterpret_cast<const uint32_t*>(d_tab + T.csize_at), c.cur_bytes, (uint32_t)nframes,
                                (uint32_t)(std::max<uint64_t>(chunk, c.range_ix.block_bytes) + sqy::kLz4FrameGap), (uint32_t)prefix.size(), (uint32_t)suffix.size(),
                                (uint32_t)u.elem};
    if (!sqy::lz4_splice_job_ok(job)) { std::fprintf(stderr, "[sqeazy]\t update box: more frames than one launch takes\n"); return 1; }
    return update_box_splice(c, u, T, job, stride);
}

// what needs no header, before a device is looked for; the view rules; then, against the header: the voxel type, the rank and the box,
// the single call's refusals for the blob's shape under `pipeline` -- all before a byte is written
int update_box_device(const char* pipeline, const void* d_src, long srclength, const long* origin, const void* d_view, const long* view_shape, const long* view_strides,
                      unsigned rank, int elem_size, void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream)
{
    if (!dstlength) return 1;
    *dstlength = 0;
    if (!pipeline || !box_arguments_ok(d_src, srclength, origin, d_dst, view_shape, rank) || !d_view || dst_capacity <= 0) {
        std::fprintf(stderr, "[sqeazy]\t update box: bad arguments\n");
        return 1;
    }
    Pipeline pipe;
    if (admit_pipeline(pipeline, elem_size, nthreads, &pipe)) return 1;
    std::vector<sqy::BatchView> views;
    const void* const ptrs[1] = {d_view};
    if (admit_views("update box", ptrs, view_shape, view_strides, rank, 1, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Context& cx = *lease.ctx;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    sqy::HeaderInfo h;
    uint64_t raw_bytes = 0;
    sqy::BatchWindow w;
    {
        DrainOnExit drain{stream, &cx.pending, cx.side};
        if (fetch_header(src, (uint64_t)srclength, stream, h)) return 1;
        if (!admit_blob(h, (uint64_t)srclength, elem_size, &raw_bytes)) return 1;
        if (!sqy::admit_window(h.shape, origin, view_shape, rank, &w)) {
            std::fprintf(stderr, "[sqeazy]\t update box: the box does not lie inside the blob's shape, or has another rank\n");
            return 1;
        }
        std::vector<long> shape(h.shape.begin(), h.shape.end());
        std::vector<uint64_t> dims;
        uint64_t len = 0;
        if (admit_shape(&pipe, shape.data(), rank, &dims, &len)) return 1;
    }
    const WindowView v = window_view(w, view_strides, rank);
    const UpdateBoxCall u{cx, stream, pipeline, pipe, src, (uint64_t)srclength, h, raw_bytes, w, v, (uint64_t)origin[0], (uint64_t)view_shape[0], rank, d_view, elem_size, d_dst, (uint64_t)dst_capacity, dstlength, nthreads};
    bool taken = false;
    WindowLaunch l;                                                     // (waits for the stream before its tables go)
    if (const int rc = update_box_subset(u, g_opt.update_box_subset.load() != 0, {{u.z0, u.nz}}, [&](DecodeCall& c) { return update_box_patch(c, u, l); }, &taken)) return rc;
    return taken ? 0 : update_box_whole(u);
}

// ---- many boxes written into one large blob (SQYAMD_Update_Boxes_*) --------------------------------------------------------------
// SQYAMD_Update_Box_*'s stages for a table of boxes, each stage ONCE: one header fetch, one frame index, one frames_subset over the
// SEGMENTS of sqy::update_boxes_plan (every LZ4 frame decoded once), one patch launch (bitswap1_range_patches_kernel; `lz4`: one window
// paste per layer), one parse of all selected chunks with the old frames' verdict at its round trip, one splice.  The whole path: one
// decode into Workspace::range_full, the pastes layer by layer, one single-call encode.  New blob = what a chain of SQYAMD_Update_Box_*
// calls gives: box 0, then box 1, .. pasted in that order.
struct UpdateBoxesTable {
    std::vector<sqy::BatchWindow> ws;
    std::vector<WindowView> vs;
    const void* const* d_views = nullptr;
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                  // box i's range along the header's first dimension
    sqy::UpdateBoxesPlan plan;                                          // (ok only where the subset path may run)
    std::vector<uint32_t> layer_first;                                  // the layers of the paste launches, whichever path
};
// the device tables of bitswap1_range_patches_kernel in Workspace::boxes_jobs: segments | boxes | first workgroups; alive until the stream
// has been waited for
struct PatchTables {
    std::vector<unsigned char> host;
    hipStream_t queued_on = nullptr;
    bool queued = false;
    PatchTables() = default;
    PatchTables(const PatchTables&) = delete;
    PatchTables& operator=(const PatchTables&) = delete;
    ~PatchTables() { if (queued) (void)hipStreamSynchronize(queued_on); }
};

// the whole path's pastes into Workspace::range_full, layer by layer in stream order
int update_boxes_whole_paste(const UpdateBoxCall& u, const UpdateBoxesTable& t)
{
    Context& cx = u.cx;
    DrainOnExit drain{u.stream, &cx.pending, cx.side};
    for (size_t l = 0; l + 1 < t.layer_first.size(); ++l) {
        WindowLaunch paste;
        for (uint32_t i = t.layer_first[l]; i < t.layer_first[l + 1]; ++i) paste.add(t.d_views[i], cx.ws.range_full.p, t.ws[i], t.vs[i], false);
        if (launch_windows(cx, u.stream, paste, WindowLaunch::paste, u.elem)) return 1;
        paste.wait();                                                   // (the next layer's table goes to the same buffer)
    }
    return 0;
}

// subset path, stage 2 for a table of boxes: ONE launch of the patch kernel over the plan's segments, or (plain) one paste per layer
int update_boxes_patch(DecodeCall& c, const UpdateBoxCall& u, const UpdateBoxesTable& t, PatchTables& pt)
{
    hipStream_t stream = c.stream;
    std::vector<PendingEvent>* pend = c.pend;
    const sqy::FrameRangesPlan& p = c.ranges_plan;
    const std::vector<sqy::UpdateBoxesSegment>& segs = t.plan.segments;
    if (p.boxes.size() != segs.size()) { std::fprintf(stderr, "[sqeazy]\t internal error: update boxes: the frame plan does not hold the segments\n"); return 1; }
    if (c.range_form == sqy::RangeForm::planes) {
        const uint32_t wpt = 128u / (8u * (uint32_t)p.we), nsegs = (uint32_t)segs.size(), nboxes = (uint32_t)t.ws.size();
        const uint64_t boxes_at = (uint64_t)nsegs * sizeof(sqy::Bitswap1PatchSegment), tiles_at = boxes_at + (uint64_t)nboxes * sizeof(sqy::Bitswap1PatchBox);
        pt.host.assign(tiles_at + ((uint64_t)nsegs + 1) * 4, 0);
        sqy::Bitswap1PatchSegment* hs = reinterpret_cast<sqy::Bitswap1PatchSegment*>(pt.host.data());
        sqy::Bitswap1PatchBox* hb = reinterpret_cast<sqy::Bitswap1PatchBox*>(pt.host.data() + boxes_at);
        uint32_t* ht = reinterpret_cast<uint32_t*>(pt.host.data() + tiles_at);
        uint64_t groups = 0;
        uint32_t named = 0;
        for (uint32_t s = 0; s < nsegs; ++s) {
            const sqy::FrameRangesBox& b = p.boxes[s];
            std::copy(b.plane, b.plane + 16, hs[s].r.plane);
            hs[s].r.tail = b.tail; hs[s].r.w0 = b.w0; hs[s].r.w1 = b.w1; hs[s].r.v0 = b.v0; hs[s].r.v1 = b.v1; hs[s].r.L = b.L;
            hs[s].t0 = sqy::range_first_thread(b.w0, wpt);
            hs[s].box0 = named;
            hs[s].nbox = (uint32_t)segs[s].boxes.size();
            for (uint32_t i : segs[s].boxes) {
                const sqy::BatchWindow& w = t.ws[i];
                hb[named].view = t.d_views[i];
                hb[named].g = sqy::window_geometry(w, t.vs[i].sz, t.vs[i].sy);
                ++named;
            }
            ht[s] = (uint32_t)groups;
            groups += sqy::range_job_groups(b.w0, b.w1, wpt);
            if (groups > 0x7fffffffull) { std::fprintf(stderr, "[sqeazy]\t update boxes: too many workgroups for one launch\n"); return 1; }
        }
        ht[nsegs] = (uint32_t)groups;
        if (!sqy::bitswap1_patch_tables_ok(hs, nsegs, hb, nboxes, p.we)) { std::fprintf(stderr, "[sqeazy]\t internal error: the segments do not hold the boxes\n"); return 1; }
        if (c.cx.ws.boxes_jobs.ensure(pt.host.size())) return 1;
        uint8_t* d_tab = static_cast<uint8_t*>(c.cx.ws.boxes_jobs.p);
        pt.queued_on = stream;
        pt.queued = true;
        SQY_HIP(hipMemcpyAsync(d_tab, pt.host.data(), pt.host.size(), hipMemcpyHostToDevice, stream));
        SQY_TIMED("bitswap1_range_patches",
                  sqy::launch_bitswap1_range_patches(c.range_buf, reinterpret_cast<const sqy::Bitswap1PatchSegment*>(d_tab),
                                                     reinterpret_cast<const sqy::Bitswap1PatchBox*>(d_tab + boxes_at), reinterpret_cast<const uint32_t*>(d_tab + tiles_at), nsegs,
                                                     (uint32_t)groups, p.we, stream));
        return 0;
    }
    // plain: a segment's range in the workspace is a blob of its frames (box_range_out's rule); one launch per layer, in stream order
    std::vector<uint32_t> seg_of(t.ws.size(), 0);
    for (size_t s = 0; s < segs.size(); ++s) for (uint32_t i : segs[s].boxes) seg_of[i] = (uint32_t)s;
    for (size_t l = 0; l + 1 < t.layer_first.size(); ++l) {
        WindowLaunch paste;
        for (uint32_t i = t.layer_first[l]; i < t.layer_first[l + 1]; ++i) {
            const sqy::UpdateBoxesSegment& sg = segs[seg_of[i]];
            sqy::BatchWindow in_range = t.ws[i];
            if (u.rank == 3) { in_range.bZ = sg.nz; in_range.oz -= sg.z0; }
            else if (u.rank == 2) { in_range.bY = sg.nz; in_range.oy -= sg.z0; }
            else { in_range.bX = sg.nz; in_range.ox -= sg.z0; }
            paste.add(t.d_views[i], c.range_buf + p.boxes[seg_of[i]].range_at, in_range, t.vs[i], false);
        }
        const uint32_t* d_tiles = nullptr;
        if (paste.upload(stream, c.cx.ws.boxes_jobs, &d_tiles)) return 1;
        SQY_TIMED("boxes_window_paste", sqy::launch_batch_window_paste(static_cast<const sqy::BatchWindowJob*>(c.cx.ws.boxes_jobs.p), d_tiles, (uint32_t)paste.jobs.size(),
                                                                       paste.ntiles, u.elem, stream));
        paste.wait();                                                   // (the next layer's table goes to the same buffer)
    }
    return 0;
}

// Box i = [origins + i rank, .. + view_shapes + i rank) of the old blob replaced by the view at d_views[i].  What needs the header: the
// voxel type, the rank and every box, the single call's refusals for the blob's shape under `pipeline`, the launches' sizes -- all
// before a byte is written
int update_boxes_on_device(Context& cx, const char* pipeline, const Pipeline& pipe, const void* d_src, uint64_t srclen, size_t count, const long* origins,
                           const void* const* d_views, const long* view_shapes, const long* view_strides, unsigned rank, int elem_size, void* d_dst, uint64_t capacity,
                           long* dstlength, int nthreads, hipStream_t stream)
{
    const uint8_t* src = static_cast<const uint8_t*>(d_src);
    sqy::HeaderInfo h;
    uint64_t raw_bytes = 0;
    UpdateBoxesTable t;
    t.ws.resize(count); t.vs.resize(count); t.ranges.resize(count);
    t.d_views = d_views;
    Pipeline admitted = pipe;
    {
        DrainOnExit drain{stream, &cx.pending, cx.side};
        if (fetch_header(src, srclen, stream, h)) return 1;
        if (!admit_blob(h, srclen, elem_size, &raw_bytes)) return 1;
        const uint64_t frame_voxels = raw_bytes / (uint64_t)elem_size / h.shape[0];
        uint64_t paste_tiles = 0, range_groups = 0;          // what one launch may hold, whichever it is
        for (size_t i = 0; i < count; ++i) {
            const long* o = origins + i * rank;
            const long* e = view_shapes + i * rank;
            if (!sqy::admit_window(h.shape, o, e, rank, &t.ws[i])) {
                std::fprintf(stderr, "[sqeazy]\t update boxes: box %zu does not lie inside the blob's shape, or has another rank\n", i);
                return 1;
            }
            t.vs[i] = window_view(t.ws[i], view_strides ? view_strides + i * rank : nullptr, rank);
            t.ranges[i] = {(uint64_t)o[0], (uint64_t)e[0]};
            paste_tiles += sqy::batch_bitswap1_tiles(t.ws[i].Z * t.ws[i].Y * t.ws[i].X);
            range_groups += (uint64_t)e[0] * frame_voxels / sqy::kBatchTileVoxels + 2;      // (at least range_job_groups of the box's words)
        }
        if (std::max(paste_tiles, range_groups) > 0x7fffffffull) {
            std::fprintf(stderr, "[sqeazy]\t update boxes: too many workgroups for one launch\n");
            return 1;
        }
        std::vector<long> shape(h.shape.begin(), h.shape.end());
        std::vector<uint64_t> dims;
        uint64_t len = 0;
        if (admit_shape(&admitted, shape.data(), rank, &dims, &len)) return 1;
    }
    t.layer_first = sqy::update_boxes_layers(t.ws);
    const UpdateBoxCall u{cx, stream, pipeline, admitted, src, srclen, h, raw_bytes, t.ws[0], t.vs[0], t.ranges[0].first, t.ranges[0].second, rank, d_views[0], elem_size, d_dst,
                          capacity, dstlength, nthreads};
    bool taken = false;
    const bool option_on = g_opt.update_boxes_subset.load() != 0;
    if (option_on && sqy::update_box_form_ok(admitted)) {
        t.plan = sqy::update_boxes_plan(admitted.stages.size() == 1 ? sqy::RangeForm::plain : sqy::RangeForm::planes, raw_bytes / (uint64_t)elem_size, elem_size, h.shape[0],
                                        t.ranges, t.ws);
        if (!t.plan.ok) { std::fprintf(stderr, "[sqeazy]\t internal error: update boxes: no plan\n"); return 1; }
        std::vector<std::pair<uint64_t, uint64_t>> segments;
        for (const sqy::UpdateBoxesSegment& s : t.plan.segments) segments.push_back({s.z0, s.nz});
        PatchTables pt;                                                 // (waits for the stream before its tables go)
        if (const int rc = update_box_subset(u, option_on, segments, [&](DecodeCall& c) { return update_boxes_patch(c, u, t, pt); }, &taken)) return rc;
    }
    return taken ? 0 : update_box_whole(u, &t);
}

// what needs no header, before a device is looked for: the arguments, the pipeline, the view rules
int update_boxes_admit(const char* who, const char* pipeline, const void* src, long srclength, long count, const long* origins, const void* const* views, const long* extents,
                       unsigned rank, const void* dst, long dst_capacity, long* dstlength, int elem_size, int nthreads, Pipeline* pipe)
{
    if (!dstlength) return 1;
    *dstlength = 0;
    if (!pipeline || !dst || dst_capacity <= 0 || !boxes_arguments_ok(src, srclength, count, origins, views, extents, rank)) {
        std::fprintf(stderr, "[sqeazy]\t %s: bad arguments\n", who);
        return 1;
    }
    return admit_pipeline(pipeline, elem_size, nthreads, pipe);
}

int update_boxes_device(const char* pipeline, const void* d_src, long srclength, long count, const long* origins, const void* const* d_views, const long* view_shapes,
                        const long* view_strides, unsigned rank, int elem_size, void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream)
{
    Pipeline pipe;
    if (!d_views) { if (dstlength) *dstlength = 0; std::fprintf(stderr, "[sqeazy]\t update boxes: bad arguments\n"); return 1; }
    if (update_boxes_admit("update boxes", pipeline, d_src, srclength, count, origins, d_views, view_shapes, rank, d_dst, dst_capacity, dstlength, elem_size, nthreads, &pipe)) return 1;
    std::vector<sqy::BatchView> views;
    if (admit_views("update boxes", d_views, view_shapes, view_strides, rank, (int)count, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return update_boxes_on_device(*lease.ctx, pipeline, pipe, d_src, (uint64_t)srclength, (size_t)count, origins, d_views, view_shapes, view_strides, rank, elem_size, d_dst,
                                  (uint64_t)dst_capacity, dstlength, nthreads, static_cast<hipStream_t>(hip_stream));
}

// host pointers: the header and every box are checked here, before anything is staged; views: the boxes' new voxels dense, back to back
// in box order, exactly views_bytes of them.  The blob and the views are staged once, the new blob comes back
int update_boxes_from_host(const char* pipeline, const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views,
                           long views_bytes, char* dst, long dst_capacity, long* dstlength, int elem_size, int nthreads)
{
    Pipeline pipe;
    if (!views) { if (dstlength) *dstlength = 0; std::fprintf(stderr, "[sqeazy]\t update boxes: bad arguments\n"); return 1; }
    if (update_boxes_admit("update boxes", pipeline, src, srclength, count, origins, nullptr, extents, rank, dst, dst_capacity, dstlength, elem_size, nthreads, &pipe)) return 1;
    // (without a header: every extent positive, the views' bytes their sum; a product that does not fit 63 bits is no such sum)
    uint64_t sum = 0;
    for (long i = 0; i < count; ++i) {
        uint64_t vox = 1;
        for (unsigned k = 0; k < rank; ++k) {
            const long e = extents[(size_t)i * rank + k];
            if (e <= 0 || vox > (uint64_t)LONG_MAX / (uint64_t)e) { std::fprintf(stderr, "[sqeazy]\t update boxes: box %ld has no such extent\n", i); return 1; }
            vox *= (uint64_t)e;
        }
        if (vox > ((uint64_t)LONG_MAX - sum) / (uint64_t)elem_size) { sum = (uint64_t)LONG_MAX; break; }
        sum += vox * (uint64_t)elem_size;
    }
    if (views_bytes < 0 || sum != (uint64_t)views_bytes) { std::fprintf(stderr, "[sqeazy]\t update boxes: the views hold another number of bytes than the boxes\n"); return 1; }
    sqy::HeaderInfo h;
    uint64_t raw = 0;
    std::vector<uint64_t> bytes, at;
    if (!host_header_ok(src, srclength, elem_size, &h, &raw) || !host_box_bytes("update boxes", h, count, origins, extents, rank, elem_size, &bytes)) return 1;
    (void)sqy::output_offsets(bytes, views_bytes, &at);               // (the views' bytes are the boxes': checked above)
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Context& cx = *lease.ctx;
    hipStream_t stream = cx.own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    // the blob and, on the 16-byte grid behind it, the views in one staging buffer; the destination no larger than a blob can get
    const uint64_t views_at = ((uint64_t)srclength + 15) & ~(uint64_t)15;
    const uint64_t room = std::min<uint64_t>((uint64_t)dst_capacity, std::max(Pipeline::from_string(pipeline, elem_size).max_encoded_size(raw, elem_size), pipe.max_encoded_size(raw, elem_size)));
    if (cx.ws.io_src.ensure(std::max<uint64_t>(views_at + at.back(), 16)) || cx.ws.io_dst.ensure(std::max<uint64_t>(room, 16))) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    uint8_t* d_io = static_cast<uint8_t*>(cx.ws.io_src.p);
    if (!cx.stager.copy(d_io, const_cast<char*>(src), (size_t)srclength, true, dev_id) || !cx.stager.copy(d_io + views_at, const_cast<char*>(views), (size_t)at.back(), true, dev_id)) {
        std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n");
        return 1;
    }
    std::vector<const void*> ptrs((size_t)count);
    for (long i = 0; i < count; ++i) ptrs[(size_t)i] = d_io + views_at + at[(size_t)i];
    if (const int rc = update_boxes_on_device(cx, pipeline, pipe, d_io, (uint64_t)srclength, (size_t)count, origins, ptrs.data(), extents, nullptr, rank, elem_size,
                                              cx.ws.io_dst.p, room, dstlength, nthreads, stream))
        return rc;
    if (!cx.stager.copy(cx.ws.io_dst.p, dst, (size_t)*dstlength, false, dev_id)) { *dstlength = 0; std::fprintf(stderr, "[sqeazy]\t device to host transfer failed\n"); return 1; }
    return 0;
}

// the host-pointer variant (not tuned): every volume staged up, one call of the device driver, the blobs brought back
int encode_batch_from_host(const char* pipeline, const char* const* srcs, const long* shapes, unsigned rank, int elem_size, int nvolumes, char* dst,
                           long slot_capacity, long* offsets, long* lengths, int nthreads)
{
    BatchAdmit a;
    if (admit_batch(pipeline, reinterpret_cast<const void* const*>(srcs), shapes, rank, elem_size, nvolumes, dst, slot_capacity, offsets, lengths, nthreads, &a)) return 1;
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Workspace* ws = &lease.ctx->ws;
    hipStream_t stream = lease.ctx->own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    std::vector<uint64_t> at((size_t)nvolumes);
    uint64_t raw = 0;
    for (int i = 0; i < nvolumes; ++i) { at[(size_t)i] = raw; raw += (a.len[(size_t)i] * (uint64_t)elem_size + 15) & ~(uint64_t)15; }
    if (ws->io_src.ensure(std::max<uint64_t>(raw, 16)) || ws->io_dst.ensure((uint64_t)nvolumes * (uint64_t)slot_capacity)) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    std::vector<const void*> d_srcs((size_t)nvolumes);
    for (int i = 0; i < nvolumes; ++i) {
        d_srcs[(size_t)i] = static_cast<char*>(ws->io_src.p) + at[(size_t)i];
        if (!lease.ctx->stager.copy(const_cast<void*>(d_srcs[(size_t)i]), const_cast<char*>(srcs[i]), a.len[(size_t)i] * (uint64_t)elem_size, true, dev_id)) {
            std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n");
            return 1;
        }
    }
    const int rc = encode_batch_on_device(*lease.ctx, pipeline, a, d_srcs.data(), shapes, rank, elem_size, nvolumes, ws->io_dst.p, (uint64_t)slot_capacity, offsets,
                                          lengths, nthreads, stream);
    if (rc) return rc;
    for (int i = 0; i < nvolumes; ++i)
        if (!lease.ctx->stager.copy(static_cast<char*>(ws->io_dst.p) + offsets[i], dst + offsets[i], (size_t)lengths[i], false, dev_id)) {
            std::fprintf(stderr, "[sqeazy]\t device to host transfer failed\n");
            for (int k = 0; k < nvolumes; ++k) { offsets[k] = 0; lengths[k] = 0; }
            return 1;
        }
    return 0;
}

// SQYAMD_PipelineEncode_BatchPacked_*: the Batch call's checks with the capacity of all of dst, then total and align -- on the host,
// before the device is touched; offsets, lengths and *total are zeroed whatever comes of it
int admit_batch_packed(const char* pipeline, const void* const* srcs, const long* shapes, unsigned rank, int elem_size, int nvolumes, const void* dst,
                       long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads, BatchAdmit* a)
{
    if (total) *total = 0;
    if (admit_batch(pipeline, srcs, shapes, rank, elem_size, nvolumes, dst, dst_capacity, offsets, lengths, nthreads, a)) return 1;
    if (!total) return 1;
    if (align < 1 || align > (long)sqy::kPackedAlignMax || (align & (align - 1))) {
        std::fprintf(stderr, "[sqeazy]\t encode batch: align %ld is no power of two from 1 to %llu\n", align, (unsigned long long)sqy::kPackedAlignMax);
        return 1;
    }
    return 0;
}

int encode_batch_packed_device(const char* pipeline, const void* const* d_srcs, const long* shapes, const long* strides, unsigned rank, int elem_size, int nvolumes,
                               void* d_dst, long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads, void* hip_stream)
{
    BatchAdmit a;
    if (admit_batch_packed(pipeline, d_srcs, shapes, rank, elem_size, nvolumes, d_dst, dst_capacity, align, offsets, lengths, total, nthreads, &a)) return 1;
    std::vector<sqy::BatchView> views;
    if (admit_views("encode batch", d_srcs, shapes, strides, rank, nvolumes, elem_size, &views)) return 1;
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    const PackedArgs packed{(uint64_t)align, total};
    return encode_batch_on_device(*lease.ctx, pipeline, a, d_srcs, shapes, rank, elem_size, nvolumes, d_dst, (uint64_t)dst_capacity, offsets, lengths, nthreads,
                                  static_cast<hipStream_t>(hip_stream), strides ? &views : nullptr, &packed);
}

// the host-pointer variant (not tuned): every volume staged up, one call of the device driver, ONE copy of *total bytes back
int encode_batch_packed_from_host(const char* pipeline, const char* const* srcs, const long* shapes, unsigned rank, int elem_size, int nvolumes, char* dst,
                                  long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads)
{
    BatchAdmit a;
    if (admit_batch_packed(pipeline, reinterpret_cast<const void* const*>(srcs), shapes, rank, elem_size, nvolumes, dst, dst_capacity, align, offsets, lengths, total,
                           nthreads, &a))
        return 1;
    if (!device_present()) { std::fprintf(stderr, "[sqeazy]\t no MI355X (HIP device) visible: sqeazy_amd has no CPU path\n"); return 1; }
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    Workspace* ws = &lease.ctx->ws;
    hipStream_t stream = lease.ctx->own_stream();
    if (!stream) { std::fprintf(stderr, "[sqeazy]\t no HIP stream\n"); return 1; }
    std::vector<uint64_t> at((size_t)nvolumes);
    // the device buffer: the caller's capacity, but no more than what needs no retry
    uint64_t raw = 0, enough = 0;
    for (int i = 0; i < nvolumes; ++i) {
        at[(size_t)i] = raw;
        raw += (a.len[(size_t)i] * (uint64_t)elem_size + 15) & ~(uint64_t)15;
        enough += align_up(a.pipe.max_encoded_size(a.len[(size_t)i] * (uint64_t)elem_size, elem_size), (uint64_t)align);
    }
    const uint64_t capacity = std::min<uint64_t>((uint64_t)dst_capacity, enough);
    if (ws->io_src.ensure(std::max<uint64_t>(raw, 16)) || ws->io_dst.ensure(std::max<uint64_t>(capacity, 16))) return 1;
    int dev_id = 0;
    SQY_HIP(hipGetDevice(&dev_id));
    std::vector<const void*> d_srcs((size_t)nvolumes);
    for (int i = 0; i < nvolumes; ++i) {
        d_srcs[(size_t)i] = static_cast<char*>(ws->io_src.p) + at[(size_t)i];
        if (!lease.ctx->stager.copy(const_cast<void*>(d_srcs[(size_t)i]), const_cast<char*>(srcs[i]), a.len[(size_t)i] * (uint64_t)elem_size, true, dev_id)) {
            std::fprintf(stderr, "[sqeazy]\t host to device transfer failed\n");
            return 1;
        }
    }
    // (align > 1: the gap bytes come back with the blobs -- zeros, not what the workspace held)
    if (align > 1) SQY_HIP(hipMemsetAsync(ws->io_dst.p, 0, capacity, stream));
    const PackedArgs packed{(uint64_t)align, total};
    const int rc = encode_batch_on_device(*lease.ctx, pipeline, a, d_srcs.data(), shapes, rank, elem_size, nvolumes, ws->io_dst.p, capacity, offsets, lengths, nthreads,
                                          stream, nullptr, &packed);
    if (rc) return rc;
    if (!lease.ctx->stager.copy(ws->io_dst.p, dst, (size_t)*total, false, dev_id)) {
        std::fprintf(stderr, "[sqeazy]\t device to host transfer failed\n");
        for (int k = 0; k < nvolumes; ++k) { offsets[k] = 0; lengths[k] = 0; }
        *total = 0;
        return 1;
    }
    return 0;
}

int max_compressed_length(const char* pipeline, long pipeline_length, long* length, int elem_size, uint64_t raw_bytes)
{
    if (!pipeline || !length || pipeline_length < 0) return 1;
    const std::string s(pipeline, pipeline + pipeline_length);
    if (!Pipeline::supported(s, elem_size)) return 1;
    const Pipeline p = Pipeline::from_string(s, elem_size);
    if (p.stages.empty()) {
        std::fprintf(stderr, "[sqeazy]\t received %spipeline of size 0, cannot compite Max_Compressed_Length\n", p.name().c_str());
        return 1;
    }
    *length = (long)p.max_encoded_size(raw_bytes, elem_size);
    return 0;
}

// No C++ exception may cross the C-ABI (std::bad_alloc from a std::string / std::vector, anything a parser throws):
// every entry point runs inside one of these and turns an exception into the reference's generic error code.
template <class F>
int guarded(F&& f) noexcept
{
    try { return f(); }
    catch (const std::exception& e) { std::fprintf(stderr, "[sqeazy]\t %s\n", e.what()); return 1; }
    catch (...) { std::fprintf(stderr, "[sqeazy]\t unknown exception\n"); return 1; }
}
template <class F>
bool guarded_bool(F&& f) noexcept
{
    try { return f(); } catch (...) { return false; }
}

} // namespace

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

int SQY_Header_Size(const char* src, long* length)
{
    return guarded([&]() -> int {
    if (!src || !length) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(src, src + *length);
    *length = h.valid ? (long)h.size : 0;
    return 0;
    });
}

int SQY_Decompressed_NDims(const char* src, long* num)
{
    return guarded([&]() -> int {
    if (!src || !num) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(src, src + *num);
    *num = (long)h.shape.size();
    return 0;
    });
}

int SQY_Decompressed_Shape(const char* src, long* shape)
{
    return guarded([&]() -> int {
    if (!src || !shape) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(src, src + shape[0]);
    for (size_t i = 0; i < h.shape.size(); ++i) shape[i] = (long)h.shape[i];
    return 0;
    });
}

int SQY_Decompressed_Sizeof(const char* src, long* Sizeof)
{
    return guarded([&]() -> int {
    if (!src || !Sizeof) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(src, src + *Sizeof);
    *Sizeof = h.valid ? h.elem_size() : 0;
    return 0;
    });
}

int SQY_Decompressed_Length(const char* data, long* length)
{
    return guarded([&]() -> int {
    if (!data || !length) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(data, data + *length);
    uint64_t n = 1;
    for (uint64_t d : h.shape) n *= d;
    *length = h.valid ? (long)(n * (uint64_t)h.elem_size()) : 0;
    return 0;
    });
}

int SQY_Version_Triple(int* version)
{
    return guarded([&]() -> int {
    if (!version) return 1;
    version[0] = sqy::kVersionTriple[0];
    version[1] = sqy::kVersionTriple[1];
    version[2] = sqy::kVersionTriple[2];
    return 0;
    });
}

int SQY_PipelineEncode_UI8(const char* pipeline, const char* src, long* shape, unsigned shape_size, char* dst, long* dstlength, int nthreads)
{
    return guarded([&]() -> int {
    return encode_from_host(pipeline, src, shape, shape_size, 1, dst, dstlength, nthreads);
    });
}

int SQY_PipelineEncode_UI16(const char* pipeline, const char* src, long* shape, unsigned shape_size, char* dst, long* dstlength, int nthreads)
{
    return guarded([&]() -> int {
    return encode_from_host(pipeline, src, shape, shape_size, 2, dst, dstlength, nthreads);
    });
}

int SQY_Pipeline_Max_Compressed_Length_UI8(const char* pipeline, long pipeline_length, long* length)
{
    return guarded([&]() -> int {
    return length ? max_compressed_length(pipeline, pipeline_length, length, 1, (uint64_t)*length) : 1;
    });
}

int SQY_Pipeline_Max_Compressed_Length_UI16(const char* pipeline, long pipeline_length, long* length)
{
    return guarded([&]() -> int {
    return length ? max_compressed_length(pipeline, pipeline_length, length, 2, (uint64_t)*length) : 1;
    });
}

static int max_len_3d(const char* pipeline, long* shape, unsigned shape_size, long* length, int elem)
{
    if (!shape || !length) return 1;
    long n = 1;
    for (unsigned i = 0; i < shape_size; ++i) n *= shape[i];   // std::accumulate(..., 1, multiplies<long>) (sqeazy.cpp:195)
    return max_compressed_length(pipeline, *length, length, elem, (uint64_t)n * (uint64_t)elem);
}

int SQY_Pipeline_Max_Compressed_Length_3D_UI8(const char* pipeline, long* shape, unsigned shape_size, long* length)
{
    return guarded([&]() -> int {
    return max_len_3d(pipeline, shape, shape_size, length, 1);
    });
}

int SQY_Pipeline_Max_Compressed_Length_3D_UI16(const char* pipeline, long* shape, unsigned shape_size, long* length)
{
    return guarded([&]() -> int {
    return max_len_3d(pipeline, shape, shape_size, length, 2);
    });
}

bool SQY_Pipeline_Possible_UI16(const char* s) { return guarded_bool([&]() -> bool { return s && Pipeline::supported(s, 2); }); }
bool SQY_Pipeline_Possible_UI8(const char* s) { return guarded_bool([&]() -> bool { return s && Pipeline::supported(s, 1); }); }
bool SQY_Pipeline_Possible(const char* s, int sizeofpixel)
{
    return guarded_bool([&]() -> bool {
    return s && (sizeofpixel == 1 || sizeofpixel == 2) && Pipeline::supported(s, sizeofpixel);
    });
}

int SQY_Decode_UI16(const char* src, long srclength, char* dst, int nthreads)
{
    return guarded([&]() -> int {
    (void)nthreads;   // the layout is read from the blob; the GPU decodes every frame in parallel
    return decode_from_host(src, srclength, dst, 2);
    });
}

int SQY_Decode_UI8(const char* src, long srclength, char* dst, int nthreads)
{
    return guarded([&]() -> int {
    (void)nthreads;
    return decode_from_host(src, srclength, dst, 1);
    });
}

int SQYAMD_PipelineEncode_UI16_Device(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, void* d_dst,
                                      long dst_capacity, long* dstlength, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
    return encode_device(pipeline, d_src, shape, shape_size, 2, d_dst, dst_capacity, nullptr, dstlength, nthreads, hip_stream, false);
    });
}

int SQYAMD_PipelineEncode_UI8_Device(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, void* d_dst,
                                     long dst_capacity, long* dstlength, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
    return encode_device(pipeline, d_src, shape, shape_size, 1, d_dst, dst_capacity, nullptr, dstlength, nthreads, hip_stream, false);
    });
}

int SQYAMD_PipelineEncode_UI16_DeviceAt(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, void* d_dst,
                                        long dst_capacity, long* dstoffset, long* dstlength, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
    return encode_device(pipeline, d_src, shape, shape_size, 2, d_dst, dst_capacity, dstoffset, dstlength, nthreads, hip_stream, true);
    });
}

int SQYAMD_PipelineEncode_UI16_DeviceAt_Frames(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, void* d_dst,
                                               long dst_capacity, long* dstoffset, long* dstlength, int nthreads, void* hip_stream, int every,
                                               long* frame_offsets, int max_entries, int* count)
{
    return guarded([&]() -> int {
    FrameQuery fq{every, frame_offsets, max_entries, 0};
    return encode_device(pipeline, d_src, shape, shape_size, 2, d_dst, dst_capacity, dstoffset, dstlength, nthreads, hip_stream, true, &fq, count);
    });
}

int SQYAMD_PipelineEncode_UI8_DeviceAt_Frames(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, void* d_dst,
                                              long dst_capacity, long* dstoffset, long* dstlength, int nthreads, void* hip_stream, int every,
                                              long* frame_offsets, int max_entries, int* count)
{
    return guarded([&]() -> int {
    FrameQuery fq{every, frame_offsets, max_entries, 0};
    return encode_device(pipeline, d_src, shape, shape_size, 1, d_dst, dst_capacity, dstoffset, dstlength, nthreads, hip_stream, true, &fq, count);
    });
}

int SQYAMD_PipelineEncode_UI8_DeviceAt(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, void* d_dst,
                                       long dst_capacity, long* dstoffset, long* dstlength, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
    return encode_device(pipeline, d_src, shape, shape_size, 1, d_dst, dst_capacity, dstoffset, dstlength, nthreads, hip_stream, true);
    });
}

// A volume as `nslabs` independent z-slab blobs, `inflight` slab calls at a time on library-owned streams (one host thread, context
// and stream per call in flight -- what three caller threads would do, available to a plain C caller with one call).
static int encode_slabs(const char* pipeline, const void* d_src, const long* shape, unsigned rank, int elem_size, int nslabs, void* d_dst,
                        long slab_capacity, long* offsets, long* lengths, int nthreads, int inflight)
{
    if (!pipeline || !d_src || !shape || !d_dst || !offsets || !lengths || rank == 0 || nslabs <= 0 || slab_capacity <= 0) return 1;
    for (unsigned i = 0; i < rank; ++i) if (shape[i] <= 0) return 1;
    if ((long)nslabs > shape[0]) { std::fprintf(stderr, "[sqeazy]\t more slabs (%d) than frames (%ld)\n", nslabs, shape[0]); return 1; }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    uint64_t per_frame = (uint64_t)elem_size;
    for (unsigned i = 1; i < rank; ++i) per_frame *= (uint64_t)shape[i];
    const long base = shape[0] / nslabs, rem = shape[0] % nslabs;           // the first Z % nslabs slabs get one frame more
    if (inflight <= 0) inflight = 3;
    if (inflight > nslabs) inflight = nslabs;
    if (inflight > (int)kMaxCtxPerDev) inflight = (int)kMaxCtxPerDev;
    std::atomic<int> first_error(0);
    for (int i = 0; i < nslabs; ++i) { offsets[i] = 0; lengths[i] = 0; }      // (defined whatever happens below)
    // The slab calls run on streams of the library's own (non-blocking ones: nothing orders them behind the default stream by itself), the
    // caller passes none -- so what the caller has queued on the DEFAULT stream up to now (the kernel that makes d_src, a fill of d_dst: a
    // framework's allocations and copies usually live there) is put in front of them here: an event on the default stream, waited for by
    // every worker's stream.  Found by the full-size slab test of round 6, whose fill of d_dst overtook the first slabs' transposes and
    // was parsed in their place.  Work on OTHER streams of the caller has to be complete when the call is made (include/sqeazy_amd.h).
    hipEvent_t front = nullptr;
    if (hipEventCreateWithFlags(&front, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); front = nullptr; }
    struct EventGuard { hipEvent_t& e; ~EventGuard() { if (e) (void)hipEventDestroy(e); } } front_guard{front};
    if (!front || hipEventRecord(front, nullptr) != hipSuccess) {            // (no event to be had: wait here for everything instead)
        (void)hipGetLastError();
        if (front) { (void)hipEventDestroy(front); front = nullptr; }
        if (hipDeviceSynchronize() != hipSuccess) return 1;
    }
    auto work = [&](int t) {
        if (hipSetDevice(dev) != hipSuccess) { int z = 0; first_error.compare_exchange_strong(z, 1); return; }
        bool ordered = front == nullptr;
        for (int i = t; i < nslabs && first_error.load() == 0; i += inflight) {
            const long z0 = (long)i * base + std::min<long>(i, rem), nz = base + (i < rem ? 1 : 0);
            std::vector<long> shp(shape, shape + rank);
            shp[0] = nz;
            long at = 0, len = 0;
            int rc;
            {
                ContextLease lease;
                if (!lease.ctx) rc = 1;
                else {
                    hipStream_t stream = lease.ctx->own_stream();
                    // (every lease may be another context with another stream: each call waits; an event that has completed costs nothing)
                    if (stream && !ordered && hipStreamWaitEvent(stream, front, 0) != hipSuccess) { (void)hipGetLastError(); stream = nullptr; }
                    rc = stream ? encode_on_device(*lease.ctx, pipeline, static_cast<const char*>(d_src) + (uint64_t)z0 * per_frame, shp.data(), rank,
                                                   elem_size, static_cast<char*>(d_dst) + (uint64_t)i * (uint64_t)slab_capacity,
                                                   (uint64_t)slab_capacity, &len, nthreads, stream, &at)
                                : 1;
                }
            }
            if (rc) { int z = 0; first_error.compare_exchange_strong(z, rc); return; }
            offsets[i] = (long)((uint64_t)i * (uint64_t)slab_capacity) + at;
            lengths[i] = len;
        }
    };
    // no exception leaves a worker (a thrown std::bad_alloc etc. becomes the call's error code), and the threads are joined on every
    // way out of this function -- they hold references to its locals (round-3 advice)
    auto worker = [&](int t) {
        try { work(t); }
        catch (const std::exception& e) { std::fprintf(stderr, "[sqeazy]\t slab worker: %s\n", e.what()); int z = 0; first_error.compare_exchange_strong(z, 1); }
        catch (...) { int z = 0; first_error.compare_exchange_strong(z, 1); }
    };
    std::vector<std::thread> th;
    struct Joiner { std::vector<std::thread>& t; ~Joiner() { for (auto& x : t) if (x.joinable()) x.join(); } } joiner{th};
    try {
        th.reserve((size_t)inflight);
        for (int t = 1; t < inflight; ++t) th.emplace_back(worker, t);
    } catch (...) {                                                            // (no thread to be had: the call fails, the threads that did start are joined)
        int z = 0; first_error.compare_exchange_strong(z, 1);
    }
    worker(0);
    for (auto& x : th) x.join();
    return first_error.load();
}

int SQYAMD_PipelineEncode_Slabs_UI16_Device(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, int nslabs,
                                            void* d_dst, long slab_capacity, long* offsets, long* lengths, int nthreads, int inflight)
{
    return guarded([&]() -> int {
    return encode_slabs(pipeline, d_src, shape, shape_size, 2, nslabs, d_dst, slab_capacity, offsets, lengths, nthreads, inflight);
    });
}

int SQYAMD_PipelineEncode_Slabs_UI8_Device(const char* pipeline, const void* d_src, const long* shape, unsigned shape_size, int nslabs,
                                           void* d_dst, long slab_capacity, long* offsets, long* lengths, int nthreads, int inflight)
{
    return guarded([&]() -> int {
    return encode_slabs(pipeline, d_src, shape, shape_size, 1, nslabs, d_dst, slab_capacity, offsets, lengths, nthreads, inflight);
    });
}

int SQYAMD_PipelineEncode_Batch_UI16_Device(const char* pipeline, const void* const* d_srcs, const long* shapes, unsigned shape_size, int nvolumes,
                                            void* d_dst, long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
    return encode_batch_device(pipeline, d_srcs, shapes, shape_size, 2, nvolumes, d_dst, slot_capacity, offsets, lengths, nthreads, hip_stream);
    });
}

int SQYAMD_PipelineEncode_Batch_UI8_Device(const char* pipeline, const void* const* d_srcs, const long* shapes, unsigned shape_size, int nvolumes,
                                           void* d_dst, long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
    return encode_batch_device(pipeline, d_srcs, shapes, shape_size, 1, nvolumes, d_dst, slot_capacity, offsets, lengths, nthreads, hip_stream);
    });
}

int SQYAMD_PipelineEncode_BatchStrided_UI16_Device(const char* pipeline, const void* const* d_srcs, const long* shapes, const long* strides, unsigned shape_size,
                                                   int nvolumes, void* d_dst, long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
        return encode_batch_strided_device(pipeline, d_srcs, shapes, strides, shape_size, 2, nvolumes, d_dst, slot_capacity, offsets, lengths, nthreads, hip_stream);
    });
}

int SQYAMD_PipelineEncode_BatchStrided_UI8_Device(const char* pipeline, const void* const* d_srcs, const long* shapes, const long* strides, unsigned shape_size,
                                                  int nvolumes, void* d_dst, long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
        return encode_batch_strided_device(pipeline, d_srcs, shapes, strides, shape_size, 1, nvolumes, d_dst, slot_capacity, offsets, lengths, nthreads, hip_stream);
    });
}

int SQYAMD_PipelineEncode_BatchPacked_UI16_Device(const char* pipeline, const void* const* d_srcs, const long* shapes, const long* strides, unsigned shape_size,
                                                  int nvolumes, void* d_dst, long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads,
                                                  void* hip_stream)
{
    return guarded([&]() -> int {
        return encode_batch_packed_device(pipeline, d_srcs, shapes, strides, shape_size, 2, nvolumes, d_dst, dst_capacity, align, offsets, lengths, total, nthreads,
                                          hip_stream);
    });
}

int SQYAMD_PipelineEncode_BatchPacked_UI8_Device(const char* pipeline, const void* const* d_srcs, const long* shapes, const long* strides, unsigned shape_size,
                                                 int nvolumes, void* d_dst, long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads,
                                                 void* hip_stream)
{
    return guarded([&]() -> int {
        return encode_batch_packed_device(pipeline, d_srcs, shapes, strides, shape_size, 1, nvolumes, d_dst, dst_capacity, align, offsets, lengths, total, nthreads,
                                          hip_stream);
    });
}

int SQYAMD_PipelineEncode_BatchPacked_UI16(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size, int nvolumes, char* dst,
                                           long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads)
{
    return guarded([&]() -> int {
        return encode_batch_packed_from_host(pipeline, srcs, shapes, shape_size, 2, nvolumes, dst, dst_capacity, align, offsets, lengths, total, nthreads);
    });
}

int SQYAMD_PipelineEncode_BatchPacked_UI8(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size, int nvolumes, char* dst,
                                          long dst_capacity, long align, long* offsets, long* lengths, long* total, int nthreads)
{
    return guarded([&]() -> int {
        return encode_batch_packed_from_host(pipeline, srcs, shapes, shape_size, 1, nvolumes, dst, dst_capacity, align, offsets, lengths, total, nthreads);
    });
}

int SQYAMD_PipelineEncode_Batch_UI16(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size, int nvolumes, char* dst,
                                     long slot_capacity, long* offsets, long* lengths, int nthreads)
{
    return guarded([&]() -> int {
    return encode_batch_from_host(pipeline, srcs, shapes, shape_size, 2, nvolumes, dst, slot_capacity, offsets, lengths, nthreads);
    });
}

int SQYAMD_PipelineEncode_Batch_UI8(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size, int nvolumes, char* dst,
                                    long slot_capacity, long* offsets, long* lengths, int nthreads)
{
    return guarded([&]() -> int {
    return encode_batch_from_host(pipeline, srcs, shapes, shape_size, 1, nvolumes, dst, slot_capacity, offsets, lengths, nthreads);
    });
}

int SQYAMD_PipelineEncode_UI16_Cap(const char* pipeline, const char* src, long* shape, unsigned shape_size, char* dst,
                                   long dst_capacity, long* dstlength, int nthreads)
{
    return guarded([&]() -> int {
    return encode_from_host(pipeline, src, shape, shape_size, 2, dst, dstlength, nthreads, std::max(dst_capacity, 0l));
    });
}

int SQYAMD_PipelineEncode_UI8_Cap(const char* pipeline, const char* src, long* shape, unsigned shape_size, char* dst,
                                  long dst_capacity, long* dstlength, int nthreads)
{
    return guarded([&]() -> int {
    return encode_from_host(pipeline, src, shape, shape_size, 1, dst, dstlength, nthreads, std::max(dst_capacity, 0l));
    });
}

int SQYAMD_Decode_UI16_Device(const void* d_src, long srclength, void* d_dst, long dst_capacity, void* hip_stream)
{
    return guarded([&]() -> int {
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_on_device(*lease.ctx, d_src, (uint64_t)std::max(srclength, 0l), d_dst, (uint64_t)std::max(dst_capacity, 0l), 2, static_cast<hipStream_t>(hip_stream));
    });
}

int SQYAMD_Decode_Frames_UI16_Device(const void* d_src, long srclength, long z0, long nz, void* d_dst, long dst_capacity, void* hip_stream)
{
    return guarded([&]() -> int {
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_frames_on_device(*lease.ctx, d_src, (uint64_t)std::max(srclength, 0l), z0, nz, d_dst, (uint64_t)std::max(dst_capacity, 0l), 2,
                                   static_cast<hipStream_t>(hip_stream));
    });
}

int SQYAMD_Decode_Frames_UI8_Device(const void* d_src, long srclength, long z0, long nz, void* d_dst, long dst_capacity, void* hip_stream)
{
    return guarded([&]() -> int {
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_frames_on_device(*lease.ctx, d_src, (uint64_t)std::max(srclength, 0l), z0, nz, d_dst, (uint64_t)std::max(dst_capacity, 0l), 1,
                                   static_cast<hipStream_t>(hip_stream));
    });
}

int SQYAMD_Decode_Frames_UI16(const char* src, long srclength, long z0, long nz, char* dst, long dst_capacity)
{
    return guarded([&]() -> int { return decode_frames_from_host(src, srclength, z0, nz, dst, dst_capacity, 2); });
}

int SQYAMD_Decode_Frames_UI8(const char* src, long srclength, long z0, long nz, char* dst, long dst_capacity)
{
    return guarded([&]() -> int { return decode_frames_from_host(src, srclength, z0, nz, dst, dst_capacity, 1); });
}

int SQYAMD_Decode_Box_UI16_Device(const void* d_src, long srclength, const long* origin, void* d_dst, const long* dst_shape, const long* dst_strides, unsigned rank,
                                  void* hip_stream)
{
    return guarded([&]() -> int { return decode_box_device(d_src, srclength, origin, d_dst, dst_shape, dst_strides, rank, 2, hip_stream); });
}

int SQYAMD_Decode_Box_UI8_Device(const void* d_src, long srclength, const long* origin, void* d_dst, const long* dst_shape, const long* dst_strides, unsigned rank,
                                 void* hip_stream)
{
    return guarded([&]() -> int { return decode_box_device(d_src, srclength, origin, d_dst, dst_shape, dst_strides, rank, 1, hip_stream); });
}

int SQYAMD_Decode_Box_UI16(const char* src, long srclength, const long* origin, const long* extent, unsigned rank, char* dst, long dst_capacity)
{
    return guarded([&]() -> int { return decode_box_from_host(src, srclength, origin, extent, rank, dst, dst_capacity, 2); });
}

int SQYAMD_Decode_Box_UI8(const char* src, long srclength, const long* origin, const long* extent, unsigned rank, char* dst, long dst_capacity)
{
    return guarded([&]() -> int { return decode_box_from_host(src, srclength, origin, extent, rank, dst, dst_capacity, 1); });
}

int SQYAMD_Decode_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, void* const* d_dsts, const long* dst_shapes,
                                    const long* dst_strides, unsigned rank, void* hip_stream)
{
    return guarded([&]() -> int { return decode_boxes_device(d_src, srclength, count, origins, d_dsts, dst_shapes, dst_strides, rank, 2, hip_stream); });
}

int SQYAMD_Decode_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, void* const* d_dsts, const long* dst_shapes,
                                   const long* dst_strides, unsigned rank, void* hip_stream)
{
    return guarded([&]() -> int { return decode_boxes_device(d_src, srclength, count, origins, d_dsts, dst_shapes, dst_strides, rank, 1, hip_stream); });
}

int SQYAMD_Decode_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, char* dst, long dst_capacity)
{
    return guarded([&]() -> int { return decode_boxes_from_host(src, srclength, count, origins, extents, rank, dst, dst_capacity, 2); });
}

int SQYAMD_Decode_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, char* dst, long dst_capacity)
{
    return guarded([&]() -> int { return decode_boxes_from_host(src, srclength, count, origins, extents, rank, dst, dst_capacity, 1); });
}

int SQYAMD_Compare_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const void* const* d_views, const long* view_shapes,
                                     const long* view_strides, unsigned rank, unsigned long long* stats, void* hip_stream)
{
    return guarded([&]() -> int { return compare_boxes_device(d_src, srclength, count, origins, d_views, view_shapes, view_strides, rank, stats, 2, hip_stream); });
}

int SQYAMD_Compare_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const void* const* d_views, const long* view_shapes,
                                    const long* view_strides, unsigned rank, unsigned long long* stats, void* hip_stream)
{
    return guarded([&]() -> int { return compare_boxes_device(d_src, srclength, count, origins, d_views, view_shapes, view_strides, rank, stats, 1, hip_stream); });
}

int SQYAMD_Compare_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views, long views_bytes,
                              unsigned long long* stats)
{
    return guarded([&]() -> int { return compare_boxes_from_host(src, srclength, count, origins, extents, rank, views, views_bytes, stats, 2); });
}

int SQYAMD_Compare_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views, long views_bytes,
                             unsigned long long* stats)
{
    return guarded([&]() -> int { return compare_boxes_from_host(src, srclength, count, origins, extents, rank, views, views_bytes, stats, 1); });
}

int SQYAMD_Project_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op,
                                     void* const* d_outs, const long* out_strides, void* hip_stream)
{
    return guarded([&]() -> int { return project_boxes_device(d_src, srclength, count, origins, extents, rank, axis, op, d_outs, out_strides, 2, hip_stream); });
}

int SQYAMD_Project_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op,
                                    void* const* d_outs, const long* out_strides, void* hip_stream)
{
    return guarded([&]() -> int { return project_boxes_device(d_src, srclength, count, origins, extents, rank, axis, op, d_outs, out_strides, 1, hip_stream); });
}

int SQYAMD_Project_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op, char* out,
                              long out_capacity)
{
    return guarded([&]() -> int { return project_boxes_from_host(src, srclength, count, origins, extents, rank, axis, op, out, out_capacity, 2); });
}

int SQYAMD_Project_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis, int op, char* out,
                             long out_capacity)
{
    return guarded([&]() -> int { return project_boxes_from_host(src, srclength, count, origins, extents, rank, axis, op, out, out_capacity, 1); });
}

int SQYAMD_Bin_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op,
                                 void* const* d_outs, const long* out_strides, void* hip_stream)
{
    return guarded([&]() -> int { return bin_boxes_device(d_src, srclength, count, origins, extents, rank, bins, op, d_outs, out_strides, 2, hip_stream); });
}

int SQYAMD_Bin_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op,
                                void* const* d_outs, const long* out_strides, void* hip_stream)
{
    return guarded([&]() -> int { return bin_boxes_device(d_src, srclength, count, origins, extents, rank, bins, op, d_outs, out_strides, 1, hip_stream); });
}

int SQYAMD_Bin_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, char* out,
                          long out_capacity)
{
    return guarded([&]() -> int { return bin_boxes_from_host(src, srclength, count, origins, extents, rank, bins, op, out, out_capacity, 2); });
}

int SQYAMD_Bin_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const long* bins, int op, char* out,
                         long out_capacity)
{
    return guarded([&]() -> int { return bin_boxes_from_host(src, srclength, count, origins, extents, rank, bins, op, out, out_capacity, 1); });
}

int SQYAMD_Pyramid_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins,
                                     int op, void* const* d_outs, const long* out_strides, void* hip_stream)
{
    return guarded([&]() -> int { return pyramid_boxes_device(d_src, srclength, count, origins, extents, rank, levels, bins, op, d_outs, out_strides, 2, hip_stream); });
}

int SQYAMD_Pyramid_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins,
                                     int op, void* const* d_outs, const long* out_strides, void* hip_stream)
{
    return guarded([&]() -> int { return pyramid_boxes_device(d_src, srclength, count, origins, extents, rank, levels, bins, op, d_outs, out_strides, 1, hip_stream); });
}

int SQYAMD_Pyramid_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, int op,
                              char* out, long out_capacity)
{
    return guarded([&]() -> int { return pyramid_boxes_from_host(src, srclength, count, origins, extents, rank, levels, bins, op, out, out_capacity, 2); });
}

int SQYAMD_Pyramid_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, long levels, const long* bins, int op,
                              char* out, long out_capacity)
{
    return guarded([&]() -> int { return pyramid_boxes_from_host(src, srclength, count, origins, extents, rank, levels, bins, op, out, out_capacity, 1); });
}

int SQYAMD_Histogram_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift,
                                       void* const* d_hists, void* hip_stream)
{
    return guarded([&]() -> int { return histogram_boxes_device(d_src, srclength, count, origins, extents, rank, shift, d_hists, 2, hip_stream); });
}

int SQYAMD_Histogram_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift,
                                      void* const* d_hists, void* hip_stream)
{
    return guarded([&]() -> int { return histogram_boxes_device(d_src, srclength, count, origins, extents, rank, shift, d_hists, 1, hip_stream); });
}

int SQYAMD_Histogram_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, char* out,
                                long out_capacity)
{
    return guarded([&]() -> int { return histogram_boxes_from_host(src, srclength, count, origins, extents, rank, shift, out, out_capacity, 2); });
}

int SQYAMD_Histogram_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int shift, char* out,
                               long out_capacity)
{
    return guarded([&]() -> int { return histogram_boxes_from_host(src, srclength, count, origins, extents, rank, shift, out, out_capacity, 1); });
}

int SQYAMD_Decode_Slabs_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nslabs, void* d_dst, long dst_capacity,
                                    long* frames, int inflight, void* hip_stream)
{
    return guarded([&]() -> int {
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_slabs_on_device(*lease.ctx, d_src, offsets, lengths, nslabs, d_dst, (uint64_t)std::max(dst_capacity, 0l), frames, inflight, 2,
                                  static_cast<hipStream_t>(hip_stream));
    });
}

int SQYAMD_Decode_Slabs_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nslabs, void* d_dst, long dst_capacity,
                                   long* frames, int inflight, void* hip_stream)
{
    return guarded([&]() -> int {
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_slabs_on_device(*lease.ctx, d_src, offsets, lengths, nslabs, d_dst, (uint64_t)std::max(dst_capacity, 0l), frames, inflight, 1,
                                  static_cast<hipStream_t>(hip_stream));
    });
}

int SQYAMD_Decode_Slabs_UI16(const char* src, const long* offsets, const long* lengths, int nslabs, char* dst, long dst_capacity, long* frames)
{
    return guarded([&]() -> int { return decode_slabs_from_host(src, offsets, lengths, nslabs, dst, dst_capacity, frames, 2); });
}

int SQYAMD_Decode_Slabs_UI8(const char* src, const long* offsets, const long* lengths, int nslabs, char* dst, long dst_capacity, long* frames)
{
    return guarded([&]() -> int { return decode_slabs_from_host(src, offsets, lengths, nslabs, dst, dst_capacity, frames, 1); });
}

int SQYAMD_Decode_Batch_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, void* const* d_dsts, const long* dst_capacities,
                                    long* decoded_bytes, void* hip_stream)
{
    return guarded([&]() -> int { return decode_batch_device(d_src, BatchDecodeArgs{offsets, lengths, nblobs, d_dsts, dst_capacities, decoded_bytes}, 2, hip_stream); });
}

int SQYAMD_Decode_Batch_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, void* const* d_dsts, const long* dst_capacities,
                                   long* decoded_bytes, void* hip_stream)
{
    return guarded([&]() -> int { return decode_batch_device(d_src, BatchDecodeArgs{offsets, lengths, nblobs, d_dsts, dst_capacities, decoded_bytes}, 1, hip_stream); });
}

int SQYAMD_Decode_BatchStrided_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, void* const* d_dsts, const long* dst_shapes,
                                           const long* dst_strides, unsigned shape_size, long* decoded_bytes, void* hip_stream)
{
    return guarded([&]() -> int { return decode_batch_strided_device(d_src, offsets, lengths, nblobs, d_dsts, dst_shapes, dst_strides, shape_size, decoded_bytes, 2, hip_stream); });
}

int SQYAMD_Decode_BatchStrided_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, void* const* d_dsts, const long* dst_shapes,
                                          const long* dst_strides, unsigned shape_size, long* decoded_bytes, void* hip_stream)
{
    return guarded([&]() -> int { return decode_batch_strided_device(d_src, offsets, lengths, nblobs, d_dsts, dst_shapes, dst_strides, shape_size, decoded_bytes, 1, hip_stream); });
}

int SQYAMD_Decode_BatchWindow_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, const long* src_origins, void* const* d_dsts,
                                          const long* dst_shapes, const long* dst_strides, unsigned shape_size, long* decoded_bytes, void* hip_stream)
{
    return guarded([&]() -> int {
        return decode_batch_window_device(d_src, offsets, lengths, nblobs, src_origins, d_dsts, dst_shapes, dst_strides, shape_size, decoded_bytes, 2, hip_stream);
    });
}

int SQYAMD_Decode_BatchWindow_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, const long* src_origins, void* const* d_dsts,
                                         const long* dst_shapes, const long* dst_strides, unsigned shape_size, long* decoded_bytes, void* hip_stream)
{
    return guarded([&]() -> int {
        return decode_batch_window_device(d_src, offsets, lengths, nblobs, src_origins, d_dsts, dst_shapes, dst_strides, shape_size, decoded_bytes, 1, hip_stream);
    });
}

int SQYAMD_Compare_BatchWindow_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, const long* src_origins, const void* const* d_views,
                                           const long* view_shapes, const long* view_strides, unsigned shape_size, unsigned long long* stats, void* hip_stream)
{
    return guarded([&]() -> int {
        return compare_batch_window_device(d_src, offsets, lengths, nblobs, src_origins, d_views, view_shapes, view_strides, shape_size, stats, 2, hip_stream);
    });
}

int SQYAMD_Compare_BatchWindow_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs, const long* src_origins, const void* const* d_views,
                                          const long* view_shapes, const long* view_strides, unsigned shape_size, unsigned long long* stats, void* hip_stream)
{
    return guarded([&]() -> int {
        return compare_batch_window_device(d_src, offsets, lengths, nblobs, src_origins, d_views, view_shapes, view_strides, shape_size, stats, 1, hip_stream);
    });
}

int SQYAMD_Update_BatchWindow_UI16_Device(const char* pipeline, const void* d_src, const long* src_offsets, const long* src_lengths, int nblobs, const long* origins,
                                          const void* const* d_wins, const long* win_shapes, const long* win_strides, unsigned shape_size, void* d_dst, long slot_capacity,
                                          long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
        return update_batch_window_device(pipeline, d_src, src_offsets, src_lengths, nblobs, origins, d_wins, win_shapes, win_strides, shape_size, 2, d_dst, slot_capacity,
                                          offsets, lengths, nthreads, hip_stream);
    });
}

int SQYAMD_Update_BatchWindow_UI8_Device(const char* pipeline, const void* d_src, const long* src_offsets, const long* src_lengths, int nblobs, const long* origins,
                                         const void* const* d_wins, const long* win_shapes, const long* win_strides, unsigned shape_size, void* d_dst, long slot_capacity,
                                         long* offsets, long* lengths, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
        return update_batch_window_device(pipeline, d_src, src_offsets, src_lengths, nblobs, origins, d_wins, win_shapes, win_strides, shape_size, 1, d_dst, slot_capacity,
                                          offsets, lengths, nthreads, hip_stream);
    });
}

int SQYAMD_Update_Box_UI16_Device(const char* pipeline, const void* d_src, long srclength, const long* origin, const void* d_view, const long* view_shape,
                                  const long* view_strides, unsigned rank, void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
        return update_box_device(pipeline, d_src, srclength, origin, d_view, view_shape, view_strides, rank, 2, d_dst, dst_capacity, dstlength, nthreads, hip_stream);
    });
}

int SQYAMD_Update_Box_UI8_Device(const char* pipeline, const void* d_src, long srclength, const long* origin, const void* d_view, const long* view_shape,
                                 const long* view_strides, unsigned rank, void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream)
{
    return guarded([&]() -> int {
        return update_box_device(pipeline, d_src, srclength, origin, d_view, view_shape, view_strides, rank, 1, d_dst, dst_capacity, dstlength, nthreads, hip_stream);
    });
}

int SQYAMD_Update_Boxes_UI16_Device(const char* pipeline, const void* d_src, long srclength, long count, const long* origins, const void* const* d_views,
                                    const long* view_shapes, const long* view_strides, unsigned rank, void* d_dst, long dst_capacity, long* dstlength, int nthreads,
                                    void* hip_stream)
{
    return guarded([&]() -> int {
        return update_boxes_device(pipeline, d_src, srclength, count, origins, d_views, view_shapes, view_strides, rank, 2, d_dst, dst_capacity, dstlength, nthreads, hip_stream);
    });
}

int SQYAMD_Update_Boxes_UI8_Device(const char* pipeline, const void* d_src, long srclength, long count, const long* origins, const void* const* d_views,
                                   const long* view_shapes, const long* view_strides, unsigned rank, void* d_dst, long dst_capacity, long* dstlength, int nthreads,
                                   void* hip_stream)
{
    return guarded([&]() -> int {
        return update_boxes_device(pipeline, d_src, srclength, count, origins, d_views, view_shapes, view_strides, rank, 1, d_dst, dst_capacity, dstlength, nthreads, hip_stream);
    });
}

int SQYAMD_Update_Boxes_UI16(const char* pipeline, const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views,
                             long views_bytes, char* dst, long dst_capacity, long* dstlength, int nthreads)
{
    return guarded([&]() -> int { return update_boxes_from_host(pipeline, src, srclength, count, origins, extents, rank, views, views_bytes, dst, dst_capacity, dstlength, 2, nthreads); });
}

int SQYAMD_Update_Boxes_UI8(const char* pipeline, const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, const char* views,
                            long views_bytes, char* dst, long dst_capacity, long* dstlength, int nthreads)
{
    return guarded([&]() -> int { return update_boxes_from_host(pipeline, src, srclength, count, origins, extents, rank, views, views_bytes, dst, dst_capacity, dstlength, 1, nthreads); });
}

int SQYAMD_Decode_Batch_UI16(const char* src, const long* offsets, const long* lengths, int nblobs, char* const* dsts, const long* dst_capacities, long* decoded_bytes)
{
    return guarded([&]() -> int {
        return decode_batch_from_host(src, BatchDecodeArgs{offsets, lengths, nblobs, reinterpret_cast<void* const*>(dsts), dst_capacities, decoded_bytes}, 2);
    });
}

int SQYAMD_Decode_Batch_UI8(const char* src, const long* offsets, const long* lengths, int nblobs, char* const* dsts, const long* dst_capacities, long* decoded_bytes)
{
    return guarded([&]() -> int {
        return decode_batch_from_host(src, BatchDecodeArgs{offsets, lengths, nblobs, reinterpret_cast<void* const*>(dsts), dst_capacities, decoded_bytes}, 1);
    });
}

int SQYAMD_Decode_UI8_Device(const void* d_src, long srclength, void* d_dst, long dst_capacity, void* hip_stream)
{
    return guarded([&]() -> int {
    ContextLease lease;
    if (!lease.ctx) { std::fprintf(stderr, "[sqeazy]\t no usable HIP device\n"); return 1; }
    return decode_on_device(*lease.ctx, d_src, (uint64_t)std::max(srclength, 0l), d_dst, (uint64_t)std::max(dst_capacity, 0l), 1, static_cast<hipStream_t>(hip_stream));
    });
}

void SQYAMD_Profile_Enable(int enable)
{
    g_prof_on.store(enable != 0);
}

void SQYAMD_Profile_Reset(void)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof.clear();
}

const char* SQYAMD_Profile_Get(int i, double* total_ms, long* launches)
{
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (i < 0 || (size_t)i >= g_prof.size()) return nullptr;
    if (total_ms) *total_ms = g_prof[i].ms;
    if (launches) *launches = g_prof[i].launches;
    return g_prof[i].name.c_str();
}

int SQYAMD_Set_Option(const char* name, long value)
{
    std::atomic<long>* o = g_opt.find(name);
    if (!o) return 1;
    if (o == &g_opt.block_parallel_warmup) { if (value < 0 || value > kWarmupMax) return 1; }
    else if (o == &g_opt.transpose_tiles_per_wave) { if (value < 1 || value > 64) return 1; sqy::set_bitswap1_tiles_per_wave(value); }
    else if (o == &g_opt.host_l2_bytes) { if (value < 0 || value > (long)UINT32_MAX) return 1; }
    else if (o == &g_opt.stage_lanes || o == &g_opt.histogram_boxes_merge) { if (value < 0 || value > 2) return 1; }
    else if (o == &g_opt.encode_batch_group_bytes) { if (value < 1 || value > kBatchBytesMax) return 1; }
    else if (o == &g_opt.decode_batch_group_bytes) { if (value < 1 || value > (long)kSlabsGroupBytes) return 1; }
    else if (o == &g_opt.encode_batch_joint_max_bytes) { if (value < 0 || value > kBatchBytesMax) return 1; }
    else if (o == &g_opt.lane_calls || o == &g_opt.lane_backlog_fallbacks || o == &g_opt.lane_blocked_fallbacks) { if (value != 0) return 1; }
    else if (o == &g_opt.parse_lanes) { if (value < 1 || value > sqy::LanePicker::kMaxLanes) return 1; }
    else if (o == &g_opt.call_stamps) {
        if (value != 0 && value != 1) return 1;
        if (value) { std::lock_guard<std::mutex> lock(g_stamps_mu); g_stamps.clear(); g_stamps_next = 0; }      // switching on starts a new record
    }
    else if (o == &g_opt.dedupe_report) {
        if (value != 0 && value != 1) return 1;
        if (value) { std::lock_guard<std::mutex> lock(g_dedupe_report_mu); g_dedupe_report = DedupeReport(); }  // switching on drops the record kept
    }
    else if (value != 0 && value != 1) return 1;
    o->store(value);
    return 0;
}

long SQYAMD_Get_Option(const char* name)
{
    std::atomic<long>* o = g_opt.find(name);
    return o ? o->load() : -1;
}

long SQYAMD_Call_Stamps(long* out, long max_records)
{
    std::lock_guard<std::mutex> lock(g_stamps_mu);
    const size_t have = g_stamps.size();
    if (!out || max_records <= 0) return (long)have;
    const size_t n = std::min<size_t>(have, (size_t)max_records), first = (have < kStampRing ? 0 : g_stamps_next) + (have - n);
    for (size_t i = 0; i < n; ++i) {
        const CallStamps& r = g_stamps[(first + i) % have];
        long* o = out + i * SQYAMD_CALL_STAMP_FIELDS;
        o[0] = r.seq; o[1] = r.lane; o[2] = r.thread;
        for (int k = 0; k < CallStamps::kStamps; ++k) o[3 + k] = r.ns[k];
    }
    return (long)n;
}

long SQYAMD_Dedupe_Report(unsigned long long* keys, unsigned* dup_of, long max)
{
    std::lock_guard<std::mutex> lock(g_dedupe_report_mu);
    const DedupeReport& r = g_dedupe_report;
    if (max > 0 && keys) for (size_t i = 0; i < std::min<size_t>(r.keys.size(), (size_t)max); ++i) keys[i] = r.keys[i];
    if (max > 0 && dup_of) for (size_t i = 0; i < std::min<size_t>(r.dup_of.size(), (size_t)max); ++i) dup_of[i] = r.dup_of[i];
    return (long)r.dup_of.size();
}

void SQYAMD_Release_Workspace(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return;
    std::lock_guard<std::mutex> lock(g_pool_mu);
    for (auto& c : g_pool[dev]) if (!c->busy) c->ws.release_buffers();
}

int SQYAMD_Header_Pipeline(const char* src, long srclength, char* out, long* outlength)
{
    return guarded([&]() -> int {
    if (!src || !outlength || srclength <= 0) return 1;
    const sqy::HeaderInfo h = sqy::header_unpack(src, src + srclength);
    if (!h.valid) return 1;
    const long need = (long)h.pipename.size() + 1;
    const long have = out ? *outlength : 0;
    *outlength = need;
    if (!out) return 0;                          // size query
    if (have < need) return 1;
    std::memcpy(out, h.pipename.c_str(), (size_t)need);
    return 0;
    });
}

int SQYAMD_Header_Build(const char* pipeline, int sizeof_voxel, const long* shape, unsigned shape_size, long encoded_bytes,
                        char* out, long* outlength)
{
    return guarded([&]() -> int {
    if (!pipeline || !shape || !outlength || shape_size == 0 || (sizeof_voxel != 1 && sizeof_voxel != 2) || encoded_bytes < 0) return 1;
    try {
        if (!sqy::Pipeline::supported(pipeline, sizeof_voxel)) return 1;
        const sqy::Pipeline p = sqy::Pipeline::from_string(pipeline, sizeof_voxel);
        std::vector<uint64_t> shp(shape, shape + shape_size);
        // what one encode call can have produced: < 2^31 voxels, every extent too, at most INT_MAX payload bytes (decode refuses anything else)
        const uint64_t nvox = voxel_count(shape, shape_size);
        if (nvox == 0 || nvox >= ((uint64_t)1 << 31) || *std::max_element(shp.begin(), shp.end()) >= ((uint64_t)1 << 31)) return 1;
        if (encoded_bytes > (long)INT_MAX) return 1;
        const std::string hdr = sqy::header_pack(sizeof_voxel, false, shp, p.name(), (uint64_t)encoded_bytes);
        const long need = (long)hdr.size();
        const long have = out ? *outlength : 0;
        *outlength = need;
        if (!out) return 0;                      // size query
        if (have < need) return 1;
        std::memcpy(out, hdr.data(), hdr.size());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "[sqeazy]\t %s\n", e.what());
        return 1;
    }
    });
}

const char* SQYAMD_Version(void) { return "sqeazy_amd 0.1.0 (gfx950, sqy header 0.5.2)"; }

} // extern "C"
