// sqy_pipeline.hpp -- host-side mirror of the reference's pipeline object for the hot path:
// pipeline grammar, per-stage configuration strings, size bounds and the sqy header.
//
// Mirrors (paths relative to /root/reference/src/cpp/src):
//   string_parsers.hpp:285-471        pipeline_parser::to_pairs / minors (with <verbatim> protection)
//   dynamic_pipeline.hpp:137-226      from_string / can_be_built_from
//   dynamic_pipeline.hpp:476-503      name()
//   dynamic_pipeline.hpp:866-890      max_encoded_size
//   sqeazy_header.hpp:146-193,294-344 header pack / unpack
//   encoders/lz4.hpp:58-188           lz4 parameter logic, config string, chunking, size bound
//   sqeazy_algorithms.hpp:14-22       thread-count clamp
#ifndef SQY_PIPELINE_HPP_
#define SQY_PIPELINE_HPP_

#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "sqy_batch_window.hpp"

namespace sqy {

typedef std::vector<std::pair<std::string, std::string>> pairs_t;

// split on `sep` outside <verbatim>...</verbatim>; returns {} for a malformed (unbalanced) string
std::vector<std::string> split_outside_verbatim(const std::string& s, const std::string& sep, bool* ok = nullptr);
pairs_t parse_pairs(const std::string& pipeline);
std::map<std::string, std::string> parse_minors(const std::string& cfg);

enum class StageKind { diff3x3x1, bitswap1, bitshuffle, frame_shuffle, raster_reorder, zcurve_reorder, tile_shuffle, quantiser, lz4, pass_through,
                       rmestbkrd, rmbkrd_neighbor5, unsupported };

struct Lz4Params {
    int accel = 1;
    uint32_t blocksize_kb = 256, framestep_kb = 256, n_chunks = 0;
    int block_id = 5;                       // LZ4F blockSizeID 4..7
    explicit Lz4Params(const std::string& cfg = "");
    std::string config() const;
    uint64_t block_bytes() const;
    uint64_t bytes_per_chunk(uint64_t nbytes) const;                       // lz4.hpp:146-156
    uint64_t max_encoded_size(uint64_t nbytes, unsigned nthreads) const;   // lz4.hpp:166-188
    static uint64_t compress_bound(uint64_t src, int block_id);            // LZ4F_compressBound, autoFlush = 0
};

// ---- block-linked LZ4 frames (lz4::encode_serial, encoders/lz4_utils.hpp:99-173) ----
// One entry per LZ4 block in stream order; same layout as sqy::Lz4Block (sqy_kernels.h), which the kernels read.
struct Lz4BlockPlan {
    uint64_t start;          // byte offset of the block in the stream
    uint32_t n;              // bytes
    uint32_t flags;          // bit 0: opens a frame (fresh LZ4 stream), bit 1: closes it
    int64_t low_in, low_dict;   // liblz4's lowLimit for matches that start inside the block / in the history in front of it
};
struct Lz4Plan {
    std::vector<Lz4BlockPlan> blocks;
    std::vector<uint32_t> frame_first;      // frame f = blocks [frame_first[f], frame_first[f+1])
    uint32_t max_block = 0;
    bool ok = true;                         // false: a case liblz4 would run in a mode the kernels do not model
};
// What liblz4 1.9.3's frame layer does with `total` bytes under sqeazy's preferences (block-linked, autoFlush 0, stableSrc 0):
// serial = true : ONE frame, LZ4F_compressUpdate every `step` bytes (encode_serial, nthreads == 1)
// serial = false: one frame per `step` bytes, each fed by a single update (encode_parallel -> encode_serial per chunk)
Lz4Plan lz4_plan_blocks(uint64_t total, uint64_t step, uint64_t block_bytes, bool serial);

// ---- encode planning: every layout decision of the LZ4 stage and of the stages that prepare its input, stated once ----
// How `total` bytes in front of the LZ4 stage become frames (lz4.hpp:227-234), and liblz4's acceleration for them
//   chunked: one frame of one LZ4 block per chunk, every chunk independent | serial: nthreads == 1 and more than one chunk, ONE block-linked
//   frame fed a chunk at a time | linked_chunks: one block-linked frame per chunk, chunks of several LZ4 blocks
enum class Lz4LayoutKind { chunked, serial, linked_chunks };
struct Lz4EncodeLayout {
    uint64_t chunk = 1, nchunks = 0;        // (lz4_decode_geometry's)
    Lz4LayoutKind kind = Lz4LayoutKind::chunked;
    // LZ4F turns a negative compression level -k into acceleration k + 1 (lz4frame.c, LZ4F_compressBlock),
    // LZ4_compress_fast_continue caps it at 65537 (lz4.c, LZ4_ACCELERATION_MAX)
    uint32_t accel = 1;
    bool chunked() const { return kind == Lz4LayoutKind::chunked; }
};
Lz4EncodeLayout lz4_encode_layout(const Lz4Params& p, uint64_t total, unsigned nthreads);

// ---- batch encode (SQYAMD_PipelineEncode_Batch_*): many volumes, one launch per kernel ----
// One entry of a group's joint chunk table; same layout as sqy::Lz4BatchChunk (sqy_kernels.h), which the kernels read.
struct Lz4BatchChunkPlan {
    uint64_t off;            // where the chunk starts in the group's stream workspace
    uint32_t n;              // bytes (the last chunk of a volume may be short, wherever it sits in the table)
    uint32_t vol;            // the volume it belongs to (index into the batch)
    uint32_t slot;           // its scratch slot: compressed bytes at scratch + slot * scratch_stride
    uint32_t pad = 0;
};
// The volumes that share one launch of every kernel.  Volume vols[j]'s LZ4 input (its stream) lies at stream_at[j] of the stream
// workspace (16-byte aligned, stream_bytes in all) and is cut into the table entries [first_chunk[j], first_chunk[j + 1]).
struct Lz4BatchGroup {
    std::vector<uint32_t> vols;                 // ascending
    std::vector<uint64_t> stream_at;
    std::vector<uint32_t> first_chunk;          // vols.size() + 1 entries
    std::vector<Lz4BatchChunkPlan> chunks;      // the joint chunk table, volume by volume, stream order inside a volume
    uint64_t stream_bytes = 0;
    uint64_t scratch_stride = 0;                // the largest chunk, rounded up to 16 bytes
    uint32_t max_chunk = 0;
};
struct Lz4BatchPlan {
    std::vector<int32_t> group_of;              // per volume: its group, -1: not joint-eligible (the single-call path takes it)
    std::vector<Lz4BatchGroup> groups;
};
// totals[i]: the bytes in front of the LZ4 stage for volume i (> 0: empty volumes are refused before planning).  A volume is
// joint-eligible when its layout (lz4_encode_layout) is `chunked` with acceleration 1 and totals[i] <= joint_max.  Eligible volumes are
// dealt to groups in order; a group is closed when the next volume would take its streams past group_bytes (a group holds at least
// one volume, so a volume larger than the bound gets a group of its own).  extra_bytes: workspace every eligible volume takes besides
// its stream (the quantised form's tables); it counts against group_bytes with the stream, not against joint_max.
Lz4BatchPlan lz4_batch_plan(const Lz4Params& p, const std::vector<uint64_t>& totals, unsigned nthreads, uint64_t group_bytes, uint64_t joint_max,
                            uint64_t extra_bytes = 0);
// Which joint form a pipeline takes in a batch -- the stages in front of the LZ4 stage that the group's kernels do for all volumes at once:
//   none: every volume through the single-call path | lz4: the stream is the volume | bitswap1_lz4: the batched transposer |
//   quantiser_bitswap1_lz4: 16-bit voxels, the quantiser with the default weighting (no weighting_function) and the decode LUT in the
//   header (no decode_lut_path) -- histograms, LUTs, look-up and transpose batched, one byte per voxel in front of the LZ4 stage
enum class EncodeBatchForm : uint8_t { none, lz4, bitswap1_lz4, quantiser_bitswap1_lz4 };
struct Pipeline;
EncodeBatchForm encode_batch_form(const Pipeline& pipe, int elem_size);
// the quantised form's tables per volume: histogram (65536 x 4 bytes), encode LUT (65536 bytes), decode LUT (256 x 2 bytes)
constexpr uint64_t kQuantiserBatchHistoBytes = 65536 * 4, kQuantiserBatchLutBytes = 65536, kQuantiserBatchDecodeBytes = 256 * 2,
                   kQuantiserBatchTableBytes = kQuantiserBatchHistoBytes + kQuantiserBatchLutBytes + kQuantiserBatchDecodeBytes;
// the bytes in front of the LZ4 stage for a volume of `voxels` voxels, and what lz4_batch_plan takes as extra_bytes
uint64_t encode_batch_stream_bytes(EncodeBatchForm form, uint64_t voxels, int elem_size);
uint64_t encode_batch_extra_bytes(EncodeBatchForm form);

// ---- packed batch encode (SQYAMD_PipelineEncode_BatchPacked_*): the blobs back to back in one buffer ----
// The placement rule, stated once (lz4_batch_place_kernel computes the same numbers for the volumes of a group).  Volume j of lengths[j]
// bytes lies at at[j]: the first one at base + gaps[0], every later one at the end of the one before it rounded up to `align`, plus
// gaps[j] -- the room in front of volume j that others take (a multiple of align where the caller wants at[j] aligned; gaps empty: none).
// end: where the last volume ends (not rounded; base for no volume) -- what a capacity must be for every volume to fit.  first_unfit: the
// first volume with at[j] + lengths[j] > capacity, lengths.size() when all fit; volumes behind it are placed as if it had fitted.  All
// arithmetic in 64 unsigned bits.  ok = false (at empty, end 0, first_unfit 0): align no power of two in [1, kPackedAlignMax], a gap table
// of another size than lengths, or a place, end or rounded end above 2^63 - 1 -- refused, never wrapped.
constexpr uint64_t kPackedAlignMax = 65536;
struct PackedPlaces { std::vector<uint64_t> at; uint64_t end = 0; size_t first_unfit = 0; bool ok = false; };
PackedPlaces packed_places(const std::vector<uint64_t>& lengths, const std::vector<uint64_t>& gaps, uint64_t align, uint64_t base, uint64_t capacity);

// ---- strided views (SQYAMD_PipelineEncode_BatchStrided_*, SQYAMD_Decode_BatchStrided_*): a volume cut out of a larger allocation ----
// Z x Y x X voxels, x innermost with stride 1, rows sy voxels apart, frames sz voxels apart.  dense: sy = X and sz = Y X, the view is one
// run of Z Y X voxels (Z = Y = 1 then: a dense view is folded into one row)
struct BatchView { uint64_t Z, Y, X, sz, sy; bool dense; };
// A caller's view of `rank` dimensions (1 .. 3, outermost first; ranks 1 and 2 are padded with leading 1s), strides in voxels, nullptr: the
// dense ones.  false: rank 0 or above 3, an extent below 1, an innermost stride other than 1, a stride below 1, a dimension that overlaps
// the next one's reach (stride[k] < shape[k + 1] * stride[k + 1]), or a reach (shape x stride) past 2^62 voxels.  The view is folded where
// the strides allow: rows that follow each other without a gap (sy = X) become one row, frames without a gap (sz = Y sy) one frame -- so
// a tile that spans whole rows of its parent has fewer, longer rows.
bool admit_view(const long* shape, const long* strides, unsigned rank, BatchView* view);
// lz4_batch_plan for views: pack_bytes[i] is what volume i's packed copy takes in the group's workspace (0: read in place); it counts
// against group_bytes with the stream and extra_bytes.  All zeros: lz4_batch_plan's result.
Lz4BatchPlan lz4_batch_plan_views(const Lz4Params& p, const std::vector<uint64_t>& totals, const std::vector<uint64_t>& pack_bytes, unsigned nthreads,
                                  uint64_t group_bytes, uint64_t joint_max, uint64_t extra_bytes = 0);
// a view job of the pack, unpack and strided transposer launches (sqy::BatchViewJob, sqy_kernels.h)
constexpr uint64_t kBatchViewJobBytes = 56;

// ---- windows (SQYAMD_Decode_BatchWindow_*): a box of a blob decoded into a view of the box's shape ----
// The blob's shape bZ x bY x bX, the window's first voxel (oz, oy, ox) in it and its extent Z x Y x X, all padded to three dimensions with
// leading 1s (origins: 0s).  whole: the window is the blob
struct BatchWindow { uint64_t bZ, bY, bX, oz, oy, ox, Z, Y, X; bool whole; };
// A caller's window of `rank` dimensions (outermost first) inside a blob whose header gives header_shape; origin nullptr: all zeros.
// false: rank 0 or above 3, a header of another rank, an origin below 0, an extent below 1, or origin + extent past the header's shape
// (a sum that overflows `long` is past it)
bool admit_window(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, BatchWindow* out);
// the clip's geometry of a window and the destination's two pitches
inline WindowGeometry window_geometry(const BatchWindow& w, uint64_t sz, uint64_t sy) { return WindowGeometry{w.bY, w.bX, w.oz, w.oy, w.ox, w.Z, w.Y, w.X, sz, sy}; }
// A window rebased onto a buffer that holds only its own frames: the blob's first dimension shrinks to the window's and the window begins
// at its first frame.  The frames are the HEADER's first dimension: of a header of rank 2 the rows, of rank 1 the voxels
inline BatchWindow window_in_own_frames(BatchWindow w, unsigned rank)
{
    if (rank == 3) { w.bZ = w.Z; w.oz = 0; }
    else if (rank == 2) { w.bY = w.Y; w.oy = 0; }
    else { w.bX = w.X; w.ox = 0; }
    return w;
}
// the smallest shape that holds the box [origin, origin + extent): what an admit_* is given where there is no header yet (origins not
// below 0; an extent below 1 counts as 0 and is refused by the admit_*; both below 2^63: no wrap)
inline std::vector<uint64_t> smallest_holding_shape(const long* origin, const long* extent, unsigned rank)
{
    std::vector<uint64_t> shape(rank);
    for (unsigned k = 0; k < rank; ++k) shape[k] = (uint64_t)origin[k] + (uint64_t)(extent[k] > 0 ? extent[k] : 0);
    return shape;
}
// Outputs back to back in one buffer: at[i] the first byte of output i, at.back() the bytes of all (bytes.size() + 1 entries; the callers'
// outputs are no larger than a volume and fewer than 2^31: no wrap).  false: more than `capacity` bytes (a capacity below 0 holds nothing)
inline bool output_offsets(const std::vector<uint64_t>& bytes, long capacity, std::vector<uint64_t>* at)
{
    at->assign(bytes.size() + 1, 0);
    for (size_t i = 0; i < bytes.size(); ++i) (*at)[i + 1] = (*at)[i] + bytes[i];
    return at->back() <= (uint64_t)(capacity > 0 ? capacity : 0);
}
// a window job of the window copy and the windowed transposer (sqy::BatchWindowJob, sqy_kernels.h)
constexpr uint64_t kBatchWindowJobBytes = 112;
// The tables of one window launch, one upload: njobs jobs at 0 | tiles_at (16-byte aligned): njobs + 1 words of prefix sums | total
struct BatchWindowLayout { uint64_t tiles_at = 0, total = 0; };
BatchWindowLayout batch_window_layout(uint64_t njobs, uint64_t job_bytes = kBatchWindowJobBytes);
// ---- the compare of a window with its view (SQYAMD_Compare_BatchWindow_*) ----
// a job of the compare launches (sqy::BatchCompareJob, sqy_kernels.h: a window job and its record); the tables have the window launches'
// layout with jobs of this size.  A record: kCompareFields 64-bit words per blob, records side by side in one workspace buffer
constexpr uint64_t kBatchCompareJobBytes = 128;
constexpr uint64_t kCompareFields = 8, kCompareViewMin = 6;

// ---- batch decode (SQYAMD_Decode_Batch_*): many blobs, one launch per kernel ----
// What the planner knows of blob i: the bytes its LZ4 stage decodes to, the LZ4 block size, whether it may take the joint path at all
// (the last stage lz4, chunk <= block_bytes), and what follows the LZ4 decode --
//   stages: its remaining inverses, blob by blob | planes: `bitswap1->lz4`, one job of the batched inverse transposer (len voxels) |
//   plain: `lz4`, one job of the batched copy (len = total bytes) |
//   quantised: `quantiser->bitswap1->lz4`, one job of the batched inverse transposer with the look-up (len voxels, total = len bytes) |
//   diff_planes, diff_plain: `diff3x3x1->bitswap1->lz4`, `diff3x3x1->lz4` of 16-bit voxels in the chain geometry (Z x Y x X = len voxels,
//   chain_columns of a row through the chain): one job of the batched diff inverse; diff_planes: one of the inverse transposer in front
enum class DecodeBatchForm : uint8_t { stages, planes, plain, quantised, diff_planes, diff_plain };
struct DecodeBatchBlob {
    uint64_t total = 0, block_bytes = 0, len = 0;
    bool eligible = false;
    DecodeBatchForm form = DecodeBatchForm::stages;
    uint32_t Z = 0, Y = 0, X = 0, chain_columns = 0;    // the diff forms only
};
constexpr uint64_t kBatchTileVoxels = 256 * 128;        // a workgroup of the batched transposers and of the batched copy: 256 threads x 128 voxels
// the batched diff inverse: a workgroup decodes up to kDiffChainFrames frames of a strip of kDiffStripRows rows (the kernels' DDK_K, DDK_R)
constexpr uint32_t kDiffStripRows = 32, kDiffChainFrames = 8;
// A launch's job list and tile table: jobs[j] is a blob, its tiles are [first_tile[j], first_tile[j + 1]) (max(1, ceil(len / tile)) each)
struct DecodeBatchTiles { std::vector<uint32_t> jobs, first_tile; uint32_t ntiles = 0; };
// The diff blobs of a group (both forms).  Job j's residual volume lies at res_at[j] of the workspace: its LZ4 output (diff_plain), or a
// region of its own behind that, where the inverse transposer puts it (diff_planes).  The chain launches: job j's strips are
// [first_strip[j], first_strip[j + 1]) (ceil(Y / kDiffStripRows) each), step s covers frames [1 + s K, 1 + (s + 1) K) of every job that
// has them (frames 1 .. min(X, Z) - 1 go through the chain), `steps` of them.  The launch for everything else -- frame 0, the frames that
// cannot change, the columns right of the chain -- has tiles of kBatchTileVoxels voxels: first_tile.  max_columns: the widest chain.
struct DecodeBatchDiff {
    std::vector<uint32_t> jobs, first_strip, first_tile;
    std::vector<uint64_t> res_at;
    uint32_t nstrips = 0, ntiles = 0, steps = 0, max_columns = 0;
};
// The blobs that share one launch of every kernel: blob blobs[j]'s LZ4 output lies at out_at[j] of the group's workspace (256-byte
// aligned, out_bytes in all -- a diff_planes blob's residual volume behind its LZ4 output included); planes (the planes blobs, and the
// diff_planes ones, whose voxels go to the workspace), plain, quantised: the tables of the batched launches behind the LZ4 decode; diff
struct DecodeBatchGroup {
    std::vector<uint32_t> blobs;                // ascending
    std::vector<uint64_t> out_at;
    uint64_t out_bytes = 0, block_bytes = 0;
    DecodeBatchTiles planes, plain, quantised;
    DecodeBatchDiff diff;
};
struct DecodeBatchPlan {
    std::vector<int32_t> group_of;              // per blob: its group, -1: not joint-eligible (the single-call path takes it)
    std::vector<DecodeBatchGroup> groups;
};
// Eligible blobs are dealt to groups in order; a group is closed when the next blob would take its workspace (every blob's LZ4 output
// rounded up to 256 bytes, as much again for a diff_planes blob) past group_bytes or has another block size.  A group holds at least one
// blob, so a blob larger than the bound gets a group of its own.  dropped (optional, one flag per blob): blobs the frame ranking refused
// -- they keep their place in the group and in the workspace but get no job in any table.
DecodeBatchPlan decode_batch_plan(const std::vector<DecodeBatchBlob>& blobs, uint64_t group_bytes, const std::vector<uint8_t>* dropped = nullptr);

// ---- window update (SQYAMD_Update_BatchWindow_*): old blob + a window's new voxels -> new blob ----
// Every old blob gets a place in ONE workspace buffer, place_at[i] on the 256-byte grid, raw_bytes[i] long (`bytes` in all): its voxels
// decoded dense -- or, for a blob that takes the fused way, its LZ4 output, the plane stream of just as many bytes.
// keep_planes[i]: the batch decode is asked to stop behind blob i's LZ4 stage IF it finds the blob to be DecodeBatchForm::planes on its
// joint path.  That is asked where the new blob can be made from patched planes: the option (fused_on: batch_update_fused and both
// joint options), the new pipeline in the form bitswap1_lz4, and the volume in a group of the encode's plan (encode_group_of[i] >= 0).
struct UpdateBatchPlan {
    std::vector<uint8_t> keep_planes;
    std::vector<uint64_t> place_at;
    uint64_t bytes = 0;
};
UpdateBatchPlan update_batch_plan(const std::vector<uint64_t>& raw_bytes, EncodeBatchForm new_form, const std::vector<int32_t>& encode_group_of, bool fused_on);
// What became of blob i: patched (its place holds the old plane stream, the encode group's patch launch reads it and the window's view)
// only if the decode was asked, found the planes form and kept the blob on the joint path to the end; otherwise its place holds the
// voxels, the call's ONE paste launch writes the window into them and the encode reads them as a dense volume
inline bool update_blob_patched(bool keep_planes, DecodeBatchForm old_form, bool decoded_jointly)
{
    return keep_planes && old_form == DecodeBatchForm::planes && decoded_jointly;
}
// Whether blob i's LZ4 output is what its place holds -- planned_form: the form the batch decode plans it in, `plain` for an `lz4` blob
// (the volume) and for a blob that keeps its planes (the plane stream).  A decode group whose members ALL are such blobs decodes straight
// into the places, which lie in one buffer, and launches nothing behind its LZ4 decode; any other group keeps the workspace and its
// launches, a batched copy for such members (the rule of a slab set's group).  fused_on as above: off, no group does.
inline bool update_lz4_into_place(bool fused_on, DecodeBatchForm planned_form) { return fused_on && planned_form == DecodeBatchForm::plain; }
inline bool update_group_into_places(const std::vector<uint32_t>& members, const std::vector<uint8_t>& lz4_into_place)
{
    for (uint32_t b : members) if (!lz4_into_place[b]) return false;
    return !members.empty();
}
// a job of the patch launch (sqy::BatchPatchJob, sqy_kernels.h); its tables have the window launches' layout (batch_window_layout)
constexpr uint64_t kBatchPatchJobBytes = 112;

// The slab set's groups (SQYAMD_Decode_Slabs_*): joint blob j decodes `total` bytes in LZ4 blocks of block_bytes.  The blobs are dealt to
// groups in order; a group is closed when the next blob would take its LZ4 output (every blob's rounded up to 256 bytes) past group_bytes,
// when it holds `inflight` blobs (inflight <= 0: no bound on the count), or when the next blob has another block size.  A group holds at
// least one blob.  The groups hold indices into `joint`.
struct SlabJointBlob { uint64_t total = 0, block_bytes = 0; };
std::vector<std::vector<size_t>> decode_slab_groups(const std::vector<SlabJointBlob>& joint, uint64_t group_bytes, int inflight);

// ---- device tables of the batch and slab-set drivers: byte offsets into ONE buffer each, in ascending order, each region ending where the
// next begins (but for the padding in front of an aligned one), `total` the end of the last region.  The element sizes are those of the
// kernels' structs (sqy_kernels.h), which sqy_capi.cpp pins with static_asserts ----
constexpr uint64_t kBitswap1JobBytes = 24, kDiffBatchJobBytes = 32, kLz4JointPartBytes = 64, kLz4BatchChunkBytes = 24, kLz4BatchVolumeBytes = 48;
constexpr uint64_t kLz4BlockIndexBytes = 16;            // an entry of a block index (blk, jblk) and of the frame output table (jout)
constexpr uint64_t kDecodeTableAlign = 256, kEncodeTableAlign = 16;

// The ranking workspace of a decode group (Workspace::slabs_index).  Per blob, 256-byte aligned each: the ranking's scratch (scratch_bytes:
// lz4_frame_rank_scratch_bytes of its chunks) | its block index (max_blocks entries) | its frame starts (max_blocks + 2 words); then
// counts_at: 16 words per blob | flag_at: the group's error flag (64 bytes) | desc_at: launch_lz4_frame_rank_batch's descriptors
struct DecodeRankBlob { uint64_t scratch_bytes = 0, max_blocks = 0; };
struct DecodeRankLayout {
    struct Blob { uint64_t scratch_at = 0, blk_at = 0, frame_first_at = 0; };
    std::vector<Blob> blobs;
    uint64_t counts_at = 0, flag_at = 0, desc_at = 0, total = 0;
};
DecodeRankLayout decode_rank_layout(const std::vector<DecodeRankBlob>& blobs, uint64_t desc_bytes);

// The joint decode tables of a group (Workspace::slabs_joint): parts_at: an Lz4JointPart per blob | maps_at: the frame_shuffle maps | jblk_at,
// jff_at, jout_at: the joint index of `nframes` frames (16 bytes, a word + 1, 16 bytes per frame).  The first upload_bytes are the host's
// (parts and maps), the rest is built on the device.  A batch (batch != nullptr) has behind them what the launches that follow the LZ4
// decode read, one upload of jobs_bytes at jobs_upload_at; per job family its job array at jobs_at (Bitswap1Job, the diff family's
// DiffBatchJob), njobs + 1 words of prefix sums at tiles_at (first_tile; diff: first_strip) and at extra_at
//   quantised: a decode LUT of 512 bytes per job | diff: its second prefix table (first_tile) | planes, plain: nothing
struct DecodeJointLayout {
    uint64_t parts_at = 0, maps_at = 0, jblk_at = 0, jff_at = 0, jout_at = 0, upload_bytes = 0;
    struct Family { uint64_t jobs_at = 0, tiles_at = 0, extra_at = 0; } planes, plain, quantised, diff;      // (as DecodeBatchGroup names them)
    uint64_t jobs_upload_at = 0, jobs_bytes = 0, total = 0;
};
DecodeJointLayout decode_joint_layout(uint64_t nparts, uint64_t map_bytes, uint64_t nframes, const DecodeBatchGroup* batch = nullptr);

// The tables of an encode batch group, 16-byte aligned each.  What the host writes, in the pinned staging area and in Workspace::batch_tables
// alike: table_at: the chunk table | volof_at: a word per chunk | jobs_at: a Bitswap1Job per volume | tiles_at: nvols + 1 words | vols_at:
// an Lz4BatchVolume each | text_at: text_bytes of header text -- `upload` bytes in all.  Behind them in batch_tables what the kernels hand
// each other: csize_at, redo_at (nchunks + 1 words), foff_at (8 bytes a chunk), vinfo_at (16 bytes a volume); `tables` bytes in all.  Behind
// them in the staging area, at decode_at, a quantised group's decode LUTs come back (512 bytes a volume); staging_bytes in all.  A
// quantised group knows its text only after its first round trip: it is laid out for the worst case, kBatchHeaderTextMax bytes a volume.
constexpr uint64_t kBatchHeaderTextMax = 4000;          // prefix + suffix of one volume's header
struct EncodeBatchLayout {
    uint64_t table_at = 0, volof_at = 0, jobs_at = 0, tiles_at = 0, vols_at = 0, text_at = 0, upload = 0;
    uint64_t csize_at = 0, redo_at = 0, foff_at = 0, vinfo_at = 0, tables = 0;
    uint64_t decode_at = 0, staging_bytes = 0;
};
EncodeBatchLayout encode_batch_layout(uint64_t nchunks, uint64_t nvols, bool quantised, uint64_t text_bytes);

// Frames in place: a 16-bit bitswap1 in front of lz4 writes chunk k of the plane stream into the destination at body0 + k * in_stride,
// where it is the body of the stored frame it may become -- kLz4FrameHead bytes (frame header 7, block size field 4) in front, the end
// mark behind: kLz4FrameGap bytes between two chunks.  t0 (>= header_max, the longest sqy header) is where frame 0 begins.
constexpr uint64_t kLz4FrameHead = 7 + 4, kLz4FrameGap = kLz4FrameHead + 4;
struct Lz4InplacePlan { bool on = false; uint64_t chunk = 0, t0 = 0, in_stride = 0, body0 = 0; };     // (all 0 when off)
// on: piece hashes offered and a duplicate search behind them (lz4_dedupe_layout), lz4 the last stage, a power-of-two chunk, a caller who
// takes the blob where it ends up, and room in the destination (dst_mod16: its address modulo 16 -- body0 lands on a 16-byte boundary)
Lz4InplacePlan lz4_inplace_plan(const Lz4EncodeLayout& lay, uint64_t piece_hash_words, bool lz4_is_last, bool takes_offset, unsigned dst_mod16,
                                uint64_t capacity, uint64_t header_max);
// words per chunk of the noise digest a frames-in-place call gets (probes of a search that starts with the chunk and never finds anything,
// liblz4's step schedule, from probe 961 on); 0 = none: the option off, a chunk size without one, a plane segment (segment_bytes) that is
// no whole number of chunks, or not liblz4's plain search behind it (accel < 0)
uint32_t lz4_noise_digest_words(const Lz4Params& p, const Lz4EncodeLayout& lay, bool option_on, uint64_t segment_bytes);

// The duplicate-chunk search's workspace (one buffer), byte offsets in ascending order, each region ending where the next begins: bitswap1's
// piece hashes at 0 | work_at: a key per chunk | tab_key_at, tab_val_at: the hash table's keys and values (`table` slots) | dup_at: dup_of |
// holes_at: the holes map (frames in place: which 1 KiB pieces the transpose left unwritten) | total
struct Lz4DedupeLayout { uint64_t table = 0, work_at = 0, tab_key_at = 0, tab_val_at = 0, dup_at = 0, holes_at = 0, total = 0; };     // total 0: no search
// the search runs on piece hashes (piece_hash_words of them, 0: none offered) of a chunked layout of more than one chunk of whole KiB
Lz4DedupeLayout lz4_dedupe_layout(const Lz4EncodeLayout& lay, uint64_t piece_hash_words);
// Who empties the search's table (keys 0, values ~0) and the dense list's counter of a single-volume encode call, in front of the key table:
//   fills       no frames in place: launch_lz4_dedupe's two fill dispatches behind the transpose
//   kernel      frames in place: launch_lz4_dedupe_clear in front of the transpose
//   transposer  frames in place on the library's lanes: the transposer's own launch (Bitswap1Clear: table_at = tab_key_at, key_bytes and
//               bytes of the keys and of keys + values) -- the clear launch would sit on the one lane every call's transpose goes through.
//               A call that stays on its caller's stream keeps the kernel, and so does a table the transposer's stores do not fit
//               (never one that lz4_dedupe_layout laid out: 64 slots and more, 8-byte aligned, values right behind the keys)
struct Lz4TableClearPlan {
    enum Who { fills, kernel, transposer } who = fills;
    uint64_t table_at = 0;
    uint32_t key_bytes = 0, bytes = 0;
};
Lz4TableClearPlan lz4_table_clear_plan(const Lz4DedupeLayout& d, bool frames_in_place, bool on_lanes);
// The transposer's stores of that clear (the kernel and tests/sanitize/table_clear_test.cpp call these two).  The table starts behind a
// key per chunk, 8 bytes each, so it may begin and end 8 bytes off a 16-byte boundary: `head` bytes (0 or 8) in front of the first whole
// 16-byte vector, nvec vectors at head + 16 i, and what is left from tail_at on (== bytes: nothing), head and tail as one 8-byte store each.
#if defined(__HIP__) || defined(__HIPCC__)
#define SQY_PIPE_HD __host__ __device__
#else
#define SQY_PIPE_HD
#endif
struct Lz4TableClearStores { uint32_t head, nvec, tail_at; };
SQY_PIPE_HD inline Lz4TableClearStores lz4_table_clear_stores(uint64_t table_address, uint32_t bytes)
{
    Lz4TableClearStores s;
    s.head = (16u - (uint32_t)(table_address & 15u)) & 15u;
    s.nvec = (bytes - s.head) >> 4;
    s.tail_at = s.head + (s.nvec << 4);
    return s;
}
// the dword at byte `off` of the table: a key's half (0) or a value (~0)
SQY_PIPE_HD inline uint32_t lz4_table_clear_dword(uint32_t off, uint32_t key_bytes) { return off < key_bytes ? 0u : 0xffffffffu; }

// ---- a box written into one large blob (SQYAMD_Update_Box_*): the splice of old LZ4 frames and new ones into one blob ----
// Frame f of the new blob is either REPLACED -- chunk k = slot_of[f] of the selection parsed again: csize[k] compressed bytes, 0 when
// the chunk's n bytes are stored, as lz4_batch_gather writes a frame -- or the OLD frame, copied as it stands: the frame index names its
// one block (data offset in the payload, size field with the raw bit), the frame's span is [data offset - kLz4FrameHead, data offset +
// size + 4).  The kernels (lz4_splice_scan_kernel, lz4_splice_gather_kernel) and the host (lz4_splice_plan,
// tests/sanitize/update_box_test.cpp) compute every number with the functions below.
constexpr uint32_t kSpliceOldFrame = 0xffffffffu;       // slot_of[f] of a frame that is carried over
constexpr uint64_t kSpliceDone = 1, kSpliceNoRoom = 2, kSplicePayloadTooLong = 3, kSpliceBadIndex = 4;
SQY_PIPE_HD inline uint64_t lz4_splice_new_frame_bytes(uint32_t csize, uint32_t n) { return kLz4FrameHead + (csize ? csize : n) + 4; }
SQY_PIPE_HD inline uint64_t lz4_splice_old_frame_bytes(uint32_t size_field) { return kLz4FrameHead + (size_field & 0x7fffffffu) + 4; }
// an old frame's span lies inside the old payload of src_payload bytes
SQY_PIPE_HD inline bool lz4_splice_old_frame_ok(uint64_t data_off, uint32_t size_field, uint64_t src_payload)
{
    return data_off >= kLz4FrameHead && data_off <= src_payload && (uint64_t)(size_field & 0x7fffffffu) + 4 <= src_payload - data_off;
}
SQY_PIPE_HD inline uint32_t decimal_digits(uint64_t v) { uint32_t nd = 0; do { ++nd; v /= 10; } while (v); return nd; }
// the sqy header's length: prefix | payload bytes in decimal | suffix, padded in front to a multiple of the voxel size (sqeazy_header.hpp:172-178)
SQY_PIPE_HD inline uint64_t lz4_splice_header_bytes(uint32_t prefix_len, uint32_t suffix_len, uint64_t payload, uint32_t elem_size)
{
    const uint64_t text = (uint64_t)prefix_len + decimal_digits(payload) + suffix_len;
    return text + (elem_size - text % elem_size) % elem_size;
}
SQY_PIPE_HD inline uint64_t lz4_splice_status(uint64_t header_bytes, uint64_t payload, uint64_t capacity)
{
    return payload > 0x7fffffffull ? kSplicePayloadTooLong : (header_bytes + payload > capacity ? kSpliceNoRoom : kSpliceDone);
}
// The plan on the host: frame_off[f] = where frame f begins behind the header (nframes + 1 entries, the last one the payload's length),
// the header's length and the verdict.  old_off / old_size: the frame index' data offset and size field per frame; slot_of as above;
// csize / n: per selected chunk.  kSpliceBadIndex: an old frame whose span does not lie inside src_payload, or a slot out of range
struct Lz4SplicePlan { std::vector<uint64_t> frame_off; uint64_t payload = 0, header_bytes = 0, status = 0; };
Lz4SplicePlan lz4_splice_plan(const std::vector<uint64_t>& old_off, const std::vector<uint32_t>& old_size, const std::vector<uint32_t>& slot_of,
                              const std::vector<uint32_t>& csize, const std::vector<uint32_t>& n, uint64_t src_payload, uint32_t prefix_len, uint32_t suffix_len,
                              uint32_t elem_size, uint64_t capacity);
// The launches' job geometry, checked on the host before any of them: at least one frame, every selected chunk 0 .. nselected - 1 named
// by exactly one frame, in ascending order
bool lz4_splice_ok(const std::vector<uint32_t>& slot_of, size_t nselected);

// What runs for SQYAMD_Update_Box_*, stated once.
//   subset_patch  only the LZ4 frames the box's z-range needs are decoded, patched where they lie, parsed again and spliced between
//                 the old frames, which are copied verbatim
//   whole         the whole blob decoded, one paste launch, the single call's encode
// subset_patch needs ALL of: the option update_box_subset; `pipeline`, parsed, equal to the header's stage for stage (names and the lz4
// parameters); the form `lz4` or `bitswap1->lz4` with no head filter in front (the quantiser's table and frame_shuffle's order depend on
// the whole volume); lz4_encode_layout of the new blob `chunked` with acceleration 1 and more than one chunk; and the old blob taken by
// DecodeCall::frames_subset with one single-block frame per chunk of that same size.
enum class UpdateBoxPath { subset_patch, whole };
struct UpdateBoxFacts {
    bool option_on = false;                 // update_box_subset
    bool same_stages = false;               // pipelines_same_stages(asked, held)
    bool form_ok = false;                   // update_box_form_ok(asked)
    Lz4EncodeLayout layout;                 // lz4_encode_layout(asked's lz4 parameters, total, nthreads)
    bool subset_taken = false;              // frames_subset took the old blob ..
    uint64_t frames = 0, blocks = 0, frame_chunk = 0;      // .. and indexed that many frames and blocks, cut at frame_chunk bytes
};
UpdateBoxPath update_box_path(const UpdateBoxFacts& f);
struct Pipeline;
bool pipelines_same_stages(const Pipeline& a, const Pipeline& b);
bool update_box_form_ok(const Pipeline& p);

// ---- many boxes written into one large blob (SQYAMD_Update_Boxes_*) ----
// update_box_path decides for the whole call (pipeline, header, layout and frame index are the same for every box).  The plan turns the
// boxes' ranges (z0, nz) along the header's first dimension into SEGMENTS: ranges [z0, z0 + nz) of frames, ascending and pairwise
// disjoint, each the hull of the ranges that went into it, with the indices of its boxes in ascending box order.  Two ranges go into
// one segment when they overlap or abut, or (planes) when their plane-word intervals [w0, w1) intersect -- across a gap of frames where
// a frame has fewer voxels than a plane word, or where a word straddles a frame boundary.  Ranges that share a tail voxel share a voxel,
// so they overlap: that rule needs no test of its own, the plan only counts where the shared voxels were tail voxels alone.
// THE INVARIANT (tests/sanitize/update_boxes_test.cpp checks it by brute force): no plane word, no tail voxel and no byte of the
// stream in front of lz4 belongs to two segments.  So one thread of bitswap1_range_patches_kernel owns every word it writes, whatever
// boxes meet in it, and the segments are the `ranges` of DecodeCall::frames_subset: FrameRangesPlan::boxes[s] is segment s's addressing.
// plain: the box list is also cut into LAYERS, maximal runs of consecutive boxes [layer_first[l], layer_first[l + 1]) that are pairwise
// voxel-disjoint; one paste launch per layer in stream order gives "the box with the higher index holds" (the cut costs the layer's
// size squared in box comparisons; the usual call has one layer).  windows[i]: box i as admit_window gives it (its z-range is ranges[i]).
enum class RangeForm;                       // (below: plain, planes, ..)
struct UpdateBoxesSegment { uint64_t z0 = 0, nz = 0; std::vector<uint32_t> boxes; };
struct UpdateBoxesPlan {
    bool ok = false;                        // false: no box, ranges outside shape0 or a table of another length (nothing else is filled in)
    std::vector<UpdateBoxesSegment> segments;
    std::vector<uint32_t> layer_first;      // plain: nlayers + 1 entries
    uint64_t merged_overlap = 0, merged_word = 0, merged_tail = 0;       // ranges joined to the one in front: overlapping or abutting |
                                                                        // by a shared plane word alone | overlapping in tail voxels alone
};
UpdateBoxesPlan update_boxes_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, const std::vector<std::pair<uint64_t, uint64_t>>& ranges,
                                  const std::vector<BatchWindow>& windows);
// the layers alone, for any form (the whole path pastes by them too): nlayers + 1 entries, empty for no window
std::vector<uint32_t> update_boxes_layers(const std::vector<BatchWindow>& windows);
// two admitted windows of one blob share a voxel
inline bool windows_overlap(const BatchWindow& a, const BatchWindow& b)
{
    return a.oz < b.oz + b.Z && b.oz < a.oz + a.Z && a.oy < b.oy + b.Y && b.oy < a.oy + a.Y && a.ox < b.ox + b.X && b.ox < a.ox + a.X;
}

// The block-parallel parse of block-linked frames (sqy_kernels.h: Lz4SpecArgs).  Worth it for few long frames: the frame walks would
// leave the chip empty
bool lz4_spec_wanted(const Lz4Plan& plan);
// mode 1: block k is parsed behind a warm-up over blocks [first[k], k) of its frame: the fewest that hold `warmup` bytes, or all of them
void lz4_warmup_windows(const Lz4Plan& plan, uint64_t warmup, std::vector<uint32_t>* first, std::vector<uint32_t>* last);
// mode 2: every maximal stretch of failed blocks (ok[k] == 0) that lies in one frame gives one run [first[r], last[r]] from its first
// block, at most run_max blocks long (the rest fail the next check again).  first / last: at least ok.size() entries, nruns are written
struct Lz4RedoRuns { uint64_t nruns = 0, longest = 0; };      // longest: the longest stretch, uncapped
Lz4RedoRuns lz4_redo_runs(const Lz4Plan& plan, const std::vector<uint32_t>& ok, uint64_t run_max, std::vector<uint32_t>* first, std::vector<uint32_t>* last);

// ---- decode planning: host arithmetic on untrusted input (a header's shape, LZ4 parameters and reorder_map, a caller's range) ----
// What the decoder of one LZ4 stage indexes: `total` bytes in front of the stage in `nchunks` chunks of `chunk` (the last one may be
// short), at most `max_blocks` LZ4 blocks of up to `block_bytes`
struct Lz4DecodeGeometry { uint64_t chunk = 1, nchunks = 0, block_bytes = 0, max_blocks = 0; };
Lz4DecodeGeometry lz4_decode_geometry(const Lz4Params& p, uint64_t total);
// the chunked layout with every chunk full: one frame per chunk, more than one
bool lz4_chunks_whole(uint64_t nframes, uint64_t nchunks, uint64_t total, uint64_t chunk);
// .. and every chunk inside one of frame_shuffle's Z places of fb bytes: the LZ4 frames can be decoded straight to the shuffle's places
bool lz4_folds_into_shuffle(uint64_t nframes, uint64_t nchunks, uint64_t total, uint64_t chunk, uint64_t Z, uint64_t fb);
// frame_shuffle's inverse from the decoded reorder_map (Z 64-bit slots: slot i's frame goes to place map[i]).  *map becomes the device's
// copy: every slot but the LAST one named for a place struck (~0) -- the reference's decode walks the slots in order, the last writer
// stays (frame_shuffle_utils.hpp:337-344).  *unnamed: the places no slot names, ascending.  false: wrong length, or an entry >= Z
bool frame_shuffle_decode_map(std::vector<unsigned char>* map, uint64_t Z, std::vector<uint64_t>* unnamed, bool* permutation);

// Frames [z0, z0 + nz) of a volume of n voxels (elem bytes each, shape0 frames) out of the chunked LZ4 layout (nframes frames of `chunk`
// bytes, `total` in all) in front of which the stream is
//   plain: the voxels | planes: bitswap1's planes of them | planes_lut: bitswap1's planes of one quantised byte per voxel |
//   shuffle: frame_shuffle's `places` places of place_bytes (struck_map: frame_shuffle_decode_map's; lz4_folds_into_shuffle holds)
enum class RangeForm { plain, planes, planes_lut, shuffle };
struct FrameRangePlan {
    bool ok = false;                        // false: arguments that name no range of such a stream (nothing else is filled in)
    std::vector<uint32_t> ids;              // the LZ4 frames to decode: ascending, unique
    uint64_t out_bytes = 0;                 // what they decode to, back to back (shuffle: places [pa, pb))
    uint64_t range_at = 0;                  // plain, shuffle: the range's first byte in there
    std::vector<uint64_t> coff;             // plain, planes: offset of frame f in there (frames of ids only)
    // planes: sqy::Bitswap1Range's values -- words [w0, w1) of plane segment s at plane[s], voxels [max(v0, L), v1) at tail; we bytes a word
    uint64_t plane[16] = {}, tail = 0, v0 = 0, v1 = 0, w0 = 0, w1 = 0, L = 0;
    int we = 1;
    // shuffle: the place (relative to pa) of every slot decoded, in slot order; direct: the range starts and ends on place boundaries;
    // zero_runs: the places [first, second) (relative to pa) no slot names
    std::vector<uint64_t> remap;
    uint64_t pa = 0, pb = 0;
    bool direct = false;
    std::vector<std::pair<uint64_t, uint64_t>> zero_runs;
};
FrameRangePlan frame_range_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, uint64_t z0, uint64_t nz, uint64_t chunk, uint64_t total,
                                uint32_t nframes, const std::vector<unsigned char>& struck_map = {}, uint64_t place_bytes = 0, uint64_t places = 0);
// The same for a SET of ranges (z0, nz) of one blob (SQYAMD_Decode_Boxes_*): the LZ4 frames united -- each once, ascending -- and, per
// range, where its bytes lie in the united frames' compaction.  A range's span of a plane segment (of the voxels, for plain) is
// contiguous in the stream and all frames that cover it are selected, so it is contiguous in the compaction as well, whatever frames of
// other ranges lie in between.  shuffle: the places of all ranges, compacted in ascending place order (a range's own places stay
// consecutive); remap and zero_runs name compacted places.  frame_range_plan is the case of one range: frame_range_plan_of(plan, 0)
struct FrameRangesBox {
    uint64_t range_at = 0;                  // plain, shuffle: the range's first byte in the compaction
    uint64_t plane[16] = {}, tail = 0, v0 = 0, v1 = 0, w0 = 0, w1 = 0, L = 0;      // planes: as FrameRangePlan's
    uint64_t pa = 0, pb = 0;                // shuffle: the range's places
    bool direct = false;                    // shuffle: the compaction IS the range
};
// planes: the box's range as the range transposers take it (Range: sqy::Bitswap1Range of sqy_kernels.h, whose fields these are)
template <class Range>
Range bitswap1_range_of(const FrameRangesBox& b)
{
    Range r;
    for (int s = 0; s < 16; ++s) r.plane[s] = b.plane[s];
    r.tail = b.tail; r.w0 = b.w0; r.w1 = b.w1; r.v0 = b.v0; r.v1 = b.v1; r.L = b.L;
    return r;
}
struct FrameRangesPlan {
    bool ok = false;
    std::vector<uint32_t> ids;
    uint64_t out_bytes = 0;
    std::vector<uint64_t> coff;
    int we = 1;
    std::vector<uint64_t> remap;
    std::vector<std::pair<uint64_t, uint64_t>> zero_runs;
    std::vector<FrameRangesBox> boxes;      // one per range, in the caller's order
};
FrameRangesPlan frame_ranges_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, const std::vector<std::pair<uint64_t, uint64_t>>& ranges, uint64_t chunk,
                                  uint64_t total, uint32_t nframes, const std::vector<unsigned char>& struck_map = {}, uint64_t place_bytes = 0, uint64_t places = 0);
FrameRangePlan frame_range_plan_of(const FrameRangesPlan& u, size_t box);

// A box of one large blob (SQYAMD_Decode_Box_*): what runs for it.  subset_form: the blob is one the frame-range plan takes (the chunked
// layout of a RangeForm pipeline with more than one LZ4 frame -- where DecodeCall::frames_subset says `taken`), then `form` is its form;
// option_on: decode_box_subset.
//   subset_transposer  the LZ4 frames the box's z-range needs, then the windowed range transposer (planes, planes_lut)
//   subset_copy        .. then one window copy out of the range in the workspace (plain, shuffle)
//   whole_copy         the whole blob decoded into the workspace, one window copy (every other blob; the option off)
enum class BoxPath { subset_transposer, subset_copy, whole_copy };
BoxPath decode_box_path(bool subset_form, RangeForm form, bool option_on);
// Many boxes of one blob (SQYAMD_Decode_Boxes_*).  joint_option: decode_boxes_joint; the rest as for decode_box_path.
//   box_by_box         the option off: everything admitted up front, then the single-box driver box by box
//   subset_transposer  the LZ4 frames of all boxes' z-ranges united, then ONE launch of the job-table range transposer
//   subset_copy        .. then ONE window copy with a job per box out of the compaction
//   whole_copy         the whole blob decoded ONCE into the workspace, ONE window copy with a job per box
enum class BoxesPath { box_by_box, subset_transposer, subset_copy, whole_copy };
BoxesPath decode_boxes_path(bool subset_form, RangeForm form, bool subset_option, bool joint_option);
// Many boxes of one blob compared with resident voxels (SQYAMD_Compare_Boxes_*).  option_on: compare_boxes_subset; the rest as for
// decode_box_path.  One record per box, ONE output launch on every path:
//   subset_transposer  planes, planes_lut: the LZ4 frames of all boxes' z-ranges united, then the comparing job-table range transposer
//   subset_copy        plain, shuffle: .. then ONE window compare with a job per box in the compaction
//   whole_copy         every other blob, and every blob with the option off: decoded whole ONCE, ONE window compare with a job per box
BoxPath compare_boxes_path(bool subset_form, RangeForm form, bool option_on);
// Many boxes of one blob projected along an axis (SQYAMD_Project_Boxes_*).  option_on: project_boxes_subset; the rest as for
// compare_boxes_path.  One job per box, ONE output launch on every path:
//   subset_transposer  planes, planes_lut: the LZ4 frames of all boxes' z-ranges united, the outputs' neutral elements, then the projecting
//                      job-table range transposer (integer atomics on the images; the box's voxels never exist in memory)
//   subset_copy        plain, shuffle: .. then ONE projection launch with a job per box in the compaction (a thread per image element: it
//                      stores every element itself, no neutral elements first)
//   whole_copy         every other blob, and every blob with the option off: decoded whole ONCE, the same projection launch
BoxPath project_boxes_path(bool subset_form, RangeForm form, bool option_on);
// The admission of one box's projection, stated once (SQYAMD_Project_Boxes_*).  The box as admit_window admits it; `axis` in
// [0, rank) and the same for every box; op 0 .. 2 (max, min, sum); the image at `out` (not NULL, 4-byte aligned) has the box's extent with
// `axis` removed -- rank - 1 dimensions, ONE element for rank 1 -- and out_strides (rank - 1 pitches in elements, nullptr: dense) under
// admit_view's rules.  The sum is refused where it might not fit 32 bits: maxvoxel x extent[axis] >= 2^32 (maxvoxel: 65535 for 16-bit
// voxels, 255 for 8-bit ones).  On success: the window, and how the kernels address the image --
//   axis3   the axis among the window's three padded dimensions (axis + 3 - rank)
//   E0, E1  the image's extent padded to two dimensions, p0 its row pitch in elements
//   sz, sy  the WindowGeometry pitches that make the clip's dst_off the image's element (sqy_batch_window.hpp states the rule)
//   n       the box's extent along the axis; su, sv, sa: the steps in the BLOB's dense order from image row to row, column to column, and
//           along the axis (the thread-per-element projection of a dense volume)
struct Projection { uint32_t axis3 = 0; uint64_t E0 = 1, E1 = 1, p0 = 1, sz = 0, sy = 0, n = 1, su = 0, sv = 0, sa = 0; };
bool admit_projection(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, int axis, int op, uint64_t maxvoxel,
                      const void* out, const long* out_strides, BatchWindow* w, Projection* p);
// Many boxes of one blob read at a coarser resolution (SQYAMD_Bin_Boxes_*).  option_on: bin_boxes_subset; the rest as for
// project_boxes_path.  One job per box, ONE output launch on every path, no neutral-element launch on any:
//   subset_transposer  planes, planes_lut: the LZ4 frames of all boxes' z-ranges united, then the binning job-table kernel -- a workgroup
//                      per block of cells (bin_boxes_plan), accumulators in LDS, every cell stored once
//   subset_copy        plain, shuffle: .. then ONE launch with a thread per output cell in the compaction
//   whole_copy         every other blob, and every blob with the option off: decoded whole ONCE, the same per-cell launch
BoxPath bin_boxes_path(bool subset_form, RangeForm form, bool option_on);
// The admission of one box's binning, stated once (SQYAMD_Bin_Boxes_*).  The box as admit_window admits it; bins: `rank`
// longs, each >= 1; op 0 .. 2 (max, min, sum); the output at `out` (not NULL, 4-byte aligned) keeps the rank, its extent ceil(extent /
// bins) per dimension, and out_strides (rank pitches in elements, nullptr: dense) under admit_view's rules.  The sum is refused where a
// cell might not fit 32 bits: with V = the product of min(bins[d], extent[d]) -- each factor clamped first, the product saturating --,
// V > 65536 for 16-bit voxels (maxvoxel 65535) and maxvoxel V >= 2^32 for 8-bit ones (maxvoxel 255).  On success: the window, and
//   bins    padded to (z, y, x) and clamped to the extent (the same cells: a bin larger than the extent is one cell)
//   C       the cell grid, padded;  pz, py: the output's pitches in elements from cell layer to layer and cell row to row
struct Binning { uint64_t bins[3] = {1, 1, 1}, C[3] = {1, 1, 1}, pz = 1, py = 1; };
bool admit_binning(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, const long* bins, int op, uint64_t maxvoxel,
                   const void* out, const long* out_strides, BatchWindow* w, Binning* b);
// The tiling of one box's cell grid C into the blocks a workgroup of the bit-plane kernel owns (sqy_batch_window.hpp states what a block
// is), stated once.  `bins` as admit_binning clamps them, X the box's width.  A block holds at most budget_cells cells: whole cell rows
// where a row fits (as many as the budget takes, but no more than keep the block's footprint near cap_voxels voxels: small blocks fill
// the device), else ONE cell row cut into strips of budget_cells columns.  blocks = C[0] nbands nstrips.
BinPlan bin_boxes_plan(const uint64_t C[3], const uint64_t bins[3], uint64_t X, uint64_t budget_cells = kBinBlockCells, uint64_t cap_voxels = kBinBlockVoxels);
// A whole resolution pyramid of many boxes of one blob (SQYAMD_Pyramid_Boxes_*).  subset_option: pyramid_boxes_subset, fused_option:
// pyramid_boxes_fused; the rest as for bin_boxes_path.  ONE header fetch, ONE frame index, the LZ4 frames of all boxes' z-ranges united and
// decoded ONCE on the subset paths (the blob decoded whole ONCE on whole_copy); then, with `fused`:
//   subset_transposer  planes, planes_lut: ONE launch of the pyramid job-table kernel -- a workgroup per block of level-T cells
//                      (pyramid_boxes_plan), all fused levels' accumulators in LDS, every cell of every fused level stored once --, and where
//                      some box has levels above its T ONE pyramid_reduce launch that takes them all from the stored level-T cells
//   subset_copy        plain, shuffle: level 0 by Bin_Boxes' launch with a thread per cell in the compaction, then ONE pyramid_reduce
//                      launch that takes every further level straight from level 0
//   whole_copy         every other blob, and every blob with the subset option off: the same two launches on the whole volume
// and without: level 0 by Bin_Boxes' launch of the path, every further level by a pyramid_reduce launch of its own from the level below
// -- the same outputs, the layer to fall back on.
struct PyramidPath { BoxPath path; bool fused; };
PyramidPath pyramid_boxes_path(bool subset_form, RangeForm form, bool subset_option, bool fused_option);
// The admission of one box's pyramid, stated once (SQYAMD_Pyramid_Boxes_*), on admit_binning.  levels in [1,
// kPyramidMaxLevels]; bins: levels x rank longs, row l for level l; the rows nest: bins[l + 1][d] is a whole multiple of bins[l][d] for
// every d, on the caller's unclamped values (a multiple of 1 -- a repeated level -- included).  outs: the box's `levels` outputs, each as
// admit_binning wants it; out_strides: levels x rank pitches, or nullptr: all dense.  Every level is admitted by admit_binning -- the sum
// bound binds on the coarsest level's cell, the largest --, and where `sizes` is given the box's workgroups are added to each launch's
// count and the box refused where one passes 2^31 - 1.  On success: the window, every level's Binning, and the caller's bins padded to
// (z, y, x) with ones (`raw`: the ratios are taken on them).
struct Pyramid { uint32_t levels = 0; Binning q[kPyramidMaxLevels]; uint64_t raw[kPyramidMaxLevels][3]; };
struct PyramidSizes { uint64_t cell_groups = 0, blocks = 0, bin_blocks = 0, reduce_groups = 0; };
bool admit_pyramid(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, long levels, const long* bins, int op,
                   uint64_t maxvoxel, const void* const* outs, const long* out_strides, BatchWindow* w, Pyramid* p, PyramidSizes* sizes = nullptr);
// What a workgroup of the pyramid kernel owns, per box, stated once (sqy_batch_window.hpp states what a block is).  E: the box's extent
// padded to (z, y, x).  T is the highest level of which ONE cell, counted in level-0 cells of one layer after clamping to the grid, fits
// budget_level0 accumulators, whose fused levels' accumulators for ONE level-T cell fit budget_cells together, and of which ONE row of
// cells over the box's width and all its frames -- the least a block walks, layer after layer -- holds no more than cap_voxels voxels
// (level 0 is always fused).  The level-T grid is tiled as bin_boxes_plan tiles: whole rows of level-T cells where one fits both budgets
// (as many as fit, but no more than keep the block's footprint near cap_voxels: small blocks fill the device), else ONE row cut into the
// widest strips that fit.  off[l]: level l's accumulators in LDS for a block of the full band and strip.
PyramidPlan pyramid_boxes_plan(const Pyramid& p, const uint64_t E[3], uint64_t budget_level0 = kBinBlockCells, uint64_t budget_cells = kPyramidLdsCells,
                               uint64_t cap_voxels = kPyramidBlockVoxels);
// the accumulators that the level-l cells (l <= T) under band x strip level-T cells take: one layer of them
uint64_t pyramid_level_cells(const PyramidPlan& p, uint32_t l, uint64_t band, uint64_t strip);
// The intensity histograms of many boxes of one blob (SQYAMD_Histogram_Boxes_*).  option_on: histogram_boxes_subset; the rest as for
// project_boxes_path.  One job per box; on every path ONE launch that zeroes all histograms, then ONE counting launch that adds into them:
//   subset_transposer  planes, planes_lut: the LZ4 frames of all boxes' z-ranges united, then the counting job-table range transposer --
//                      a workgroup-private histogram (or a voted window of it) in LDS, flushed with no-return global atomics
//   subset_copy        plain, shuffle: .. then ONE window histogram with a job per box in the compaction
//   whole_copy         every other blob, and every blob with the option off: decoded whole ONCE, the same window histogram
BoxPath histogram_boxes_path(bool subset_form, RangeForm form, bool option_on);
// The admission of one box's histogram, stated once (SQYAMD_Histogram_Boxes_*).  The box as admit_window admits it; shift
// in [0, 8 elem_size) -- voxel v falls into bin v >> shift of (256^elem_size) >> shift bins --; the histogram at `out` not NULL and on
// the 4-byte grid.  On success the window.  A blob has fewer than 2^31 voxels, so no 32-bit counter can wrap: there is no bound on the box.
bool admit_histogram(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, int shift, int elem_size, const void* out,
                     BatchWindow* w);
// the bins of a histogram (0: shift or elem_size out of range)
inline uint32_t histogram_bins(int elem_size, int shift)
{
    return (elem_size == 1 || elem_size == 2) && shift >= 0 && shift < 8 * elem_size ? (elem_size == 2 ? 65536u : 256u) >> shift : 0u;
}

struct Stage {
    std::string name;
    StageKind kind = StageKind::unsupported;
    std::map<std::string, std::string> cfg;   // parsed (k=v,...) payload; std::map => sorted like the reference's config_map
    Lz4Params lz4;
    // rmbkrd_neighbor5x5x5 (flatten_to_neighborhood_scheme_impl.hpp:44-80): std::stoi into the voxel type (wrapped to 8 / 16 bits when
    // from_string knows the voxel size), std::stof
    long nb_threshold = 1;
    float nb_fraction = 0.5f;
    std::string config() const;               // re-serialised configuration, as the reference's config()
    std::string full_name() const;            // name or name(config)
};

// which factory lists know a name (sqeazy_pipelines.hpp:31-77; optional ffmpeg/bitshuffle stages are not built)
bool known_head_filter(const std::string& n);
bool known_sink(const std::string& n);
bool known_tail_filter(const std::string& n);

struct Pipeline {
    std::vector<Stage> stages;
    int sink_index = -1;                      // index of the sink stage, -1 when the pipeline only filters
    unsigned nthreads = 1;                    // stage default (dynamic_stage.hpp:21-24)

    // the reference's validity rule over its full stage lists
    static bool reference_accepts(const std::string& s);
    // true when every stage is one this library implements (subset of the above)
    static bool supported(const std::string& s, int elem_size, std::string* why = nullptr);
    // elem_size > 0 fills the defaults that depend on the voxel type (raster_reorder: tile_size = 16 / sizeof(T))
    static Pipeline from_string(const std::string& s, int elem_size = 0);

    std::string name() const;
    uint64_t max_encoded_size(uint64_t nbytes, int elem_size) const;
    void set_n_threads(int n);
};

int clean_number_of_threads(int n);

// raster_reorder (encoders/raster_reorder_utils.hpp:36-367): false for the geometries whose result the reference leaves
// undefined (a remainder in some but not all dimensions; tile_size a proper multiple of the 16-byte SSE block on a
// remainder-free shape)
bool raster_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X, uint64_t tile_size, int elem_size);

// zcurve_reorder (encoders/zcurve_reorder_utils.hpp): tile sizes 2..128 (powers of two) -- inside a tile the reference's
// morton_at_ct<log2(tile)> code is plain row-major, so the stage is "tiles of tile^3 (smaller at the high ends) in (z,y,x) tile
// order"; false where the reference runs past its buffers (other tile sizes; encode_full with a tile that does not divide the shape)
bool zcurve_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X, uint64_t tile_size);
// tile_shuffle (encoders/tile_shuffle_utils.hpp:104-224, encode_full): only shapes that are whole multiples of the tile
bool tile_shuffle_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X, uint64_t tile_size);
// metric = (T)(sequential float sum / voxels per tile), sorted ascending, slot i <- first tile whose metric equals sorted[i]
void tile_shuffle_order(const float* sums, size_t ntiles, size_t per_tile, int elem_size, uint64_t* decode_map, bool signed_char = false);
// rmbkrd_neighbor5x5x5's parameters as the reference's constructor reads them: false where std::stoi / std::stof would throw, and for a
// fraction that is not finite.  *threshold is the int std::stoi returns (not yet narrowed to the voxel type)
bool neighbor5_parse(const std::map<std::string, std::string>& cfg, long* threshold, float* fraction);
// rmbkrd_neighbor5x5x5 (flatten_to_neighborhood_scheme_impl.hpp:90-150, neighborhood_utils.hpp:141-240): false for the geometries whose row
// length the reference takes from an element its offset list does not have (X < 5, Y < 5, X = Y = 5, exactly one offset)
bool neighbor5_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X);
// centres of the 5x5x5 filter: z in [2, z_end), y in [2, Y - 2), x in [2, X - 1); z_end = max(2, min(X - 2, Z))
uint64_t neighbor5_z_end(uint64_t Z, uint64_t X);
// the host CPU's L2 size in bytes as the reference's compass reads it (compass.hpp:950-1035): CPUID leaf 4 on Intel, 0x80000006 on AMD,
// 0 on any other vendor or architecture.  rmestbkrd samples `frame > L2 ? (size_t)(L2 * .75) : frame` voxels of the z faces
uint32_t host_l2_cache_bytes();
uint64_t rmestbkrd_face_portion(uint64_t frame_voxels, uint32_t l2_bytes);
// bitshuffle: elements per block (bshuf_default_block_size for 0); 0 when the configured size is not a multiple of 8
uint64_t bitshuffle_block_elems(int elem_size, uint64_t block_size);

// ---- header ----
std::string header_pack(int elem_size, bool is_signed8, const std::vector<uint64_t>& shape, const std::string& pipename,
                        uint64_t payload_bytes);
void header_pack_parts(int elem_size, bool is_signed8, const std::vector<uint64_t>& shape, const std::string& pipename,
                       std::string* prefix, std::string* suffix);
struct HeaderInfo {
    bool valid = false;
    std::string pipename, type;
    std::vector<uint64_t> shape;
    uint64_t payload_bytes = 0;
    uint64_t size = 0;       // header bytes including the delimiter
    int elem_size() const;
};
HeaderInfo header_unpack(const char* begin, const char* end);

// quantiser `weighting_function` as quantiser_scheme::encode reads it (encoders/quantiser_scheme_impl.hpp:186-198, extract_ratio
// :25-47): "none" anywhere in the string -> weights 1; otherwise every run of digits is an integer (one: n/1, two: n/d, else
// 0/0) and "offset" anywhere selects offset_power_of (encoders/quantiser_weighters.hpp:20-95) instead of power_of (:98-160).
struct QuantiserWeighting {
    int mode = 0;            // 0 none, 1 power_of, 2 offset_power_of
    int num = 1, den = 1;    // exponent = float(num) / den
};
// false: the reference's exponent would be NaN or infinite (no "_" in the string, not one or two integers, denominator 0)
bool quantiser_parse_weighting(const std::string& text, QuantiserWeighting* out);
// quantiser LUTs from a 65536-bin histogram (encoders/quantiser_utils.hpp:386-418, :227-306, weights :317-322):
// lut_encode[65536] bytes, lut_decode[256] raw values.  IEEE binary32/64 in the reference's statement order.
void quantiser_build_luts(const uint32_t* histo, size_t nbins, unsigned char* lut_encode, uint16_t* lut_decode,
                          const QuantiserWeighting& weighting = QuantiserWeighting());
// quantiser::lut_to_file / lut_from_file (encoders/quantiser_utils.hpp:490-515): one decimal value per line
bool quantiser_lut_to_file(const std::string& path, const uint16_t* lut, size_t n);
bool quantiser_lut_from_file(const std::string& path, uint16_t* lut, size_t n);

// frame_shuffle ordering from the per-frame float sums (encoders/frame_shuffle_utils.hpp:126-166):
// metric = sum / per_frame, sorted ascending, slot i <- first frame whose metric equals sorted[i]
void frame_shuffle_order(const float* sums, size_t Z, size_t per_frame, uint64_t* decode_map);

std::string base64_encode(const unsigned char* src, size_t n);
std::vector<unsigned char> base64_decode(const std::string& s);
std::string to_verbatim(const void* data, size_t bytes);
// its inverse: false for a string shorter than the two tags (21 characters); else the 10 and 11 characters at its ends are stripped
// (not checked) and the rest base64-decoded into *out
bool from_verbatim(const std::string& v, std::vector<unsigned char>* out);

uint32_t xxh32(const unsigned char* p, size_t len, uint32_t seed);

extern const char* const kVersion;
extern const char* const kHeadRef;
extern const int kVersionTriple[3];

} // namespace sqy
#endif
