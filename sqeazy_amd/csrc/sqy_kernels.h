// sqy_kernels.h -- launchers of the HIP kernels in sqy_kernels.hip (device pointers, explicit stream).
#ifndef SQY_KERNELS_H_
#define SQY_KERNELS_H_

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "sqy_batch_window.hpp"

namespace sqy {

struct Lz4DedupeLayout;          // sqy_pipeline.hpp (as kLz4FrameHead and kLz4FrameGap)

// the duplicate search's tables, handed to launch_lz4_chunks when the decision per chunk is made by the chunk's own parse wavefront
// (launch_lz4_dedupe(.., fused) fills it in); chunk_key == nullptr: not in use
struct Lz4DedupeArgs {
    const uint64_t* chunk_key = nullptr;
    const uint64_t* tab_key = nullptr;
    const uint32_t* tab_val = nullptr;
    uint32_t tab_mask = 0;
    uint32_t* dup_of = nullptr;          // out: dup_of[k] = k, or the earlier chunk that chunk k equals byte for byte
    const uint32_t* piece_hash = nullptr;
    const uint64_t* holes_map = nullptr;
    uint64_t nchunks_full = 0;
    const uint32_t* digest = nullptr;    // the noise digest the transpose left (launch_bitswap1_u16), digest_stride words per chunk
    uint32_t digest_stride = 0;
};
// bitswap1: bit-plane transpose of `len` elements (encoders/bitswap_scheme_impl.hpp:97-145)
// piece_hash != nullptr (bitswap1_piece_hash_words(..) words, only offered when that is non-zero): a hash of every 1 KiB piece of
// plane data is left there for launch_lz4_dedupe
// gap_chunk != 0 ("frames in place", see launch_lz4_tail_marks): the plane stream is written as the bodies of the LZ4 frames it
// will be cut into -- chunk k (gap_chunk bytes, a power of two) at out + k * (gap_chunk + kLz4FrameGap), `out` any alignment; needs
// len % 8192 == 0
// side != nullptr (launch_diff3x3x1_side): columns x < side_w of every row of X voxels are read from the compact buffer `side`
// digest != nullptr (round 6, frames in place only, len / 8 a multiple of gap_chunk): the NOISE DIGEST -- bucket << 17 | tag of the five bytes at
// every position liblz4's search probes from probe 961 on when it starts with a chunk and finds nothing, digest_stride
// (= lz4_noise_digest_stride(gap_chunk)) words per chunk of the plane stream; the LZ4 parse of a chunk takes its batches from there as long
// as nothing has matched (Lz4DedupeArgs::digest) instead of reading the plane bytes again
// clear (frames in place only; bytes == 0: nothing): the launch also empties the duplicate search's table -- `key_bytes` bytes of keys (0)
// and, right behind them, bytes - key_bytes bytes of values (~0) at `table` (8-byte aligned, bytes a multiple of 16: what
// lz4_dedupe_layout lays out), and *zero_word = 0 -- so that no launch_lz4_dedupe_clear is needed in front of it (sqy_pipeline.hpp:
// lz4_table_clear_plan decides who clears).  Complete for any len; the first reader is a kernel behind this one.
struct Bitswap1Clear {
    uint8_t* table = nullptr;
    uint32_t key_bytes = 0, bytes = 0;
    uint32_t* zero_word = nullptr;
};
hipError_t launch_bitswap1_u16(const uint16_t* in, uint16_t* out, uint64_t len, hipStream_t stream, uint32_t* piece_hash = nullptr,
                               uint32_t gap_chunk = 0, const uint16_t* side = nullptr, uint32_t side_w = 0, uint32_t X = 0,
                               uint32_t* digest = nullptr, uint32_t digest_stride = 0, const Bitswap1Clear* clear = nullptr);
// frames in place: the transposer's grid is tiles / (2 waves x tiles per wave) workgroups -- how many tiles of 8192 voxels one of its
// wavefronts takes, one after the other (a measurement switch; the default is what profiles/transpose_grid.txt measured: the shorter
// the waves, the sooner the other calls' parse and small kernels find a slot)
constexpr long kBitswap1TilesPerWave = 1;
void set_bitswap1_tiles_per_wave(long n);
uint64_t bitswap1_piece_hash_words(const void* in, const void* out, uint64_t len);
// duplicate chunks of a plane stream (chunk a multiple of 1 KiB): dup_of[k] = the earliest chunk with the same bytes (k itself when
// there is none); the hashes only nominate, a byte compare decides.  base: the search's workspace, laid out by lz4_dedupe_layout -- the
// piece hashes are read and dup_of is written there
// in_stride (all LZ4 launchers; 0 = chunk): chunk k of the stream starts at in + k * in_stride
// holes (with gap_chunk): launch_bitswap1_u16 leaves the all-zero 1 KiB pieces of the stream UNWRITTEN (their hash is the exact zero
// marker, 0); launch_lz4_dedupe(.., holes: the workspace's holes map is used) compares through the markers and then fills the pieces
// in (writes into `in`) for every chunk anybody will read -- the bit planes above the data's range are neither written nor read
hipError_t launch_lz4_dedupe(const uint8_t* in, uint64_t total, uint32_t chunk, void* base, const Lz4DedupeLayout& lay, hipStream_t stream,
                             uint64_t in_stride = 0, bool holes = false, bool table_is_clear = false, Lz4DedupeArgs* fused = nullptr);
// the search's table emptied and *zero_word = 0 by one small kernel (a call launches it in front of its bit-plane transpose)
hipError_t launch_lz4_dedupe_clear(void* base, const Lz4DedupeLayout& lay, uint32_t* zero_word, hipStream_t stream);
hipError_t launch_bitswap1_u8(const uint8_t* in, uint8_t* out, uint64_t len, hipStream_t stream);

// diff3x3x1 on a {Z,Y,X} volume of 1- or 2-byte unsigned voxels (encoders/diff_scheme_impl.hpp:78-139)
// diff3x3x1 with a 16-bit bit-plane transpose right behind it: the stage can only touch columns x < 1 + hx, hx = Z - 2 (the reference
// takes the row extent from the DEPTH).  side_width = those columns rounded up to the 128 voxels a lane of the transpose
// owns (0: not applicable -- other geometry, 8-bit, or no column left out); launch_diff3x3x1_side writes just them (rows side_w
// voxels apart, Z*Y*side_w voxels), launch_bitswap1_u16(.., side, side_w, X) reads them from there and the rest from the input.
uint32_t diff3x3x1_side_width(uint64_t Z, uint64_t Y, uint64_t X, int elem_size);
hipError_t launch_diff3x3x1_side(const uint16_t* in, uint16_t* side, uint64_t Z, uint64_t Y, uint64_t X, uint32_t side_w, hipStream_t stream);
// schar (8-bit only): the stage as a tail filter on the sink's `char` output -- signed bytes, the sum sign-extended before the division
hipError_t launch_diff3x3x1(const void* in, void* out, uint64_t Z, uint64_t Y, uint64_t X, int elem_size, hipStream_t stream,
                            bool schar = false);

// LZ4: every `chunk` bytes of in[0,total) compressed on its own into scratch + k*stride (capacity chunk-1);
// csize[k] = compressed bytes, 0 when the chunk has to be stored raw.
// frame_map != nullptr: the stream is frame frame_map[f] of `in` for f = 0, 1, .. (frame_bytes each, a multiple of chunk),
// read in place (frame_shuffle directly in front of lz4)
// redo != nullptr (nchunks + 1 words): chunks that turn out to be streams of short sequences are not finished but listed
// there (redo[0] = count, redo[1..] = chunk numbers); launch_lz4_chunks_dense then parses exactly those
hipError_t launch_lz4_chunks(const uint8_t* in, uint64_t total, uint32_t chunk, uint8_t* scratch, uint64_t stride,
                             uint32_t* csize, uint64_t nchunks, hipStream_t stream, const uint64_t* frame_map = nullptr,
                             uint64_t frame_bytes = 0, uint32_t* redo = nullptr, const uint32_t* dup_of = nullptr, uint64_t in_stride = 0,
                             uint32_t acceleration = 1,      // liblz4's acceleration (1, or k + 1 for sqeazy's lz4(accel=-k))
                             bool redo_is_zero = false,      // redo[0] has been zeroed already (launch_lz4_dedupe_clear)
                             const Lz4DedupeArgs* dedupe = nullptr);
hipError_t launch_lz4_chunks_dense(const uint8_t* in, uint64_t total, uint32_t chunk, uint8_t* scratch, uint64_t stride,
                                   uint32_t* csize, uint32_t* redo, uint32_t redo_count, hipStream_t stream,
                                   const uint64_t* frame_map = nullptr, uint64_t frame_bytes = 0, uint64_t in_stride = 0);
// One block of a block-linked LZ4 frame (liblz4's LZ4F_blockLinked, what lz4::encode_serial produces: lz4_utils.hpp:99-173):
// where it sits in the stream and how far liblz4's backward catch-up may move a match that starts inside the block
// (low_in) or in the history in front of it (low_dict); stream offsets, may lie below `start - 64 KiB`.
struct Lz4Block {
    uint64_t start;          // byte offset of the block in the stream
    uint32_t n;              // bytes
    uint32_t flags;          // bit 0: first block of its frame (fresh LZ4 stream), bit 1: last block of its frame
    int64_t low_in, low_dict;
};
// block-linked frames: wavefront f compresses blocks [frame_first[f], frame_first[f+1]) in order, hash table carried from
// block to block; block k -> scratch + k*stride, csize[k] (0 = store raw).  max_block = largest blocks[k].n (<= 4 MiB)
hipError_t launch_lz4_linked(const uint8_t* in, const Lz4Block* blocks, const uint32_t* frame_first, uint64_t nframes,
                             uint32_t max_block, uint8_t* scratch, uint64_t stride, uint32_t* csize, hipStream_t stream, uint32_t acceleration = 1);
// Block-linked frames, block-parallel (round 4).  liblz4's table only matters as far as it holds positions of the last 64 KiB, so a
// wavefront can rebuild the table a block starts from by parsing the blocks in front of it (>= 64 KiB of them, output thrown away)
// from an empty table -- a guess that is almost always right and is CHECKED: every parse leaves the table it started from and the
// table it ended with in `tables`, launch_lz4_linked_verify compares block k's start with what block k - 1 really left (after the
// same re-basing; entries more than 64 KiB behind are parked at one value by it, so equality is equivalence), and the blocks that
// fail are parsed again from the true table (mode 2, runs of blocks in order).  When every block verifies, induction from the frame's
// first block (a fresh table, no guess) makes every block's output liblz4's.
//   mode 1: wavefront w walks blocks [wave_first[w], wave_last[w]]; the first starts from an empty table; only the last one's output,
//           size and tables count (the others are the warm-up)
//   mode 2: wavefront w walks blocks [wave_first[w], wave_last[w]], all of them for real; the first starts from the table block
//           wave_first[w] - 1 left (tables) unless it opens a frame
// tables: nblocks x 2 x 4096 words ([k][0] = the table block k was parsed from, [k][1] = the table it left)
struct Lz4SpecArgs {
    const uint32_t* wave_first = nullptr;
    const uint32_t* wave_last = nullptr;
    uint32_t* tables = nullptr;
    uint32_t mode = 0;
};
constexpr uint64_t kLz4SpecTableWords = 2 * 4096;
hipError_t launch_lz4_linked_spec(const uint8_t* in, const Lz4Block* blocks, const Lz4SpecArgs& spec, uint64_t nwaves,
                                  uint32_t max_block, uint8_t* scratch, uint64_t stride, uint32_t* csize, hipStream_t stream, uint32_t acceleration = 1);
// ok[k] = 1 when block k opens a frame or started from the table block k - 1 left, else 0
hipError_t launch_lz4_linked_verify(const Lz4Block* blocks, uint64_t nblocks, const uint32_t* tables, uint32_t max_block, uint32_t* ok, hipStream_t stream);
// frame_off[k] = byte offset of frame k in the concatenated stream, frame_off[nchunks] = total payload bytes
// (blocks != nullptr: offset of what block k contributes -- frame header if it opens a frame, size field, body, end mark
// if it closes one)
hipError_t launch_lz4_frame_scan(const uint32_t* csize, uint64_t nchunks, uint64_t total, uint32_t chunk,
                                 uint64_t* frame_off, hipStream_t stream, const Lz4Block* blocks = nullptr,
                                 const uint32_t* dup_of = nullptr, uint64_t* tail_info = nullptr,
                                 // frames in place, one host round trip per call: guard[0] != 0 (chunks left to the dense pass) makes the
                                 // kernel return at once; body0 != nullptr: the stored tail's frame marks are written here as well
                                 const uint32_t* guard = nullptr, uint8_t* body0 = nullptr, uint64_t in_stride = 0, uint32_t bd_byte = 0,
                                 uint32_t hc_byte = 0);
// Frames in place: everything between the frame scan and the finished blob, driven from the device -- the stored chunks in front of
// the tail put aside, the frames in front of the tail gathered up against it, the sqy header (hdr_prefix | payload bytes in decimal |
// hdr_suffix, padded in front to a multiple of elem_size) written in front of them.  record (pinned host memory, 7 words) takes
// [0] 1 done / 2 dense pass needed (guard[0] != 0: nothing was touched) / 3 no room for the header, [1] blob offset in `out`,
// [2] blob bytes, [3] payload bytes, [4] chunks in front of the stored tail, [5] stored chunks among them, [6] guard[0].
// (round 6) the same in one kernel; record[0] = 4 when stored chunks sit in front of the stored tail (then: the kernels above / below)
hipError_t launch_lz4_inplace_tail_fused(uint8_t* out, uint64_t t0, uint64_t in_stride, uint64_t total, uint32_t chunk, uint64_t nchunks,
                                         const uint8_t* scratch, uint64_t stride, const uint32_t* csize, uint64_t* frame_off, const uint32_t* dup_of,
                                         uint64_t* tail_info, uint32_t bd_byte, uint32_t hc_byte, const char* hdr_prefix, uint32_t prefix_len,
                                         const char* hdr_suffix, uint32_t suffix_len, uint32_t elem_size, const uint32_t* guard, uint64_t* record,
                                         hipStream_t stream);
hipError_t launch_lz4_inplace_tail(uint8_t* out, uint64_t t0, uint64_t in_stride, uint64_t total, uint32_t chunk, uint64_t nchunks,
                                   uint8_t* scratch, uint64_t stride, const uint32_t* csize, const uint64_t* frame_off, const uint32_t* dup_of,
                                   const uint64_t* tail_info, uint32_t bd_byte, uint32_t hc_byte, const char* hdr_prefix, uint32_t prefix_len,
                                   const char* hdr_suffix, uint32_t suffix_len, uint32_t elem_size, const uint32_t* guard, uint64_t* record,
                                   hipStream_t stream);
constexpr uint32_t kLz4InplaceHeaderTextMax = 3000;   // prefix + suffix bytes the finish kernel takes as an argument
// Frames in place (chunked layout; the stage in front wrote chunk k of the stream at body0 + k * in_stride, in_stride = chunk + kLz4FrameGap):
// tail_info (4 words, from the scan) = {j, bytes of frames 0..j-1, stored chunks among them, payload bytes}, j = first chunk of
// the run of stored chunks that ends the stream.  Those are final where they stand: tail_marks writes header / size field / end
// mark around them.  The frames in front are gathered (launch_lz4_frame_gather over j chunks) to END at body0 - kLz4FrameHead + j * in_stride;
// stored chunks among THEM are first put aside in their scratch slots (stash_raw; gather then with raw_from_scratch).
hipError_t launch_lz4_tail_marks(uint8_t* body0, uint64_t in_stride, uint64_t total, uint32_t chunk, uint64_t nchunks, uint32_t bd_byte,
                                 uint32_t hc_byte, const uint64_t* tail_info, hipStream_t stream);
hipError_t launch_lz4_stash_raw(const uint8_t* body0, uint64_t in_stride, uint64_t total, uint32_t chunk, uint8_t* scratch, uint64_t stride,
                                const uint32_t* csize, const uint32_t* dup_of, uint64_t nhead, hipStream_t stream);
// writes [04 22 4D 18 | 40 | BD | HC][u32 size][data][00 00 00 00] per chunk at out + frame_off[k]
hipError_t launch_lz4_frame_gather(const uint8_t* in, uint64_t total, uint32_t chunk, const uint8_t* scratch, uint64_t stride,
                                   const uint32_t* csize, const uint64_t* frame_off, uint8_t* out, uint32_t bd_byte,
                                   uint32_t hc_byte, uint64_t nchunks, hipStream_t stream, const uint64_t* frame_map = nullptr,
                                   uint64_t frame_bytes = 0, const Lz4Block* blocks = nullptr, const uint32_t* dup_of = nullptr,
                                   uint64_t in_stride = 0, bool raw_from_scratch = false);

// ---- batch encode (SQYAMD_PipelineEncode_Batch_*): the volumes of a group share one launch of every kernel ----
// bitswap1 of job j: `len` voxels at `in` (any voxel-aligned address) into planes + tail at `out` (16-byte aligned), laid out as
// launch_bitswap1_u16 / _u8 lay them out.  first_tile: njobs + 1 words, the prefix sums of batch_bitswap1_tiles(len) -- workgroup ->
// (job, tile) by a binary search over it
struct Bitswap1Job { const void* in; void* out; uint64_t len; };
uint32_t batch_bitswap1_tiles(uint64_t len);
hipError_t launch_bitswap1_batch(const Bitswap1Job* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);
// quantiser->bitswap1->lz4 on the same tables (16-bit voxels): the 65536-bin histogram of job j at d_histos + 65536 j (zeroed by the
// launcher); its encode LUT (65536 bytes at d_luts_encode + 65536 j) and decode LUT (256 values at d_luts_decode + 256 j) -- exactly
// sqy::quantiser_build_luts' for the default weighting, one workgroup per histogram, no host involved; look-up and 8-bit bit-plane
// transpose in one pass into job j's `out` (launch_quantiser_apply_bitswap1_u8's layout)
hipError_t launch_batch_quantiser_histogram(const Bitswap1Job* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, uint32_t* d_histos,
                                            hipStream_t stream);
hipError_t launch_batch_quantiser_lut(const uint32_t* d_histos, uint32_t njobs, uint8_t* d_luts_encode, uint16_t* d_luts_decode, hipStream_t stream);
hipError_t launch_batch_quantiser_bitswap1(const Bitswap1Job* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, const uint8_t* d_luts_encode,
                                           hipStream_t stream);
// ---- strided views (SQYAMD_*_BatchStrided_*): job j is a view of Z x Y x X voxels at `view` (voxel-aligned; rows sy, frames sz voxels
// apart, sqy::BatchView) and its dense form at `dense`.  first_tile as above, over batch_bitswap1_tiles(Z Y X).  Nothing outside the
// view's voxels is read or written on the view's side.
struct BatchViewJob { void* view; void* dense; uint64_t Z, Y, X, sz, sy; };
// the copy between the two: to_view = false packs the view into `dense` (any voxel-aligned address), true unpacks `dense` into the view
hipError_t launch_batch_view_copy(const BatchViewJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, bool to_view,
                                  hipStream_t stream);
// launch_bitswap1_batch with the voxels gathered from the view: planes + tail to `dense` (16-byte aligned), no packed copy in between
hipError_t launch_bitswap1_batch_strided(const BatchViewJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);
// launch_bitswap1_decode_batch with the voxels scattered into the view: planes + tail at `dense` (16-byte aligned)
hipError_t launch_bitswap1_decode_batch_strided(const BatchViewJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size,
                                                hipStream_t stream);
// ---- windows (SQYAMD_Decode_BatchWindow_*): job j is the box [oz, oz + Z) x [oy, oy + Y) x [ox, ox + X) of a blob of bZ x bY x bX voxels
// (sqy::BatchWindow) and the view of Z x Y x X voxels at `view` that takes it (voxel-aligned; rows sy, frames sz voxels apart).  Nothing
// but the view's voxels is written.
struct BatchWindowJob { void* view; const void* dense; uint64_t Z, Y, X, sz, sy, bZ, bY, bX, oz, oy, ox, tile0; };
// the copy out of the blob's dense volume at `dense` (any voxel-aligned address).  first_tile: the prefix sums of
// batch_bitswap1_tiles(Z Y X), the WINDOW's voxels; tile0 is not read
hipError_t launch_batch_window_copy(const BatchWindowJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);
// launch_bitswap1_decode_batch_strided with only the window's voxels stored: planes + tail of the whole blob at `dense` (16-byte aligned).
// Job j's workgroups are the tiles [tile0, tile0 + count) of the BLOB's dense order that hold its frames [oz, oz + Z)
// (sqy::window_first_tile, window_tile_count); first_tile: the prefix sums of those counts
hipError_t launch_bitswap1_decode_batch_window(const BatchWindowJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size,
                                               hipStream_t stream);
// ---- the compare of a window with its view (SQYAMD_Compare_BatchWindow_*) ----
// A BatchWindowJob whose view is only read, and the job's record: eight 64-bit words in device memory (the header's SQYAMD_COMPARE_*
// indices; word 0 is the host's).  Every workgroup that holds a voxel of the window adds its sums into the record with ONE set of integer
// atomics; nothing else is written.  The records are made ready by launch_batch_compare_init: zeros, VIEW_MIN all ones.
struct BatchCompareJob { const void* view; const void* dense; uint64_t Z, Y, X, sz, sy, bZ, bY, bX, oz, oy, ox, tile0; unsigned long long* record; uint64_t pad; };
hipError_t launch_batch_compare_init(unsigned long long* d_records, uint32_t nrecords, hipStream_t stream);
// launch_batch_window_copy's walk with both sides loaded: `dense` is the blob's dense volume (any voxel-aligned address); tile0 is not read
hipError_t launch_batch_window_compare(const BatchCompareJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);
// launch_bitswap1_decode_batch_window's geometry and tables: planes + tail of the whole blob at `dense` (16-byte aligned)
hipError_t launch_bitswap1_decode_batch_window_compare(const BatchCompareJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size,
                                                       hipStream_t stream);
// ---- the update of a window (SQYAMD_Update_BatchWindow_*) ----
// launch_batch_window_copy the other way round: the view's voxels are read and stored into the window inside the dense volume at `dense`
// (written, whatever the job's type says); nothing else of it is touched
hipError_t launch_batch_window_paste(const BatchWindowJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);
// Job j: the plane stream (planes + tail, launch_bitswap1_batch's layout) of a blob of bZ x bY x bX voxels at old_stream, the window of a
// BatchWindowJob in it and the view that holds the window's new voxels.  new_stream (no overlap with old_stream) takes the plane stream of
// the blob with the window's voxels replaced.  The streams at any voxel-aligned address (sixteen bytes at a time where both and the plane
// size are on the 16-byte grid); first_tile: the prefix sums of batch_bitswap1_tiles(bZ bY bX)
struct BatchPatchJob { const void* view; const void* old_stream; void* new_stream; uint64_t Z, Y, X, sz, sy, bZ, bY, bX, oz, oy, ox; };
hipError_t launch_bitswap1_batch_patch(const BatchPatchJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);

// One entry of the joint chunk table (sqy::Lz4BatchChunkPlan, sqy_pipeline.hpp): chunk e is the n bytes at in + off, compressed on its
// own into scratch + slot * stride, csize[e] (0: stored); redo as for launch_lz4_chunks (nentries + 1 words, the launcher zeroes redo[0])
struct Lz4BatchChunk { uint64_t off; uint32_t n, vol, slot, pad; };
hipError_t launch_lz4_chunks_table(const uint8_t* in, const Lz4BatchChunk* d_table, uint32_t nentries, uint8_t* scratch, uint64_t stride, uint32_t* csize,
                                   uint32_t* redo, hipStream_t stream);
hipError_t launch_lz4_chunks_table_dense(const uint8_t* in, const Lz4BatchChunk* d_table, uint8_t* scratch, uint64_t stride, uint32_t* csize,
                                         uint32_t* redo, uint32_t redo_count, hipStream_t stream);
// Volume v of a group: table entries [first_chunk, first_chunk + nchunks); its blob goes to out + dst_at, at most capacity bytes; the
// sqy header is text[text_at, +prefix_len) | payload bytes in decimal | text[text_at + prefix_len, +suffix_len), padded in front to a
// multiple of elem_size; record (3 words of pinned host memory per volume, index `record`): status, blob bytes, payload bytes
struct Lz4BatchVolume { uint64_t dst_at, capacity; uint32_t first_chunk, nchunks, text_at, prefix_len, suffix_len, elem_size, record, pad; };
constexpr uint64_t kBatchDone = 1, kBatchNoRoom = 2, kBatchPayloadTooLong = 3;
// scan (one workgroup per volume): frame_off[e] = where entry e's frame starts behind its volume's header, vinfo[2 v] = payload bytes,
// vinfo[2 v + 1] = header bytes | status << 32.  gather: every frame behind its volume's header ([04 22 4D 18 | 40 | BD | HC][u32
// size][data][00 00 00 00]), the header and the record -- nothing at all for a volume whose blob does not fit its capacity
hipError_t launch_lz4_batch_scan(const Lz4BatchChunk* d_table, const Lz4BatchVolume* d_vols, uint32_t nvols, const uint32_t* csize,
                                 uint64_t* frame_off, uint64_t* vinfo, hipStream_t stream);
hipError_t launch_lz4_batch_gather(const uint8_t* in, const Lz4BatchChunk* d_table, uint32_t nentries, uint32_t max_chunk, const Lz4BatchVolume* d_vols,
                                   const uint32_t* d_vol_of /* per entry: index into d_vols */, const uint8_t* scratch, uint64_t stride,
                                   const uint32_t* csize, const uint64_t* frame_off, const uint64_t* vinfo, const char* d_text, uint8_t* out,
                                   uint32_t bd_byte, uint32_t hc_byte, uint64_t* records, hipStream_t stream, const uint64_t* d_place = nullptr);
// The packed layout (SQYAMD_PipelineEncode_BatchPacked_*), between the scan and the gather, one workgroup: d_place[j] = where volume j of
// the group lies relative to `out` by sqy::packed_places' rule (base: where the group begins, a multiple of align; d_gap[j]: what volumes
// outside the group take in front of volume j, nullptr: all zero; align a power of two), and a kBatchDone volume that ends behind `capacity` becomes
// kBatchNoRoom in vinfo.  The gather with d_place writes blob j at out + d_place[j] (dst_at is not read; the scan is given capacity ~0)
// and leaves a kBatchNoRoom volume's blob length in its record.
hipError_t launch_lz4_batch_place(uint64_t* vinfo, const uint64_t* d_gap, uint32_t nvols, uint64_t align, uint64_t base, uint64_t capacity, uint64_t* d_place,
                                  hipStream_t stream);

// ---- the splice of old LZ4 frames and new ones into one blob (SQYAMD_Update_Box_*) ----
// The new blob has the old blob's nframes single-block frames.  Frame f is carried over from the old payload `src` (slot_of[f] =
// sqy::kSpliceOldFrame; blk: the old payload's frame index, launch_lz4_frame_rank's, one block per frame) or replaced by entry k =
// slot_of[f] of the chunk table that launch_lz4_chunks_table parsed (csize[k], its scratch slot, or the chunk's own bytes at in + off where
// it is stored).  src_payload: the old payload's bytes; max_frame: the longest frame the gather copies (chunk or block bytes +
// kLz4FrameGap; a longer old frame is kSpliceBadIndex); the header is text[0, prefix_len) | payload bytes in decimal | text[prefix_len,
// + suffix_len), padded in front to a multiple of elem_size.  All arithmetic: sqy_pipeline.hpp's lz4_splice_* functions.
struct Lz4SpliceJob {
    const void* blk;
    const uint32_t* slot_of;
    const Lz4BatchChunk* table;
    const uint32_t* csize;
    uint64_t src_payload;
    uint32_t nframes, max_frame, prefix_len, suffix_len, elem_size;
};
bool lz4_splice_job_ok(const Lz4SpliceJob& j);
// scan (one workgroup): frame_off[f] = where frame f begins behind the header (nframes + 1 entries), info[0] = payload bytes, info[1] =
// header bytes | status << 32 (sqy::kSpliceDone .. kSpliceBadIndex; kSpliceNoRoom: header + payload > capacity)
hipError_t launch_lz4_splice_scan(const Lz4SpliceJob& j, uint64_t capacity, uint64_t* frame_off, uint64_t* info, hipStream_t stream);
// gather: the header and every frame at out (any byte address; `src` too -- sixteen-byte stores from out's grid on, bytes in front and
// behind), and the record (3 words of pinned host memory: status, blob bytes -- for kSpliceNoRoom what a retry needs --, payload bytes).
// Nothing but the record is written unless the status is kSpliceDone; then exactly the blob's bytes are.
hipError_t launch_lz4_splice_gather(const Lz4SpliceJob& j, const uint8_t* src, const uint8_t* in, const uint8_t* scratch, uint64_t stride, const uint64_t* frame_off,
                                    const uint64_t* info, const char* d_text, uint8_t* out, uint32_t bd_byte, uint32_t hc_byte, uint64_t* record, hipStream_t stream);

// quantiser: 65536-bin histogram of u16 voxels (histo is zeroed by the launcher), and out[i] = lut[in[i]]
// background removal, 1- or 2-byte voxels of a {Z, Y, X} volume
// rmestbkrd (encoders/remove_estimated_background_scheme_impl.hpp:71-110): four face histograms (frames z = 0 and Z-1: their first
// `portion` voxels; rows y = 0 and Y-1 of frames 1, Z/2, Z-2), the 99 % support of each, out = in > t ? in - t : 0 with t = (T)min of the
// supports -- all on the stream, no host round trip.  work: rmestbkrd_work_bytes(elem_size) bytes of the call's own workspace.  Z >= 2
uint64_t rmestbkrd_work_bytes(int elem_size);
hipError_t launch_rmestbkrd(const void* in, void* out, uint64_t Z, uint64_t Y, uint64_t X, uint64_t portion, int elem_size, void* work,
                            hipStream_t stream);
// rmbkrd_neighbor5x5x5: every voxel of `out` written; centres z in [2, z_end), y in [2, Y-2), x in [2, X-1) with in >= threshold keep
// their value when (float)(neighbours below threshold) <= cut (= fraction * 124.f), all else 0 (neighbours past the end: not counted)
hipError_t launch_rmbkrd_neighbor5(const void* in, void* out, uint64_t Z, uint64_t Y, uint64_t X, uint32_t threshold, float cut,
                                   uint64_t z_end, int elem_size, hipStream_t stream);
hipError_t launch_histogram_u16(const uint16_t* in, uint64_t len, uint32_t* histo, hipStream_t stream);
hipError_t launch_quantiser_apply_u16(const uint16_t* in, uint8_t* out, uint64_t len, const uint8_t* lut, hipStream_t stream);
// .. with the 8-bit bit-plane transpose of the sink's bytes in the same pass (quantiser->bitswap1; `in` 16-byte aligned): out = the 8
// plane segments of len / 8 bytes, MSB plane first, + the len % 8 tail
hipError_t launch_quantiser_apply_bitswap1_u8(const uint16_t* in, uint8_t* out, uint64_t len, const uint8_t* lut, hipStream_t stream);

// raster_reorder (encoders/raster_reorder_utils.hpp): tiles of tile_size^3 (remainder tiles at the high ends) appended in
// (z,y,x) tile order, row-major inside; decode = the inverse permutation
hipError_t launch_raster_reorder(const void* in, void* out, uint64_t Z, uint64_t Y, uint64_t X, uint64_t tile_size, int elem_size,
                                 bool decode, hipStream_t stream);

// bitshuffle (bshuf_bitshuffle / bshuf_bitunshuffle of kiyo-masui/bitshuffle) of n_elems elements of 1 or 2 bytes in blocks of
// block_elems elements (a multiple of 8)
hipError_t launch_bitshuffle(const void* in, void* out, uint64_t n_elems, int elem_size, uint64_t block_elems, bool decode, hipStream_t stream);

// frame_shuffle: per-frame mean in the reference's sequential binary32 order; frame gather out[i] = in[map[i]]
// schar (8-bit only): frames of signed bytes (the stage as a tail filter)
hipError_t launch_frame_metric(const void* in, uint64_t Z, uint64_t per_frame, int elem_size, float* metric, hipStream_t stream,
                               void* scratch = nullptr, uint64_t scratch_bytes = 0, bool schar = false);
// scratch that lets long frames take the block-parallel path (16 bytes per 4 KiB block)
uint64_t frame_metric_scratch_bytes(uint64_t Z, uint64_t per_frame, int elem_size);
hipError_t launch_frame_gather(const void* in, void* out, uint64_t Z, uint64_t frame_bytes, const uint64_t* map, hipStream_t stream);

// ---- decode ----
// index of every LZ4 block of the concatenated frames: blk[i] = {data offset lo, hi, size | raw << 31, block id in frame}
hipError_t launch_lz4_frame_index(const uint8_t* in, uint64_t n, void* blk, uint32_t* frame_first, uint64_t max_blocks,
                                  uint32_t* counts /* frames, blocks, error */, hipStream_t stream);
// parallel variant for the chunked layout (single-block frames): counts[2] == 100 means "not covered, run the serial walk"
uint64_t lz4_frame_rank_scratch_bytes(uint64_t expected_frames);
hipError_t launch_lz4_frame_rank(const uint8_t* in, uint64_t n, void* blk, uint32_t* frame_first, uint64_t max_blocks,
                                 uint32_t* counts, uint64_t expected_frames, void* scratch, hipStream_t stream, uint64_t chunk = 0, uint64_t last = 0);
// (chunk, last: the bytes every frame but the last / the last frame decodes to -- frames at the stream's end that are STORED blocks of
//  those sizes are found where they must start instead of by the scan; 0 = scan everything.  counts: 16 words, [6] = frames found so)
// The ranking of several streams at once (SQYAMD_Decode_Slabs_*): job i is launch_lz4_frame_rank(in, n, blk, frame_first, max_blocks,
// counts, expected_frames, scratch, .., chunk, last) -- its own scratch (lz4_frame_rank_scratch_bytes), counts (16 words, zeroed here) --,
// all jobs in one launch per kernel, the single-workgroup tail and rank kernels of the jobs side by side.  d_desc: device memory of
// lz4_frame_rank_batch_desc_bytes(njobs) bytes; h_desc: host memory of as many, alive until the stream has passed the launch.
struct Lz4RankJob {
    const uint8_t* in;
    uint64_t n;
    void* blk;
    uint32_t* frame_first;
    uint64_t max_blocks;
    uint32_t* counts;
    uint64_t expected_frames;
    void* scratch;
    uint64_t chunk, last;
};
uint64_t lz4_frame_rank_batch_desc_bytes(uint32_t njobs);
hipError_t launch_lz4_frame_rank_batch(const Lz4RankJob* jobs, uint32_t njobs, void* d_desc, void* h_desc, hipStream_t stream);
// One LZ4 decode launch over the ranked frames of several streams (SQYAMD_Decode_Slabs_*).  Part p (device array d_parts): nframes
// single-block frames indexed at blk (offsets relative to its stream, which starts at in + in_off), `total` bytes decoded in frames of
// `chunk`; frame f goes to out + out_base + f * chunk, or with remap (frame_shuffle in front) to out + out_base + remap[o / remap_bytes] *
// remap_bytes + o % remap_bytes, o = f * chunk (~0 in remap: struck).  jblk (16 B), jff (4 B + 1) and jout (16 B) per frame of all parts:
// the joint index the launch builds on the device.  The kernel choice of launch_lz4_frames_decode on the joint counts; *errflag as there.
struct Lz4JointPart {
    const void* blk;
    uint64_t in_off, out_base, chunk, total;
    const uint64_t* remap;
    uint64_t remap_bytes;
    uint32_t jbase, nframes;
};
hipError_t launch_lz4_frames_joint_decode(const uint8_t* in, const Lz4JointPart* d_parts, uint32_t nparts, uint32_t max_part_frames, void* jblk,
                                          uint32_t* jff, uint64_t* jout, uint32_t nframes, uint8_t* out, uint64_t out_bytes, uint64_t block_bytes,
                                          uint32_t ncompressed, uint32_t* errflag, hipStream_t stream, hipStream_t copy_stream = nullptr,
                                          hipEvent_t fork = nullptr, hipEvent_t join = nullptr, bool two_waves = false);
// frame f decodes to out + f*frame_stride; every block decodes to at most block_bytes
// ONE block-linked frame (the serial layout) decoded block-parallel: every block at once with the history as an unknown (16-bit
// references in `refs`, out_bytes words), the tails resolved in order by one workgroup, the rest at once.  blk: the frame's blocks
// (launch_lz4_frame_index).  *errflag != 0 afterwards: not a frame of full blocks, or damaged -- the one-wavefront walk decides.
bool lz4_linked_decode_parallel_possible(uint32_t nblocks, uint64_t out_bytes, uint64_t block_bytes);
// scan_scratch (lz4_linked_decode_scan_scratch_bytes(nblocks) bytes, optional): long frames resolve their tails as a scan over ranges of
// blocks instead of one walk
uint64_t lz4_linked_decode_scan_scratch_bytes(uint32_t nblocks);
hipError_t launch_lz4_linked_decode_parallel(const uint8_t* in, const void* blk, uint32_t nblocks, uint8_t* out, uint16_t* refs, uint64_t out_bytes,
                                             uint64_t block_bytes, uint32_t* errflag, hipStream_t stream, uint8_t* scan_scratch = nullptr);
hipError_t launch_lz4_frames_decode(const uint8_t* in, const void* blk, const uint32_t* frame_first, uint32_t nframes, uint8_t* out,
                                    uint64_t out_bytes, uint64_t frame_stride, uint64_t block_bytes, uint32_t ncompressed,
                                    uint32_t* errflag, hipStream_t stream, hipStream_t copy_stream = nullptr, hipEvent_t fork = nullptr,
                                    hipEvent_t join = nullptr, const uint64_t* remap = nullptr, uint64_t remap_bytes = 0, bool two_waves = false);
// (two_waves: every frame is ONE block -- two wavefronts per frame, lz4_frames_decode2_kernel)
// (remap: the inverse of frame_shuffle folded into the decode -- the chunk that starts at byte o of the sorted stream goes to
// remap[o / remap_bytes] * remap_bytes + o % remap_bytes; remap_bytes a multiple of frame_stride, out_bytes = nframes * frame_stride)
// decode of quantiser->bitswap1: inverse transpose of the 8-bit planes and the quantiser's look-up in one pass
bool bitswap1_u8_decode_lut_possible(const void* in, const void* out, uint64_t len);
hipError_t launch_bitswap1_u8_decode_lut(const uint8_t* in, uint16_t* out, uint64_t len, const uint16_t* lut, hipStream_t stream);
hipError_t launch_bitswap1_decode(const void* in, void* out, uint64_t len, int elem_size, hipStream_t stream);
// ---- frame-range decode (SQYAMD_Decode_Frames_*) ----
// LZ4 frames ids[0..nsel) of a chunked-layout stream (the full index: blk, frame_first of nframes frames), decoded by the kernels of
// launch_lz4_frames_decode: subset frame i to out + i * frame_stride (ids ascending: the frames' bytes back to back, out_bytes = their
// sum), or with remap to remap[i * frame_stride / remap_bytes] * remap_bytes + the rest (out_bytes a multiple of remap_bytes).
// sblk (nsel * max_per_frame * 16 bytes) and sff (nsel + 1 words): the subset's block index, built on the device.  *errflag as there.
hipError_t launch_lz4_frames_subset_decode(const uint8_t* in, const void* blk, const uint32_t* frame_first, uint32_t nframes,
                                           const uint32_t* ids, uint32_t nsel, uint32_t max_per_frame, void* sblk, uint32_t* sff,
                                           uint8_t* out, uint64_t out_bytes, uint64_t frame_stride, uint64_t block_bytes, uint32_t ncompressed,
                                           uint32_t* errflag, hipStream_t stream, const uint64_t* remap = nullptr, uint64_t remap_bytes = 0,
                                           bool two_waves = false);
// inverse bitswap1 of plane words [w0, w1) into voxels [v0, v1) (out[v - v0]; W = 8 * elem_size voxels per word): stored plane segment s
// of the range starts at in + plane[s] (byte offsets), the voxels [max(v0, L), v1) behind the planes (L = segment words * W) at
// in + tail.  lut != nullptr (elem_size 1): 16-bit voxels out of the quantiser's decode table (quantiser->bitswap1)
struct Bitswap1Range {
    uint64_t plane[16];
    uint64_t tail;
    uint64_t w0, w1, v0, v1, L;
};
hipError_t launch_bitswap1_decode_range(const uint8_t* in, void* out, const Bitswap1Range& r, int elem_size, const uint16_t* lut, hipStream_t stream);
// ---- the box of one large blob (SQYAMD_Decode_Box_*) ----
// launch_bitswap1_decode_range with only a box's voxels stored, each to its place in a view: the windowed transposer's clip and scatter
// (launch_bitswap1_decode_batch_window) on the range's addressing.  box: the blob's shape, the box in it and the view that takes it
// (`dense` and tile0 are not read); the range must hold the box, its first voxel at or behind v0 and its last in front of v1 (refused
// otherwise: the voxels outside [v0, v1) count as outside the box).  Sixteen-byte plane loads
// where in + plane[s] - w0 elem_size is on the 16-byte grid for every s, word by word where not.  Nothing but the view's voxels is written.
hipError_t launch_bitswap1_decode_range_window(const uint8_t* in, const Bitswap1Range& r, const BatchWindowJob& box, int elem_size, const uint16_t* lut,
                                               hipStream_t stream);
// ---- many boxes of one large blob (SQYAMD_Decode_Boxes_*) ----
// launch_bitswap1_decode_range_window for a table of boxes in ONE launch: job j stores the voxels of its box (g: the blob's rows, the box
// and the view's pitches, as sqy::WindowGeometry; view: its base) out of the range r, whose offsets point into the ONE buffer `in` that
// holds the united LZ4 frames of all boxes; t0 = sqy::range_first_thread(r.w0, words per thread).  d_first_tile: njobs + 1 words, the
// prefix sums of sqy::range_job_groups(r.w0, r.w1, words per thread); ngroups their sum.  Every job must pass bitswap1_box_job_ok (the
// range holds the box).  Nothing but the views' voxels is written.
struct Bitswap1BoxJob {
    void* view;
    WindowGeometry g;
    Bitswap1Range r;
    uint64_t t0;
};
bool bitswap1_box_job_ok(const Bitswap1BoxJob& j);
hipError_t launch_bitswap1_decode_range_windows(const uint8_t* in, const Bitswap1BoxJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups,
                                                int elem_size, const uint16_t* lut, hipStream_t stream);
// ---- many boxes of one large blob compared with resident voxels (SQYAMD_Compare_Boxes_*) ----
// launch_bitswap1_decode_range_windows with loads where its stores were: job j's view is only READ, and the sums over its box's voxels
// (a = the decoded voxel -- behind the look-up the 16-bit voxel out of the table --, b = the view's) go into its record, eight 64-bit words
// made ready by launch_batch_compare_init, with ONE set of integer atomics per workgroup that holds a voxel of the box.  The job is
// Bitswap1BoxJob's fields and the record; the tables, the groups and bitswap1_box_compare_job_ok as there.  Nothing but the records is
// written.
struct Bitswap1BoxCompareJob {
    const void* view;
    WindowGeometry g;
    Bitswap1Range r;
    uint64_t t0;
    unsigned long long* record;
    uint64_t pad;
};
constexpr uint64_t kBitswap1BoxCompareJobBytes = 288;     // (a multiple of 16: the tile table behind the jobs stays on the 16-byte grid)
bool bitswap1_box_compare_job_ok(const Bitswap1BoxCompareJob& j);
hipError_t launch_bitswap1_decode_range_windows_compare(const uint8_t* in, const Bitswap1BoxCompareJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs,
                                                        uint32_t ngroups, int elem_size, const uint16_t* lut, hipStream_t stream);
// ---- many boxes of one large blob projected along an axis (SQYAMD_Project_Boxes_*) ----
// launch_bitswap1_decode_range_windows with a combine where its stores were: job j's decoded voxels (behind the look-up the 16-bit voxels
// out of the table) go into its image of 32-bit elements at `out` with no-return integer atomics at device scope -- max, min or add, so
// the result does not depend on the order the threads finish in --, the element being the clip's dst_off under the geometry
// sqy::admit_projection fills (sqy_batch_window.hpp: window_project16; axis 2 reduced per sub-run in the thread first).  The images hold
// their neutral elements beforehand: launch_boxes_project_init over the SAME tables, in front on the stream -- workgroup `own` of a job's
// groups fills the elements own 256 + tid, + groups 256, .. of the job's image (E0 rows of E1 elements, p0 apart).  The job is
// Bitswap1BoxJob's fields and the image's; the tables, the groups and bitswap1_box_project_job_ok as there.  Nothing but the images'
// elements is written.
struct Bitswap1BoxProjectJob {
    void* out;
    WindowGeometry g;
    Bitswap1Range r;
    uint64_t t0;
    uint32_t op, axis;       // sqy::kProjectMax .. ; the axis among (z, y, x)
    uint64_t E0, E1, p0;
};
constexpr uint64_t kBitswap1BoxProjectJobBytes = 304;    // (a multiple of 16: the tile table behind the jobs stays on the 16-byte grid)
bool bitswap1_box_project_job_ok(const Bitswap1BoxProjectJob& j);
hipError_t launch_boxes_project_init(const Bitswap1BoxProjectJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, hipStream_t stream);
hipError_t launch_bitswap1_decode_range_windows_project(const uint8_t* in, const Bitswap1BoxProjectJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs,
                                                        uint32_t ngroups, int elem_size, const uint16_t* lut, hipStream_t stream);
// The second form for axis 0 (frames), where a frame is a whole number of 32-voxel runs: no atomics, no neutral elements beforehand.  A
// thread owns ONE frame-local run of 32 voxels -- four bytes of every plane per frame, on the 4-byte grid -- and walks z over the box's
// frames: it loads the plane pieces of each frame, transposes them and reduces by position in registers; the clip of its run in the box's
// first frame (the same in every frame) says which positions are image elements, and it stores those once.  Job j owns
// project_walk_groups(g) workgroups: the runs [first, last] that hold a voxel of the box's footprint in a frame; a run with nothing
// inside loads no plane word.  Every job of a launch must pass bitswap1_box_project_walk_ok (and bitswap1_box_project_job_ok); `in` is on
// the 4-byte grid.
SQY_VIEW_HD inline uint64_t project_walk_first_run(const WindowGeometry& g) { return (g.oy * g.bX + g.ox) / 32; }
SQY_VIEW_HD inline uint64_t project_walk_groups(const WindowGeometry& g)
{
    return (((g.oy + g.Y - 1) * g.bX + g.ox + g.X - 1) / 32 - project_walk_first_run(g)) / 256 + 1;
}
// elem_size: of a STORED voxel (1 behind the look-up)
inline bool bitswap1_box_project_walk_ok(const Bitswap1BoxProjectJob& j, int elem_size)
{
    const uint64_t W = 8u * (uint64_t)elem_size, frame = j.g.bY * j.g.bX;
    if (j.axis != 0 || frame == 0 || frame % 32 != 0) return false;
    // every word of the box's frames lies in the range's plane words, none of its voxels in the tail
    if (j.r.w0 * W > j.g.oz * frame || (j.g.oz + j.g.Z) * frame > j.r.w1 * W || (j.g.oz + j.g.Z) * frame > j.r.L) return false;
    for (uint64_t p = 0; p < W; ++p)                                  // a run's four bytes of plane p: on the 4-byte grid
        if ((j.r.plane[p] % 4 + 4 - (j.r.w0 * (uint64_t)elem_size) % 4) % 4 != 0) return false;
    return true;
}
hipError_t launch_bitswap1_decode_range_windows_project_walk(const uint8_t* in, const Bitswap1BoxProjectJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs,
                                                             uint32_t ngroups, int elem_size, const uint16_t* lut, hipStream_t stream);
// The projection of boxes of a DENSE volume (the compaction of `lz4` and `frame_shuffle->lz4` blobs, the whole decode): a thread per image
// element walks the axis -- element (u, v) reads dense[base + u su + v sv + k sa], k < n, and stores out[u p0 + v] once: no atomics, and
// no neutral elements beforehand.  Job j owns ceil(E0 E1 / 256) workgroups; d_first_tile their prefix sums.
struct BoxProjectJob {
    const void* dense;
    void* out;
    uint64_t base, E0, E1, p0, su, sv, sa, n;
    uint32_t op, pad0;
    uint64_t pad1;
};
constexpr uint64_t kBoxProjectJobBytes = 96;
hipError_t launch_boxes_window_project(const BoxProjectJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, int elem_size, hipStream_t stream);
// ---- many boxes of one large blob read at a coarser resolution (SQYAMD_Bin_Boxes_*) ----
// No global atomics, no neutral elements beforehand, every output cell stored once.  Job j is a box (g: the blob's rows and the box; g.sz,
// g.sy the OUTPUT's pitches in elements from cell layer to layer and cell row to row), its range, its clamped bins and the tiling of its
// cell grid (sqy::bin_boxes_plan); it owns plan.blocks workgroups, d_first_tile their prefix sums.  Workgroup `own` takes the block
// sqy::bin_block_of(plan, own): it sets the block's accumulators in LDS to the op's neutral element, its threads share the block's items
// (sqy_batch_window.hpp: a 32-voxel run of a footprint frame each; zreg != 0: the run's positions reduced over the layer's frames in
// registers first -- only where bitswap1_box_bin_zreg_ok), load the run's owned plane words -- four bytes of a plane at once where that
// lies on the 4-byte grid and the run's words all belong to the range, word by word elsewhere; tail voxels verbatim --, transpose, look
// up, reduce each cell's row piece in registers (sqy::bin_run_cells) and combine it into LDS with an LDS integer atomic; behind a barrier
// the cells go out with plain 32-bit stores, a cell row's columns in consecutive threads.  A run with no voxel of the footprint loads no
// plane word.  Every job must pass bitswap1_box_bin_job_ok.  Nothing but the outputs' cells is written.
struct Bitswap1BoxBinJob {
    void* out;
    WindowGeometry g;
    Bitswap1Range r;
    uint64_t t0;             // (Bitswap1BoxJob's field; not used: a block finds its words from its footprint)
    uint64_t bins[3];
    BinPlan plan;
    uint32_t op, zreg;
};
constexpr uint64_t kBitswap1BoxBinJobBytes = 368;       // (a multiple of 16: the tile table behind the jobs stays on the 16-byte grid)
bool bitswap1_box_bin_job_ok(const Bitswap1BoxBinJob& j);
// a frame is a whole number of 32-voxel runs (so the blob has no tail and every run of the box's frames lies in the range's words)
inline bool bitswap1_box_bin_zreg_ok(const Bitswap1BoxBinJob& j) { const uint64_t frame = j.g.bY * j.g.bX; return frame != 0 && frame % 32 == 0; }
hipError_t launch_bitswap1_decode_range_windows_bin(const uint8_t* in, const Bitswap1BoxBinJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups,
                                                    int elem_size, const uint16_t* lut, hipStream_t stream);
// The binning of boxes of a DENSE volume (the compaction of `lz4` and `frame_shuffle->lz4` blobs, the whole decode): a thread per output
// cell walks the cell's voxels -- cell (cz, cy, cx) reads dense[base + z plane + y row + x] over [c bins, min((c + 1) bins, extent)) --
// and stores out[cz pz + cy py + cx] once.  Job j owns ceil(C[0] C[1] C[2] / 256) workgroups; d_first_tile their prefix sums.
struct BoxBinJob {
    const void* dense;
    void* out;
    uint64_t base, plane, row;
    uint64_t E[3], bins[3], C[3];
    uint64_t pz, py;
    uint32_t op, pad0;
    uint64_t pad1;
};
constexpr uint64_t kBoxBinJobBytes = 144;
hipError_t launch_boxes_window_bin(const BoxBinJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, int elem_size, hipStream_t stream);
// ---- a whole resolution pyramid of many boxes of one large blob (SQYAMD_Pyramid_Boxes_*) ----
// Bitswap1BoxBinJob with an output, its pitches and a cell grid per level: job j is a box, its range, its level-0 bins (clamped) and its
// sqy::PyramidPlan; it owns plan.blocks workgroups, d_first_tile their prefix sums.  Workgroup `own` takes the block
// sqy::bin_block_of(pyramid_top_plan(plan), own) of level-T cells and walks the level-0 cell layers under it one after another: the
// accumulators of the layer set to the op's neutral element, the layer's items shared by the threads exactly as in
// launch_bitswap1_decode_range_windows_bin (the same device functions; zreg the same), behind a barrier the layer stored with plain
// stores and folded LDS to LDS into the level-1 accumulators at plan.off[1] (a thread per level-1 cell: sqy::pyramid_fold_cell), a
// level-1 layer that is complete stored and folded into level 2, and so on up to T.  Every cell of the levels 0 .. T is stored once; no
// global atomic, no neutral-element launch; no plane word is loaded twice within a block.  Static LDS: sqy::kPyramidLdsCells
// accumulators (40 KiB) and the look-up, under 64 KiB.  Every job must pass bitswap1_box_pyramid_job_ok.  Nothing but the outputs' cells is
// written.  The levels above T are launch_pyramid_reduce's.
struct Bitswap1BoxPyramidJob {
    void* out[kPyramidMaxLevels];
    uint64_t pz[kPyramidMaxLevels], py[kPyramidMaxLevels];         // level l's pitches in elements from cell layer to layer and cell row to row
    WindowGeometry g;                                               // (sz, sy not used: the pitches stand per level)
    Bitswap1Range r;
    uint64_t t0;             // (Bitswap1BoxJob's field; not used)
    uint64_t bins[3];        // level 0's, clamped to the extent
    PyramidPlan plan;
    uint32_t op, zreg;
    uint64_t pad;
};
constexpr uint64_t kBitswap1BoxPyramidJobBytes = 1152;  // (a multiple of 16: the tile table behind the jobs stays on the 16-byte grid)
bool bitswap1_box_pyramid_job_ok(const Bitswap1BoxPyramidJob& j);
hipError_t launch_bitswap1_decode_range_windows_pyramid(const uint8_t* in, const Bitswap1BoxPyramidJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs,
                                                        uint32_t ngroups, int elem_size, const uint16_t* lut, hipStream_t stream);
// A level of a pyramid from a stored finer one: a thread per cell of `out` (grid C, pitches pz, py) reduces the cells
// [c r, min((c + 1) r, Cs)) per dimension of `src` (grid Cs, pitches spz, spy; uint32_t both) and stores its cell once.  No atomics.  Job
// j owns ceil(C[0] C[1] C[2] / 256) workgroups; d_first_tile their prefix sums.  `src` is written by a launch in front on the stream.
struct PyramidReduceJob {
    const void* src;
    void* out;
    uint64_t Cs[3], C[3], r[3];
    uint64_t spz, spy, pz, py;
    uint32_t op, pad0;
};
constexpr uint64_t kPyramidReduceJobBytes = 128;
hipError_t launch_pyramid_reduce(const PyramidReduceJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, hipStream_t stream);
// ---- the intensity histograms of many boxes of one large blob (SQYAMD_Histogram_Boxes_*) ----
// launch_bitswap1_decode_range_windows_compare with a count where it compares: job j is a Bitswap1BoxJob whose `view` is the box's
// histogram -- nbins = (65536 or 256) >> shift counters of uint32_t, dense; the 16-bit range behind the look-up --, the tables, the
// groups and bitswap1_box_job_ok as there.  A workgroup counts the box's voxels of its 32768 into a private LDS array of
// sqy::hist_window_bins(nbins) counters (sqy_batch_window.hpp: the whole histogram up to 16384 bins, else a window voted from the first
// voxel each thread counts; bins outside it go to the output by a no-return global atomic), and behind a barrier adds its non-zero
// counters into the output with no-return 32-bit atomics at device scope; zero counters issue nothing.  merge: how equal
// neighbours are added, sqy::kHistMergeNone, kHistMergeRuns or kHistMergePieces.  A thread whose run holds nothing of the box loads no
// plane word but reaches every barrier; a workgroup in which no thread holds a voxel of the box returns before it zeroes anything.  The histograms hold zeros beforehand: launch_boxes_histogram_init over the SAME tables, in front on the stream --
// workgroup `own` of a job's groups zeroes the counters own 256 + tid, + groups 256, ...  Nothing but the histograms is written.
hipError_t launch_boxes_histogram_init(const Bitswap1BoxJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, uint32_t nbins, hipStream_t stream);
hipError_t launch_bitswap1_decode_range_windows_histogram(const uint8_t* in, const Bitswap1BoxJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups,
                                                          int elem_size, const uint16_t* lut, uint32_t shift, int merge, hipStream_t stream);
// The histograms of boxes of a DENSE volume (the compaction of `lz4` and `frame_shuffle->lz4` blobs, the whole decode): the grid of
// launch_batch_window_compare -- job j is a BatchWindowJob whose `view` is the box's histogram and whose `dense` is the volume (sz, sy,
// tile0 are not read), a workgroup per 32768 voxels of the box, its rows gathered sixteen bytes at a time -- with the same LDS
// histogram, vote and flush.  elem_size: of a voxel of the dense volume (2 behind the quantiser's whole decode).  The init launch takes
// these tables too.
hipError_t launch_boxes_histogram_init(const BatchWindowJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, uint32_t nbins, hipStream_t stream);
hipError_t launch_boxes_window_histogram(const BatchWindowJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ngroups, int elem_size, uint32_t shift,
                                         int merge, hipStream_t stream);
// ---- a box written into one large blob (SQYAMD_Update_Box_*) ----
// launch_bitswap1_decode_range_window the other way round, in place: the box's voxels are read from the view (box.view; `dense` and tile0
// are not read) and merged into the plane words [w0, w1) and the tail of the range r inside the compaction at buf (launch_bitswap1_batch_patch's
// mask and merge).  The range must hold the box (bitswap1_range_patch_ok; refused otherwise).  A thread touches only the words of its own
// 128-voxel run, and only where the box has a voxel in them; nothing else of buf and nothing of the view is written.
bool bitswap1_range_patch_ok(const Bitswap1Range& r, const BatchWindowJob& box, int elem_size);
hipError_t launch_bitswap1_range_patch(uint8_t* buf, const Bitswap1Range& r, const BatchWindowJob& box, int elem_size, hipStream_t stream);
// ---- many boxes written into one large blob (SQYAMD_Update_Boxes_*) ----
// launch_bitswap1_range_patch for a table of SEGMENTS (sqy::update_boxes_plan: no plane word and no tail voxel belongs to two of them)
// in ONE launch.  Segment s has its range r inside the one compaction at buf, t0 = sqy::range_first_thread(r.w0, words per thread) and
// the boxes d_boxes[box0 .. box0 + nbox) in ascending box order, every one inside the range (bitswap1_patch_tables_ok; refused
// otherwise).  d_first_tile: nsegs + 1 words, the prefix sums of sqy::range_job_groups(r.w0, r.w1, words per thread); ngroups their sum.
// A thread owns the words of its 128-voxel run as in the single-box kernel and walks its segment's boxes in that order, a later box
// over an earlier one, so every word is read and written by one thread: boxes that overlap, and disjoint boxes that share a word, need
// no atomics and no second launch.  Nothing else of buf and nothing of the views is written.
struct Bitswap1PatchSegment {
    Bitswap1Range r;
    uint64_t t0;
    uint32_t box0, nbox;
};
struct Bitswap1PatchBox {
    const void* view;
    WindowGeometry g;
    uint64_t pad;
};
constexpr uint64_t kBitswap1PatchSegmentBytes = 192, kBitswap1PatchBoxBytes = 96;       // (multiples of 16: the tables behind one another stay on the 16-byte grid)
bool bitswap1_patch_tables_ok(const Bitswap1PatchSegment* segs, uint32_t nsegs, const Bitswap1PatchBox* boxes, uint32_t nboxes, int elem_size);
hipError_t launch_bitswap1_range_patches(uint8_t* buf, const Bitswap1PatchSegment* d_segs, const Bitswap1PatchBox* d_boxes, const uint32_t* d_first_tile, uint32_t nsegs,
                                         uint32_t ngroups, int elem_size, hipStream_t stream);
// ---- batch decode (SQYAMD_Decode_Batch_*): the blobs of a group share one launch of every kernel ----
// The inverse of launch_bitswap1_batch on the same tables: job j's planes + tail at `in` (16-byte aligned) become its `len` voxels at
// `out` (any voxel-aligned address; sixteen-byte stores where it and the plane size allow, word by word where not).  first_tile: njobs + 1
// words, the prefix sums of batch_bitswap1_tiles(len) (sqy::decode_batch_plan makes them)
hipError_t launch_bitswap1_decode_batch(const Bitswap1Job* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, int elem_size, hipStream_t stream);
// plain copies on the same kind of table: job j's `len` BYTES from `in` to `out`, first_tile the prefix sums of batch_bitswap1_tiles(bytes)
hipError_t launch_batch_copy(const Bitswap1Job* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, hipStream_t stream);
// `quantiser->bitswap1->lz4` blobs on the same kind of table: job j's 8 planes + tail of `len` quantised voxels at `in` (16-byte aligned) become
// `len` 16-bit voxels at `out` (any voxel-aligned address) through the decode table d_luts[256 j .. 256 j + 256)
hipError_t launch_bitswap1_quantiser_decode_batch(const Bitswap1Job* d_jobs, const uint32_t* d_first_tile, const uint16_t* d_luts, uint32_t njobs, uint32_t ntiles,
                                                  hipStream_t stream);
// The diff3x3x1 inverses of many 16-bit volumes in the chain geometry (diff3x3x1_decode_chain_columns != 0, diff3x3x1_decode_frames_fit of
// it): job j's residual volume of Z x Y x X voxels at `in`, the decoded one to `out` (both 16-byte aligned, apart), w its chain columns.
// _copy: one launch for frame 0, the frames that cannot change and the columns right of the chain of all jobs (d_first_tile: the prefix sums
// of batch_bitswap1_tiles(Z Y X)).  _step, behind it, for step = 0, 1, ..: one launch that decodes frames [1 + 8 step, 9 + 8 step) of every
// job that has them, a workgroup per strip of 32 rows (d_first_strip: the prefix sums of ceil(Y / 32)); max_columns: the largest w of the
// table.  (sqy::decode_batch_plan makes the tables and counts the steps)
struct DiffBatchJob { const void* in; void* out; uint32_t Z, Y, X, w; };
bool diff3x3x1_decode_frames_fit(uint64_t w);
hipError_t launch_diff3x3x1_decode_batch_copy(const DiffBatchJob* d_jobs, const uint32_t* d_first_tile, uint32_t njobs, uint32_t ntiles, hipStream_t stream);
hipError_t launch_diff3x3x1_decode_batch_step(const DiffBatchJob* d_jobs, const uint32_t* d_first_strip, uint32_t njobs, uint32_t nstrips, uint32_t step,
                                              uint32_t max_columns, hipStream_t stream);
// one launch per frame over the columns the stage can touch (frame z needs the decoded frame z-1), the other columns one plain copy
// -- on copy_stream next to the chain when that, fork and join are given.  (scratch: unused since round 3)
// diff3x3x1_decode_chain_columns: how many leading columns of a row go through that chain in the usual 16-bit geometry (a multiple of 8;
// 0: another geometry).  left_tmp != nullptr (that geometry, in == out, both 16-byte aligned): the volume is decoded where it lies --
// the encoded chain columns are first copied to left_tmp (same indices, a buffer of the volume's size), nothing else moves
uint64_t diff3x3x1_decode_chain_columns(uint64_t Z, uint64_t Y, uint64_t X, int elem_size);
hipError_t launch_diff3x3x1_decode(const void* in, void* out, uint64_t Z, uint64_t Y, uint64_t X, int elem_size, void* scratch,
                                   hipStream_t stream, bool schar = false, hipStream_t copy_stream = nullptr, hipEvent_t fork = nullptr,
                                   hipEvent_t join = nullptr, void* left_tmp = nullptr);
hipError_t launch_quantiser_decode(const uint8_t* in, uint16_t* out, uint64_t len, const uint16_t* lut, hipStream_t stream);
hipError_t launch_frame_scatter(const void* in, void* out, uint64_t Z, uint64_t frame_bytes, const uint64_t* map, hipStream_t stream);

} // namespace sqy
#endif
