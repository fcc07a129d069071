/*
 * sqeazy_amd.h -- C-ABI of libsqeazy_amd.so, the MI355X-native drop-in for sqeazy's pipeline
 * encode path (filter stages + LZ4 block compression).
 *
 * Section A re-declares, with identical names, argument order and meaning, the entry points of the
 * reference's libsqeazy that belong to this path.  Each declaration cites the reference interface
 * it replaces (paths relative to /root/reference/src/cpp): `inc/sqeazy.h` for the declaration and
 * `src/sqeazy.cpp` for the behaviour.  A maintainer binds them exactly as they bind libsqeazy
 * today.  All pointers are HOST pointers; the library stages data through
 * HBM itself.  Return convention: 0 success, 1 failure ("[sqeazy]\t..." on stderr), never throws.
 *
 * Section B adds entry points for callers whose volumes already live in MI355X HBM.
 *
 * No HDF5 entry points (SQY_h5_*): out of scope of the hot path.
 */
#ifndef SQEAZY_AMD_H_
#define SQEAZY_AMD_H_

#ifdef __cplusplus
#define SQY_FUNCTION_PREFIX extern "C" __attribute__((visibility("default")))
#else
#include <stdbool.h>
#define SQY_FUNCTION_PREFIX __attribute__((visibility("default")))
#endif

/* ------------------------------------------------------------------------------------------------
 * Section A -- sqeazy's own C-ABI for the pipeline path
 * ---------------------------------------------------------------------------------------------- */

/* inc/sqeazy.h:26, src/sqeazy.cpp:16-22.  *length in: bytes available at src; out: header bytes
 * (JSON + "|01307#!" delimiter, including leading pad). */
SQY_FUNCTION_PREFIX int SQY_Header_Size(const char* src, long* length);

/* inc/sqeazy.h:41, src/sqeazy.cpp:24-33.  *num in: bytes at src; out: rank of the stored volume. */
SQY_FUNCTION_PREFIX int SQY_Decompressed_NDims(const char* src, long* num);

/* inc/sqeazy.h:56, src/sqeazy.cpp:35-46.  shape[0] in: bytes at src; out: shape[0..rank) = {z,y,x}. */
SQY_FUNCTION_PREFIX int SQY_Decompressed_Shape(const char* src, long* shape);

/* inc/sqeazy.h:70, src/sqeazy.cpp:48-58.  *Sizeof in: bytes at src; out: bytes per voxel. */
SQY_FUNCTION_PREFIX int SQY_Decompressed_Sizeof(const char* src, long* Sizeof);

/* inc/sqeazy.h:81, src/sqeazy.cpp:61-69.  version[0..3) = major, minor, patch. */
SQY_FUNCTION_PREFIX int SQY_Version_Triple(int* version);

/* inc/sqeazy.h:109-115, src/sqeazy.cpp:72-106.  Encode a uint8 volume.
 *   pipeline    e.g. "frame_shuffle->lz4"; must satisfy SQY_Pipeline_Possible_UI8
 *   src         contiguous voxels, row-major {z,y,x}, x fastest
 *   shape       long[shape_size], voxels per dimension
 *   dst         at least SQY_Pipeline_Max_Compressed_Length_* bytes
 *   dstlength   out only: bytes written (header + payload)
 *   nthreads    <=0 or > hardware threads: all hardware threads (src/sqeazy_algorithms.hpp:14-22).  The value selects
 *               the LZ4 LAYOUT exactly as in the reference (encoders/lz4.hpp:227-239): effective 1 -> ONE frame of
 *               block-linked 256 KiB blocks (lz4_utils.hpp:99-173; bit-identical).  Its blocks are parsed in parallel from hash-table
 *               guesses that are verified and parsed again, in order, where they fail: 2-4 x the chunked layout's time on ordinary
 *               stacks (3 ms against 1.4 for a 1 GiB stack, 21 ms against 5.4 for a diff3x3x1 slab of 2 GiB) -- but SECONDS where no
 *               guess holds: a stream of short sequences such as the top plane of quantised data (511 blocks in a row, one wavefront,
 *               ~10 ms per block: 4.7 s for a 2048x2048x256 slab of quantiser->bitswap1->lz4, slower than one CPU core; the library
 *               says so once on stderr).  >=2 -> one independent frame per 256 KiB chunk (lz4_utils.hpp:193-274; byte-identical for
 *               every count >= 2; the fast path: 12 ms for that slab).  Same decoder for both. */
SQY_FUNCTION_PREFIX int SQY_PipelineEncode_UI8(const char* pipeline, const char* src, long* shape, unsigned shape_size,
                                               char* dst, long* dstlength, int nthreads);

/* inc/sqeazy.h:140-146, src/sqeazy.cpp:108-142.  Same for uint16 voxels (little endian). */
SQY_FUNCTION_PREFIX int SQY_PipelineEncode_UI16(const char* pipeline, const char* src, long* shape, unsigned shape_size,
                                                char* dst, long* dstlength, int nthreads);

/* inc/sqeazy.h:159-161 / :190, src/sqeazy.cpp:144-183.  *length in: raw bytes; out: upper bound of
 * the encoded blob = 2*header + max over stages (dynamic_pipeline.hpp:866-890). */
SQY_FUNCTION_PREFIX int SQY_Pipeline_Max_Compressed_Length_UI8(const char* pipeline, long pipeline_length, long* length);
SQY_FUNCTION_PREFIX int SQY_Pipeline_Max_Compressed_Length_UI16(const char* pipeline, long pipeline_length, long* length);

/* inc/sqeazy.h:175-178 / :204-207, src/sqeazy.cpp:185-231.  *length in: strlen(pipeline) (sic); out: bound. */
SQY_FUNCTION_PREFIX int SQY_Pipeline_Max_Compressed_Length_3D_UI8(const char* pipeline, long* shape, unsigned shape_size, long* length);
SQY_FUNCTION_PREFIX int SQY_Pipeline_Max_Compressed_Length_3D_UI16(const char* pipeline, long* shape, unsigned shape_size, long* length);

/* inc/sqeazy.h:219-243, src/sqeazy.cpp:233-268.  true iff the string parses as head filters -> sink -> tail filters
 * (src/sqeazy_pipelines.hpp:31-77) AND every stage is implemented here.  Head filters: diff3x3x1, bitswap1, bitshuffle,
 * raster_reorder, tile_shuffle, frame_shuffle, zcurve_reorder, rmestbkrd, rmbkrd_neighbor5x5x5 (threshold / fraction that std::stoi /
 * std::stof accept, a finite fraction; {Z, Y, X} shapes only, see DESIGN.md 7 for the shapes refused at encode time); sinks: pass_through, quantiser (16-bit input; every
 * weighting_function with a finite exponent, decode_lut_path), lz4 (accel <= 2, negative = liblz4's acceleration; last stage);
 * tail filters on the sink's `char` stream: diff3x3x1, bitswap1, bitshuffle, lz4, raster_reorder, tile_shuffle, frame_shuffle,
 * zcurve_reorder -- the reference's whole list but the video codecs.  false where the reference says true: remove_background,
 * the video sinks / filters (h264, hevc), lz4 with accel >= 3 (LZ4HC),
 * stages behind an lz4 sink.  (A geometry the reference leaves undefined for a stage is refused at encode time: error 1.) */
SQY_FUNCTION_PREFIX bool SQY_Pipeline_Possible_UI16(const char* pipeline_string);
SQY_FUNCTION_PREFIX bool SQY_Pipeline_Possible_UI8(const char* pipeline_string);
SQY_FUNCTION_PREFIX bool SQY_Pipeline_Possible(const char* pipeline_string, int sizeofpixel);

/* inc/sqeazy.h:255, src/sqeazy.cpp:270-279.  *length in: bytes at data; out: decoded bytes. */
SQY_FUNCTION_PREFIX int SQY_Decompressed_Length(const char* data, long* length);

/* inc/sqeazy.h:274-299, src/sqeazy.cpp:281-335.  Decode a blob produced by SQY_PipelineEncode_* (either
 * LZ4 layout).  dst must hold SQY_Decompressed_Length bytes. */
SQY_FUNCTION_PREFIX int SQY_Decode_UI16(const char* src, long srclength, char* dst, int nthreads);
SQY_FUNCTION_PREFIX int SQY_Decode_UI8(const char* src, long srclength, char* dst, int nthreads);

/* ------------------------------------------------------------------------------------------------
 * Section B -- HBM-resident variants (no reference counterpart; same semantics as above)
 * ---------------------------------------------------------------------------------------------- */

/* d_src / d_dst are device pointers on the current HIP device; dst_capacity is checked (1 when the
 * blob does not fit).  hip_stream is a hipStream_t (NULL = default stream).  The call returns after the
 * blob is complete in d_dst.  Ordering: the call starts behind everything queued on hip_stream at the time of the call (whatever made
 * d_src has to be in front of it there, or complete) and is complete on return; work on OTHER streams that touches d_src or d_dst is
 * the caller's to synchronise.  The work itself runs on hip_stream -- or, for the frames-in-place path of the _DeviceAt entry points
 * below where the option "stage_lanes" says so, on streams of the library's own. */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI16_Device(const char* pipeline, const void* d_src, const long* shape,
                                                          unsigned shape_size, void* d_dst, long dst_capacity,
                                                          long* dstlength, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI8_Device(const char* pipeline, const void* d_src, const long* shape,
                                                         unsigned shape_size, void* d_dst, long dst_capacity,
                                                         long* dstlength, int nthreads, void* hip_stream);
/* The same, but the blob may start anywhere inside [d_dst, d_dst + dst_capacity): *dstoffset says where, *dstlength how long it is
 * (bytes identical to the entry points above).  This is the fast path: for `...->bitswap1->lz4` on 16-bit voxels the bit-plane
 * transpose writes the plane stream straight into d_dst as the bodies of the LZ4 frames it will become (one frame per 256 KiB
 * chunk, encoders/lz4_utils.hpp:193-274); the stored frames that end the payload -- the noise planes, 98 % of the payload of a
 * microscopy stack -- then never move, only the compressed frames in front of them are gathered (no second pass over the
 * payload).  dst_capacity as above; every other pipeline returns *dstoffset = 0.
 * Lanes ("stage_lanes" = 1, or 2 with "transpose_chain_caller_streams" on): a frames-in-place call waits on the CALLING THREAD until everything queued on hip_stream is complete
 * (it polls; nothing is queued on hip_stream), then runs on the library's lanes of the device -- one stream for the bit-plane
 * transposes of all such calls, in call order, and "parse_lanes" streams for what follows, dealt to the calls in flight -- and returns
 * when its blob is complete.  The lanes are 1 + parse_lanes plain non-blocking streams per device, created on first use; with them
 * it is the library, not the number of streams its callers happen to bring, that decides which kernels of the calls in flight can
 * run side by side on the hardware queues the process has.  A hip_stream that still has work in flight after 2 ms (a backlog)
 * delays nobody: that call runs on hip_stream itself, as with "stage_lanes" = 0 (a stage of the call's own in front of the transpose,
 * diff3x3x1, runs on hip_stream too and is waited for the same way: one host round trip inside the call, and a stage longer than
 * 2 ms keeps the call on hip_stream).  A call that finds no other call on the lanes first asks the two lanes it would take for an
 * answer (a marker each, 0.25 ms at most): a lane that does not answer has a kernel of some other stream in front of it in its
 * hardware queue, and the call stays on hip_stream.  With other calls on the lanes that is not asked, and such a kernel holds up the
 * calls on the lane it blocks -- the reason for the default of "stage_lanes". */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI16_DeviceAt(const char* pipeline, const void* d_src, const long* shape,
                                                            unsigned shape_size, void* d_dst, long dst_capacity, long* dstoffset,
                                                            long* dstlength, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI8_DeviceAt(const char* pipeline, const void* d_src, const long* shape,
                                                           unsigned shape_size, void* d_dst, long dst_capacity, long* dstoffset,
                                                           long* dstlength, int nthreads, void* hip_stream);
/* As _DeviceAt; additionally tells where every `every`-th LZ4 frame of the payload starts (pipelines that end in lz4 in the
 * chunked layout, one frame per chunk: encoders/lz4_utils.hpp:193-274): frame_offsets[i] = start of frame i * every relative to
 * the blob start, i = 0 .. *count - 1, and frame_offsets[*count] = the blob length (max_entries >= *count + 1, else 1).  With
 * every = chunks per bit plane this is the byte range of every bit plane of a `bitswap1->lz4` blob -- what the single-blob mode of
 * the multi-GPU path re-orders (the frame sizes come from the encoder's own table in HBM, nobody walks the frames). */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI16_DeviceAt_Frames(const char* pipeline, const void* d_src, const long* shape,
                                                                   unsigned shape_size, void* d_dst, long dst_capacity,
                                                                   long* dstoffset, long* dstlength, int nthreads, void* hip_stream,
                                                                   int every, long* frame_offsets, int max_entries, int* count);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI8_DeviceAt_Frames(const char* pipeline, const void* d_src, const long* shape,
                                                                  unsigned shape_size, void* d_dst, long dst_capacity,
                                                                  long* dstoffset, long* dstlength, int nthreads, void* hip_stream,
                                                                  int every, long* frame_offsets, int max_entries, int* count);
/* A whole volume as `nslabs` independent z-slab blobs with ONE call (the reference encodes one volume of < 2^31 voxels per call,
 * src/sqeazy.cpp:108-142; larger volumes are cut into z-slabs by its callers).  shape is the WHOLE volume {z,y,x}; slab i holds
 * frames [i*(Z/n) + min(i, Z%n), ...) -- the first Z % nslabs slabs get one frame more -- and is encoded exactly as
 * SQYAMD_PipelineEncode_*_DeviceAt would encode it (every blob is a complete sqeazy blob, bytes identical to the single calls).
 * Blob i lies inside d_dst[i*slab_capacity, (i+1)*slab_capacity) (slab_capacity >= SQY_Pipeline_Max_Compressed_Length_3D_* of the
 * largest slab): offsets[i] = its start relative to d_dst, lengths[i] = its bytes.  `inflight` slab calls (<= 0: three) run at a
 * time on library-owned streams: the transposes, LZ4 parses and gathers of different slabs overlap.  Returns when all are done.
 * Ordering: the slab calls start behind everything queued on the DEFAULT stream when the call is made (the kernels that made d_src, a
 * fill of d_dst); work on other streams that touches d_src or d_dst has to be complete (synchronised) before the call. */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_Slabs_UI16_Device(const char* pipeline, const void* d_src, const long* shape,
                                                                unsigned shape_size, int nslabs, void* d_dst, long slab_capacity,
                                                                long* offsets, long* lengths, int nthreads, int inflight);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_Slabs_UI8_Device(const char* pipeline, const void* d_src, const long* shape,
                                                               unsigned shape_size, int nslabs, void* d_dst, long slab_capacity,
                                                               long* offsets, long* lengths, int nthreads, int inflight);
/* Many small volumes -- tiles, time points, dataset chunks: separately allocated, shapes may differ -- as one blob each with ONE call.
 * d_srcs: a HOST array of nvolumes device pointers, each aligned at least to the voxel size.  shapes: a host array of nvolumes x
 * shape_size longs, row i = volume i's {z,y,x}.  Blob i is written inside d_dst[i*slot_capacity, (i+1)*slot_capacity) and nothing
 * outside a volume's own slot is written; offsets[i] = its start relative to d_dst, lengths[i] = its bytes (host arrays, as for
 * _Slabs_*_Device).  Blob i is byte for byte what SQYAMD_PipelineEncode_*_Device gives for volume i with the same pipeline and nthreads.
 * Volumes of `lz4`, `bitswap1->lz4` and -- 16-bit voxels, the quantiser with its default weighting (no weighting_function) and its decode
 * LUT in the header (no decode_lut_path) -- `quantiser->bitswap1->lz4` in the chunked layout (nthreads != 1 or a single chunk) with
 * liblz4's acceleration 1 and at most "encode_batch_joint_max_bytes" of LZ4 input (a byte per voxel behind the quantiser) are encoded in
 * groups ("encode_batch_group_bytes" of LZ4 input each -- a quantised volume also counts its tables, 320.5 KiB --, at least one volume):
 * per group one launch of every kernel for all its volumes and two host round trips, whatever their number; their blobs start at the
 * slot's first byte.  The quantiser's histograms and look-up tables are made on the GPU for the whole group; the tables are exactly the
 * single call's.  Every other volume (other pipelines, other weightings, a LUT file, the serial or block-linked layout, accel < 0, larger
 * volumes) is encoded as by _DeviceAt into its slot, in volume order on the same stream; a batch may mix both kinds.
 * Stream, context, ordering and thread-safety rules are those of SQYAMD_PipelineEncode_*_Device: the work runs behind what is queued
 * on hip_stream and is complete on return; several host threads may call at once.
 * Returns 0 or 1.  Bad arguments -- a NULL pointer (also in d_srcs), nvolumes <= 0, shape_size 0, slot_capacity <= 0, a non-positive
 * extent, a pipeline not admitted for the voxel type, a geometry the single call refuses for any volume, a misaligned source -- return
 * 1 before anything is written, with offsets and lengths zeroed.  A blob that does not fit its slot makes the call return 1 (offsets and
 * lengths zeroed); nothing of that volume is written, and no slot's neighbours are touched. */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_Batch_UI16_Device(const char* pipeline, const void* const* d_srcs, const long* shapes,
                                                                unsigned shape_size, int nvolumes, void* d_dst, long slot_capacity,
                                                                long* offsets, long* lengths, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_Batch_UI8_Device(const char* pipeline, const void* const* d_srcs, const long* shapes,
                                                               unsigned shape_size, int nvolumes, void* d_dst, long slot_capacity,
                                                               long* offsets, long* lengths, int nthreads, void* hip_stream);
/* _Batch_*_Device for views: volume i is a strided view of a larger resident allocation -- a tile of a dataset, a region of interest, a
 * padded or pitched volume -- encoded where it lies, without a dense copy of the caller's.  strides: a HOST array of nvolumes x shape_size
 * longs in VOXELS, row i = view i's strides, outermost dimension first.  The rules, all checked on the host before the device is touched
 * or anything is written (1, offsets and lengths zeroed): shape_size is 1, 2 or 3; the innermost stride is 1; every stride is positive and
 * stride[k] >= shape[k+1] * stride[k+1] (a view never overlaps itself); d_srcs[i] is aligned to the voxel size.  Only the view's voxels
 * are read.  strides == NULL: every view is dense and the call IS SQYAMD_PipelineEncode_Batch_*_Device (same kernels); the same holds for
 * any view whose strides are the dense ones.  Blob i is byte for byte what SQYAMD_PipelineEncode_*_Device gives for a dense copy of view
 * i; slots, offsets, lengths, capacity, errors, stream, context, ordering and thread safety are _Batch_*_Device's.
 * `bitswap1->lz4`: the group's transposer gathers its voxels from the views (no copy at all); `lz4`: one launch packs the group's views
 * into its stream workspace; every other pipeline: one launch packs the group's views into a workspace that counts against
 * "encode_batch_group_bytes", then as _Batch_*_Device.  "batch_strided_fused" = 0: packed copies for every pipeline. */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_BatchStrided_UI16_Device(const char* pipeline, const void* const* d_srcs, const long* shapes,
                                                                       const long* strides, unsigned shape_size, int nvolumes, void* d_dst,
                                                                       long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_BatchStrided_UI8_Device(const char* pipeline, const void* const* d_srcs, const long* shapes,
                                                                      const long* strides, unsigned shape_size, int nvolumes, void* d_dst,
                                                                      long slot_capacity, long* offsets, long* lengths, int nthreads, void* hip_stream);
/* _BatchStrided_*_Device into ONE packed buffer: the blobs back to back in d_dst with an index of (offset, length) -- a shard of a chunked
 * store, a container file, one device-to-host copy of exactly the compressed bytes -- instead of a slot of max_compressed_length each.
 * d_srcs, shapes, strides (NULL: dense volumes), pipeline, nthreads, stream, context, ordering and thread safety are
 * _BatchStrided_*_Device's, and so is the admission: on the host, before the device is touched.  Blob i is byte for byte what
 * SQYAMD_PipelineEncode_*_Device gives for a dense copy of volume i.
 * Placement: the blobs lie in volume order, offsets[0] = 0, offsets[i+1] = round_up(offsets[i] + lengths[i], align), *total =
 * offsets[n-1] + lengths[n-1]; all of it in 64 unsigned bits.  align is a power of two, 1 <= align <= 65536 (anything else: 1 before
 * anything is written).  Offsets are relative to d_dst, which needs no alignment.  The call writes the blobs' bytes and nothing else: no
 * byte in front of d_dst, none at or behind d_dst + dst_capacity, no gap byte between two blobs.
 * Capacity: when the packed blobs do not fit dst_capacity the call returns 1 with offsets and lengths zeroed and *total = the capacity
 * a retry needs -- every volume is still compressed, so the figure is exact.  Blobs that lie wholly inside the capacity may have been
 * written, nothing else is.  Every other failure -- bad arguments (those of _BatchStrided_*_Device, total == NULL, dst_capacity <= 0, a
 * bad align), a refused geometry, a payload that overflows the reference's int -- returns 1 with offsets, lengths and *total zeroed.  A
 * caller who wants no retry passes the sum of round_up(SQY_Pipeline_Max_Compressed_Length_3D of volume i, align).
 * The joint-eligible volumes (see _Batch_*_Device) take the group's launches plus one placement scan (one workgroup) between the frame
 * scan and the gather, which then writes every blob at its place; the number of host round trips is unchanged.  Every other volume is
 * encoded first, into a workspace slot of its max_compressed_length, and copied to its place at the end: volume order holds in a mixed
 * call too.  The way back is SQYAMD_Decode_Batch*_Device with the same offsets and lengths. */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_BatchPacked_UI16_Device(const char* pipeline, const void* const* d_srcs, const long* shapes,
                                                                      const long* strides, unsigned shape_size, int nvolumes, void* d_dst,
                                                                      long dst_capacity, long align, long* offsets, long* lengths, long* total,
                                                                      int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_BatchPacked_UI8_Device(const char* pipeline, const void* const* d_srcs, const long* shapes,
                                                                     const long* strides, unsigned shape_size, int nvolumes, void* d_dst,
                                                                     long dst_capacity, long align, long* offsets, long* lengths, long* total,
                                                                     int nthreads, void* hip_stream);
/* host-pointer variants (not tuned): every volume staged up, the device driver called once, ONE copy of *total bytes brought back to dst
 * -- the blobs and, for align > 1, the gap bytes between them, which are zeros.  Capacity and errors as above. */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_BatchPacked_UI16(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size,
                                                               int nvolumes, char* dst, long dst_capacity, long align, long* offsets, long* lengths,
                                                               long* total, int nthreads);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_BatchPacked_UI8(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size,
                                                              int nvolumes, char* dst, long dst_capacity, long align, long* offsets, long* lengths,
                                                              long* total, int nthreads);
/* host-pointer variants: srcs[i] are host pointers, dst is host memory laid out the same way (only the blobs' bytes are written).  Every
 * volume is staged up, the device driver called once and the blobs brought back; the staging does not overlap with the encode */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_Batch_UI16(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size,
                                                         int nvolumes, char* dst, long slot_capacity, long* offsets, long* lengths, int nthreads);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_Batch_UI8(const char* pipeline, const char* const* srcs, const long* shapes, unsigned shape_size,
                                                        int nvolumes, char* dst, long slot_capacity, long* offsets, long* lengths, int nthreads);
/* host-pointer encode with an explicit destination capacity (returns 1 instead of overflowing dst; the
 * reference-protocol entry points above assume dst holds exactly SQY_Pipeline_Max_Compressed_Length_* bytes) */
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI16_Cap(const char* pipeline, const char* src, long* shape, unsigned shape_size,
                                                       char* dst, long dst_capacity, long* dstlength, int nthreads);
SQY_FUNCTION_PREFIX int SQYAMD_PipelineEncode_UI8_Cap(const char* pipeline, const char* src, long* shape, unsigned shape_size,
                                                      char* dst, long dst_capacity, long* dstlength, int nthreads);

SQY_FUNCTION_PREFIX int SQYAMD_Decode_UI16_Device(const void* d_src, long srclength, void* d_dst, long dst_capacity, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_UI8_Device(const void* d_src, long srclength, void* d_dst, long dst_capacity, void* hip_stream);

/* Frames [z0, z0 + nz) of a blob -- the index along shape[0], any rank -- decoded into d_dst: nz * (shape[1] * ... ) voxels,
 * exactly the bytes SQYAMD_Decode_*_Device writes at d_dst + z0 * frame_bytes.  Nothing outside [d_dst, d_dst + nz * frame_bytes)
 * is written.  Returns 1 for a bad range, a too-small dst_capacity, a blob of the other voxel type, or a malformed header.  A damaged
 * frame that the range needs gives SQY_Decode's composite code.
 * Stream, context and ordering rules are those of SQYAMD_Decode_*_Device (several host threads may call at once).  In the chunked LZ4
 * layout (nthreads >= 2 at encode time) of `lz4`, `bitswap1->lz4`, `quantiser->bitswap1->lz4` (16-bit) and `frame_shuffle->lz4`, each
 * optionally behind rmestbkrd / rmbkrd_neighbor5x5x5 heads, only the LZ4 frames the range needs are decoded (a damaged frame OUTSIDE
 * the range then goes unnoticed: DESIGN.md 7); every other blob is decoded whole into the library's workspace and the range copied
 * out -- same bytes, the full decode's time. */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Frames_UI16_Device(const void* d_src, long srclength, long z0, long nz, void* d_dst, long dst_capacity,
                                                         void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Frames_UI8_Device(const void* d_src, long srclength, long z0, long nz, void* d_dst, long dst_capacity,
                                                        void* hip_stream);
/* host-pointer variants: the blob is staged as in SQY_Decode_*, and only the range comes back */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Frames_UI16(const char* src, long srclength, long z0, long nz, char* dst, long dst_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Frames_UI8(const char* src, long srclength, long z0, long nz, char* dst, long dst_capacity);

/* A box of ONE blob decoded into a view of the box's shape: voxel k of the view (dst_shape, `rank` extents, outermost first) is voxel
 * origin + k of the volume SQYAMD_Decode_*_Device gives for the blob.  Exactly the box's voxels are written: the gaps between the view's
 * rows and frames and everything around the view keep their bytes.  dst_strides: the view's strides in voxels under the rules of
 * SQYAMD_Decode_BatchStrided_* (innermost 1, no dimension overlaps the next one's reach), NULL: dense.  d_dst is aligned to the voxel size.
 * Checked before anything is written, every refusal returns 1: NULL pointers, a negative origin, rank 0 or above 3, srclength <= 0 (these
 * before a device is looked for), the view rules, a blob of the other voxel type, a rank that is not the header's, an extent below 1,
 * origin + extent past the header's shape (a sum that overflows `long` is past it).  A damaged LZ4 frame that the box needs gives
 * SQY_Decode's composite code; the view may then hold anything.
 * Stream, context, ordering and thread-safety rules are those of SQYAMD_Decode_Frames_*_Device.  For the blobs of that call's subset path
 * only the LZ4 frames the box's range [origin[0], origin[0] + extent[0]) needs are decoded (a damaged frame OUTSIDE that range then goes
 * unnoticed: DESIGN.md 7), and the inverse bit-plane transposer stores the box's voxels straight into the view; every other blob is
 * decoded whole into the library's workspace and the box copied out -- same bytes, the full decode's time ("decode_box_subset" = 0:
 * every blob). */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Box_UI16_Device(const void* d_src, long srclength, const long* origin, void* d_dst, const long* dst_shape,
                                                      const long* dst_strides, unsigned rank, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Box_UI8_Device(const void* d_src, long srclength, const long* origin, void* d_dst, const long* dst_shape,
                                                     const long* dst_strides, unsigned rank, void* hip_stream);
/* host-pointer variants: the blob is staged as in SQY_Decode_*, the box comes back dense (extent[0] * .. voxels; 1 where dst_capacity,
 * in bytes, is less) */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Box_UI16(const char* src, long srclength, const long* origin, const long* extent, unsigned rank, char* dst,
                                               long dst_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Box_UI8(const char* src, long srclength, const long* origin, const long* extent, unsigned rank, char* dst,
                                              long dst_capacity);

/* MANY boxes of ONE blob in one call: box i is [origins + i rank, .. + dst_shapes + i rank) (count rows of `rank` longs each), its view at
 * d_dsts[i] with the strides dst_strides + i rank (NULL: every view dense) -- each box as by SQYAMD_Decode_Box_*_Device, the same bytes.
 * The header is fetched once, the LZ4 frames that the boxes' z-ranges need are united and decoded once by one launch, and ONE launch stores
 * the voxels of all boxes; blobs off the subset path are decoded whole ONCE and one window copy cuts all boxes out.  Boxes may overlap in
 * the blob; views that overlap each other are the caller's error, as in SQYAMD_Decode_BatchStrided_*.
 * Everything is checked before a byte is written, every refusal returns 1 with every destination untouched: the rules of
 * SQYAMD_Decode_Box_* for every box, count < 1, a NULL entry of d_dsts, more workgroups than one launch takes.  A damaged LZ4 frame that
 * SOME box needs gives SQY_Decode's composite code for the call; the views may then hold anything, nothing outside them is written.  A
 * damaged frame that no box needs goes unnoticed.  ("decode_boxes_joint" = 0: admitted as above, then SQYAMD_Decode_Box_* box by box.) */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, void* const* d_dsts,
                                                        const long* dst_shapes, const long* dst_strides, unsigned rank, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, void* const* d_dsts,
                                                       const long* dst_shapes, const long* dst_strides, unsigned rank, void* hip_stream);
/* host-pointer variants: the blob is staged ONCE, the boxes come back dense and back to back in box order (box i starts at the summed bytes
 * of boxes 0 .. i-1; 1 where dst_capacity, in bytes, is less than the sum of all) */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                 char* dst, long dst_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                char* dst, long dst_capacity);

/* The volume a set of z-slab blobs makes, decoded with one call: the inverse of SQYAMD_PipelineEncode_Slabs_*_Device and the reader of
 * the multi-GPU container.  Blob i lies at d_src + offsets[i], lengths[i] bytes (host arrays; any alignment).  Every blob is a complete sqeazy
 * blob of the entry point's voxel type; all have the same rank and the same shape[1..]; their shape[0] may differ.  Slab i's voxels land at
 * d_dst + (frames[0] + .. + frames[i-1]) * frame_bytes -- exactly the bytes SQYAMD_Decode_*_Device writes for that blob.
 * frames (host, may be NULL): out, shape[0] of every blob.  Nothing outside [d_dst, d_dst + volume bytes) is written.
 * Blobs that end in lz4 in the chunked layout (nthreads >= 2 at encode time) are decoded in groups: the frame index of every blob of a group
 * in one launch, one LZ4 decode launch for all of them, then each blob's remaining inverses into its place.  A group holds blobs while their
 * LZ4 output stays within 4 GiB (at least one); inflight > 0 also caps the blobs per group (<= 0: only the 4 GiB bound) -- it bounds the
 * workspace.  Every other blob (the serial layout, no lz4, a single chunk) is decoded on its own, as by SQYAMD_Decode_*_Device; a set may mix both.
 * Stream, context and ordering rules as SQYAMD_Decode_*_Device.  Return: 0, 1 (bad arguments / headers -- nslabs <= 0, a NULL pointer, an
 * invalid header, another voxel type, rank or shape[1..], a dst_capacity below the volume -- checked before anything is written), or the
 * composite code SQY_Decode gives the first damaged blob in slab order. */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Slabs_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nslabs,
                                                        void* d_dst, long dst_capacity, long* frames, int inflight, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Slabs_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nslabs,
                                                       void* d_dst, long dst_capacity, long* frames, int inflight, void* hip_stream);
/* host-pointer variants: the blobs staged as in SQY_Decode_*, the volume comes back */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Slabs_UI16(const char* src, const long* offsets, const long* lengths, int nslabs,
                                                 char* dst, long dst_capacity, long* frames);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Slabs_UI8(const char* src, const long* offsets, const long* lengths, int nslabs,
                                                char* dst, long dst_capacity, long* frames);

/* Many independent blobs -- tiles, time points, dataset chunks of any shape and pipeline -- decoded with ONE call, each into an allocation
 * of its own: the way back from SQYAMD_PipelineEncode_Batch_*, whose offsets and lengths can be passed straight through.  Blob i lies at
 * d_src + offsets[i], lengths[i] bytes (host arrays; any alignment) and is a complete sqeazy blob of the entry point's voxel type; rank,
 * shape and pipeline may differ from blob to blob.  d_dsts: a HOST array of nblobs device pointers, each aligned at least to the voxel
 * size, destination i dst_capacities[i] bytes long (host array).  decoded_bytes (host, may be NULL): out, every blob's decoded length.
 * Blob i's voxels are byte for byte what SQYAMD_Decode_*_Device writes for it; nothing outside [d_dsts[i], d_dsts[i] + decoded length)
 * is written.  Overlapping destinations are the caller's error and are not checked.
 * Blobs that end in lz4 with chunks of one LZ4 block (the chunked layout, or a single chunk) are decoded in groups ("decode_batch_group_bytes"
 * of LZ4 output each, at least one blob, one LZ4 block size): per group one frame-ranking launch, one LZ4 decode launch into the workspace,
 * one inverse-transpose launch for all its `bitswap1->lz4` blobs and one copy launch for all its `lz4` blobs, two host round trips.  16-bit
 * blobs only: one launch of the inverse transpose with the look-up for all its `quantiser->bitswap1->lz4` blobs (the decode table from the
 * header, or from decode_lut_path, as the single call reads it), and for all its `diff3x3x1->bitswap1->lz4` and `diff3x3x1->lz4` blobs whose
 * geometry lets the single call decode several frames per launch (every row's reach inside the row, X a multiple of 8, at most 320
 * columns that can change, a destination on the 16-byte grid) one launch per 8 frames of the deepest of them plus one -- the residual
 * volumes of `diff3x3x1->bitswap1->lz4` blobs take as much workspace again, which counts against "decode_batch_group_bytes".  Other
 * lz4-terminated pipelines run their remaining inverses blob by blob.  Every other blob (no lz4, the serial layout, chunks of several
 * blocks) is decoded as by SQYAMD_Decode_*_Device, in blob order on the same stream; a batch may mix both kinds.
 * Stream, context, ordering and thread-safety rules as SQYAMD_Decode_*_Device: the work runs behind what is queued on hip_stream and is
 * complete on return; several host threads may call at once.  Return (as SQYAMD_Decode_Slabs_*): 0, 1 (bad arguments / headers -- nblobs
 * <= 0, a NULL pointer, also inside d_dsts, a negative offset, a length <= 0, an invalid header, another voxel type, a capacity below the
 * decoded length, a misaligned destination -- all checked before anything is written, decoded_bytes zeroed), or the composite code
 * SQY_Decode gives the first damaged blob in blob order, returned after every blob has been decoded: the good ones are in place. */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Batch_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                        void* const* d_dsts, const long* dst_capacities, long* decoded_bytes, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Batch_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                       void* const* d_dsts, const long* dst_capacities, long* decoded_bytes, void* hip_stream);
/* _Batch_*_Device into views: blob i is decoded into the strided view d_dsts[i] of dst_shapes row i (shape_size longs) and dst_strides row
 * i (voxels; the rules of SQYAMD_PipelineEncode_BatchStrided_*, checked on the host before anything is written; NULL: dense views, the
 * call is _Batch_*_Device with the shapes checked).  The blob's header shape must equal its dst_shapes row, rank included (else 1 before
 * anything is written).  Exactly the view's voxels are written: the voxels in the gaps between its rows and frames are not touched.  Two
 * views of one call that overlap are the caller's error.  `bitswap1->lz4` and `lz4` blobs on the joint path are written into their views
 * by the group's last launch; every other blob is decoded into a workspace place, and ONE launch at the end of the call unpacks them all
 * ("batch_strided_fused" = 0: every blob).  Return codes, stream, context, ordering and thread safety as _Batch_*_Device; the offsets and
 * lengths of SQYAMD_PipelineEncode_BatchStrided_* can be passed straight through. */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_BatchStrided_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                               void* const* d_dsts, const long* dst_shapes, const long* dst_strides,
                                                               unsigned shape_size, long* decoded_bytes, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_BatchStrided_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                              void* const* d_dsts, const long* dst_shapes, const long* dst_strides,
                                                              unsigned shape_size, long* decoded_bytes, void* hip_stream);
/* _BatchStrided_*_Device for a box of every blob -- the read of a box [origin, origin + extent) out of a tiled store, whose border cuts
 * through tiles: the window of blob i begins at its voxel src_origins row i (shape_size longs, outermost first, host array; NULL: all
 * zeros) and has the extent dst_shapes row i, which is also the shape of the view d_dsts[i] / dst_strides row i (the view rules of
 * _BatchStrided_*; NULL strides: dense views).  Checked before anything is written (else 1, decoded_bytes zeroed): everything
 * _BatchStrided_* checks but the equality of shapes; the header's rank equals shape_size; every origin >= 0, every extent >= 1,
 * origin + extent <= the header's shape in every dimension (a sum that overflows is beyond it).  Exactly the window's voxels are written,
 * to exactly the view's voxel places; decoded_bytes[i] = window voxels x voxel size.  Every blob's LZ4 stream is decoded whole; what
 * follows is cropped: `bitswap1->lz4` blobs on the joint path go through an inverse transposer that stores only the window's voxels,
 * `lz4` blobs' windows are copied straight out of the LZ4 output; every other blob is decoded dense into a workspace place and ONE launch
 * at the end of the call copies the windows out ("batch_window_fused" = 0: every blob).  A blob whose window is all of it is a view of
 * _BatchStrided_*, and a call of such blobs only IS that call: the same launches.  Return codes (a damaged blob: the composite code
 * after every blob has been handled, the good windows in place), stream, context, ordering and thread safety as _Batch_*_Device. */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_BatchWindow_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                              const long* src_origins, void* const* d_dsts, const long* dst_shapes,
                                                              const long* dst_strides, unsigned shape_size, long* decoded_bytes,
                                                              void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_BatchWindow_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                             const long* src_origins, void* const* d_dsts, const long* dst_shapes,
                                                             const long* dst_strides, unsigned shape_size, long* decoded_bytes,
                                                             void* hip_stream);
/* The check of a box of a tiled store against resident voxels: _Decode_BatchWindow_*_Device with the views READ and nothing written --
 * no decoded copy is kept.  The arguments are that call's; d_views[i] / view_strides row i is the view of view_shapes row i that window i
 * of blob i is compared with.  stats: a HOST array of nblobs rows of SQYAMD_COMPARE_FIELDS values.  With a = voxel k of window i as
 * SQYAMD_Decode_*_Device decodes it and b = voxel k of view i (the "original" side of the reference's `sqy compare` metrics), row i holds
 * the exact unsigned integers below -- a blob has fewer than 2^31 voxels, so SUM_SQ < 2^31 x 65535^2 < 2^63 and nothing wraps; no
 * floating-point value exists on the device and the order of summation cannot show. */
#define SQYAMD_COMPARE_FIELDS 8
#define SQYAMD_COMPARE_VOXELS 0   /* voxels of the window */
#define SQYAMD_COMPARE_NDIFF 1    /* number of k with a != b */
#define SQYAMD_COMPARE_SUM_ABS 2  /* sum |a - b| */
#define SQYAMD_COMPARE_SUM_SQ 3   /* sum (a - b)^2 */
#define SQYAMD_COMPARE_MAX_ABS 4  /* max |a - b| */
#define SQYAMD_COMPARE_VIEW_SUM 5 /* sum b */
#define SQYAMD_COMPARE_VIEW_MIN 6 /* min b */
#define SQYAMD_COMPARE_VIEW_MAX 7 /* max b */
/* Checked before anything runs (else 1, stats zeroed; stats == NULL: 1): exactly what _Decode_BatchWindow_* checks -- the blob entries,
 * the view rules, each window against its blob's header, the header's voxel type --; whatever needs no header (a negative origin
 * included) is checked before a device is looked for.  Views may overlap or coincide, one view may serve several blobs and the same blob
 * may be named several times: nothing is written.  Nothing is written to device memory outside the library's workspace: d_src and the
 * views keep their bytes.  A damaged blob: SQY_Decode's composite code of the first damaged blob in blob order, returned after every blob
 * has been handled; the damaged blob's row is all ones (every field ~0), the other rows are right.
 * How: the windowed decode's groups and launches with a reduction where the stores were.  The device holds one 64-byte record per blob in
 * the workspace, made ready on the stream (zeros, VIEW_MIN all ones) and brought back by ONE copy behind the call's last launch; the host
 * fills VOXELS.  `bitswap1->lz4` blobs on the joint path go through an inverse transposer that compares the window's voxels with the
 * view's where the windowed decode stores them, `lz4` blobs' windows are compared in the LZ4 output; every other blob is decoded dense
 * into a workspace place and ONE launch at the end of the call compares them all ("batch_compare_fused" = 0: every blob -- the same
 * statistics).  A thread sums its 128 voxels (SUM_SQ in 64 bits), a workgroup reduces across lanes and through LDS, and one set of 64-bit
 * integer atomics per workgroup of 32768 voxels goes into the record.  Stream, context, ordering and thread safety as _Batch_*_Device:
 * the work runs behind what is queued on hip_stream and is complete on return; safe from several host threads. */
SQY_FUNCTION_PREFIX int SQYAMD_Compare_BatchWindow_UI16_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                               const long* src_origins, const void* const* d_views, const long* view_shapes,
                                                               const long* view_strides, unsigned shape_size, unsigned long long* stats,
                                                               void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Compare_BatchWindow_UI8_Device(const void* d_src, const long* offsets, const long* lengths, int nblobs,
                                                              const long* src_origins, const void* const* d_views, const long* view_shapes,
                                                              const long* view_strides, unsigned shape_size, unsigned long long* stats,
                                                              void* hip_stream);
/* The same check for a stack stored as ONE blob: MANY boxes of one blob compared with resident voxels in one call, nothing written.  Box i
 * is [origins + i rank, .. + view_shapes + i rank) of the volume SQYAMD_Decode_*_Device gives for the blob (count rows of `rank` longs
 * each); it is compared with the view at d_views[i] (view_strides + i rank, NULL: every view dense) under the view rules of
 * SQYAMD_Decode_Boxes_*_Device.  count = 1 is the single box.  stats: a HOST array of count rows of SQYAMD_COMPARE_FIELDS values, the
 * fields and their meaning exactly SQYAMD_Compare_BatchWindow_*'s (a = the decoded voxel -- behind the quantiser's look-up the 16-bit
 * voxel out of the table --, b = the view's voxel; exact unsigned 64-bit integers).
 * Checked before anything runs on the device (else 1, stats zeroed; stats == NULL: 1): exactly what SQYAMD_Decode_Boxes_* checks -- the
 * arguments, the view rules, every box against the one header, the voxel type, more workgroups than one launch takes --; whatever needs
 * no header is checked before a device is looked for.  Views may overlap, coincide or be shared and a box may be named twice: nothing is
 * written.  Nothing is written to device memory outside the library's workspace: d_src and the views keep their bytes.  A damaged LZ4
 * frame that SOME box's z-range needs gives SQY_Decode's composite code for the call with EVERY row all ones (the frames are decoded
 * united: the call does not say whose frame it was); a damaged frame that no box needs goes unnoticed, as in SQYAMD_Decode_Boxes_*.
 * How: one header fetch, the LZ4 frames the boxes' z-ranges need united and decoded by one launch, one 64-byte record per box made ready on
 * the stream, ONE output launch -- for `bitswap1->lz4` and `quantiser->bitswap1->lz4` the range transposer of SQYAMD_Decode_Boxes_* with
 * a compare where it stores, for `lz4` and `frame_shuffle->lz4` one window compare in the compaction -- and ONE copy of the records behind
 * it; the host fills VOXELS.  Every other blob is decoded whole ONCE into the workspace and one window compare takes all boxes
 * ("compare_boxes_subset" = 0: every blob -- the same statistics).  Stream, context, ordering and thread safety as
 * SQYAMD_Decode_Boxes_*_Device. */
SQY_FUNCTION_PREFIX int SQYAMD_Compare_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const void* const* d_views,
                                                         const long* view_shapes, const long* view_strides, unsigned rank, unsigned long long* stats,
                                                         void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Compare_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const void* const* d_views,
                                                        const long* view_shapes, const long* view_strides, unsigned rank, unsigned long long* stats,
                                                        void* hip_stream);
/* host-pointer variants: the blob is staged ONCE; views holds the boxes' voxels dense and back to back in box order (1 where views_bytes is
 * not exactly their sum) */
SQY_FUNCTION_PREFIX int SQYAMD_Compare_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                  const char* views, long views_bytes, unsigned long long* stats);
SQY_FUNCTION_PREFIX int SQYAMD_Compare_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                 const char* views, long views_bytes, unsigned long long* stats);
/* The quick look at a stack stored as ONE blob: MANY boxes of one blob projected along an axis in one call -- maximum, minimum or sum --,
 * the decoded voxels never stored.  Box i is [origins + i rank, .. + extents + i rank) of the volume SQYAMD_Decode_*_Device gives for the
 * blob (count rows of `rank` longs each; ranks 1 to 3 mapped as by SQYAMD_Decode_Boxes_*: frames are the first dimension).  axis lies in
 * [0, rank) and is the same for all boxes; op is one of SQYAMD_PROJECT_MAX, _MIN, _SUM.  Image i has the box's extent with `axis` removed
 * -- rank - 1 dimensions, ONE element for rank 1 -- and its elements are uint32_t for every op and both voxel types: element (u, v) is the
 * max, min or sum of the box's voxels along `axis`, exact (behind the quantiser's look-up: of the 16-bit voxels out of the table).  The
 * mean is the caller's division.  d_outs[i] is 4-byte aligned; out_strides + i (rank - 1) gives image i's pitches in ELEMENTS under the
 * view rules of SQYAMD_Decode_Boxes_*_Device (innermost 1, no dimension reaches into the next; NULL: every image dense).  Every element of
 * every image is written and nothing else: not the gaps between pitched rows, not d_src.  Images that overlap each other are the caller's
 * error.
 * Checked before a byte is written (else 1, every image untouched): what SQYAMD_Decode_Boxes_* checks for every box; axis or op out of
 * range; a NULL or misaligned image; the stride rules; more workgroups than one launch takes; and SQYAMD_PROJECT_SUM where the sum might
 * not fit: maxvoxel x extent[axis] >= 2^32 with maxvoxel 255 for 8-bit voxels (extents up to 16843009 are taken), and for 16-bit voxels
 * every extent above 65536.  Whatever needs no header is checked before a device is looked for.  A damaged LZ4 frame that SOME box's
 * z-range needs gives SQY_Decode's composite code; the images may then hold anything, and nothing outside them is written.  A damaged
 * frame that no box needs goes unnoticed.
 * How: one header fetch, the LZ4 frames the boxes' z-ranges need united and decoded by one launch, ONE output launch -- for
 * `bitswap1->lz4` and `quantiser->bitswap1->lz4` the range transposer of SQYAMD_Decode_Boxes_* with a 32-bit integer atomic on the image
 * where it stores (the images get the op's neutral element by one small launch in front of it; along axis 0, where every frame is a
 * whole number of 32-voxel runs, a thread walks z over the box's frames instead, reduces in registers and stores once:
 * "project_boxes_walk"), for `lz4` and `frame_shuffle->lz4` one launch with a thread per image element in the compaction.  Every other blob is decoded whole ONCE into the workspace and the same
 * per-element launch takes all boxes ("project_boxes_subset" = 0: every blob -- the same images).  Stream, context, ordering and thread
 * safety as SQYAMD_Decode_Boxes_*_Device. */
#define SQYAMD_PROJECT_MAX 0
#define SQYAMD_PROJECT_MIN 1
#define SQYAMD_PROJECT_SUM 2
SQY_FUNCTION_PREFIX int SQYAMD_Project_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                         int axis, int op, void* const* d_outs, const long* out_strides, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Project_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                        int axis, int op, void* const* d_outs, const long* out_strides, void* hip_stream);
/* host-pointer variants: the blob is staged ONCE; the images come back dense and back to back in box order, as uint32_t (1 where
 * out_capacity, in bytes, is too small) */
SQY_FUNCTION_PREFIX int SQYAMD_Project_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis,
                                                  int op, char* out, long out_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Project_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank, int axis,
                                                 int op, char* out, long out_capacity);
/* The same boxes at a coarser resolution: MANY boxes of one blob binned in one call -- an overview, a pyramid level, binned crops --, the
 * full-resolution voxels never stored.  Boxes, rank, device, stream and thread rules are SQYAMD_Decode_Boxes_*'s (ranks 1 to 3, frames the
 * first dimension).  bins: `rank` longs, each >= 1, the same for every box; op is one of SQYAMD_PROJECT_MAX, _MIN, _SUM.  Output i keeps
 * the rank; its extent in dimension d is ceil(extent[d] / bins[d]).  Cell c covers the box's voxels [c bins, min((c + 1) bins, extent))
 * per dimension: a partial cell at the box's far edge reduces the voxels it has, a bin larger than the extent is one cell.  Elements are
 * uint32_t for every op and both voxel types, exact (behind the quantiser's look-up: of the 16-bit voxels out of the table); the mean is
 * the caller's division by the cell's voxel count.  d_outs[i] is 4-byte aligned; out_strides + i rank gives output i's pitches in ELEMENTS
 * under the view rules of SQYAMD_Decode_Boxes_*_Device (innermost 1, no dimension reaches into the next; NULL: every output dense).  Every
 * element of every output is written once and nothing else: not the gaps between pitched rows, not d_src.  bins of all ones give
 * SQYAMD_Decode_Boxes_*'s voxels, widened; bins[axis] >= extent[axis] with ones elsewhere SQYAMD_Project_Boxes_*'s image with a kept
 * dimension of 1 -- correct, but such a box has few cells and so few workgroups: a projection is SQYAMD_Project_Boxes_*'s to do.
 * Checked before a byte is written (else 1, every output untouched): what SQYAMD_Decode_Boxes_* checks for every box; bins NULL or an
 * entry < 1; op out of range; a NULL or misaligned output; the stride rules; more workgroups than one launch takes; and SQYAMD_PROJECT_SUM
 * where a cell might not fit: with V the product of min(bins[d], extent[d]) of the box, 16-bit voxels at V > 65536, 8-bit voxels at
 * 255 V >= 2^32.  Whatever needs no header is checked before a device is looked for.  A damaged LZ4 frame that SOME box's z-range needs
 * gives SQY_Decode's composite code; the outputs may then hold anything, and nothing outside them is written.  A damaged frame that no
 * box needs goes unnoticed.
 * How: one header fetch, the LZ4 frames the boxes' z-ranges need united and decoded by one launch, ONE output launch -- for
 * `bitswap1->lz4` and `quantiser->bitswap1->lz4` a workgroup per block of one box's cells (one cell layer, a band of cell rows, a strip of
 * cell columns): accumulators in LDS, the plane words of the block's footprint transposed and reduced in registers, LDS integer atomics,
 * every cell stored once -- no global atomic, no neutral-element launch; for `lz4` and `frame_shuffle->lz4` one launch with a thread per
 * output cell in the compaction.  Every other blob is decoded whole ONCE into the workspace and the same per-cell launch takes all boxes
 * ("bin_boxes_subset" = 0: every blob -- the same outputs). */
SQY_FUNCTION_PREFIX int SQYAMD_Bin_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                     const long* bins, int op, void* const* d_outs, const long* out_strides, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Bin_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                    const long* bins, int op, void* const* d_outs, const long* out_strides, void* hip_stream);
/* host-pointer variants: the blob is staged ONCE; the outputs come back dense and back to back in box order, as uint32_t (1 where
 * out_capacity, in bytes, is too small) */
SQY_FUNCTION_PREFIX int SQYAMD_Bin_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                              const long* bins, int op, char* out, long out_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Bin_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                             const long* bins, int op, char* out, long out_capacity);
/* A whole resolution pyramid of the same boxes in one call: SQYAMD_Bin_Boxes_* at `levels` sets of bins -- a viewer's multiscale overview,
 * the pyramid levels of a chunked store, crops at 1x / 2x / 4x --, the header fetched, the frames indexed and the LZ4 frames of the boxes'
 * z-ranges decoded ONCE for all levels.  Boxes, rank, device, stream and thread rules are SQYAMD_Bin_Boxes_*'s.  levels: 1 to
 * SQYAMD_PYRAMID_MAX_LEVELS; bins: levels x rank longs, row l for level l, the same for every box; op is one of SQYAMD_PROJECT_MAX, _MIN,
 * _SUM.  Level l of box i is exactly what SQYAMD_Bin_Boxes_* gives for row l: uint32_t, of the box's rank, its extent in dimension d
 * ceil(extent[d] / min(bins[l][d], extent[d])); it lies at d_outs[i levels + l] (4-byte aligned) with the pitches out_strides +
 * (i levels + l) rank in ELEMENTS under SQYAMD_Bin_Boxes_*'s rules (NULL: every output dense).  The levels must NEST: bins[l + 1][d] is
 * a whole multiple of bins[l][d] for every d, on the values as given (a multiple of 1, a repeated level, is allowed).  Cells begin at the
 * box's origin, so a cell of level l + 1 is the union of whole cells of level l -- partial cells at the far edge and bins beyond the
 * extent included -- and max, min and sum of it are those of their results: every level is exact.  Every element of every output is
 * written once and nothing else.
 * Checked before a byte is written (else 1, every output untouched): what SQYAMD_Bin_Boxes_* checks, for every level of every box;
 * levels out of range; a row that is no multiple of the row before; a NULL or misaligned output or the stride rules, for every output;
 * more workgroups than one launch takes; and SQYAMD_PROJECT_SUM where a cell of the coarsest level might not fit (V of that level: 16-bit
 * voxels at V > 65536, 8-bit voxels at 255 V >= 2^32).  Whatever needs no header is checked before a device is looked for.  Damaged LZ4
 * frames: as SQYAMD_Bin_Boxes_*.
 * How: for `bitswap1->lz4` and `quantiser->bitswap1->lz4` ONE launch in which a workgroup owns a block of cells of the box's top fused
 * level T -- the highest level of which a cell fits the accumulators in LDS --, walks the level-0 cell layers under it as
 * SQYAMD_Bin_Boxes_*'s kernel walks its one, stores each and folds it LDS to LDS into level 1, a completed layer of level 1 into level 2,
 * and so on: no plane word is loaded twice, no global atomic, every cell stored once.  Levels above T -- their cells span workgroups --
 * come from ONE further small launch with a thread per cell over the stored level-T cells.  For `lz4`, `frame_shuffle->lz4` and every
 * blob decoded whole: level 0 by SQYAMD_Bin_Boxes_*'s per-cell launch, every further level by that same small launch straight from level
 * 0.  "pyramid_boxes_subset" = 0: every blob decoded whole once; "pyramid_boxes_fused" = 0: level 0 by SQYAMD_Bin_Boxes_*'s launch and
 * every further level by a launch of its own from the level below -- the same outputs both. */
#define SQYAMD_PYRAMID_MAX_LEVELS 8
SQY_FUNCTION_PREFIX int SQYAMD_Pyramid_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                         long levels, const long* bins, int op, void* const* d_outs, const long* out_strides, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Pyramid_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                        long levels, const long* bins, int op, void* const* d_outs, const long* out_strides, void* hip_stream);
/* host-pointer variants: the blob is staged ONCE; the outputs come back dense and back to back, box by box and levels ascending within a
 * box, as uint32_t (1 where out_capacity, in bytes, is too small) */
SQY_FUNCTION_PREFIX int SQYAMD_Pyramid_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                  long levels, const long* bins, int op, char* out, long out_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Pyramid_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                 long levels, const long* bins, int op, char* out, long out_capacity);
/* The intensity distribution of the same boxes: MANY boxes of one blob counted in one call -- display range and percentiles, an Otsu or
 * background threshold per crop, saturation checks, the 65536-bin histogram a re-quantisation starts from --, the decoded voxels never
 * stored.  Boxes, rank, device, stream and thread rules are SQYAMD_Decode_Boxes_*'s (ranks 1 to 3, frames the first dimension).  Voxel v
 * of box i falls into bin v >> shift; histogram i is nbins = R >> shift counters of uint32_t, dense, at d_hists[i] (4-byte aligned), with
 * R = 65536 for the 16-bit entry points and 256 for the 8-bit ones and shift in [0, 16) resp. [0, 8).  Behind the quantiser's look-up the
 * counted voxel is the 16-bit one out of the table, as for SQYAMD_Compare_Boxes_*.  Counts are exact: a blob has fewer than 2^31 voxels,
 * so no counter wraps.  Every counter of every histogram is written, zeros included, and nothing else: not d_src, not a byte around the
 * histograms.  Boxes may overlap in the blob; histograms that overlap each other are the caller's error.
 * Checked before a byte is written (else 1, every histogram untouched): what SQYAMD_Decode_Boxes_* checks for every box; shift out of
 * range; d_hists NULL, a NULL entry in it or one off the 4-byte grid.  Whatever needs no header is checked before a device is looked for.
 * A damaged LZ4 frame that SOME box's z-range needs gives SQY_Decode's composite code; the histograms may then hold anything, and nothing
 * outside them is written.  A damaged frame that no box needs goes unnoticed.
 * How: one header fetch, the LZ4 frames the boxes' z-ranges need united and decoded by one launch, one launch that zeroes all histograms,
 * ONE counting launch -- for `bitswap1->lz4` and `quantiser->bitswap1->lz4` the range transposer driven by a job table, a workgroup per
 * 32768 voxels of a box's word range: it counts the box's voxels into a private histogram in LDS (up to 16384 bins whole; above, a window
 * of 16384 bins voted from its first voxels, the bins outside it by global atomics) and adds its non-zero counters into the output with
 * no-return 32-bit atomics; for `lz4` and `frame_shuffle->lz4` one launch over the boxes' rows in the compaction with the same LDS
 * histogram.  Every other blob is decoded whole ONCE into the workspace and the same launch takes all boxes ("histogram_boxes_subset" = 0:
 * every blob -- the same histograms). */
SQY_FUNCTION_PREFIX int SQYAMD_Histogram_Boxes_UI16_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                           int shift, void* const* d_hists, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Histogram_Boxes_UI8_Device(const void* d_src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                          int shift, void* const* d_hists, void* hip_stream);
/* host-pointer variants: the blob is staged ONCE; the histograms come back dense and back to back in box order, nbins uint32_t each (1
 * where out_capacity, in bytes, is below count nbins 4) */
SQY_FUNCTION_PREFIX int SQYAMD_Histogram_Boxes_UI16(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                    int shift, char* out, long out_capacity);
SQY_FUNCTION_PREFIX int SQYAMD_Histogram_Boxes_UI8(const char* src, long srclength, long count, const long* origins, const long* extents, unsigned rank,
                                                   int shift, char* out, long out_capacity);
/* The write of a box into a tiled store, whose border cuts through tiles: every tile under the box is read, modified and written again
 * with ONE call.  Old blob i lies at d_src + src_offsets[i], src_lengths[i] bytes (host arrays; any alignment): a complete sqeazy blob of
 * the entry point's voxel type, any pipeline, any layout.  Window i is the box [origins row i, + win_shapes row i) of that blob's volume
 * (shape_size longs a row, outermost first, host arrays; origins NULL: all zeros); its new voxels are read from the view d_wins[i] /
 * win_strides row i (d_wins: a HOST array of device pointers; strides in voxels, the view rules of _BatchStrided_*; NULL: dense views).
 * Only the view's voxels are read.  New blob i is BYTE FOR BYTE what SQYAMD_PipelineEncode_*_Device(pipeline, .., nthreads) gives for the
 * volume V_i = what SQYAMD_Decode_*_Device gives for old blob i, with the window's voxels replaced by the view's.  It is written into slot
 * i of d_dst; slot layout, offsets, lengths and the capacity rule are exactly SQYAMD_PipelineEncode_Batch_*_Device's.  `pipeline` is the
 * new blobs' pipeline and may differ from an old blob's.  A lossy old blob (quantiser) is RE-QUANTISED from its decoded voxels: that is
 * the definition above, so voxels outside the window may change again.  The same old blob may be named several times in one call; each
 * result is the old blob with its own window only.  Overlap of d_dst with the old blobs or the views is the caller's error.
 * Checked before anything is written (else 1, offsets and lengths zeroed): everything _Batch_*_Device checks for the encode side; every
 * blob entry (offset >= 0, length > 0); the view rules; the windows, against each blob's header: its rank equals shape_size, every
 * origin >= 0, every extent >= 1, origin + extent <= the header's shape in every dimension (a sum that overflows is beyond it); the
 * header's voxel type; the single call's geometry refusals for the blob's shape under `pipeline`.  Whatever needs no header is checked
 * before a device is looked for.  A damaged old blob: SQY_Decode's composite code of the first damaged blob in blob order, offsets and
 * lengths zeroed, nothing written to d_dst.  A blob that does not fit its slot: 1, the tables zeroed, as in the batch encode.  In every
 * failure nothing is written outside [d_dst, d_dst + nblobs * slot_capacity).
 * How: every old blob is decoded dense into a place of the workspace (the batch decode's groups), ONE launch pastes every window into
 * its place, the batch encode reads the places (its groups and single-call fallbacks) -- a call holds a dense copy of every blob at
 * once.  A `bitswap1->lz4` old blob on the batch decode's joint path that is written as joint-eligible `bitswap1->lz4` is never
 * transposed back: its LZ4-decoded bit planes are patched with the window's voxels by one launch per encode group; such planes and
 * the volumes of old `lz4` blobs are LZ4-decoded straight into their places where a decode group holds nothing else
 * ("batch_update_fused" = 0: the dense way for every blob -- same bytes).  Stream, context, ordering and thread safety as
 * _Batch_*_Device: the work runs behind what is queued on hip_stream and is complete on return; safe from several host threads. */
SQY_FUNCTION_PREFIX int SQYAMD_Update_BatchWindow_UI16_Device(const char* pipeline, const void* d_src, const long* src_offsets, const long* src_lengths,
                                                              int nblobs, const long* origins, const void* const* d_wins, const long* win_shapes,
                                                              const long* win_strides, unsigned shape_size, void* d_dst, long slot_capacity, long* offsets,
                                                              long* lengths, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Update_BatchWindow_UI8_Device(const char* pipeline, const void* d_src, const long* src_offsets, const long* src_lengths,
                                                             int nblobs, const long* origins, const void* const* d_wins, const long* win_shapes,
                                                             const long* win_strides, unsigned shape_size, void* d_dst, long slot_capacity, long* offsets,
                                                             long* lengths, int nthreads, void* hip_stream);
/* A box written into ONE large blob: old blob + a box's new voxels -> new blob.  Let V = what SQYAMD_Decode_*_Device gives for the old
 * blob d_src[0, srclength), and V' = V with the box [origin, origin + view_shape) (`rank` longs each, outermost first) replaced by the
 * voxels of the view at d_view / view_strides (strides in voxels, the view rules of _BatchStrided_*; NULL: dense; only the view's voxels
 * are read).  The new blob, d_dst[0, *dstlength), decodes to V' under `pipeline`; whenever the old blob is what
 * SQYAMD_PipelineEncode_*_Device(pipeline, V, nthreads) gives, the new blob is BYTE FOR BYTE what that call gives for V'.  A lossy old
 * blob (quantiser) is re-quantised from its decoded voxels, as in SQYAMD_Update_BatchWindow_*.
 * Admission, all before a byte is written; every refusal returns 1 with *dstlength = 0.  Before a device is looked for: NULL pointers,
 * rank 0 or above 3, srclength <= 0, dst_capacity <= 0, a negative origin, a pipeline not admitted for the voxel type.  Then the view
 * rules.  Then, against the header: the voxel type, the header's rank, origin + extent inside the shape (extents >= 1; a sum that
 * overflows is beyond it), the single call's geometry refusals for the blob's shape under `pipeline`.  d_dst overlapping d_src or the view
 * is the caller's error.
 * Errors: a damaged LZ4 frame that is needed gives SQY_Decode's composite code with d_dst untouched.  A new blob that does not fit
 * dst_capacity returns 1 with *dstlength set to the exact bytes a retry needs, and nothing at or behind d_dst + dst_capacity is
 * written; SQY_Pipeline_Max_Compressed_Length_* of the shape is always enough.
 * How: where `pipeline` equals the old blob's pipeline stage for stage, is `lz4` or `bitswap1->lz4`, and both are the
 * chunked LZ4 layout with acceleration 1 and more than one chunk, only the LZ4 frames that the box's range [origin[0], origin[0] +
 * view_shape[0]) needs are decoded, patched where they lie, compressed again and spliced between the old frames -- which are copied from
 * the old blob VERBATIM, whoever wrote them: a damaged frame outside the range goes unnoticed and is carried over, as
 * SQYAMD_Decode_Box_* leaves it unnoticed.  Every other blob is decoded whole into the library's workspace, the box pasted, and the
 * volume encoded as by the single call -- same bytes wherever both apply ("update_box_subset" = 0: every blob).
 * Stream, context, ordering and thread safety are SQYAMD_Decode_Box_*_Device's. */
SQY_FUNCTION_PREFIX int SQYAMD_Update_Box_UI16_Device(const char* pipeline, const void* d_src, long srclength, const long* origin, const void* d_view,
                                                      const long* view_shape, const long* view_strides, unsigned rank, void* d_dst, long dst_capacity,
                                                      long* dstlength, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Update_Box_UI8_Device(const char* pipeline, const void* d_src, long srclength, const long* origin, const void* d_view,
                                                     const long* view_shape, const long* view_strides, unsigned rank, void* d_dst, long dst_capacity,
                                                     long* dstlength, int nthreads, void* hip_stream);
/* MANY boxes written into ONE large blob in one call: SQYAMD_Update_Box_* for a table of `count` boxes (the table layout of
 * SQYAMD_Decode_Boxes_* and SQYAMD_Compare_Boxes_*: `count` rows of `rank` longs in origins, view_shapes and view_strides; d_views a
 * HOST array of `count` device pointers; view_strides NULL: every view dense).  Let V = what SQYAMD_Decode_*_Device gives for the old
 * blob and V' = V with box 0, then box 1, .. then box count - 1 replaced by their views, in that order: boxes may overlap, and where
 * they do the box with the higher index holds.  The new blob decodes to V' under `pipeline`; whenever the old blob is what the single
 * call gives for V, the new blob is BYTE FOR BYTE what the single call gives for V' -- exactly what a chain of `count`
 * SQYAMD_Update_Box_*_Device calls gives; count = 1 is SQYAMD_Update_Box_*.  A lossy old blob is re-quantised from its decoded voxels.
 * Admission, all before a byte is written; every refusal returns 1 with *dstlength = 0.  Per box SQYAMD_Update_Box_*'s rules; in
 * addition count < 1, a NULL entry of d_views, more workgroups than one launch takes.  Whatever needs no header is checked before a
 * device is looked for.
 * Errors are SQYAMD_Update_Box_*'s: a damaged LZ4 frame that SOME box's range needs gives SQY_Decode's composite code with d_dst
 * untouched, one that no box needs is carried over unnoticed; a blob that does not fit returns 1 with *dstlength set to the exact
 * bytes a retry needs, nothing at or behind d_dst + dst_capacity is written.
 * How: where SQYAMD_Update_Box_* would take its subset path, its stages run ONCE each for all boxes -- one header
 * fetch, one frame index, one decode of the LZ4 frames the boxes' ranges need (each once), one patch launch (`lz4`: one paste per
 * layer of pairwise disjoint consecutive boxes, usually one), one parse, one splice.  Every other blob, and every blob with
 * "update_boxes_subset" = 0 (SQY_NO_UPDATE_BOXES_SUBSET=1), is decoded whole once, pasted and encoded by the single call -- same bytes.
 * Stream, context, ordering and thread safety are SQYAMD_Update_Box_*_Device's. */
SQY_FUNCTION_PREFIX int SQYAMD_Update_Boxes_UI16_Device(const char* pipeline, const void* d_src, long srclength, long count, const long* origins,
                                                        const void* const* d_views, const long* view_shapes, const long* view_strides, unsigned rank,
                                                        void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream);
SQY_FUNCTION_PREFIX int SQYAMD_Update_Boxes_UI8_Device(const char* pipeline, const void* d_src, long srclength, long count, const long* origins,
                                                       const void* const* d_views, const long* view_shapes, const long* view_strides, unsigned rank,
                                                       void* d_dst, long dst_capacity, long* dstlength, int nthreads, void* hip_stream);
/* host-pointer variants: the blob staged once, the views dense and back to back in box order -- exactly views_bytes bytes of them, the
 * boxes' summed bytes (checked, like the arguments, before a device is looked for); the new blob comes back to dst */
SQY_FUNCTION_PREFIX int SQYAMD_Update_Boxes_UI16(const char* pipeline, const char* src, long srclength, long count, const long* origins, const long* extents,
                                                 unsigned rank, const char* views, long views_bytes, char* dst, long dst_capacity, long* dstlength,
                                                 int nthreads);
SQY_FUNCTION_PREFIX int SQYAMD_Update_Boxes_UI8(const char* pipeline, const char* src, long srclength, long count, const long* origins, const long* extents,
                                                unsigned rank, const char* views, long views_bytes, char* dst, long dst_capacity, long* dstlength,
                                                int nthreads);
/* host-pointer variants: blobs in host memory at src + offsets[i], dsts[i] host pointers (any alignment); arguments and headers are checked
 * on the host before any device is looked for */
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Batch_UI16(const char* src, const long* offsets, const long* lengths, int nblobs,
                                                 char* const* dsts, const long* dst_capacities, long* decoded_bytes);
SQY_FUNCTION_PREFIX int SQYAMD_Decode_Batch_UI8(const char* src, const long* offsets, const long* lengths, int nblobs,
                                                char* const* dsts, const long* dst_capacities, long* decoded_bytes);

/* ------------------------------------------------------------------------------------------------
 * Section C -- several GPUs (no reference counterpart: sqeazy is a single process with OpenMP loops)
 *
 * z-slabs of a volume are independent sqeazy blobs (one encode call per slab, one process per GPU); the only exchange step
 * of the path is the final gather of the compressed slabs to one rank over RCCL / xGMI.  RCCL is loaded at first use.
 * ---------------------------------------------------------------------------------------------- */

/* A communicator over `world` ranks, one per GPU (wraps ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy, so that a C caller
 * needs no RCCL header): rank 0 makes the 128-byte id, hands it to the other ranks by whatever means it has (MPI, a file, a
 * socket), every rank then calls Comm_Init with its HIP device current. */
SQY_FUNCTION_PREFIX int SQYAMD_Comm_UniqueId(char* id128);
SQY_FUNCTION_PREFIX int SQYAMD_Comm_Init(void** comm, int world, int rank, const char* id128);
SQY_FUNCTION_PREFIX int SQYAMD_Comm_Destroy(void* comm);
/* Variable-length gather to `root`: every rank passes its blob (device pointer, nbytes); sizes[0..world) (host, out on EVERY rank)
 * are the blob sizes in rank order -- the index of a sharded container --; the root receives the blobs back to back, in rank order,
 * at d_recv (blob r at the sum of the sizes in front of it).  One 8-byte all-gather + grouped ncclSend / ncclRecv (point to point
 * over xGMI) on hip_stream; returns when the bytes have arrived.  A root buffer that is too small makes EVERY rank return 1 (the
 * ranks agree before anybody sends).  d_recv / recv_capacity are only read on the root. */
SQY_FUNCTION_PREFIX int SQYAMD_Gather_Blobs(void* comm, int root, const void* d_blob, long nbytes, void* d_recv, long recv_capacity,
                                            long* sizes, void* hip_stream);

/* per-kernel device timing (hipEvents on the call's stream), for bench.py's roofline line.
 *   enable != 0 starts collecting, Reset clears.  Get: i-th kernel name seen since the last reset
 *   (NULL when i is past the end), total milliseconds and number of launches. */
SQY_FUNCTION_PREFIX void SQYAMD_Profile_Enable(int enable);
SQY_FUNCTION_PREFIX void SQYAMD_Profile_Reset(void);
SQY_FUNCTION_PREFIX const char* SQYAMD_Profile_Get(int i, double* total_ms, long* launches);

/* release the cached HBM workspace of the current device */
SQY_FUNCTION_PREFIX void SQYAMD_Release_Workspace(void);

/* Run-time options (measurement / test switches; none changes a byte of any result).  The environment is read once, when the
 * library is loaded (the names in brackets); afterwards only these two calls change / read them -- thread safe.
 *   "transpose_chain"                 1 [SQY_NO_TRANSPOSE_CHAIN=1 -> 0]  the bit-plane transposes of calls in flight on streams the
 *                                     LIBRARY owns (host-pointer entry points, the Slabs workers) run one after the other
 *   "transpose_chain_caller_streams"  0 [SQY_TRANSPOSE_CHAIN_CALLER_STREAMS=1]  .. on streams the CALLER brings as well.  This puts a
 *                                     hipStreamWaitEvent between two caller streams: only for callers whose streams carry nothing but
 *                                     these calls (a backlog or a host function on one stream would hold the other up)
 *   "stage_lanes"                     2 [SQY_STAGE_LANES=<0..2>]  frames-in-place calls of the _DeviceAt / _DeviceAt_Frames entry points run on
 *                                     the library's lanes (see there), not on the stream the caller passes: 0 never, 1 always, 2 when
 *                                     "transpose_chain_caller_streams" is on -- the caller's statement that its streams carry nothing but
 *                                     these calls, which now also means lanes.  (The lanes occupy every hardware queue of the process: a long
 *                                     kernel of the caller's own on ANY of its streams shares a queue with one lane and holds up the calls
 *                                     on it; a call on its caller's stream meets that only when the runtime puts the two streams behind one
 *                                     queue.)  The Slabs workers and the host-pointer entry points keep their own streams and the chain above
 *   "parse_lanes"                     3 [SQY_PARSE_LANES=<1..8>]  how many parse lanes a device has.  3 + the transpose lane = the four hardware
 *                                     queues a process gets by default; a fourth parse lane shares a queue with the transpose lane (measured: no
 *                                     faster than without lanes)
 *   "lane_calls", "lane_backlog_fallbacks", "lane_blocked_fallbacks"   counters, not switches (Get reads, Set takes 0 only): calls that
 *                                     ran on the lanes; calls that stayed on their caller's stream because it had a backlog; .. because a
 *                                     lane did not answer
 *   "call_stamps"                     0  1: every device-memory encode call leaves host time stamps for SQYAMD_Call_Stamps (setting 1 drops
 *                                     the stamps kept so far); 0: a call pays one relaxed load
 *   "dedupe_report"                   0  1: every chunked encode call that ran the duplicate-chunk search keeps the search's keys and decisions
 *                                     for SQYAMD_Dedupe_Report (one small copy and one more synchronisation at the call's end; setting 1 drops
 *                                     the record kept so far); 0: a call pays one relaxed load
 *   "block_parallel"                  1 [SQY_NO_BLOCK_PARALLEL=1 -> 0]  block-linked frames (nthreads = 1) encoded / decoded block-parallel
 *   "block_parallel_warmup"           65536 [SQY_BLOCK_PARALLEL_WARMUP=<bytes>, 0 .. 2^30]  stream parsed in front of a block to guess its table
 *   "block_parallel_stats"            0 [SQY_BLOCK_PARALLEL_STATS=1]  print the blocks whose guess failed
 *   "tail_scan"                       1 [SQY_NO_TAIL_SCAN=1 -> 0]  serial-layout decode: the walk over the block tails as a scan
 *   "decode_two_waves"                1 [SQY_NO_DECODE_TWO_WAVES=1 -> 0]  chunked-layout decode: two wavefronts per frame (0: one)
 *   "noise_digest"                    1 [SQY_NO_NOISE_DIGEST=1 -> 0]  frames in place: the bit-plane transpose leaves bucket and tag of every position
 *                                     liblz4's search probes in a chunk of noise; the LZ4 parse proves such chunks incompressible from them
 *                                     instead of reading the plane stream again (0: it reads)
 *   "transpose_tiles_per_wave"        1 [SQY_TRANSPOSE_TILES_PER_WAVE=<1..64>]  frames in place: tiles of 8192 voxels one wavefront of the transposer
 *                                     takes, one after the other; its grid is tiles / (2 x this) workgroups of two wavefronts (a measurement
 *                                     switch, same bytes at every value: longer waves keep the kernels of other calls in flight waiting for a
 *                                     slot -- measured: slower.  Replaces "transpose_blocks_per_cu", which capped the grid per CU)
 *   "stored_tail_index"               1 [SQY_NO_STORED_TAIL_INDEX=1 -> 0]  decode of the chunked layout: the stored frames at the end of the LZ4
 *                                     stream (bit planes of noise) are looked for where they must start, the scan for frame headers stops in
 *                                     front of them (0: it reads the whole stream)
 *   "host_l2_bytes"                   the host CPU's L2 size as the reference reads it (CPUID; 0 .. 2^32-1)  rmestbkrd samples
 *                                     `Y*X > L2 ? (size_t)(L2 * .75) : Y*X` voxels of its two z faces -- a PARAMETER of the stage's result
 *                                     (the one option that changes bytes): set it to the value of the host whose blobs are to be matched
 *   "decode_frames_subset"            1 [SQY_NO_DECODE_FRAMES_SUBSET=1 -> 0]  SQYAMD_Decode_Frames_*: only the LZ4 frames the range needs, where
 *                                     the pipeline allows (0: every blob decoded whole and the range copied out -- same bytes)
 *   "decode_box_subset"               1 [SQY_NO_DECODE_BOX_SUBSET=1 -> 0]  SQYAMD_Decode_Box_*: only the LZ4 frames the box's z-range needs, where
 *                                     the pipeline allows (0: every blob decoded whole and the box copied out -- same bytes)
 *   "decode_boxes_joint"              1 [SQY_NO_DECODE_BOXES_JOINT=1 -> 0]  SQYAMD_Decode_Boxes_*: the boxes' LZ4 frames united and decoded once, one
 *                                     output launch for all boxes (0: every box on its own, as by SQYAMD_Decode_Box_* -- same bytes)
 *   "compare_boxes_subset"            1 [SQY_NO_COMPARE_BOXES_SUBSET=1 -> 0]  SQYAMD_Compare_Boxes_*: only the LZ4 frames the boxes' z-ranges need, the
 *                                     comparing range transposer or one compare in the compaction, where the pipeline allows (0: every blob
 *                                     decoded whole once and one window compare -- same statistics)
 *   "update_boxes_subset"             1 [SQY_NO_UPDATE_BOXES_SUBSET=1 -> 0]  SQYAMD_Update_Boxes_*: SQYAMD_Update_Box_*'s subset path, every stage once for
 *                                     all boxes (0: the blob decoded whole once, the pastes layer by layer, the single call's encode -- same bytes)
 *   "project_boxes_subset"            1 [SQY_NO_PROJECT_BOXES_SUBSET=1 -> 0]  SQYAMD_Project_Boxes_*: only the LZ4 frames the boxes' z-ranges need, the
 *                                     projecting range transposer or one projection in the compaction, where the pipeline allows (0: every blob
 *                                     decoded whole once and one projection launch -- same images)
 *   "project_boxes_walk"              1 [SQY_NO_PROJECT_BOXES_WALK=1 -> 0]  SQYAMD_Project_Boxes_* along axis 0 on the transposer path: a thread walks z over
 *                                     the box's frames, reduces in registers and stores once, where every box's frames are whole 32-voxel runs on the
 *                                     4-byte grid (0: always the integer atomics -- same images)
 *   "bin_boxes_subset"                1 [SQY_NO_BIN_BOXES_SUBSET=1 -> 0]  SQYAMD_Bin_Boxes_*: only the LZ4 frames the boxes' z-ranges need, the binning
 *                                     kernel (a workgroup per block of cells, LDS accumulators) or one per-cell launch in the compaction, where the
 *                                     pipeline allows (0: every blob decoded whole once and one per-cell launch -- same outputs)
 *   "pyramid_boxes_subset"            1 [SQY_NO_PYRAMID_BOXES_SUBSET=1 -> 0]  SQYAMD_Pyramid_Boxes_*: only the LZ4 frames the boxes' z-ranges need, decoded
 *                                     once for all levels, where the pipeline allows (0: every blob decoded whole once -- same outputs)
 *   "pyramid_boxes_fused"             1 [SQY_NO_PYRAMID_BOXES_FUSED=1 -> 0]  SQYAMD_Pyramid_Boxes_*: all fused levels from one pass over the planes and ONE
 *                                     small launch for the rest (0: level 0 by SQYAMD_Bin_Boxes_*'s launch, every further level by a launch of its
 *                                     own from the level below -- same outputs; the in-call baseline)
 *   "histogram_boxes_subset"          1 [SQY_NO_HISTOGRAM_BOXES_SUBSET=1 -> 0]  SQYAMD_Histogram_Boxes_*: only the LZ4 frames the boxes' z-ranges need,
 *                                     the counting range transposer or one window histogram in the compaction, where the pipeline allows (0: every
 *                                     blob decoded whole once and one window histogram -- same histograms)
 *   "histogram_boxes_merge"           2 [SQY_NO_HISTOGRAM_BOXES_MERGE=1 -> 0]  SQYAMD_Histogram_Boxes_*: how a thread adds equal neighbours into LDS -- 2: a
 *                                     piece of sixteen bytes whose bins are all equal with one atomic; 1: equal consecutive voxels of its whole run
 *                                     with one; 0: one LDS atomic per voxel -- same histograms
 *   "decode_slabs_joint"              1 [SQY_NO_DECODE_SLABS_JOINT=1 -> 0]  SQYAMD_Decode_Slabs_*: the chunked LZ4 blobs of a group indexed and
 *                                     decoded by one launch each (0: every blob on its own, as by SQYAMD_Decode_*_Device -- same bytes)
 *   "decode_batch_joint"              1 [SQY_NO_DECODE_BATCH_JOINT=1 -> 0]  SQYAMD_Decode_Batch_*: the joint-eligible blobs of a group ranked, decoded and
 *                                     transposed back by one launch each (0: every blob on its own, as by SQYAMD_Decode_*_Device -- same bytes)
 *   "decode_batch_group_bytes"        2^32 [SQY_DECODE_BATCH_GROUP_BYTES=<bytes>, 1 .. 2^32]  .. the LZ4 output of one group, and the residual
 *                                     volumes of its `diff3x3x1->bitswap1->lz4` blobs (a group holds at least one blob): bounds the workspace
 *   "encode_batch_joint"              1 [SQY_NO_ENCODE_BATCH_JOINT=1 -> 0]  SQYAMD_PipelineEncode_Batch_*: the joint-eligible volumes of a group share
 *                                     one launch of every kernel (0: every volume through the single-call path -- same bytes)
 *   "encode_batch_group_bytes"        2^30 [SQY_ENCODE_BATCH_GROUP_BYTES=<bytes>, 1 .. 2^32-1]  .. the LZ4 input of one group (a group holds at
 *                                     least one volume): bounds the workspace -- twice that and the tables
 *   "encode_batch_joint_max_bytes"    2^27 [SQY_ENCODE_BATCH_JOINT_MAX_BYTES=<bytes>, 0 .. 2^32-1]  .. a volume with more LZ4 input is encoded
 *                                     on its own, frames in place (the faster path for large stacks; the default is measured: DESIGN.md 5)
 *   "batch_strided_fused"             1 [SQY_NO_BATCH_STRIDED_FUSED=1 -> 0]  SQYAMD_*_BatchStrided_*: the bitswap1 transposers gather from and scatter
 *                                     into the views, `lz4` packs into the stream and unpacks from the LZ4 output (0: packed copies for every
 *                                     pipeline -- same bytes)
 *   "batch_window_fused"              1 [SQY_NO_BATCH_WINDOW_FUSED=1 -> 0]  SQYAMD_Decode_BatchWindow_*: the inverse transposer stores only the window's
 *                                     voxels, `lz4` windows are copied out of the LZ4 output (0: every blob decoded dense into the workspace, one
 *                                     window copy at the end of the call -- same bytes)
 *   "batch_update_fused"              1 [SQY_NO_BATCH_UPDATE_FUSED=1 -> 0]  SQYAMD_Update_BatchWindow_*: `bitswap1->lz4` blobs written as `bitswap1->lz4`
 *                                     keep their bit planes, the window is patched into them; these and `lz4` blobs are LZ4-decoded straight
 *                                     into their workspace places (0: every blob decoded dense into the workspace by the batch decode's
 *                                     launches, one window paste, the batch encode -- same bytes)
 *   "batch_compare_fused"             1 [SQY_NO_BATCH_COMPARE_FUSED=1 -> 0]  SQYAMD_Compare_BatchWindow_*: the inverse transposer compares the window's
 *                                     voxels with the view's, `lz4` windows are compared in the LZ4 output (0: every blob decoded dense into the
 *                                     workspace, one compare launch at the end of the call -- same statistics)
 * Set: 0 = done, 1 = unknown name or value out of range.  Get: the value, -1 for an unknown name. */
SQY_FUNCTION_PREFIX int SQYAMD_Set_Option(const char* name, long value);
SQY_FUNCTION_PREFIX long SQYAMD_Get_Option(const char* name);

/* Where the host side of the device-memory encode calls spends its time (option "call_stamps" = 1 while they run).  Copies the
 * newest max_records records, oldest first, SQYAMD_CALL_STAMP_FIELDS longs each, and returns how many (out == NULL: how many are
 * kept; the last 8192 calls are).  A record: [0] the call's place in the order of the transpose lane since "lane_calls" was reset
 * (-1: it did not run on the lanes), [1] its parse lane, [2] a number that stands for the calling thread, then
 * std::chrono::steady_clock nanoseconds at [3] entry of the C call, [4] lanes taken (the caller's stream polled, the lane mutex
 * held), [5] clear launched, [6] transpose launched, [7] everything queued on the parse lane, [8] hipStreamSynchronize returned,
 * [9] just before the C call returns (drained, context given back).
 * A stamp the call did not pass is 0.  tools/inflight_timeline.py reads them next to a kernel trace of the same run. */
#define SQYAMD_CALL_STAMP_FIELDS 10
SQY_FUNCTION_PREFIX long SQYAMD_Call_Stamps(long* out, long max_records);

/* What the duplicate-chunk search decided in the newest chunked encode call that ran it while option "dedupe_report" was 1 (a 16-bit
 * bitswap1 directly in front of lz4, more than one chunk).  Returns that call's number of chunks, 0 when there is no record.  Copies
 * at most max entries each of: keys[k], the 64-bit key of FULL chunk k (1: every byte zero; a ragged last chunk has none, so one entry
 * less than chunks is written then), and dup_of[k], k itself or the earlier chunk whose frame chunk k shares.  Either pointer may be NULL;
 * with max <= 0 nothing is written.  A test diagnostic: the keys are hashes anyone can collide (tests/dedupe_collisions.py does), equal
 * keys only nominate, a byte compare decides -- and a wrong or a missed decision is visible here where the blob may hide it. */
SQY_FUNCTION_PREFIX long SQYAMD_Dedupe_Report(unsigned long long* keys, unsigned* dup_of, long max);

/* Header helpers for callers that store blobs in containers of their own (the HDF5 filter's cd_values carry a header:
 * inc/sqeazy_h5_filter.hpp:117-121, src/hdf5_utils.hpp:730-738).  The reference does this through its C++ header class
 * (src/sqeazy_header.hpp); there is no C symbol for it there.
 *   Header_Pipeline: copies the NUL-terminated "pipename" of the header at src into out.  *outlength in: capacity of out,
 *                    out: bytes needed (out == NULL: size query).
 *   Header_Build:    writes the header (with delimiter, without payload) the encoder would put in front of
 *                    `encoded_bytes` of payload for this pipeline / voxel size / shape.  Same length protocol. */
SQY_FUNCTION_PREFIX int SQYAMD_Header_Pipeline(const char* src, long srclength, char* out, long* outlength);
SQY_FUNCTION_PREFIX int SQYAMD_Header_Build(const char* pipeline, int sizeof_voxel, const long* shape, unsigned shape_size,
                                            long encoded_bytes, char* out, long* outlength);

/* "sqeazy_amd <version> (gfx950)" */
SQY_FUNCTION_PREFIX const char* SQYAMD_Version(void);

#endif /* SQEAZY_AMD_H_ */
