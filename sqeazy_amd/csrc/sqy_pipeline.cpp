// sqy_pipeline.cpp -- see sqy_pipeline.hpp.  Pure host logic, no HIP.
#include "sqy_pipeline.hpp"

// IEEE evaluation in statement order for the quantiser / frame metric host code: no fused multiply-adds (hipcc defaults to
// -ffp-contract=fast for HIP sources; the declared parity target is the reference compiled without fast-math)
#pragma clang fp contract(off)

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <sys/stat.h>
#include <thread>
#if defined(__x86_64__) || defined(__i386__)
#include <cpuid.h>
#endif

namespace sqy {

const char* const kVersion = "0.5.2";    // sqy.version: a build-time constant in the reference (sqeazy_header.hpp:172)
const char* const kHeadRef = "mi355x";   // sqy.headref: `git describe --always` of the reference build (:173)
const int kVersionTriple[3] = {0, 5, 2};

static const std::string kVerbOpen = "<verbatim>";
static const std::string kVerbClose = "</verbatim>";
static const std::string kHeaderEnd = "|01307#!";   // sqeazy_header.hpp:586

std::vector<std::string> split_outside_verbatim(const std::string& s, const std::string& sep, bool* ok)
{
    std::vector<std::string> out;
    if (ok) *ok = true;
    std::string cur;
    size_t i = 0;
    while (i < s.size()) {
        if (s.compare(i, kVerbOpen.size(), kVerbOpen) == 0) {
            const size_t j = s.find(kVerbClose, i);
            if (j == std::string::npos) {            // "found only 1 verbatim delimeter" (string_parsers.hpp:150-153)
                if (ok) *ok = false;
                return {};
            }
            cur.append(s, i, j + kVerbClose.size() - i);
            i = j + kVerbClose.size();
            continue;
        }
        if (s.compare(i, sep.size(), sep) == 0) {
            out.push_back(cur);
            cur.clear();
            i += sep.size();
            continue;
        }
        cur.push_back(s[i]);
        ++i;
    }
    out.push_back(cur);
    return out;
}

pairs_t parse_pairs(const std::string& pipeline)
{
    pairs_t value;
    if (pipeline.empty()) return value;
    for (const std::string& major : split_outside_verbatim(pipeline, "->")) {
        const size_t d = major.find('(');
        if (d == std::string::npos)
            value.emplace_back(major, "");
        else
            value.emplace_back(major.substr(0, d), major.size() > d + 1 ? major.substr(d + 1, major.size() - d - 2) : "");
    }
    return value;
}

std::map<std::string, std::string> parse_minors(const std::string& cfg)
{
    std::map<std::string, std::string> value;
    if (cfg.empty()) return value;
    for (const std::string& item : split_outside_verbatim(cfg, ",")) {
        const size_t d = item.find('=');
        if (d == std::string::npos) {
            value[item] = item;
        } else {
            value[item.substr(0, d)] = (d + 1 < item.size()) ? item.substr(d + 1) : item;
        }
    }
    return value;
}

// ---- lz4 parameters (encoders/lz4.hpp:58-114) ----
static uint32_t closest_blocksize_kb(uint32_t kb)
{
    static const uint32_t sizes[4] = {64, 256, 1024, 4096};   // lz4_utils.hpp:60-93
    const uint32_t* it = std::lower_bound(sizes, sizes + 4, kb);
    if (it == sizes + 4) return sizes[3];
    if (it == sizes) return sizes[0];
    const uint32_t lo = *(it - 1), hi = *it;
    const uint32_t middle = lo + (hi - lo) / 2;
    return kb >= middle ? hi : lo;
}

static float stof_or(const std::string& s, float dflt)
{
    char* end = nullptr;
    const float v = std::strtof(s.c_str(), &end);
    return (end == s.c_str()) ? dflt : v;
}

Lz4Params::Lz4Params(const std::string& cfg)
{
    const auto m = parse_minors(cfg);
    auto f = m.find("accel");
    if (f != m.end()) accel = (int)stof_or(f->second, 1.f);
    f = m.find("blocksize_kb");
    if (f != m.end()) blocksize_kb = (uint32_t)stof_or(f->second, 256.f);
    f = m.find("framestep_kb");
    if (f != m.end()) framestep_kb = (uint32_t)stof_or(f->second, 256.f);
    f = m.find("n_chunks_of_input");
    if (f != m.end()) n_chunks = (uint32_t)stof_or(f->second, 0.f);
    if (blocksize_kb == 0) blocksize_kb = 256;
    if (framestep_kb < blocksize_kb)
        framestep_kb = blocksize_kb;
    else
        framestep_kb = (uint32_t)(std::round(framestep_kb / float(blocksize_kb)) * blocksize_kb);
    if (n_chunks != 0) framestep_kb = 0;
    const uint32_t c = closest_blocksize_kb(blocksize_kb);
    block_id = c == 64 ? 4 : c == 256 ? 5 : c == 1024 ? 6 : 7;
}

std::string Lz4Params::config() const
{
    std::ostringstream msg;
    msg << "accel=" << accel << ",blocksize_kb=" << blocksize_kb << ",framestep_kb=" << framestep_kb
        << ",n_chunks_of_input=" << n_chunks;
    return msg.str();
}

uint64_t Lz4Params::block_bytes() const
{
    static const uint64_t b[8] = {0, 0, 0, 0, 64u << 10, 256u << 10, 1u << 20, 4u << 20};
    return b[block_id];
}

uint64_t Lz4Params::bytes_per_chunk(uint64_t nbytes) const
{
    uint64_t value = framestep_kb ? (uint64_t)framestep_kb << 10 : (n_chunks ? nbytes / n_chunks : nbytes);
    if (value >= nbytes || n_chunks >= nbytes) value = nbytes;
    return value;
}

uint64_t Lz4Params::compress_bound(uint64_t srcSize, int block_id)
{
    static const uint64_t b[8] = {0, 0, 0, 0, 64u << 10, 256u << 10, 1u << 20, 4u << 20};
    const uint64_t blockSize = b[block_id];
    const uint64_t maxSrcSize = srcSize + (blockSize - 1);        // autoFlush = 0: a full tmp buffer is assumed
    const uint64_t nbFullBlocks = maxSrcSize / blockSize;
    const uint64_t partial = maxSrcSize & (blockSize - 1);
    const uint64_t last = (srcSize == 0) ? partial : 0;
    const uint64_t nbBlocks = nbFullBlocks + (last > 0);
    return 4 * nbBlocks + blockSize * nbFullBlocks + last + 4;
}

uint64_t Lz4Params::max_encoded_size(uint64_t nbytes, unsigned nthreads) const
{
    const uint64_t per_chunk = bytes_per_chunk(nbytes);
    const uint64_t hdr_max = 19;                                   // LZ4F_HEADER_SIZE_MAX (liblz4 1.9.3)
    if (per_chunk >= nbytes) return hdr_max + compress_bound(per_chunk, block_id);
    if (nthreads == 0) nthreads = 1;
    const uint64_t nchunks = (nbytes + per_chunk - 1) / per_chunk;
    const uint64_t per_thread = (nchunks + nthreads - 1) / nthreads;
    return per_thread * (compress_bound(per_chunk, block_id) + hdr_max) * nthreads;
}

// ---- block-linked frames: liblz4 1.9.3's LZ4F buffer management, as far as it decides the bytes ----
// LZ4F_compressUpdate compresses whole blocks straight from the caller's buffer and parks a remainder in tmpBuff; after an
// update that compressed from the caller's buffer it copies the last 64 KiB of history into tmpBuff (LZ4F_localSaveDict,
// stableSrc = 0).  LZ4_compress_fast_continue then runs a block in PREFIX mode when it follows its dictionary in memory
// (lowLimit = start of the dictionary) and in EXTERNAL-DICTIONARY mode otherwise (lowLimit = block start for matches
// inside the block, dictionary start for matches in the history).  Both see the same logical history; lowLimit bounds the
// backward catch-up of a match and is what this model hands to the kernel per block.
namespace {
struct Lz4fModel {
    enum Space { kNone, kCaller, kTmp };
    // LZ4_stream_t: where the dictionary sits and how long it is, plus the index counter that triggers LZ4_renormDictT
    Space dict_space = kNone;
    uint64_t dict_addr = 0;
    uint32_t dict_size = 0;
    uint32_t current_offset = 0;
    // LZ4F_cctx
    uint64_t block_size, max_buffer;
    uint64_t tmp_in = 0, tmp_fill = 0, tmp_stream_pos = 0;
    Lz4Plan* plan;
    bool* ok;

    void compress_block(uint64_t stream_pos, uint64_t n, Space where, uint64_t addr)
    {
        if ((uint64_t)current_offset + n > 0x80000000ull) {          // LZ4_renormDictT: table rescaled (transparent), dictionary clipped
            current_offset = 64u << 10;
            if (dict_size > (64u << 10)) { dict_addr += dict_size - (64u << 10); dict_size = 64u << 10; }
        }
        bool follows = dict_space == where && dict_addr + dict_size == addr;
        if (dict_size >= 1 && dict_size <= 3 && !follows) { dict_size = 0; dict_space = where; dict_addr = addr; follows = true; }
        if (dict_size < (64u << 10) && dict_size < current_offset) *ok = false;      // liblz4's dictSmall variant: never reached with blocks >= 64 KiB
        Lz4BlockPlan b;
        b.start = stream_pos; b.n = (uint32_t)n; b.flags = 0;
        b.low_dict = (int64_t)stream_pos - (int64_t)dict_size;
        b.low_in = follows ? b.low_dict : (int64_t)stream_pos;
        plan->blocks.push_back(b);
        if (n > plan->max_block) plan->max_block = (uint32_t)n;
        current_offset += (uint32_t)n;
        if (follows) dict_size += (uint32_t)n;
        else { dict_space = where; dict_addr = addr; dict_size = (uint32_t)n; }
    }
    uint64_t save_dict()                                             // LZ4_saveDict(stream, tmpBuff, 64 KB)
    {
        const uint32_t d = dict_size < (64u << 10) ? dict_size : (64u << 10);
        dict_space = kTmp; dict_addr = 0; dict_size = d;
        return d;
    }
    void update(uint64_t pos, uint64_t size)                         // LZ4F_compressUpdate(ctx, .., src + pos, size, NULL)
    {
        uint64_t p = pos;
        const uint64_t end = pos + size;
        bool from_caller = false;
        if (tmp_fill > 0) {
            const uint64_t to_copy = block_size - tmp_fill;
            if (to_copy > size) { tmp_fill += size; p = end; }
            else {
                p += to_copy;
                compress_block(tmp_stream_pos, block_size, kTmp, tmp_in);
                tmp_in += block_size;
                tmp_fill = 0;
            }
        }
        while (end - p >= block_size) {
            from_caller = true;
            compress_block(p, block_size, kCaller, p);
            p += block_size;
        }
        if (from_caller) tmp_in = save_dict();
        if (tmp_in + block_size > max_buffer) tmp_in = save_dict();
        if (p < end) { tmp_stream_pos = p; tmp_fill = end - p; }
    }
    void finish() { if (tmp_fill > 0) compress_block(tmp_stream_pos, tmp_fill, kTmp, tmp_in); tmp_fill = 0; }   // LZ4F_compressEnd -> LZ4F_flush
};
} // namespace

Lz4Plan lz4_plan_blocks(uint64_t total, uint64_t step, uint64_t block_bytes, bool serial)
{
    Lz4Plan plan;
    if (total == 0 || step == 0 || block_bytes == 0) { plan.frame_first.push_back(0); return plan; }
    const uint64_t nframes = serial ? 1 : (total + step - 1) / step;
    for (uint64_t f = 0; f < nframes; ++f) {
        const uint64_t f_begin = serial ? 0 : f * step;
        const uint64_t f_end = serial ? total : std::min(total, f_begin + step);
        plan.frame_first.push_back((uint32_t)plan.blocks.size());
        Lz4fModel m;
        m.block_size = block_bytes; m.max_buffer = block_bytes + (128u << 10); m.plan = &plan; m.ok = &plan.ok;
        // positions handed to the model are relative to the frame's first byte (its own LZ4 stream); `start` is made absolute below
        const size_t first = plan.blocks.size();
        for (uint64_t pos = f_begin; pos < f_end; pos += step) m.update(pos - f_begin, std::min(step, f_end - pos));
        m.finish();
        for (size_t i = first; i < plan.blocks.size(); ++i) {
            plan.blocks[i].start += f_begin; plan.blocks[i].low_in += (int64_t)f_begin; plan.blocks[i].low_dict += (int64_t)f_begin;
        }
        if (plan.blocks.size() > first) { plan.blocks[first].flags |= 1u; plan.blocks.back().flags |= 2u; }
    }
    plan.frame_first.push_back((uint32_t)plan.blocks.size());
    return plan;
}

// ---- encode planning ----
Lz4EncodeLayout lz4_encode_layout(const Lz4Params& p, uint64_t total, unsigned nthreads)
{
    const Lz4DecodeGeometry g = lz4_decode_geometry(p, total);
    Lz4EncodeLayout lay;
    lay.chunk = g.chunk; lay.nchunks = g.nchunks;
    if (nthreads == 1 && g.nchunks > 1) lay.kind = Lz4LayoutKind::serial;
    else if (g.chunk > g.block_bytes) lay.kind = Lz4LayoutKind::linked_chunks;
    if (p.accel < 0) lay.accel = (uint32_t)std::min<int64_t>(1 - (int64_t)p.accel, 65537);
    return lay;
}

static uint64_t round_up(uint64_t v, uint64_t to) { return (v + to - 1) / to * to; }

EncodeBatchForm encode_batch_form(const Pipeline& pipe, int elem_size)
{
    const std::vector<Stage>& st = pipe.stages;
    if (st.empty() || st.back().kind != StageKind::lz4) return EncodeBatchForm::none;
    if (st.size() == 1) return EncodeBatchForm::lz4;
    if (st.size() == 2 && st[0].kind == StageKind::bitswap1) return EncodeBatchForm::bitswap1_lz4;
    if (st.size() == 3 && st[0].kind == StageKind::quantiser && st[1].kind == StageKind::bitswap1 && elem_size == 2 &&
        !st[0].cfg.count("weighting_function") && !st[0].cfg.count("decode_lut_path"))
        return EncodeBatchForm::quantiser_bitswap1_lz4;
    return EncodeBatchForm::none;
}

uint64_t encode_batch_stream_bytes(EncodeBatchForm form, uint64_t voxels, int elem_size)
{
    return form == EncodeBatchForm::quantiser_bitswap1_lz4 ? voxels : voxels * (uint64_t)elem_size;
}

uint64_t encode_batch_extra_bytes(EncodeBatchForm form) { return form == EncodeBatchForm::quantiser_bitswap1_lz4 ? kQuantiserBatchTableBytes : 0; }

Lz4BatchPlan lz4_batch_plan(const Lz4Params& p, const std::vector<uint64_t>& totals, unsigned nthreads, uint64_t group_bytes, uint64_t joint_max,
                            uint64_t extra_bytes)
{
    return lz4_batch_plan_views(p, totals, std::vector<uint64_t>(), nthreads, group_bytes, joint_max, extra_bytes);
}

PackedPlaces packed_places(const std::vector<uint64_t>& lengths, const std::vector<uint64_t>& gaps, uint64_t align, uint64_t base, uint64_t capacity)
{
    constexpr uint64_t lim = (uint64_t)1 << 63;                            // every place and every end stays below it
    const size_t n = lengths.size();
    if (align == 0 || align > kPackedAlignMax || (align & (align - 1)) || (!gaps.empty() && gaps.size() != n) || base >= lim) return PackedPlaces();
    PackedPlaces p;
    p.at.resize(n);
    p.first_unfit = n;
    uint64_t cur = base;
    p.end = base;
    for (size_t j = 0; j < n; ++j) {
        const uint64_t gap = gaps.empty() ? 0 : gaps[j];
        if (gap >= lim - cur || lengths[j] >= lim - (cur + gap)) return PackedPlaces();
        p.at[j] = cur + gap;
        p.end = p.at[j] + lengths[j];
        if (p.end > capacity && p.first_unfit == n) p.first_unfit = j;
        if (j + 1 == n) break;
        if (p.end > lim - align) return PackedPlaces();                   // (the rounded end as well)
        cur = (p.end + align - 1) & ~(align - 1);
    }
    p.ok = true;
    return p;
}

bool admit_view(const long* shape, const long* strides, unsigned rank, BatchView* view)
{
    if (!shape || !view || rank == 0 || rank > 3) return false;
    constexpr uint64_t kReachMax = (uint64_t)1 << 62;
    uint64_t d[3] = {1, 1, 1}, s[3] = {0, 0, 1};
    for (unsigned k = 0; k < rank; ++k) {
        if (shape[k] < 1 || (strides && strides[k] < 1)) return false;
        d[3 - rank + k] = (uint64_t)shape[k];
    }
    if (d[2] >= kReachMax || d[1] >= kReachMax / d[2] || d[0] >= kReachMax / (d[1] * d[2])) return false;
    s[1] = d[2];
    s[0] = d[1] * d[2];
    if (strides) {
        if (strides[rank - 1] != 1) return false;
        for (unsigned k = 0; k < rank; ++k) s[3 - rank + k] = (uint64_t)strides[k];
        // the padded dimensions in front: the dense strides over what follows them
        for (int k = 2 - (int)rank; k >= 0; --k) {
            if (s[k + 1] >= kReachMax / d[k + 1]) return false;
            s[k] = d[k + 1] * s[k + 1];
        }
        for (int k = 1; k >= 0; --k) {
            if (s[k + 1] >= kReachMax / d[k + 1]) return false;               // (the reach of dimension k + 1 in 64 bits)
            if (s[k] < d[k + 1] * s[k + 1]) return false;
        }
        if (s[0] >= kReachMax / d[0]) return false;
    }
    BatchView v{d[0], d[1], d[2], s[0], s[1], false};
    if (v.sy == v.X) { v.X *= v.Y; v.Y = 1; v.sy = v.X; }                   // rows without a gap: one row per frame
    if (v.Y == 1) { v.Y = v.Z; v.Z = 1; v.sy = v.sz; v.sz = v.Y * v.sy; }   // .. the frames are the rows
    else if (v.sz == v.Y * v.sy) { v.Y *= v.Z; v.Z = 1; v.sz = v.Y * v.sy; }
    if (v.sy == v.X || v.Y == 1) { v.X *= v.Y; v.Y = 1; v.sy = v.X; v.sz = v.X; }
    if (v.Z == 1) v.sz = v.Y * v.sy;                                        // (one frame: no frame pitch to speak of)
    v.dense = v.Z == 1 && v.Y == 1;
    *view = v;
    return true;
}

bool admit_window(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, BatchWindow* out)
{
    if (!extent || !out || rank == 0 || rank > 3 || header_shape.size() != rank) return false;
    uint64_t b[3] = {1, 1, 1}, o[3] = {0, 0, 0}, e[3] = {1, 1, 1};
    bool whole = true;
    for (unsigned k = 0; k < rank; ++k) {
        const long og = origin ? origin[k] : 0;
        if (og < 0 || extent[k] < 1) return false;
        // (both below 2^63: their sum cannot wrap in 64 unsigned bits)
        if ((uint64_t)og + (uint64_t)extent[k] > header_shape[k]) return false;
        b[3 - rank + k] = header_shape[k];
        o[3 - rank + k] = (uint64_t)og;
        e[3 - rank + k] = (uint64_t)extent[k];
        whole = whole && og == 0 && (uint64_t)extent[k] == header_shape[k];
    }
    *out = BatchWindow{b[0], b[1], b[2], o[0], o[1], o[2], e[0], e[1], e[2], whole};
    return true;
}

BatchWindowLayout batch_window_layout(uint64_t njobs, uint64_t job_bytes)
{
    BatchWindowLayout l;
    l.tiles_at = round_up(njobs * job_bytes, 16);
    l.total = l.tiles_at + (njobs + 1) * 4;
    return l;
}

UpdateBatchPlan update_batch_plan(const std::vector<uint64_t>& raw_bytes, EncodeBatchForm new_form, const std::vector<int32_t>& encode_group_of, bool fused_on)
{
    UpdateBatchPlan u;
    const size_t n = raw_bytes.size();
    u.keep_planes.assign(n, 0);
    u.place_at.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        u.keep_planes[i] = fused_on && new_form == EncodeBatchForm::bitswap1_lz4 && i < encode_group_of.size() && encode_group_of[i] >= 0;
        u.place_at[i] = u.bytes;
        u.bytes += round_up(raw_bytes[i], 256);
    }
    return u;
}

Lz4BatchPlan lz4_batch_plan_views(const Lz4Params& p, const std::vector<uint64_t>& totals, const std::vector<uint64_t>& pack_bytes, unsigned nthreads,
                                  uint64_t group_bytes, uint64_t joint_max, uint64_t extra_bytes_all)
{
    Lz4BatchPlan plan;
    plan.group_of.assign(totals.size(), -1);
    uint64_t group_sum = 0;
    for (size_t i = 0; i < totals.size(); ++i) {
        const uint64_t total = totals[i], extra_bytes = extra_bytes_all + (i < pack_bytes.size() ? pack_bytes[i] : 0);
        const Lz4EncodeLayout lay = lz4_encode_layout(p, total, nthreads);
        // (a table entry counts its bytes and its slot in 32 bits: chunks of the chunked layout are at most an LZ4 block of 4 MiB)
        if (total == 0 || !lay.chunked() || lay.accel != 1 || total > joint_max || lay.nchunks == 0 || lay.chunk > UINT32_MAX) continue;
        if (plan.groups.empty() || (group_sum && group_sum + total + extra_bytes > group_bytes) ||
            plan.groups.back().chunks.size() + lay.nchunks > (uint64_t)UINT32_MAX / 2) {
            plan.groups.emplace_back();
            plan.groups.back().first_chunk.push_back(0);
            group_sum = 0;
        }
        Lz4BatchGroup& g = plan.groups.back();
        const uint64_t at = round_up(g.stream_bytes, 16);
        g.vols.push_back((uint32_t)i);
        g.stream_at.push_back(at);
        for (uint64_t k = 0; k < lay.nchunks; ++k) {
            Lz4BatchChunkPlan c;
            c.off = at + k * lay.chunk;
            c.n = (uint32_t)std::min<uint64_t>(lay.chunk, total - k * lay.chunk);
            c.vol = (uint32_t)i;
            c.slot = (uint32_t)g.chunks.size();
            g.chunks.push_back(c);
            g.max_chunk = std::max(g.max_chunk, c.n);
        }
        g.first_chunk.push_back((uint32_t)g.chunks.size());
        g.stream_bytes = at + total;
        g.scratch_stride = round_up(g.max_chunk, 16);
        group_sum += total + extra_bytes;
        plan.group_of[i] = (int32_t)(plan.groups.size() - 1);
    }
    return plan;
}

DecodeBatchPlan decode_batch_plan(const std::vector<DecodeBatchBlob>& blobs, uint64_t group_bytes, const std::vector<uint8_t>* dropped)
{
    DecodeBatchPlan plan;
    plan.group_of.assign(blobs.size(), -1);
    auto tiles_of = [](uint64_t len) { return std::max<uint64_t>((len + kBatchTileVoxels - 1) / kBatchTileVoxels, 1); };
    auto add_tiles = [](DecodeBatchTiles& t, size_t i, uint64_t tiles) {
        t.jobs.push_back((uint32_t)i);
        t.first_tile.push_back(t.ntiles);
        t.ntiles += (uint32_t)tiles;
    };
    uint64_t group_tiles = 0;
    for (size_t i = 0; i < blobs.size(); ++i) {
        const DecodeBatchBlob& b = blobs[i];
        if (!b.eligible || i > (size_t)UINT32_MAX) continue;
        const bool diff = b.form == DecodeBatchForm::diff_planes || b.form == DecodeBatchForm::diff_plain;
        const uint64_t lz4_out = round_up(b.total, 256), need = b.form == DecodeBatchForm::diff_planes ? 2 * lz4_out : lz4_out;
        const uint64_t strips = diff ? ((uint64_t)b.Y + kDiffStripRows - 1) / kDiffStripRows : 0;
        // (a launch's grid counts its tiles in 31 bits; a diff blob has tiles in up to two tables and its strips)
        const uint64_t tiles = tiles_of(b.len), entries = diff ? 2 * tiles + strips : tiles;
        if (plan.groups.empty() || plan.groups.back().out_bytes + need > group_bytes || plan.groups.back().block_bytes != b.block_bytes ||
            group_tiles + entries > (uint64_t)INT32_MAX) {
            plan.groups.emplace_back();
            plan.groups.back().block_bytes = b.block_bytes;
            group_tiles = 0;
        }
        DecodeBatchGroup& g = plan.groups.back();
        g.blobs.push_back((uint32_t)i);
        g.out_at.push_back(g.out_bytes);
        const uint64_t at = g.out_bytes;
        g.out_bytes += need;
        group_tiles += entries;
        plan.group_of[i] = (int32_t)(plan.groups.size() - 1);
        if (b.form == DecodeBatchForm::stages || (dropped && i < dropped->size() && (*dropped)[i])) continue;
        if (!diff) {
            add_tiles(b.form == DecodeBatchForm::planes ? g.planes : b.form == DecodeBatchForm::quantised ? g.quantised : g.plain, i, tiles);
            continue;
        }
        if (b.form == DecodeBatchForm::diff_planes) add_tiles(g.planes, i, tiles);
        DecodeBatchDiff& d = g.diff;
        d.jobs.push_back((uint32_t)i);
        d.res_at.push_back(b.form == DecodeBatchForm::diff_planes ? at + lz4_out : at);
        d.first_strip.push_back(d.nstrips);
        d.nstrips += (uint32_t)strips;
        d.first_tile.push_back(d.ntiles);
        d.ntiles += (uint32_t)tiles;
        const uint64_t zlim = std::min<uint64_t>(b.X, b.Z);                 // frames 1 .. zlim - 1 go through the chain
        if (zlim > 1) d.steps = std::max(d.steps, (uint32_t)((zlim - 1 + kDiffChainFrames - 1) / kDiffChainFrames));
        d.max_columns = std::max(d.max_columns, b.chain_columns);
    }
    for (DecodeBatchGroup& g : plan.groups) {
        g.planes.first_tile.push_back(g.planes.ntiles);
        g.plain.first_tile.push_back(g.plain.ntiles);
        g.quantised.first_tile.push_back(g.quantised.ntiles);
        g.diff.first_strip.push_back(g.diff.nstrips);
        g.diff.first_tile.push_back(g.diff.ntiles);
    }
    return plan;
}

std::vector<std::vector<size_t>> decode_slab_groups(const std::vector<SlabJointBlob>& joint, uint64_t group_bytes, int inflight)
{
    std::vector<std::vector<size_t>> groups;
    uint64_t gbytes = 0;
    for (size_t j = 0; j < joint.size(); ++j) {
        const uint64_t need = round_up(joint[j].total, 256);
        if (groups.empty() || gbytes + need > group_bytes || (inflight > 0 && groups.back().size() >= (size_t)inflight) ||
            joint[groups.back()[0]].block_bytes != joint[j].block_bytes) {
            groups.emplace_back();
            gbytes = 0;
        }
        groups.back().push_back(j);
        gbytes += need;
    }
    return groups;
}

// a region of `bytes` behind *end, its start rounded up to `align`: where it starts
static uint64_t append(uint64_t* end, uint64_t bytes, uint64_t align)
{
    const uint64_t at = round_up(*end, align);
    *end = at + bytes;
    return at;
}

DecodeRankLayout decode_rank_layout(const std::vector<DecodeRankBlob>& blobs, uint64_t desc_bytes)
{
    DecodeRankLayout l;
    uint64_t end = 0;
    for (const DecodeRankBlob& b : blobs) {
        DecodeRankLayout::Blob at;
        at.scratch_at = append(&end, b.scratch_bytes, kDecodeTableAlign);
        at.blk_at = append(&end, b.max_blocks * kLz4BlockIndexBytes, kDecodeTableAlign);
        at.frame_first_at = append(&end, (b.max_blocks + 2) * 4, kDecodeTableAlign);
        l.blobs.push_back(at);
    }
    l.counts_at = append(&end, blobs.size() * 64, kDecodeTableAlign);
    l.flag_at = append(&end, 64, 64);
    l.desc_at = append(&end, desc_bytes, kDecodeTableAlign);
    l.total = end;
    return l;
}

DecodeJointLayout decode_joint_layout(uint64_t nparts, uint64_t map_bytes, uint64_t nframes, const DecodeBatchGroup* batch)
{
    DecodeJointLayout l;
    uint64_t end = 0;
    l.parts_at = append(&end, nparts * kLz4JointPartBytes, kDecodeTableAlign);
    l.maps_at = append(&end, map_bytes, kDecodeTableAlign);
    l.upload_bytes = end;
    l.jblk_at = append(&end, nframes * kLz4BlockIndexBytes, kDecodeTableAlign);
    l.jff_at = append(&end, (nframes + 1) * 4, 4);
    l.jout_at = append(&end, nframes * kLz4BlockIndexBytes, kDecodeTableAlign);
    l.jobs_upload_at = end;
    if (batch) {
        DecodeJointLayout::Family* const family[4] = {&l.planes, &l.plain, &l.quantised, &l.diff};
        const uint64_t njobs[4] = {batch->planes.jobs.size(), batch->plain.jobs.size(), batch->quantised.jobs.size(), batch->diff.jobs.size()};
        for (int k = 0; k < 4; ++k) {
            DecodeJointLayout::Family& f = *family[k];
            const bool diff = family[k] == &l.diff, quantised = family[k] == &l.quantised;
            const uint64_t tiles_bytes = (njobs[k] + 1) * 4;
            f.jobs_at = append(&end, njobs[k] * (diff ? kDiffBatchJobBytes : kBitswap1JobBytes), kDecodeTableAlign);
            f.tiles_at = append(&end, tiles_bytes, 4);
            // (the diff family's second table follows its first; the LUTs, and the empty region of the other families, start a new line)
            f.extra_at = diff ? append(&end, tiles_bytes, 4) : append(&end, quantised ? njobs[k] * 512 : 0, kDecodeTableAlign);
        }
        l.jobs_upload_at = l.planes.jobs_at;
    }
    l.jobs_bytes = end - l.jobs_upload_at;
    l.total = end;
    return l;
}

EncodeBatchLayout encode_batch_layout(uint64_t nchunks, uint64_t nvols, bool quantised, uint64_t text_bytes)
{
    EncodeBatchLayout l;
    uint64_t end = 0;
    const uint64_t a = kEncodeTableAlign;
    l.table_at = append(&end, nchunks * kLz4BatchChunkBytes, a);
    l.volof_at = append(&end, nchunks * 4, a);
    l.jobs_at = append(&end, nvols * kBitswap1JobBytes, a);
    l.tiles_at = append(&end, (nvols + 1) * 4, a);
    l.vols_at = append(&end, nvols * kLz4BatchVolumeBytes, a);
    l.text_at = append(&end, text_bytes, a);
    l.upload = round_up(end, a);
    uint64_t staging = l.upload;
    l.decode_at = append(&staging, quantised ? nvols * kQuantiserBatchDecodeBytes : 0, a);
    l.staging_bytes = staging;
    l.csize_at = append(&end, nchunks * 4, a);
    l.redo_at = append(&end, (nchunks + 1) * 4, a);
    l.foff_at = append(&end, nchunks * 8, a);
    l.vinfo_at = append(&end, nvols * 16, a);
    l.tables = end;
    return l;
}

Lz4DedupeLayout lz4_dedupe_layout(const Lz4EncodeLayout& lay, uint64_t piece_hash_words)
{
    Lz4DedupeLayout d;
    if (!piece_hash_words || !lay.chunked() || lay.chunk % 1024 != 0 || lay.nchunks < 2) return d;
    d.table = 64;
    while (d.table < 2 * lay.nchunks) d.table <<= 1;
    d.work_at = round_up(piece_hash_words * 4, 64);
    d.tab_key_at = d.work_at + lay.nchunks * 8;
    d.tab_val_at = d.tab_key_at + d.table * 8;
    d.dup_at = d.tab_val_at + d.table * 4 + 64;
    d.holes_at = d.dup_at + round_up(lay.nchunks * 4, 8);
    d.total = d.holes_at + lay.nchunks * (1u + ((lay.chunk >> 10) + 63u) / 64u) * 8u;       // per chunk: a word, and a bit per 1 KiB piece
    return d;
}

Lz4TableClearPlan lz4_table_clear_plan(const Lz4DedupeLayout& d, bool frames_in_place, bool on_lanes)
{
    Lz4TableClearPlan p;
    if (!d.total || !frames_in_place) return p;
    p.who = Lz4TableClearPlan::kernel;
    const uint64_t key_bytes = d.table * 8, bytes = d.table * 12;
    if (!on_lanes || d.tab_val_at != d.tab_key_at + key_bytes || (d.tab_key_at & 7) || (bytes & 15) || key_bytes < 16 || bytes > 0xffffffffull) return p;
    p.who = Lz4TableClearPlan::transposer;
    p.table_at = d.tab_key_at;
    p.key_bytes = (uint32_t)key_bytes;
    p.bytes = (uint32_t)bytes;
    return p;
}

Lz4InplacePlan lz4_inplace_plan(const Lz4EncodeLayout& lay, uint64_t piece_hash_words, bool lz4_is_last, bool takes_offset, unsigned dst_mod16,
                                uint64_t capacity, uint64_t header_max)
{
    Lz4InplacePlan p;
    if (!lz4_dedupe_layout(lay, piece_hash_words).total || !lz4_is_last || !takes_offset || (lay.chunk & (lay.chunk - 1))) return p;
    p.chunk = lay.chunk;
    p.t0 = header_max;
    while ((dst_mod16 + p.t0 + kLz4FrameHead) & 15) ++p.t0;         // body of chunk 0 on a 16-byte boundary
    p.in_stride = lay.chunk + kLz4FrameGap;
    p.body0 = p.t0 + kLz4FrameHead;
    p.on = p.t0 + lay.nchunks * p.in_stride <= capacity;
    return p.on ? p : Lz4InplacePlan();
}

static uint32_t lz4_noise_digest_stride(uint32_t chunk)
{
    if (chunk < 16384u || (chunk & (chunk - 1u))) return 0;
    uint64_t p = 1, st = 1, nb = 64, probes = 0;
    for (;;) {
        ++probes;
        const uint64_t p2 = p + st;
        st = nb >> 6; ++nb;
        if (p2 > (uint64_t)chunk - 12 + 1) break;
        p = p2;
    }
    if (probes <= 961) return 0;
    return (uint32_t)(((probes - 960) + 63) & ~(uint64_t)63);
}

uint32_t lz4_noise_digest_words(const Lz4Params& p, const Lz4EncodeLayout& lay, bool option_on, uint64_t segment_bytes)
{
    const uint32_t stride = lay.chunk <= 0xffffffffull ? lz4_noise_digest_stride((uint32_t)lay.chunk) : 0;
    return option_on && stride && segment_bytes % lay.chunk == 0 && p.accel >= 0 ? stride : 0;
}

bool lz4_spec_wanted(const Lz4Plan& plan)
{
    const uint64_t nframes = plan.frame_first.size() - 1;
    uint64_t longest = 0;
    for (uint64_t f = 0; f < nframes; ++f) longest = std::max<uint64_t>(longest, plan.frame_first[f + 1] - plan.frame_first[f]);
    return longest >= 3 && nframes < 1024;
}

void lz4_warmup_windows(const Lz4Plan& plan, uint64_t warmup, std::vector<uint32_t>* first, std::vector<uint32_t>* last)
{
    first->resize(plan.blocks.size()); last->resize(plan.blocks.size());
    for (size_t f = 0; f + 1 < plan.frame_first.size(); ++f)
        for (uint32_t k = plan.frame_first[f]; k < plan.frame_first[f + 1]; ++k) {
            uint32_t j = k;
            uint64_t have = 0;
            while (j > plan.frame_first[f] && have < warmup) { --j; have += plan.blocks[j].n; }
            (*first)[k] = j; (*last)[k] = k;
        }
}

Lz4RedoRuns lz4_redo_runs(const Lz4Plan& plan, const std::vector<uint32_t>& ok, uint64_t run_max, std::vector<uint32_t>* first, std::vector<uint32_t>* last)
{
    Lz4RedoRuns r;
    const uint64_t nblocks = ok.size();
    for (uint64_t k = 0; k < nblocks; ++k) {
        if (ok[k]) continue;
        uint64_t e = k;
        while (e + 1 < nblocks && !ok[e + 1] && !(plan.blocks[e + 1].flags & 1u)) ++e;
        r.longest = std::max(r.longest, e - k + 1);
        (*first)[r.nruns] = (uint32_t)k; (*last)[r.nruns] = (uint32_t)std::min(e, k + run_max - 1); ++r.nruns;
        k = e;
    }
    return r;
}

// ---- decode planning ----
Lz4DecodeGeometry lz4_decode_geometry(const Lz4Params& p, uint64_t total)
{
    Lz4DecodeGeometry g;
    g.chunk = total ? p.bytes_per_chunk(total) : 1;
    g.block_bytes = p.block_bytes();
    g.nchunks = total ? (total + g.chunk - 1) / g.chunk : 0;
    g.max_blocks = std::max<uint64_t>(g.nchunks * ((g.chunk + g.block_bytes - 1) / g.block_bytes), total / g.block_bytes + 1) + 16;
    return g;
}

bool lz4_chunks_whole(uint64_t nframes, uint64_t nchunks, uint64_t total, uint64_t chunk)
{
    return nframes == nchunks && nframes > 1 && chunk && total % chunk == 0;
}

bool lz4_folds_into_shuffle(uint64_t nframes, uint64_t nchunks, uint64_t total, uint64_t chunk, uint64_t Z, uint64_t fb)
{
    return lz4_chunks_whole(nframes, nchunks, total, chunk) && fb && fb % chunk == 0 && Z * fb == total;
}

bool frame_shuffle_decode_map(std::vector<unsigned char>* map, uint64_t Z, std::vector<uint64_t>* unnamed, bool* permutation)
{
    if (map->size() % 8 != 0 || map->size() / 8 != Z) return false;
    auto slot = [&](uint64_t i) { uint64_t v; std::memcpy(&v, map->data() + 8 * i, 8); return v; };
    std::vector<uint64_t> last(Z, ~0ull);            // the last slot named for a place
    *permutation = true;
    for (uint64_t i = 0; i < Z; ++i) {
        const uint64_t v = slot(i);
        if (v >= Z) return false;
        if (last[v] != ~0ull) *permutation = false;
        last[v] = i;
    }
    unnamed->clear();
    if (*permutation) return true;
    // A map that names a place twice (frames of equal metric on the encoder's side: same bytes -- or a crafted blob: not): the last
    // slot named for a place stays, whatever order the scatter's workgroups run in -- the earlier ones are struck.
    for (uint64_t v = 0; v < Z; ++v) if (last[v] == ~0ull) unnamed->push_back(v);
    for (uint64_t i = 0; i < Z; ++i)
        if (last[slot(i)] != i) { const uint64_t none = ~0ull; std::memcpy(map->data() + 8 * i, &none, 8); }
    return true;
}

FrameRangesPlan frame_ranges_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, const std::vector<std::pair<uint64_t, uint64_t>>& ranges, uint64_t chunk,
                                  uint64_t total, uint32_t nframes, const std::vector<unsigned char>& struck_map, uint64_t place_bytes, uint64_t places)
{
    FrameRangesPlan p;
    const uint64_t e = (uint64_t)elem;
    p.we = form == RangeForm::planes ? elem : 1;
    const uint64_t we = (uint64_t)p.we;
    // ranges inside the volume, the stream the voxels in their order, one frame per chunk
    if (shape0 == 0 || n == 0 || n % shape0 != 0 || ranges.empty() || (elem != 1 && elem != 2) || chunk == 0 ||
        total != n * (form == RangeForm::planes_lut ? 1 : e) || (uint64_t)nframes != (total + chunk - 1) / chunk)
        return p;
    for (const auto& r : ranges)
        if (r.second == 0 || r.first >= shape0 || r.second > shape0 - r.first) return p;
    const uint64_t vpf = n / shape0, fb = vpf * e;
    std::vector<FrameRangesBox> boxes(ranges.size());
    for (size_t i = 0; i < ranges.size(); ++i) {
        boxes[i].v0 = ranges[i].first * vpf;
        boxes[i].v1 = (ranges[i].first + ranges[i].second) * vpf;
    }
    if (form == RangeForm::shuffle) {
        if (!lz4_folds_into_shuffle(nframes, nframes, total, chunk, places, place_bytes) || struck_map.size() != places * 8) return p;
        // the places some range needs, compacted in ascending order: cplace[v] is place v's index in there
        std::vector<char> wanted(places, 0);
        for (size_t i = 0; i < ranges.size(); ++i) {
            FrameRangesBox& b = boxes[i];
            b.pa = ranges[i].first * fb / place_bytes;
            b.pb = ((ranges[i].first + ranges[i].second) * fb + place_bytes - 1) / place_bytes;
            for (uint64_t v = b.pa; v < b.pb; ++v) wanted[v] = 1;
        }
        std::vector<uint64_t> cplace(places, 0);
        uint64_t np = 0;
        for (uint64_t v = 0; v < places; ++v) if (wanted[v]) cplace[v] = np++;
        const uint64_t cpf = place_bytes / chunk;
        std::vector<char> named(np, 0);
        // (the struck map: the last slot named for a place wins, as in the full decode)
        for (uint64_t i = 0; i < places; ++i) {
            uint64_t v;
            std::memcpy(&v, struck_map.data() + 8 * i, 8);
            if (v == ~0ull || v >= places || !wanted[v]) continue;
            p.remap.push_back(cplace[v]);
            named[cplace[v]] = 1;
            for (uint64_t c = 0; c < cpf; ++c) p.ids.push_back((uint32_t)(i * cpf + c));
        }
        for (uint64_t k = 0; k < np;) {
            if (named[k]) { ++k; continue; }
            uint64_t k1 = k;
            while (k1 < np && !named[k1]) ++k1;
            p.zero_runs.push_back({k, k1});
            k = k1;
        }
        p.out_bytes = np * place_bytes;
        for (size_t i = 0; i < ranges.size(); ++i) {
            FrameRangesBox& b = boxes[i];
            // (a range's own places are consecutive in the compaction: all of [pa, pb) are wanted)
            const uint64_t z0 = ranges[i].first, nz = ranges[i].second, in_place = z0 * fb - b.pa * place_bytes;
            b.range_at = cplace[b.pa] * place_bytes + in_place;
            b.direct = b.range_at == 0 && in_place == 0 && b.pb * place_bytes == (z0 + nz) * fb;
        }
        p.boxes.swap(boxes);
        p.ok = true;
        return p;
    }
    // byte spans of the stream in front of lz4 that each range needs (planes: the plane segments' words in their order, then the tail)
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> spans(ranges.size());
    std::vector<char> need(nframes, 0);
    for (size_t i = 0; i < ranges.size(); ++i) {
        FrameRangesBox& b = boxes[i];
        if (form == RangeForm::plain)
            spans[i].push_back({b.v0 * e, b.v1 * e});
        else {
            // W = 8 * we plane segments of seg words (we bytes, W voxels each), then the n % W voxels behind them verbatim
            const uint64_t W = 8 * we, seg = n / W;
            b.L = seg * W;
            b.w0 = std::min(b.v0 / W, seg);
            b.w1 = std::min((b.v1 + W - 1) / W, seg);
            if (b.w0 < b.w1) for (uint64_t s = 0; s < W; ++s) spans[i].push_back({(s * seg + b.w0) * we, (s * seg + b.w1) * we});
            if (b.v1 > b.L) spans[i].push_back({std::max(b.v0, b.L) * we, b.v1 * we});
        }
        for (const auto& sp : spans[i]) for (uint64_t f = sp.first / chunk; f <= (sp.second - 1) / chunk; ++f) need[f] = 1;
    }
    p.coff.assign(nframes, 0);
    for (uint32_t f = 0; f < nframes; ++f) {
        if (!need[f]) continue;
        p.coff[f] = p.out_bytes;
        p.ids.push_back(f);
        p.out_bytes += std::min<uint64_t>(chunk, total - (uint64_t)f * chunk);
    }
    // A span is contiguous in the stream and every frame that covers it is selected: it is contiguous in the compaction too, whatever
    // frames of other ranges lie between two spans, and the address of its first byte is the address of all of it
    auto compact = [&](uint64_t b) { const uint64_t f = b / chunk; return p.coff[f] + (b - f * chunk); };
    for (size_t i = 0; i < ranges.size(); ++i) {
        FrameRangesBox& b = boxes[i];
        if (form == RangeForm::plain) b.range_at = compact(spans[i][0].first);
        else {
            for (size_t s = 0; b.w0 < b.w1 && s < (size_t)(8 * we); ++s) b.plane[s] = compact(spans[i][s].first);
            if (b.v1 > b.L) b.tail = compact(spans[i].back().first);
        }
    }
    p.boxes.swap(boxes);
    p.ok = true;
    return p;
}

FrameRangePlan frame_range_plan_of(const FrameRangesPlan& u, size_t box)
{
    FrameRangePlan p;
    p.we = u.we;
    if (!u.ok || box >= u.boxes.size()) return p;
    const FrameRangesBox& b = u.boxes[box];
    p.ok = true;
    p.ids = u.ids; p.out_bytes = u.out_bytes; p.coff = u.coff; p.remap = u.remap; p.zero_runs = u.zero_runs;
    p.range_at = b.range_at;
    std::copy(b.plane, b.plane + 16, p.plane);
    p.tail = b.tail; p.v0 = b.v0; p.v1 = b.v1; p.w0 = b.w0; p.w1 = b.w1; p.L = b.L;
    p.pa = b.pa; p.pb = b.pb; p.direct = b.direct;
    return p;
}

FrameRangePlan frame_range_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, uint64_t z0, uint64_t nz, uint64_t chunk, uint64_t total,
                                uint32_t nframes, const std::vector<unsigned char>& struck_map, uint64_t place_bytes, uint64_t places)
{
    return frame_range_plan_of(frame_ranges_plan(form, n, elem, shape0, {{z0, nz}}, chunk, total, nframes, struck_map, place_bytes, places), 0);
}

BoxPath decode_box_path(bool subset_form, RangeForm form, bool option_on)
{
    if (!subset_form || !option_on) return BoxPath::whole_copy;
    return form == RangeForm::planes || form == RangeForm::planes_lut ? BoxPath::subset_transposer : BoxPath::subset_copy;
}

BoxesPath decode_boxes_path(bool subset_form, RangeForm form, bool subset_option, bool joint_option)
{
    if (!joint_option) return BoxesPath::box_by_box;
    switch (decode_box_path(subset_form, form, subset_option)) {
    case BoxPath::subset_transposer: return BoxesPath::subset_transposer;
    case BoxPath::subset_copy: return BoxesPath::subset_copy;
    default: return BoxesPath::whole_copy;
    }
}

BoxPath compare_boxes_path(bool subset_form, RangeForm form, bool option_on)
{
    if (!subset_form || !option_on) return BoxPath::whole_copy;
    switch (form) {
    case RangeForm::planes:
    case RangeForm::planes_lut: return BoxPath::subset_transposer;
    case RangeForm::plain:
    case RangeForm::shuffle: return BoxPath::subset_copy;
    }
    return BoxPath::whole_copy;
}

BoxPath project_boxes_path(bool subset_form, RangeForm form, bool option_on)
{
    if (!subset_form || !option_on) return BoxPath::whole_copy;
    switch (form) {
    case RangeForm::planes:
    case RangeForm::planes_lut: return BoxPath::subset_transposer;
    case RangeForm::plain:
    case RangeForm::shuffle: return BoxPath::subset_copy;
    }
    return BoxPath::whole_copy;
}

bool admit_projection(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, int axis, int op, uint64_t maxvoxel,
                      const void* out, const long* out_strides, BatchWindow* w, Projection* p)
{
    if (!w || !p || !admit_window(header_shape, origin, extent, rank, w)) return false;
    if (axis < 0 || (unsigned)axis >= rank || op < 0 || op > 2) return false;
    if (!out || reinterpret_cast<uintptr_t>(out) % 4u) return false;
    const uint64_t e[3] = {w->Z, w->Y, w->X};
    Projection q;
    q.axis3 = (uint32_t)axis + 3u - rank;
    q.n = e[q.axis3];
    // the sum bound: maxvoxel n >= 2^32 is refused -- and the 16-bit extent 65537 with it (65535 x 65537 = 2^32 - 1 would still fit; the
    // stated bound for 16-bit voxels is 65536 | 65537, the stricter one, and it is kept)
    if (op == 2 && q.n > (maxvoxel > 255 ? (uint64_t)65536 : 0xffffffffull / maxvoxel)) return false;
    if (rank > 1) {
        long shape[2];
        unsigned k2 = 0;
        for (unsigned k = 0; k < rank; ++k) if (k != (unsigned)axis) shape[k2++] = extent[k];
        BatchView v;
        if (!admit_view(shape, out_strides, rank - 1, &v)) return false;
    }
    // the image padded to two dimensions: what is left of (Z, Y, X)
    const uint64_t plane = w->bY * w->bX;
    const uint64_t step[3] = {plane, w->bX, 1};
    const unsigned u = q.axis3 == 0 ? 1 : 0, v = q.axis3 == 2 ? 1 : 2;
    q.E0 = e[u]; q.E1 = e[v];
    q.su = step[u]; q.sv = step[v]; q.sa = step[q.axis3];
    q.p0 = rank == 3 && out_strides ? (uint64_t)out_strides[0] : q.E1;     // (ranks 1 and 2: E0 = 1, the pitch is never stepped over)
    if (q.axis3 == 0) { q.sz = 0; q.sy = q.p0; }
    else if (q.axis3 == 1) { q.sz = q.p0; q.sy = 0; }
    else {
        uint64_t K = 1;
        while (K < w->X) K <<= 1;                                       // (X <= the blob's row, below 2^62: no wrap)
        if (q.p0 >= ((uint64_t)1 << 62) / K) return false;
        q.sy = K; q.sz = K * q.p0;
    }
    *p = q;
    return true;
}

BoxPath bin_boxes_path(bool subset_form, RangeForm form, bool option_on)
{
    if (!subset_form || !option_on) return BoxPath::whole_copy;
    switch (form) {
    case RangeForm::planes:
    case RangeForm::planes_lut: return BoxPath::subset_transposer;
    case RangeForm::plain:
    case RangeForm::shuffle: return BoxPath::subset_copy;
    }
    return BoxPath::whole_copy;
}

bool admit_binning(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, const long* bins, int op, uint64_t maxvoxel,
                   const void* out, const long* out_strides, BatchWindow* w, Binning* b)
{
    if (!w || !b || !admit_window(header_shape, origin, extent, rank, w)) return false;
    if (!bins || op < 0 || op > 2) return false;
    if (!out || reinterpret_cast<uintptr_t>(out) % 4u) return false;
    const uint64_t e[3] = {w->Z, w->Y, w->X};
    Binning q;
    long cells[3] = {1, 1, 1};
    constexpr uint64_t kSat = (uint64_t)1 << 33;                          // (above both bounds; a factor is clamped to it before it multiplies)
    uint64_t V = 1;
    for (unsigned k = 0; k < rank; ++k) {
        if (bins[k] < 1) return false;
        const unsigned d = 3 - rank + k;
        q.bins[d] = std::min((uint64_t)bins[k], e[d]);
        q.C[d] = (e[d] + q.bins[d] - 1) / q.bins[d];
        cells[k] = (long)q.C[d];
        V = std::min(V * std::min(q.bins[d], kSat), kSat);                // (both factors <= 2^33: no wrap)
    }
    // the projection's bound applied to the cell: 16-bit voxels up to 65536 of them, 8-bit ones while 255 V < 2^32
    if (op == 2 && V > (maxvoxel > 255 ? (uint64_t)65536 : 0xffffffffull / maxvoxel)) return false;
    BatchView v;
    if (!admit_view(cells, out_strides, rank, &v)) return false;
    q.py = rank >= 2 && out_strides ? (uint64_t)out_strides[rank - 2] : q.C[2];
    q.pz = rank == 3 && out_strides ? (uint64_t)out_strides[0] : q.C[1] * q.py;     // (ranks 1 and 2: one layer, the pitch is never stepped over)
    *b = q;
    return true;
}

BinPlan bin_boxes_plan(const uint64_t C[3], const uint64_t bins[3], uint64_t X, uint64_t budget_cells, uint64_t cap_voxels)
{
    BinPlan p{};
    p.C[0] = C[0]; p.C[1] = C[1]; p.C[2] = C[2];
    if (budget_cells == 0) budget_cells = 1;
    if (C[2] > budget_cells) {                                          // a cell row does not fit: ONE row, in strips
        p.band = 1;
        p.strip = budget_cells;
    } else {
        p.strip = C[2];
        // a cell row's footprint over the layer's frames, saturating
        constexpr uint64_t lim = (uint64_t)1 << 20;                      // (far above any cap: each factor is clamped to it first)
        const uint64_t row = std::min(std::min(bins[0], lim) * std::min(bins[1], lim), lim) * std::min(std::max<uint64_t>(X, 1), lim);
        p.band = std::max<uint64_t>(1, std::min({budget_cells / C[2], cap_voxels / row, C[1]}));
    }
    p.nbands = (C[1] + p.band - 1) / p.band;
    p.nstrips = (C[2] + p.strip - 1) / p.strip;
    p.blocks = C[0] * p.nbands * p.nstrips;                             // (the caller bounds the sum over the boxes: each factor is below 2^62 / the others for an admitted box)
    return p;
}

BoxPath histogram_boxes_path(bool subset_form, RangeForm form, bool option_on)
{
    if (!subset_form || !option_on) return BoxPath::whole_copy;
    switch (form) {
    case RangeForm::planes:
    case RangeForm::planes_lut: return BoxPath::subset_transposer;
    case RangeForm::plain:
    case RangeForm::shuffle: return BoxPath::subset_copy;
    }
    return BoxPath::whole_copy;
}

bool admit_histogram(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, int shift, int elem_size, const void* out,
                     BatchWindow* w)
{
    if (!w || !admit_window(header_shape, origin, extent, rank, w)) return false;
    if (histogram_bins(elem_size, shift) == 0) return false;
    return out && reinterpret_cast<uintptr_t>(out) % 4u == 0;
}

// ---- a resolution pyramid of boxes (SQYAMD_Pyramid_Boxes_*) ----
PyramidPath pyramid_boxes_path(bool subset_form, RangeForm form, bool subset_option, bool fused_option)
{
    return PyramidPath{bin_boxes_path(subset_form, form, subset_option), fused_option};
}

bool admit_pyramid(const std::vector<uint64_t>& header_shape, const long* origin, const long* extent, unsigned rank, long levels, const long* bins, int op,
                   uint64_t maxvoxel, const void* const* outs, const long* out_strides, BatchWindow* w, Pyramid* p, PyramidSizes* sizes)
{
    if (!w || !p || !bins || !outs || levels < 1 || levels > (long)kPyramidMaxLevels || rank < 1 || rank > 3) return false;
    for (long l = 0; l < levels; ++l)
        for (unsigned k = 0; k < rank; ++k) {
            const long b = bins[(size_t)l * rank + k];
            if (b < 1 || (l > 0 && b % bins[(size_t)(l - 1) * rank + k] != 0)) return false;      // (the level below is >= 1: checked first)
        }
    Pyramid y;
    y.levels = (uint32_t)levels;
    for (long l = 0; l < levels; ++l) {
        if (!admit_binning(header_shape, origin, extent, rank, bins + (size_t)l * rank, op, maxvoxel, outs[l], out_strides ? out_strides + (size_t)l * rank : nullptr, w,
                           &y.q[l]))
            return false;
        for (unsigned d = 0; d < 3; ++d) y.raw[l][d] = d < 3 - rank ? 1u : (uint64_t)bins[(size_t)l * rank + (d - (3 - rank))];
    }
    for (uint32_t l = levels; l < kPyramidMaxLevels; ++l)
        for (unsigned d = 0; d < 3; ++d) y.raw[l][d] = 1;
    if (sizes) {
        const uint64_t E[3] = {w->Z, w->Y, w->X};
        const uint64_t lim = 0x7fffffffull;
        sizes->cell_groups += (y.q[0].C[0] * y.q[0].C[1] * y.q[0].C[2] + 255) / 256;      // (the cells are no more than the blob's voxels: no wrap)
        sizes->bin_blocks += bin_boxes_plan(y.q[0].C, y.q[0].bins, w->X).blocks;
        sizes->blocks += pyramid_boxes_plan(y, E).blocks;
        for (long l = 1; l < levels; ++l) sizes->reduce_groups += (y.q[l].C[0] * y.q[l].C[1] * y.q[l].C[2] + 255) / 256;
        if (sizes->cell_groups > lim || sizes->bin_blocks > lim || sizes->blocks > lim || sizes->reduce_groups > lim) return false;
    }
    *p = y;
    return true;
}

static uint64_t pyramid_sat_mul(uint64_t a, uint64_t b)
{
    constexpr uint64_t lim = (uint64_t)1 << 40;                         // (far above every budget and cap: each factor is clamped to it first)
    return std::min(std::min(a, lim) * std::min(b, lim), lim);
}

uint64_t pyramid_level_cells(const PyramidPlan& p, uint32_t l, uint64_t band, uint64_t strip)
{
    return pyramid_sat_mul(std::min(pyramid_sat_mul(band, p.q[l][1]), p.C[l][1]), std::min(pyramid_sat_mul(strip, p.q[l][2]), p.C[l][2]));
}

PyramidPlan pyramid_boxes_plan(const Pyramid& y, const uint64_t E[3], uint64_t budget_level0, uint64_t budget_cells, uint64_t cap_voxels)
{
    PyramidPlan p{};
    const uint32_t levels = std::min(std::max<uint32_t>(y.levels, 1), kPyramidMaxLevels);
    p.levels = levels;
    budget_level0 = std::max<uint64_t>(budget_level0, 1);
    budget_cells = std::max(budget_cells, budget_level0);
    for (uint32_t l = 0; l < kPyramidMaxLevels; ++l)
        for (int d = 0; d < 3; ++d) {
            p.C[l][d] = l < levels ? y.q[l].C[d] : 1;
            p.r[l][d] = l && l < levels ? std::min(y.raw[l][d] / y.raw[l - 1][d], p.C[l - 1][d]) : 1;
            p.q[l][d] = 1;
        }
    // level-`from` cells under one level-`to` cell (from <= to), clamped to the grid
    const auto under = [&](uint32_t to, uint32_t from, int d) { return std::min(y.raw[to][d] / y.raw[from][d], p.C[from][d]); };
    uint32_t T = 0;
    for (uint32_t t = levels - 1; t >= 1; --t) {
        if (pyramid_sat_mul(under(t, 0, 1), under(t, 0, 2)) > budget_level0) continue;
        uint64_t all = 0, voxels = 1;
        for (uint32_t l = 0; l <= t; ++l) all += pyramid_sat_mul(under(t, l, 1), under(t, l, 2));
        // (a row of level-t cells over the box's width and all its frames: the least a block walks)
        for (int d = 0; d < 3; ++d) voxels = pyramid_sat_mul(voxels, d == 2 ? std::max<uint64_t>(E[d], 1) : std::min(y.raw[t][d], std::max<uint64_t>(E[d], 1)));
        if (all > budget_cells || voxels > cap_voxels) continue;
        T = t;
        break;
    }
    p.T = T;
    for (uint32_t l = 0; l < levels; ++l)
        for (int d = 0; d < 3; ++d) p.q[l][d] = l <= T ? under(T, l, d) : std::min(y.raw[l][d] / y.raw[T][d], p.C[T][d]);
    const auto fits = [&](uint64_t band, uint64_t strip) {
        if (pyramid_level_cells(p, 0, band, strip) > budget_level0) return false;
        uint64_t all = 0;
        for (uint32_t l = 0; l <= T; ++l) all += pyramid_level_cells(p, l, band, strip);
        return all <= budget_cells;
    };
    // the largest n in [1, hi] with ok(n), ok monotone and ok(1) true
    const auto largest = [](uint64_t hi, const auto& ok) {
        uint64_t lo = 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (ok(mid)) lo = mid; else hi = mid - 1;
        }
        return lo;
    };
    const uint64_t CT1 = p.C[T][1], CT2 = p.C[T][2];
    if (!fits(1, CT2)) {                                                // a row of level-T cells does not fit: ONE row, in strips
        p.band = 1;
        p.strip = largest(CT2, [&](uint64_t s) { return fits(1, s); });
    } else {
        p.strip = CT2;
        // a row of level-T cells over all its frames, saturating: a block walks band rows of it, layer by layer
        const uint64_t row = pyramid_sat_mul(pyramid_sat_mul(std::min(y.raw[T][0], std::max<uint64_t>(E[0], 1)), std::min(y.raw[T][1], std::max<uint64_t>(E[1], 1))),
                                             std::max<uint64_t>(E[2], 1));
        p.band = largest(std::min(CT1, std::max<uint64_t>(1, cap_voxels / row)), [&](uint64_t b) { return fits(b, CT2); });
    }
    p.nbands = (CT1 + p.band - 1) / p.band;
    p.nstrips = (CT2 + p.strip - 1) / p.strip;
    p.blocks = p.C[T][0] * p.nbands * p.nstrips;                        // (the caller bounds the sum over the boxes, as for bin_boxes_plan)
    uint64_t at = 0;
    for (uint32_t l = 0; l <= T; ++l) {
        p.off[l] = (uint32_t)at;
        at += pyramid_level_cells(p, l, p.band, p.strip);
    }
    return p;
}

// ---- a box written into one large blob (SQYAMD_Update_Box_*) ----
UpdateBoxPath update_box_path(const UpdateBoxFacts& f)
{
    const bool pipeline_ok = f.option_on && f.same_stages && f.form_ok;
    const bool layout_ok = f.layout.chunked() && f.layout.accel == 1 && f.layout.nchunks > 1;
    const bool blob_ok = f.subset_taken && f.frames == f.layout.nchunks && f.blocks == f.frames && f.frame_chunk == f.layout.chunk;
    return pipeline_ok && layout_ok && blob_ok ? UpdateBoxPath::subset_patch : UpdateBoxPath::whole;
}

bool pipelines_same_stages(const Pipeline& a, const Pipeline& b)
{
    if (a.stages.size() != b.stages.size() || a.sink_index != b.sink_index) return false;
    for (size_t i = 0; i < a.stages.size(); ++i) {
        const Stage &x = a.stages[i], &y = b.stages[i];
        if (x.kind != y.kind || x.name != y.name) return false;
        if (x.kind == StageKind::lz4 ? x.lz4.config() != y.lz4.config() || x.lz4.block_id != y.lz4.block_id : x.config() != y.config()) return false;
    }
    return true;
}

bool update_box_form_ok(const Pipeline& p)
{
    const size_t ns = p.stages.size();
    if (ns == 0 || ns > 2 || p.stages[ns - 1].kind != StageKind::lz4) return false;
    return ns == 1 || p.stages[0].kind == StageKind::bitswap1;
}

// ---- many boxes written into one large blob (SQYAMD_Update_Boxes_*) ----
UpdateBoxesPlan update_boxes_plan(RangeForm form, uint64_t n, int elem, uint64_t shape0, const std::vector<std::pair<uint64_t, uint64_t>>& ranges,
                                  const std::vector<BatchWindow>& windows)
{
    UpdateBoxesPlan p;
    if (shape0 == 0 || n == 0 || n % shape0 != 0 || ranges.empty() || ranges.size() > 0xffffffffull || windows.size() != ranges.size() || (elem != 1 && elem != 2) ||
        (form != RangeForm::plain && form != RangeForm::planes))
        return p;
    for (const auto& r : ranges)
        if (r.second == 0 || r.first >= shape0 || r.second > shape0 - r.first) return p;
    const bool planes = form == RangeForm::planes;
    const uint64_t vpf = n / shape0, W = 8 * (uint64_t)elem, seg = n / W, L = seg * W;
    std::vector<uint32_t> order(ranges.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ranges[a].first != ranges[b].first ? ranges[a].first < ranges[b].first : a < b; });
    uint64_t z1 = 0;                                                    // the open segment ends in front of frame z1
    for (uint32_t i : order) {
        const uint64_t a = ranges[i].first, b = a + ranges[i].second;
        bool join = false;
        if (!p.segments.empty()) {
            // (ascending first frames: the open segment's last word is the one its last voxel lies in)
            const uint64_t open_w1 = std::min((z1 * vpf + W - 1) / W, seg), w0 = std::min(a * vpf / W, seg);
            if (a < z1) { join = true; ++(planes && a * vpf >= L ? p.merged_tail : p.merged_overlap); }
            else if (a == z1) { join = true; ++p.merged_overlap; }
            else if (planes && w0 < open_w1) { join = true; ++p.merged_word; }
        }
        if (!join) {
            p.segments.push_back(UpdateBoxesSegment{a, 0, {}});
            z1 = b;
        }
        UpdateBoxesSegment& s = p.segments.back();
        z1 = std::max(z1, b);
        s.nz = z1 - s.z0;
        s.boxes.push_back(i);
    }
    for (UpdateBoxesSegment& s : p.segments) std::sort(s.boxes.begin(), s.boxes.end());
    if (form == RangeForm::plain) p.layer_first = update_boxes_layers(windows);
    p.ok = true;
    return p;
}

std::vector<uint32_t> update_boxes_layers(const std::vector<BatchWindow>& windows)
{
    std::vector<uint32_t> first;
    if (windows.empty()) return first;
    first.push_back(0);
    for (size_t i = 1; i < windows.size(); ++i)
        for (size_t j = first.back(); j < i; ++j)
            if (windows_overlap(windows[i], windows[j])) { first.push_back((uint32_t)i); break; }
    first.push_back((uint32_t)windows.size());
    return first;
}

bool lz4_splice_ok(const std::vector<uint32_t>& slot_of, size_t nselected)
{
    if (slot_of.empty() || slot_of.size() > 0x7fffffffull || nselected > slot_of.size()) return false;
    uint32_t next = 0;
    for (uint32_t s : slot_of) {
        if (s == kSpliceOldFrame) continue;
        if (s != next) return false;
        ++next;
    }
    return next == nselected;
}

Lz4SplicePlan lz4_splice_plan(const std::vector<uint64_t>& old_off, const std::vector<uint32_t>& old_size, const std::vector<uint32_t>& slot_of,
                              const std::vector<uint32_t>& csize, const std::vector<uint32_t>& n, uint64_t src_payload, uint32_t prefix_len, uint32_t suffix_len,
                              uint32_t elem_size, uint64_t capacity)
{
    Lz4SplicePlan p;
    const size_t nf = slot_of.size();
    p.status = kSpliceBadIndex;
    if (old_off.size() != nf || old_size.size() != nf || csize.size() != n.size() || !lz4_splice_ok(slot_of, n.size()) || elem_size == 0) return p;
    p.frame_off.assign(nf + 1, 0);
    bool bad = false;
    for (size_t f = 0; f < nf; ++f) {
        const uint32_t k = slot_of[f];
        uint64_t sz;
        if (k == kSpliceOldFrame) {
            bad = bad || !lz4_splice_old_frame_ok(old_off[f], old_size[f], src_payload);
            sz = lz4_splice_old_frame_bytes(old_size[f]);
        } else
            sz = lz4_splice_new_frame_bytes(csize[k], n[k]);
        p.frame_off[f + 1] = p.frame_off[f] + sz;
    }
    p.payload = p.frame_off[nf];
    p.header_bytes = lz4_splice_header_bytes(prefix_len, suffix_len, p.payload, elem_size);
    p.status = bad ? kSpliceBadIndex : lz4_splice_status(p.header_bytes, p.payload, capacity);
    return p;
}

// ---- stages ----
static StageKind kind_of(const std::string& n)
{
    if (n == "diff3x3x1") return StageKind::diff3x3x1;
    if (n == "bitswap1") return StageKind::bitswap1;
    if (n == "frame_shuffle") return StageKind::frame_shuffle;
    if (n == "raster_reorder") return StageKind::raster_reorder;
    if (n == "zcurve_reorder") return StageKind::zcurve_reorder;
    if (n == "tile_shuffle") return StageKind::tile_shuffle;
    if (n == "bitshuffle") return StageKind::bitshuffle;
    if (n == "quantiser") return StageKind::quantiser;
    if (n == "lz4") return StageKind::lz4;
    if (n == "pass_through") return StageKind::pass_through;
    if (n == "rmestbkrd") return StageKind::rmestbkrd;
    if (n == "rmbkrd_neighbor5x5x5") return StageKind::rmbkrd_neighbor5;
    return StageKind::unsupported;
}

std::string Stage::config() const
{
    switch (kind) {
        case StageKind::bitswap1: return "num_bits_per_plane=1";                 // bitswap_scheme_impl.hpp:84-90
        case StageKind::diff3x3x1: return "";                                    // diff_scheme_impl.hpp:55-59
        case StageKind::lz4: return lz4.config();                                // lz4.hpp:132-141
        case StageKind::pass_through: return "";
        case StageKind::rmestbkrd: return "";                                    // remove_estimated_background_scheme_impl.hpp:32-40
        case StageKind::rmbkrd_neighbor5:                                        // flatten_to_neighborhood_scheme_impl.hpp:73-80 (%f)
            return "threshold=" + std::to_string(nb_threshold) + ",fraction=" + std::to_string(nb_fraction);
        case StageKind::quantiser: {                                             // quantiser_scheme_impl.hpp:102-118
            std::string s;
            size_t count = 0;
            for (const auto& kv : cfg) {
                s += kv.first + "=" + kv.second;
                if (count++ < cfg.size() - 1) s += ",";
            }
            return s;
        }
        case StageKind::raster_reorder: {                                        // raster_reorder_scheme_impl.hpp:53-59
            auto t = cfg.find("tile_size");
            return "tile_size=" + std::to_string(t != cfg.end() ? std::atoi(t->second.c_str()) : 0);
        }
        case StageKind::zcurve_reorder: {                                        // zcurve_reorder_scheme_impl.hpp:68-74 (default tile 2)
            auto t = cfg.find("tile_size");
            return "tile_size=" + std::to_string(t != cfg.end() ? std::atoi(t->second.c_str()) : 2);
        }
        case StageKind::tile_shuffle: {                                          // tile_shuffle_scheme_impl.hpp:57-66 (default tile 32)
            auto t = cfg.find("tile_size");
            auto m = cfg.find("reorder_map");
            return "tile_size=" + std::to_string(t != cfg.end() ? std::atoi(t->second.c_str()) : 32) + ",reorder_map=" + (m != cfg.end() ? m->second : "");
        }
        case StageKind::bitshuffle: {                                            // bitshuffle_scheme_impl.hpp:75-81 (default block 0 = library default)
            auto b = cfg.find("block_size");
            return "block_size=" + std::to_string(b != cfg.end() ? std::atoi(b->second.c_str()) : 0);
        }
        case StageKind::frame_shuffle: {                                         // frame_shuffle_scheme_impl.hpp:58-66
            auto c = cfg.find("frame_chunk_size");
            auto m = cfg.find("reorder_map");
            const int chunk = c != cfg.end() ? std::atoi(c->second.c_str()) : 1;
            return "frame_chunk_size=" + std::to_string(chunk) + ",reorder_map=" + (m != cfg.end() ? m->second : "");
        }
        default: return "";
    }
}

std::string Stage::full_name() const
{
    const std::string c = config();
    return c.empty() ? name : name + "(" + c + ")";
}

static bool in_list(const std::string& n, const char* const* list, size_t cnt)
{
    for (size_t i = 0; i < cnt; ++i) if (n == list[i]) return true;
    return false;
}

bool known_head_filter(const std::string& n)
{
    // (bitshuffle: present when the reference is built with USE_BITSHUFFLE, its default: CMakeLists.txt:47, sqeazy_pipelines.hpp:35-37)
    static const char* const l[] = {"diff3x3x1", "bitswap1", "bitshuffle", "remove_background", "rmbkrd_neighbor5x5x5", "rmestbkrd",
                                    "raster_reorder", "tile_shuffle", "frame_shuffle", "zcurve_reorder"};
    return in_list(n, l, sizeof(l) / sizeof(l[0]));
}
bool known_sink(const std::string& n)
{
    static const char* const l[] = {"pass_through", "quantiser", "lz4"};
    return in_list(n, l, sizeof(l) / sizeof(l[0]));
}
bool known_tail_filter(const std::string& n)
{
    static const char* const l[] = {"diff3x3x1", "bitswap1", "bitshuffle", "lz4", "raster_reorder", "tile_shuffle", "frame_shuffle",
                                    "zcurve_reorder"};
    return in_list(n, l, sizeof(l) / sizeof(l[0]));
}

bool Pipeline::reference_accepts(const std::string& s)
{
    // dynamic_pipeline.hpp:177-226
    const pairs_t pairs = parse_pairs(s);
    bool ok = true;
    const std::vector<std::string> majors = s.empty() ? std::vector<std::string>() : split_outside_verbatim(s, "->", &ok);
    if (!ok || majors.size() != pairs.size()) return false;
    uint32_t found = 0;
    bool sink_matched = false;
    for (const auto& p : pairs) {
        if (!sink_matched && known_head_filter(p.first)) { found++; continue; }
        if (known_sink(p.first)) { found++; sink_matched = true; continue; }
        if (known_tail_filter(p.first)) found++;
    }
    bool value = found == pairs.size();
    size_t rebuild = 2 * (pairs.size() - 1);          // size_t arithmetic, wraps for the empty string like the reference
    for (const auto& p : pairs) {
        rebuild += p.first.size();
        if (!p.second.empty()) rebuild += 2 + p.second.size();
    }
    return value && rebuild == s.size();
}

Pipeline Pipeline::from_string(const std::string& s, int elem_size)
{
    // dynamic_pipeline.hpp:137-170: head filters until the first sink, then tail filters; unknown names are skipped
    Pipeline p;
    for (const auto& pr : parse_pairs(s)) {
        Stage st;
        st.name = pr.first;
        st.kind = kind_of(pr.first);
        st.cfg = parse_minors(pr.second);
        if (st.kind == StageKind::lz4) st.lz4 = Lz4Params(pr.second);
        if (st.kind == StageKind::rmbkrd_neighbor5) {
            long t = 1;
            float f = 0.5f;
            if (neighbor5_parse(st.cfg, &t, &f)) {
                // `raw_type threshold = std::stoi(..)`: the int narrowed to the voxel type (modulo 2^8 / 2^16)
                st.nb_threshold = elem_size == 2 ? (long)(uint16_t)t : elem_size == 1 ? (long)(uint8_t)t : t;
                st.nb_fraction = f;
            }
        }
        if (st.kind == StageKind::raster_reorder && elem_size > 0 && !st.cfg.count("tile_size"))
            st.cfg["tile_size"] = std::to_string(16 / (p.sink_index >= 0 ? 1 : elem_size));   // raster_reorder_scheme_impl.hpp:23 (behind the sink: raster_reorder_scheme<char>)
        if (p.sink_index < 0) {
            if (known_head_filter(pr.first)) { p.stages.push_back(st); continue; }
            if (known_sink(pr.first)) { p.sink_index = (int)p.stages.size(); p.stages.push_back(st); }
        } else if (known_tail_filter(pr.first)) {
            p.stages.push_back(st);
        }
    }
    return p;
}

bool Pipeline::supported(const std::string& s, int elem_size, std::string* why)
{
    auto fail = [&](const std::string& m) { if (why) *why = m; return false; };
    if (!reference_accepts(s)) return fail("not a valid sqeazy pipeline");
    const Pipeline p = from_string(s);
    if (p.stages.empty()) return fail("empty pipeline");
    for (size_t i = 0; i < p.stages.size(); ++i) {
        const Stage& st = p.stages[i];
        switch (st.kind) {
            case StageKind::bitswap1: break;
            case StageKind::diff3x3x1:
                break;                                                           // (head filter, or tail filter on the sink's char output)
            case StageKind::frame_shuffle: {
                auto c = st.cfg.find("frame_chunk_size");
                // (N > 1: N frames per sort unit when N divides the frames -- checked against the shape at encode time)
                if (c != st.cfg.end() && std::atoi(c->second.c_str()) < 1)
                    return fail("frame_shuffle: frame_chunk_size must be positive");
                break;
            }
            case StageKind::zcurve_reorder:
                break;                                                           // (head filter, or tail filter on the sink's char output: round 5)
            case StageKind::tile_shuffle: {
                auto t = st.cfg.find("tile_size");
                if (t != st.cfg.end() && std::atoi(t->second.c_str()) <= 0) return fail("tile_shuffle: tile_size must be positive");
                break;
            }
            case StageKind::bitshuffle: {
                auto b = st.cfg.find("block_size");
                if (b != st.cfg.end() && (std::atoi(b->second.c_str()) < 0 || std::atoi(b->second.c_str()) % 8))
                    return fail("bitshuffle: block_size must be a non-negative multiple of 8");
                break;
            }
            case StageKind::raster_reorder: {
                auto t = st.cfg.find("tile_size");
                if (t != st.cfg.end() && std::atoi(t->second.c_str()) <= 0) return fail("raster_reorder: tile_size must be positive");
                break;
            }
            case StageKind::quantiser: {
                if (elem_size != 2) return fail("quantiser: only 16-bit input is implemented on MI355X");
                auto w = st.cfg.find("weighting_function");
                QuantiserWeighting qw;
                if (w != st.cfg.end() && !quantiser_parse_weighting(w->second, &qw))
                    return fail("quantiser: weighting_function=" + w->second + " gives the reference a NaN or infinite exponent; refused");
                break;
            }
            case StageKind::lz4:
                if (i + 1 != p.stages.size()) return fail("lz4 must be the last stage on MI355X");
                if (st.lz4.accel >= 3) return fail("lz4 accel >= 3 selects LZ4HC in liblz4; not implemented on MI355X");
                break;
            case StageKind::pass_through:
                break;
            case StageKind::rmestbkrd:
                break;                                                           // (head filter only; the shape is checked at encode time)
            case StageKind::rmbkrd_neighbor5: {
                long t;
                float f;
                if (!neighbor5_parse(st.cfg, &t, &f))
                    return fail("rmbkrd_neighbor5x5x5: threshold / fraction the reference's std::stoi / std::stof throws on, or a fraction that is not finite");
                break;
            }
            default:
                return fail("stage '" + st.name + "' is not implemented on MI355X");
        }
    }
    return true;
}

std::string Pipeline::name() const
{
    std::string v;
    for (size_t i = 0; i < stages.size(); ++i) {
        if (i) v += "->";
        v += stages[i].full_name();
    }
    return v;
}

bool raster_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X, uint64_t ts, int elem_size)
{
    if (ts == 0 || Z == 0 || Y == 0 || X == 0) return false;
    const int nrem = (Z % ts != 0) + (Y % ts != 0) + (X % ts != 0);
    if (nrem != 0 && nrem != 3) return false;                            // raster_reorder_utils.hpp:271-305: extent-0 tiles
    const uint64_t block = 16 / (uint64_t)elem_size;
    if (nrem == 0 && ts % block == 0 && ts != block) return false;       // :160-243: encode_full_simd overwrites the tile row's head
    return true;
}

// ---- background removal ----
bool neighbor5_parse(const std::map<std::string, std::string>& cfg, long* threshold, float* fraction)
{
    // flatten_to_neighborhood_scheme(const std::string&) (flatten_to_neighborhood_scheme_impl.hpp:44-60): fraction = std::stof,
    // threshold = std::stoi.  libstdc++ throws when nothing was converted or strtof / strtol report ERANGE (stoi: also outside int)
    *threshold = 1;
    *fraction = 0.5f;
    auto f = cfg.find("fraction");
    if (f != cfg.end()) {
        const char* p = f->second.c_str();
        char* end = nullptr;
        errno = 0;
        const float v = std::strtof(p, &end);
        if (end == p || errno == ERANGE || !std::isfinite(v)) return false;
        *fraction = v;
    }
    auto t = cfg.find("threshold");
    if (t != cfg.end()) {
        const char* p = t->second.c_str();
        char* end = nullptr;
        errno = 0;
        const long v = std::strtol(p, &end, 10);
        if (end == p || errno == ERANGE || v < INT_MIN || v > INT_MAX) return false;
        *threshold = v;
    }
    return true;
}

uint64_t neighbor5_z_end(uint64_t Z, uint64_t X)
{
    // halo::compute_offsets_in_x (neighborhood_utils.hpp:199-235): z runs to non_halo_end(2) = world[2] - 2 = X - 2 (row_major::x == 2),
    // offsets at or past the volume's end are dropped -- so z < min(X - 2, Z)
    const uint64_t e = std::min(X >= 2 ? X - 2 : 0, Z);
    return e < 2 ? 2 : e;
}

bool neighbor5_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X)
{
    if (Z == 0 || X < 5 || Y < 5) return false;          // (X - 4)(Y - 4) <= 1: the one-offset branch, halo_size_x = length - offsets[2]
    if (X == 5 && Y == 5) return false;
    const uint64_t n_offsets = (neighbor5_z_end(Z, X) - 2) * (Y - 4);
    return n_offsets != 1;                               // (one offset: `offsets.size() != 1` fails and offsets[2] is read again)
}

uint32_t host_l2_cache_bytes()
{
#if defined(__x86_64__) || defined(__i386__)
    // compass bit_view::range(b, e): bits [b, e) -- so range(16, 31) is 15 bits wide
    auto range = [](uint32_t v, uint32_t b, uint32_t e) -> uint32_t { return (v >> b) & ((1u << (e - b)) - 1u); };
    unsigned a = 0, b = 0, c = 0, d = 0;
    __cpuid_count(0, 0, a, b, c, d);
    char vendor[12];
    std::memcpy(vendor, &b, 4); std::memcpy(vendor + 4, &d, 4); std::memcpy(vendor + 8, &c, 4);
    const std::string brand(vendor, 12);
    std::vector<uint32_t> sizes;
    if (brand.find("AMD") != std::string::npos) {                  // cache::on_amd (compass.hpp:993-1021)
        __cpuid_count(0x80000005u, 0, a, b, c, d);
        if (range(c, 0, 7)) {
            sizes.push_back(range(c, 24, 31) * 1024u);
            __cpuid_count(0x80000006u, 0, a, b, c, d);
            sizes.push_back((range(c, 16, 31) & 0xffffu) * 1024u);
            sizes.push_back(range(d, 19, 31) * 512u * 1024u);
        }
    }
    if (brand.find("Intel") != std::string::npos) {                // cache::on_intel (compass.hpp:955-990)
        for (uint32_t l = 0; l < 8; ++l) {
            __cpuid_count(4, l, a, b, c, d);
            if (!(a & 2u) || range(a, 5, 8) != l) continue;
            const uint32_t ways = 1 + range(b, 22, 31), partitions = 1 + range(b, 12, 21), line = 1 + range(b, 0, 11), sets = 1 + c;
            sizes.push_back(ways * partitions * line * sets);
        }
    }
    return sizes.size() > 1 ? sizes[1] : 0;                         // cache::level(2)
#else
    return 0;
#endif
}

uint64_t rmestbkrd_face_portion(uint64_t frame_voxels, uint32_t l2_bytes)
{
    // background_scheme_utils.hpp:44-45: voxels compared with bytes, (index_type)(L2 * .75)
    return frame_voxels > (uint64_t)l2_bytes ? (uint64_t)(l2_bytes * .75) : frame_voxels;
}

int clean_number_of_threads(int n)
{
    static int max_threads = (int)std::thread::hardware_concurrency();
    if (n > max_threads || n <= 0) n = max_threads;
    return n;
}

void Pipeline::set_n_threads(int n) { nthreads = (unsigned)clean_number_of_threads(n); }

uint64_t Pipeline::max_encoded_size(uint64_t nbytes, int elem_size) const
{
    // header(incoming_t(), nbytes, name()): rank-1 shape {nbytes}, payload = nbytes*sizeof(T) (sqeazy_header.hpp:229-251)
    const std::string hdr = header_pack(elem_size, false, std::vector<uint64_t>(1, nbytes), name(), nbytes * (uint64_t)elem_size);
    uint64_t best = 0;
    for (const Stage& st : stages) {
        uint64_t v = nbytes;
        if (st.kind == StageKind::lz4) v = st.lz4.max_encoded_size(nbytes, nthreads);
        else if (st.kind == StageKind::quantiser) v = nbytes * (uint64_t)elem_size + 256u * (uint64_t)elem_size;
        best = std::max(best, v);
    }
    return 2 * hdr.size() + best;
}

// ---- header ----
static void json_escape(const std::string& s, std::string& out)
{
    // Boost.PropertyTree json writer escapes: " \ / and control characters
    static const char* hex = "0123456789ABCDEF";
    for (unsigned char c : s) {
        switch (c) {
            case '"': out += "\\\""; break;
            case '\\': out += "\\\\"; break;
            case '/': out += "\\/"; break;
            case '\b': out += "\\b"; break;
            case '\f': out += "\\f"; break;
            case '\n': out += "\\n"; break;
            case '\r': out += "\\r"; break;
            case '\t': out += "\\t"; break;
            default:
                if (c < 0x20) { out += "\\u00"; out += hex[c >> 4]; out += hex[c & 15]; }
                else out += (char)c;
        }
    }
}

// the header as  [pad] prefix | payload bytes in decimal | suffix  (pad: spaces in front up to a multiple of elem_size, which
// depends on the number of digits): what a kernel needs to write the header once the payload size is known on the device
void header_pack_parts(int elem_size, bool is_signed8, const std::vector<uint64_t>& shape, const std::string& pipename,
                       std::string* prefix, std::string* suffix)
{
    // (the byte count is the only number behind `"bytes": "`; the text is searched from the back, where nothing a caller supplies sits)
    const std::string probe = header_pack(1, is_signed8 && elem_size == 1, shape, pipename, 0);
    const std::string key = "\"bytes\": \"";
    const size_t at = probe.rfind(key);
    *prefix = probe.substr(0, at + key.size());
    *suffix = probe.substr(at + key.size() + 1);                                    // (behind the single digit "0")
    if (elem_size == 2) {
        // header_pack(1, ..) wrote the 8-bit type name; the 16-bit header differs in that word only
        const std::string t8 = "\"type\": \"uint8\"", t16 = "\"type\": \"uint16\"";
        const size_t tp = prefix->rfind(t8);
        if (tp != std::string::npos) prefix->replace(tp, t8.size(), t16);
    }
}

std::string header_pack(int elem_size, bool is_signed8, const std::vector<uint64_t>& shape, const std::string& pipename,
                        uint64_t payload_bytes)
{
    const char* type = elem_size == 2 ? "uint16" : (is_signed8 ? "int8" : "uint8");   // header_utils.hpp:19-34
    std::string j;
    j += "{\n    \"pipename\": \"";
    json_escape(pipename, j);
    j += "\",\n    \"raw\": {\n        \"type\": \"";
    j += type;
    j += "\",\n        \"rank\": \"" + std::to_string(shape.size()) + "\",\n        \"shape\": {\n";
    for (size_t i = 0; i < shape.size(); ++i) {
        j += "            \"dim\": \"" + std::to_string(shape[i]) + "\"";
        j += (i + 1 < shape.size()) ? ",\n" : "\n";
    }
    j += "        }\n    },\n    \"encoded\": {\n        \"bytes\": \"" + std::to_string(payload_bytes) + "\"\n    },\n";
    j += "    \"sqy\": {\n        \"version\": \"";
    j += kVersion;
    j += "\",\n        \"headref\": \"";
    j += kHeadRef;
    j += "\"\n    }\n}\n";
    j += kHeaderEnd;
    if (j.size() % (size_t)elem_size != 0) j.insert(0, (size_t)elem_size - j.size() % (size_t)elem_size, ' ');
    return j;
}

int HeaderInfo::elem_size() const
{
    if (type == "uint16" || type == "int16") return 2;
    if (type == "uint8" || type == "int8") return 1;
    if (type == "uint32" || type == "int32") return 4;
    if (type == "uint64" || type == "int64") return 8;
    return 0;
}

static bool read_json_string(const char*& p, const char* end, std::string& out)
{
    out.clear();
    if (p >= end || *p != '"') return false;
    ++p;
    while (p < end && *p != '"') {
        if (*p == '\\' && p + 1 < end) {
            ++p;
            switch (*p) {
                case 'n': out += '\n'; break; case 't': out += '\t'; break; case 'r': out += '\r'; break;
                case 'b': out += '\b'; break; case 'f': out += '\f'; break;
                case 'u':
                    if (p + 4 < end) { out += (char)std::strtol(std::string(p + 1, p + 5).c_str(), nullptr, 16); p += 4; }
                    break;
                default: out += *p;
            }
            ++p;
        } else {
            out += *p++;
        }
    }
    if (p >= end) return false;
    ++p;
    return true;
}

HeaderInfo header_unpack(const char* begin, const char* end)
{
    HeaderInfo h;
    const char* delim = std::search(begin, end, kHeaderEnd.begin(), kHeaderEnd.end());
    if (delim == end) return h;
    // sqeazy_header.hpp:520-531 (valid_header): balanced braces, more than one ':'
    if (std::count(begin, delim, '{') == 0 || std::count(begin, delim, '{') != std::count(begin, delim, '}')) return h;
    if (std::count(begin, delim, ':') <= 1) return h;
    const char* p = begin;
    std::string key, val;
    bool have_pipe = false, have_bytes = false;
    while (p < delim) {
        if (*p != '"') { ++p; continue; }
        if (!read_json_string(p, delim, key)) break;
        while (p < delim && (*p == ' ' || *p == '\t' || *p == '\n')) ++p;
        if (p >= delim || *p != ':') continue;
        ++p;
        while (p < delim && (*p == ' ' || *p == '\t' || *p == '\n')) ++p;
        if (p < delim && *p == '"') {
            if (!read_json_string(p, delim, val)) break;
            if (key == "pipename") { h.pipename = val; have_pipe = true; }
            else if (key == "type") h.type = val;
            else if (key == "dim") h.shape.push_back(std::strtoull(val.c_str(), nullptr, 10));
            else if (key == "bytes") { h.payload_bytes = std::strtoull(val.c_str(), nullptr, 10); have_bytes = true; }
        }
    }
    h.size = (uint64_t)(delim - begin) + kHeaderEnd.size();
    h.valid = have_pipe && have_bytes && !h.type.empty();
    return h;
}

// ---- quantiser LUT construction (host, float) ----
bool quantiser_parse_weighting(const std::string& text, QuantiserWeighting* out)
{
    QuantiserWeighting w;
    if (text.find("none") != std::string::npos) { *out = w; return true; }           // quantiser_scheme_impl.hpp:186
    if (text.rfind('_') == std::string::npos) return false;                          // extract_ratio :29-32 -> 0/0
    std::vector<long> ints;                                                          // regex_helpers.hpp:101-115, "[0-9]+"
    for (size_t i = 0; i < text.size();) {
        if (text[i] < '0' || text[i] > '9') { ++i; continue; }
        size_t j = i;
        long v = 0;
        while (j < text.size() && text[j] >= '0' && text[j] <= '9') {
            v = v * 10 + (text[j] - '0');
            if (v > INT32_MAX) return false;                                         // (std::stoi would throw)
            ++j;
        }
        ints.push_back(v);
        i = j;
    }
    if (ints.size() == 1) ints.push_back(1);
    if (ints.size() != 2 || ints[1] == 0) return false;
    w.mode = text.find("offset") != std::string::npos ? 2 : 1;                        // :189
    w.num = (int)ints[0];
    w.den = (int)ints[1];
    *out = w;
    return true;
}

bool quantiser_lut_to_file(const std::string& path, const uint16_t* lut, size_t n)
{
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    for (size_t i = 0; i < n; ++i) std::fprintf(f, "%u\n", (unsigned)lut[i]);
    return std::fclose(f) == 0;
}

// The path may come out of a blob's header, i.e. from untrusted input (decode): only a REGULAR file of at most 64 KiB is opened (a
// FIFO or a device would block the call or feed it without end), and it has to hold exactly n values that fit 16 bits -- a short
// or garbled file is an error here, where the reference decodes with whatever its stream extraction left in the table.
bool quantiser_lut_from_file(const std::string& path, uint16_t* lut, size_t n)
{
    for (size_t i = 0; i < n; ++i) lut[i] = 0;
    struct stat sb;
    if (::stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size > (64 << 10)) return false;
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) return false;
    unsigned long v = 0;
    size_t i = 0;
    bool ok = true;
    while (i < n && std::fscanf(f, "%lu", &v) == 1) {
        if (v > 65535ul) { ok = false; break; }
        lut[i++] = (uint16_t)v;
    }
    if (ok && i == n && std::fscanf(f, "%lu", &v) == 1) ok = false;          // more than n values
    std::fclose(f);
    return ok && i == n;
}

void quantiser_build_luts(const uint32_t* histo, size_t nbins, unsigned char* lut_encode, uint16_t* lut_decode,
                          const QuantiserWeighting& weighting)
{
    const size_t max_compressed = 256;                                     // quantiser<raw, char>::max_compressed_
    std::vector<float> importance(nbins);
    std::memset(lut_encode, 0, nbins);
    for (size_t i = 0; i < max_compressed; ++i) lut_decode[i] = 0;
    // computeWeights (quantiser_utils.hpp:317-322): the weights start out as 1.f (:85,104); power_of writes std::pow(i, e)
    // into every bin, offset_power_of std::pow(i - offset, e) from the first non-zero bin on (quantiser_weighters.hpp:40-84,
    // :121-136).  The index is an integer, so std::pow works in double and the result is narrowed to float.
    std::vector<float> weights(nbins, 1.f);
    if (weighting.mode != 0) {
        const float exponent = float(weighting.num) / weighting.den;
        size_t offset = 0;
        if (weighting.mode == 2) while (offset < nbins && !histo[offset]) ++offset;
        for (size_t i = offset; i < nbins; ++i) weights[i] = (float)std::pow((double)(long long)(i - offset), (double)exponent);
    }
    // computeImportance: importance = histo * weight
    for (size_t i = 0; i < nbins; ++i) importance[i] = histo[i] * weights[i];
    // std::accumulate(importance.begin(), importance.end(), 0.) -> double accumulator, assigned to float
    double total = 0.;
    for (size_t i = 0; i < nbins; ++i) total = total + importance[i];
    const float importanceSum = (float)total;
    if (!(importanceSum != 0)) return;
    uint32_t n_levels = 0;
    for (size_t i = 0; i < nbins; ++i) if (importance[i] != 0.f) ++n_levels;

    if (n_levels <= max_compressed) {
        // linear_mapping_quantisation
        uint32_t comp_idx = 0;
        for (uint32_t raw_idx = 0; raw_idx < nbins && comp_idx < max_compressed; ++raw_idx) {
            lut_encode[raw_idx] = (unsigned char)comp_idx;
            lut_decode[comp_idx] = (uint16_t)raw_idx;
            if (importance[raw_idx]) comp_idx++;
        }
        const uint16_t raw_max = nbins == 65536 ? 65535 : 255;
        if (comp_idx < max_compressed && comp_idx > 0 && lut_decode[comp_idx] == raw_max)
            for (size_t i = comp_idx; i < max_compressed; ++i) lut_decode[i] = lut_decode[comp_idx - 1];
        return;
    }
    // adaptive_lloyd_com
    size_t levels_available = max_compressed;
    float bucketSize = importanceSum / levels_available;
    float importanceIntegral = importance[0];
    float quantile_sum = importance[0];
    uint32_t comp_idx = 0;
    float weighted_mean_importance_in_bucket = 0 * importance[0];
    float index_weighted_mean_importance = 0;
    for (uint32_t raw_idx = 1; raw_idx < nbins; ++raw_idx) {
        if (quantile_sum >= bucketSize && (comp_idx < max_compressed - 1)) {
            lut_decode[comp_idx] = static_cast<uint16_t>(index_weighted_mean_importance);
            comp_idx++;
            levels_available--;
            quantile_sum = importance[raw_idx];
            weighted_mean_importance_in_bucket = raw_idx * importance[raw_idx];
            if (importanceIntegral < importanceSum) bucketSize = (importanceSum - importanceIntegral) / levels_available;
            if (quantile_sum != 0.) index_weighted_mean_importance = std::round(weighted_mean_importance_in_bucket / quantile_sum);
        } else {
            quantile_sum += importance[raw_idx];
            weighted_mean_importance_in_bucket += raw_idx * importance[raw_idx];
            if (quantile_sum != 0.) index_weighted_mean_importance = std::round(weighted_mean_importance_in_bucket / quantile_sum);
        }
        lut_encode[raw_idx] = static_cast<unsigned char>(comp_idx);
        importanceIntegral += importance[raw_idx];
    }
    lut_decode[comp_idx] = static_cast<uint16_t>(index_weighted_mean_importance);
}

bool zcurve_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X, uint64_t ts)
{
    if (Z == 0 || Y == 0 || X == 0) return false;
    if (ts < 2 || ts > 128 || (ts & (ts - 1))) return false;                  // zcurve_reorder_utils.hpp:30-67: other sizes get 1-bit Morton codes that leave the tile
    auto flog2 = [](uint64_t v) { int l = 0; while (v >>= 1) ++l; return l; };
    const uint64_t common = (uint64_t)1 << std::min(flog2(Z), std::min(flog2(Y), flog2(X)));   // :69-81 common_power_of_2
    const bool has_remainder = (Z % common) || (Y % common) || (X % common);                   // :83-94, :125-131
    if (!has_remainder && ((Z % ts) || (Y % ts) || (X % ts))) return false;                    // encode_full (:141-186) assumes whole tiles
    return true;
}

bool tile_shuffle_geometry_defined(uint64_t Z, uint64_t Y, uint64_t X, uint64_t ts)
{
    return ts > 0 && Z >= ts && Y >= ts && X >= ts && Z % ts == 0 && Y % ts == 0 && X % ts == 0;
}

void tile_shuffle_order(const float* sums, size_t ntiles, size_t per_tile, int elem_size, uint64_t* decode_map, bool signed_char)
{
    // tile_shuffle_utils.hpp:176-219: std::vector<in_value_t> metric; metric[i] = sum / n_elements_per_tile (float -> voxel type).
    // signed_char: the tail filter form, tile_shuffle_scheme<char> -- the metric is a (signed) char and sorts as one
    std::vector<int32_t> metric(ntiles);
    for (size_t i = 0; i < ntiles; ++i) {
        const float m = sums[i] / per_tile;
        metric[i] = signed_char ? (int32_t)(int8_t)m : elem_size == 2 ? (int32_t)(uint16_t)m : (int32_t)(uint8_t)m;
    }
    std::vector<int32_t> sorted_metric = metric;
    std::sort(sorted_metric.begin(), sorted_metric.end());
    // std::find(metric, sorted[i]) for every i = the first tile with that metric
    std::map<int32_t, uint64_t> first;
    for (size_t i = ntiles; i-- > 0;) first[metric[i]] = i;
    for (size_t i = 0; i < ntiles; ++i) decode_map[i] = first[sorted_metric[i]];
}

uint64_t bitshuffle_block_elems(int elem_size, uint64_t block_size)
{
    if (block_size == 0) {
        // bshuf_default_block_size (kiyo-masui/bitshuffle, bitshuffle_core.c): "needs to be absolutely stable between versions"
        uint64_t b = 8192 / (uint64_t)elem_size;
        b = (b / 8) * 8;
        return b < 128 ? 128 : b;
    }
    return block_size % 8 ? 0 : block_size;
}

void frame_shuffle_order(const float* sums, size_t Z, size_t per_frame, uint64_t* decode_map)
{
    std::vector<float> metric(Z);
    for (size_t z = 0; z < Z; ++z) metric[z] = sums[z] / per_frame;          // float / size_t
    // The reference sorts the metrics and looks every sorted value up with std::find (frame_shuffle_utils.hpp:138-161): slot i gets
    // the FIRST frame whose metric equals the i-th smallest.  The same map in Z log Z instead of Z^2 compares (0.3 ms of host time per
    // call at 1024 frames): a stable argsort puts the frames of equal metric in index order, every slot of such a run takes the run's
    // first frame.
    std::vector<uint32_t> idx(Z);
    for (size_t z = 0; z < Z; ++z) idx[z] = (uint32_t)z;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return metric[a] < metric[b]; });
    uint32_t first = 0;
    for (size_t i = 0; i < Z; ++i) {
        if (i == 0 || !(metric[idx[i]] == metric[idx[i - 1]])) first = idx[i];
        decode_map[i] = first;
    }
}

// ---- base64 (base64.hpp:135-162: standard alphabet, '=' padded) ----
std::string base64_encode(const unsigned char* src, size_t n)
{
    static const char tbl[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    std::string o;
    o.reserve(4 * ((n + 2) / 3));
    size_t i = 0;
    for (; i + 2 < n; i += 3) {
        const unsigned v = ((unsigned)src[i] << 16) | ((unsigned)src[i + 1] << 8) | src[i + 2];
        o += tbl[(v >> 18) & 63]; o += tbl[(v >> 12) & 63]; o += tbl[(v >> 6) & 63]; o += tbl[v & 63];
    }
    if (n - i == 1) {
        const unsigned v = (unsigned)src[i] << 16;
        o += tbl[(v >> 18) & 63]; o += tbl[(v >> 12) & 63]; o += "==";
    } else if (n - i == 2) {
        const unsigned v = ((unsigned)src[i] << 16) | ((unsigned)src[i + 1] << 8);
        o += tbl[(v >> 18) & 63]; o += tbl[(v >> 12) & 63]; o += tbl[(v >> 6) & 63]; o += '=';
    }
    return o;
}

std::vector<unsigned char> base64_decode(const std::string& s)
{
    std::vector<unsigned char> out;
    unsigned acc = 0;
    int bits = 0;
    for (char ch : s) {
        int v;
        if (ch >= 'A' && ch <= 'Z') v = ch - 'A';
        else if (ch >= 'a' && ch <= 'z') v = ch - 'a' + 26;
        else if (ch >= '0' && ch <= '9') v = ch - '0' + 52;
        else if (ch == '+') v = 62;
        else if (ch == '/') v = 63;
        else continue;
        acc = (acc << 6) | (unsigned)v;
        bits += 6;
        if (bits >= 8) { bits -= 8; out.push_back((unsigned char)((acc >> bits) & 0xff)); }
    }
    return out;
}

std::string to_verbatim(const void* data, size_t bytes)
{
    if (!bytes) return "";
    return kVerbOpen + base64_encode(static_cast<const unsigned char*>(data), bytes) + kVerbClose;   // string_parsers.hpp:507-534
}

bool from_verbatim(const std::string& v, std::vector<unsigned char>* out)
{
    if (v.size() < 21) return false;
    *out = base64_decode(v.substr(10, v.size() - 21));
    return true;
}

// ---- xxh32 (LZ4 frame descriptor checksum) ----
static inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
static inline uint32_t rd32(const unsigned char* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

uint32_t xxh32(const unsigned char* p, size_t len, uint32_t seed)
{
    const uint32_t P1 = 2654435761U, P2 = 2246822519U, P3 = 3266489917U, P4 = 668265263U, P5 = 374761393U;
    const unsigned char* const end = p + len;
    uint32_t h;
    if (len >= 16) {
        const unsigned char* const limit = end - 16;
        uint32_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
        do {
            v1 = rotl32(v1 + rd32(p) * P2, 13) * P1; p += 4;
            v2 = rotl32(v2 + rd32(p) * P2, 13) * P1; p += 4;
            v3 = rotl32(v3 + rd32(p) * P2, 13) * P1; p += 4;
            v4 = rotl32(v4 + rd32(p) * P2, 13) * P1; p += 4;
        } while (p <= limit);
        h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
    } else {
        h = seed + P5;
    }
    h += (uint32_t)len;
    while (p + 4 <= end) { h = rotl32(h + rd32(p) * P3, 17) * P4; p += 4; }
    while (p < end) { h = rotl32(h + (*p) * P5, 11) * P1; p++; }
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

} // namespace sqy
