// Who empties the duplicate search's table (csrc/sqy_pipeline.cpp: lz4_table_clear_plan) and where the transposer's stores of that clear
// land (sqy_pipeline.hpp: lz4_table_clear_stores / lz4_table_clear_dword, the functions the kernel itself calls): for every table that
// lz4_dedupe_layout lays out and every grid, the stores write each byte of [tab_key_at, tab_val_at + 4 table) once, keys 0 and values ~0,
// and no byte outside.  tests/test_host_table_clear.py builds and runs this with g++, sanitizers on.  Prints "table_clear ok", returns 0.
#include "../../sqeazy_amd/csrc/sqy_pipeline.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using sqy::Lz4DedupeLayout;
using sqy::Lz4TableClearPlan;

namespace {
// the kernel's clear with `threads` threads in all (grid x block), on a host copy of the workspace; false: a store left the table, was
// not where a 16-byte (8-byte: head and tail) store may go, or hit a byte twice
bool run_clear(std::vector<uint8_t>& ws, std::vector<uint8_t>& hits, uint64_t base_addr, const Lz4TableClearPlan& p, uint64_t threads)
{
    const uint64_t addr = base_addr + p.table_at;
    const sqy::Lz4TableClearStores st = sqy::lz4_table_clear_stores(addr, p.bytes);
    auto store = [&](uint64_t off, uint32_t n, const uint32_t* words) {
        if (off + n > p.bytes || (addr + off) % n != 0) return false;
        for (uint32_t b = 0; b < n; ++b) if (hits[p.table_at + off + b]++) return false;
        std::memcpy(&ws[p.table_at + off], words, n);
        return true;
    };
    for (uint64_t t = 0; t < threads; ++t)
        for (uint64_t i = t; i < st.nvec; i += threads) {
            const uint32_t off = st.head + ((uint32_t)i << 4);
            const uint32_t w[4] = {sqy::lz4_table_clear_dword(off, p.key_bytes), sqy::lz4_table_clear_dword(off + 4, p.key_bytes),
                                   sqy::lz4_table_clear_dword(off + 8, p.key_bytes), sqy::lz4_table_clear_dword(off + 12, p.key_bytes)};
            if (!store(off, 16, w)) return false;
        }
    const uint32_t zero[2] = {0u, 0u}, ones[2] = {~0u, ~0u};
    if (st.head && !store(0, st.head, zero)) return false;
    if (st.tail_at < p.bytes && !store(st.tail_at, p.bytes - st.tail_at, ones)) return false;
    return true;
}
}

int main()
{
    // who clears
    sqy::Lz4EncodeLayout lay;
    lay.chunk = 4096; lay.nchunks = 7;
    const Lz4DedupeLayout none, seven = sqy::lz4_dedupe_layout(lay, 7 * 4 * 4);
    CHECK(seven.total && seven.table == 64);
    CHECK(sqy::lz4_table_clear_plan(none, true, true).who == Lz4TableClearPlan::fills);
    CHECK(sqy::lz4_table_clear_plan(seven, false, true).who == Lz4TableClearPlan::fills && sqy::lz4_table_clear_plan(seven, false, false).who == Lz4TableClearPlan::fills);
    CHECK(sqy::lz4_table_clear_plan(seven, true, false).who == Lz4TableClearPlan::kernel && sqy::lz4_table_clear_plan(seven, true, false).bytes == 0);
    const Lz4TableClearPlan t7 = sqy::lz4_table_clear_plan(seven, true, true);
    CHECK(t7.who == Lz4TableClearPlan::transposer && t7.table_at == seven.tab_key_at && t7.key_bytes == 512 && t7.bytes == 768);
    {   // a table the stores do not fit stays with the kernel: values not right behind the keys, a table off 8 bytes, more than 2^32 bytes
        Lz4DedupeLayout d = seven;
        d.tab_val_at += 8;
        CHECK(sqy::lz4_table_clear_plan(d, true, true).who == Lz4TableClearPlan::kernel);
        d = seven; d.tab_key_at += 4; d.tab_val_at += 4;
        CHECK(sqy::lz4_table_clear_plan(d, true, true).who == Lz4TableClearPlan::kernel);
        d = seven; d.table = 1ull << 29; d.tab_val_at = d.tab_key_at + d.table * 8;
        CHECK(sqy::lz4_table_clear_plan(d, true, true).who == Lz4TableClearPlan::kernel);
    }
    // where the stores land: every chunk count 2 .. 300 (odd counts put the table 8 bytes off a 16-byte boundary) and a large one, every
    // thread count from one workgroup's 128 to more threads than vectors, and a lone thread
    uint64_t checked = 0;
    std::vector<uint64_t> counts;
    for (uint64_t n = 2; n <= 300; ++n) counts.push_back(n);
    counts.push_back(4096); counts.push_back(4097); counts.push_back(65535);
    for (uint64_t nchunks : counts) {
        lay.nchunks = nchunks;
        const Lz4DedupeLayout d = sqy::lz4_dedupe_layout(lay, nchunks * 4 * 4);
        const Lz4TableClearPlan p = sqy::lz4_table_clear_plan(d, true, true);
        CHECK(p.who == Lz4TableClearPlan::transposer && p.table_at == d.tab_key_at && p.key_bytes == d.table * 8 && p.bytes == d.table * 12);
        CHECK(p.table_at + p.bytes == d.tab_val_at + d.table * 4 && p.table_at + p.bytes <= d.dup_at);
        for (uint64_t threads : {(uint64_t)1, (uint64_t)128, (uint64_t)256, (uint64_t)128 * 33, (uint64_t)128 * 32768}) {
            if (threads == 1 && nchunks > 300) continue;
            std::vector<uint8_t> ws(d.total, 0x5a), hits(d.total, 0);
            CHECK(run_clear(ws, hits, 0x7f0000001000ull, p, threads));            // (the workspace: 256-byte aligned device memory)
            for (uint64_t b = 0; b < d.total; ++b) {
                const bool key = b >= d.tab_key_at && b < d.tab_val_at, val = b >= d.tab_val_at && b < d.tab_val_at + d.table * 4;
                CHECK(hits[b] == (key || val ? 1 : 0));
                CHECK(ws[b] == (key ? 0x00 : val ? 0xff : 0x5a));
            }
            ++checked;
        }
    }
    std::printf("table_clear ok (%llu tables x grids)\n", (unsigned long long)checked);
    return 0;
}
