// entries_tool — a serial model of the kept-order compaction (csrc/entries_kernels.hip) over the kernel's own index
// arithmetic (csrc/entries_math.h), for the host tests and for a sanitizer build (a stand-alone program: no GPU, no Python).
//   entries_tool constants                      THREADS ITEMS TILE ROWS GRID_MAX SWEEP
//   entries_tool compact <in.bin> <n> <out.bin> <tail.bin>
//       <in.bin>: n (key, index) records; writes the kept entries in order to <out.bin>, the skipped ones (their index
//       parked in range) to <tail.bin>, and prints "draw_count tiles blocks". Every buffer is allocated at exactly n
//       records, as the lane's are, so an index the arithmetic gets wrong is an out-of-bounds access the sanitizer sees.
//   entries_tool selftest                       the sizes of the GPU test on generated lists against a plain filter
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../bevy_gaussian_splatting_amd/csrc/entries_math.h"

namespace {

struct Entry { uint32_t key, index; };

// The kernel tile by tile and row by row: ballots become per-row counts, the row scan and the chain become running sums.
uint32_t compact(const std::vector<Entry>& in, uint32_t n, std::vector<Entry>& out, std::vector<Entry>& tail) {
    using namespace bgs;
    uint32_t tile_excl = 0;   // what the chained scan hands a tile: kept entries of the tiles before it
    for (uint32_t tile = 0; tile < entries_tiles(n); ++tile) {
        uint32_t cnt[ENTRIES_ROWS] = {}, off[ENTRIES_ROWS] = {};
        for (uint32_t k = 0; k < ENTRIES_ITEMS; ++k)
            for (uint32_t tid = 0; tid < ENTRIES_THREADS; ++tid) {
                const uint64_t slot = entries_slot(tile, k, tid);
                if (slot < n && entry_kept(in[slot].key, in[slot].index, n)) cnt[entries_row(k, tid / 64u)] += 1u;
            }
        uint32_t total = 0;
        for (uint32_t r = 0; r < ENTRIES_ROWS; ++r) { off[r] = total; total += cnt[r]; }
        for (uint32_t k = 0; k < ENTRIES_ITEMS; ++k)
            for (uint32_t wave = 0; wave < ENTRIES_WAVES; ++wave) {
                uint32_t below = 0;   // popcount(ballot & lanes_below)
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint64_t slot = entries_slot(tile, k, wave * 64u + lane);
                    if (slot >= n) continue;
                    const Entry e = in[slot];
                    const uint32_t before = entries_kept_dst(tile_excl, off[entries_row(k, wave)], below);
                    if (entry_kept(e.key, e.index, n)) { out.at(before) = e; below += 1u; }
                    else tail.at(entries_skipped_dst(slot, before)) = Entry{e.key, entry_parked_index(e.index, n)};
                }
            }
        tile_excl += total;
    }
    return tile_excl;
}

std::vector<Entry> generated(uint32_t n, int pattern) {
    std::vector<Entry> e(n);
    uint64_t x = 0x9E3779B97F4A7C15ull * (n + 1u);
    for (uint32_t i = 0; i < n; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        e[i] = Entry{(uint32_t)(x >> 32) & 0x7FFFFFFFu, (uint32_t)x % n};
        if (pattern == 1 && i % 4u == 0u) e[i].key = 0xFFFFFFFFu;
        if (pattern == 1 && i % 4u == 2u) e[i].index = n + i % 5u;
        if (pattern == 2 && i + 1u < n) e[i].key = 0xFFFFFFFFu;
    }
    return e;
}

}  // namespace

int main(int argc, char** argv) {
    using namespace bgs;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "constants") {
        std::printf("%u %u %u %u %u %u\n", ENTRIES_THREADS, ENTRIES_ITEMS, ENTRIES_TILE, ENTRIES_ROWS, ENTRIES_GRID_MAX, ENTRIES_SWEEP);
        return 0;
    }
    if (cmd == "compact" && argc == 6) {
        const uint32_t n = (uint32_t)std::stoul(argv[3]);
        std::vector<Entry> in(n), out(n), tail(n);
        std::ifstream f(argv[2], std::ios::binary);
        f.read((char*)in.data(), (std::streamsize)n * 8);
        if (!f && n) { std::fprintf(stderr, "entries_tool: cannot read %s\n", argv[2]); return 1; }
        const uint32_t d = compact(in, n, out, tail);
        std::ofstream(argv[4], std::ios::binary).write((const char*)out.data(), (std::streamsize)d * 8);
        std::ofstream(argv[5], std::ios::binary).write((const char*)tail.data(), (std::streamsize)(n - d) * 8);
        std::printf("%u %u %u\n", d, entries_tiles(n), entries_blocks(n));
        return 0;
    }
    if (cmd == "selftest") {
        for (uint32_t n : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 2047u, 2048u, 2049u, 4097u, ENTRIES_SWEEP + 1u})
            for (int pattern = 0; pattern < 3; ++pattern) {
                const std::vector<Entry> in = generated(n, pattern);
                std::vector<Entry> out(n), tail(n), want, want_tail;
                for (const Entry& e : in) {
                    if (e.key != 0xFFFFFFFFu && e.index < n) want.push_back(e);
                    else want_tail.push_back(Entry{e.key, e.index < n ? e.index : n - 1u});
                }
                const uint32_t d = compact(in, n, out, tail);
                auto same = [](const std::vector<Entry>& got, const std::vector<Entry>& ref) {   // the first ref.size() records
                    for (size_t i = 0; i < ref.size(); ++i)
                        if (got[i].key != ref[i].key || got[i].index != ref[i].index) return false;
                    return true;
                };
                if (d != want.size() || !same(out, want) || !same(tail, want_tail)) {
                    std::fprintf(stderr, "entries_tool: n = %u pattern %d differs\n", n, pattern);
                    return 1;
                }
            }
        std::printf("ok\n");
        return 0;
    }
    std::fprintf(stderr, "usage: entries_tool constants | compact <in> <n> <out> <tail> | selftest\n");
    return 2;
}
