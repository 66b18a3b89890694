// entries_math.h — the index arithmetic of the kept-order front end (entries_kernels.hip), shared by the device kernel and
// a g++ build (tests/cpp/entries_tool.cpp, which runs a serial model of the kernel's tiles over it), like particle_math.h.
//
// A frame whose bgs_view names a chunk of sorted entries draws that chunk as it is: the front end only drops the entries
// that cannot be drawn (entry_kept) and keeps the order of the rest. The chunk is cut into TILES of ENTRIES_TILE slots; a
// tile is 256 threads x ENTRIES_ITEMS items, thread `tid` holding slot item * 256 + tid of its tile, so that the 64 lanes
// of a wave hold 64 CONSECUTIVE slots for every item: a ROW. Rows in (item, wave) order are the tile's slots in list order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BGS_ENTRIES_HD __host__ __device__ __forceinline__
#else
#define BGS_ENTRIES_HD static inline
#endif

namespace bgs {

constexpr uint32_t ENTRIES_THREADS = 256, ENTRIES_WAVES = ENTRIES_THREADS / 64, ENTRIES_ITEMS = 8;
constexpr uint32_t ENTRIES_TILE = ENTRIES_THREADS * ENTRIES_ITEMS;   // 2048 slots: one chain word each, as many as keygen's chain has
constexpr uint32_t ENTRIES_ROWS = ENTRIES_ITEMS * ENTRIES_WAVES;     // 32 rows of 64 slots
// Workgroups of one launch at most. A launch with fewer workgroups than tiles hands the tiles out by ticket, every
// workgroup taking another one when it is done: ONE SWEEP of the grid covers ENTRIES_SWEEP slots, a longer chunk makes
// workgroups come back for a second tile.
constexpr uint32_t ENTRIES_GRID_MAX = 256;
constexpr uint32_t ENTRIES_SWEEP = ENTRIES_GRID_MAX * ENTRIES_TILE;  // 524288

// what reaches the vertex stage: not the culled sentinel (src/render/gaussian.wgsl:191-195), and a splat that exists
BGS_ENTRIES_HD bool entry_kept(uint32_t key, uint32_t index, uint32_t n) { return key != 0xFFFFFFFFu && index < n; }
// the index a SKIPPED entry is parked with (the list's tail, read by RasterizeMode::Depth only): never out of range
BGS_ENTRIES_HD uint32_t entry_parked_index(uint32_t index, uint32_t n) { return index < n ? index : n - 1u; }

BGS_ENTRIES_HD uint32_t entries_tiles(uint32_t n) { return n / ENTRIES_TILE + (n % ENTRIES_TILE ? 1u : 0u); }
BGS_ENTRIES_HD uint32_t entries_blocks(uint32_t n) { const uint32_t t = entries_tiles(n); return t < ENTRIES_GRID_MAX ? t : ENTRIES_GRID_MAX; }
// slot (position in the chunk) of thread tid's item; 64-bit: tile * ENTRIES_TILE passes 2^32 only past the last tile
BGS_ENTRIES_HD uint64_t entries_slot(uint32_t tile, uint32_t item, uint32_t tid) {
    return (uint64_t)tile * ENTRIES_TILE + (uint64_t)item * ENTRIES_THREADS + tid;
}
BGS_ENTRIES_HD uint32_t entries_row(uint32_t item, uint32_t wave) { return item * ENTRIES_WAVES + wave; }
// where a slot's entry goes: kept ones to draw_list[kept entries before it], skipped ones to tail[skipped entries before it]
BGS_ENTRIES_HD uint32_t entries_kept_dst(uint32_t tile_excl, uint32_t row_excl, uint32_t below) { return tile_excl + row_excl + below; }
BGS_ENTRIES_HD uint32_t entries_skipped_dst(uint64_t slot, uint32_t kept_before) { return (uint32_t)(slot - kept_before); }

}  // namespace bgs
