// entries_kernels.hip — the front end of a KEPT-ORDER frame (bgs_view.entries_device_ptr): instead of keygen + depth sort,
// one order-preserving compaction of the caller's sorted entries into the lane's draw list.
//
// The reference sorts only when its SortTrigger fires (src/sort/mod.rs:153-194) and draws every other frame from the
// camera's chunk of SortedEntries as the last sort left it; vs_points skips entry.key == 0xFFFFFFFF
// (src/render/gaussian.wgsl:191-195) and WebGPU's robustness rules take care of an index past the cloud. Here the vertex
// stage walks a dense draw list of ctl->draw_count ranks, so the entries that cannot be drawn (entry_kept, entries_math.h)
// are dropped first, the order of the others kept. Every test that depends on the CURRENT camera stays in the vertex stage.
//
// The kernel leaves the lane exactly as keygen leaves it for a frame without digit places (SortMode::None):
//   ctl->draw_count, ctl->splat_count       set by the workgroup of the last tile
//   *fp_out = fp                            the frame's parameters for the kernels behind it (they take them by pointer)
//   *zero_word = 0                          the heavy-tile list's count, if the frame has one
//   part_status[0 .. ceil(n / 2048))        the chain's words, which the rasteriser's clean-up zeroes for ceil(n / KEYGEN_TILE)
//   ctl->ticket[ticket_slot][0]             the tile counter (the Control block is zeroed as a whole)
// Both are zero when the kernel starts, launched directly or replayed from a captured frame graph (EntriesLaunch,
// kernels.h), because a BINNING_SCAN frame's LAST kernel re-zeroes them and that kernel is a node of the same graph: the
// frame's own rasteriser zeroes part_status[0 .. ceil(fp.n / KEYGEN_TILE)) — KEYGEN_TILE == ENTRIES_TILE, fp.n read from
// the parameters this kernel left —, and the rasteriser of the lane's PREVIOUS frame zeroed this frame's Control block
// (FrameCleanup::other_ctl; the lane's frames alternate between two blocks and run in stream order). A lane whose
// scratch is not known to be clean (Lane::scratch_clean) gets a memset and a direct launch, never a replay.
//
// GEOMETRY (entries_math.h). A tile is ENTRIES_TILE = 2048 slots = 256 threads x 8 items; a wave's 64 lanes hold 64
// consecutive slots per item (a row), loaded and stored as 8-byte words: coalesced 512-byte rows. Inside a row the rank
// of a kept entry is popcount(ballot & lanes_below) (wave64); one wave scans the tile's 32 row counts; ACROSS tiles the
// exclusive count comes from the chained scan of lookback.h, one chain per workgroup walked by one whole wave — the
// scheme and the code path of keygen_kernel's ordered tiles (sort_kernels.hip), bounded by the same spin watchdog
// (ctl->error, code 8: BGS_EINTERNAL when the frame completes). Why the chain cannot wait for ever: tiles are handed out
// by an atomic ticket, so every predecessor of a tile is owned by a workgroup that has STARTED; a workgroup publishes its
// tile's aggregate before it looks back and waits for nothing else, so the tile with the smallest unpublished ticket
// always makes progress. Nothing behind this kernel spins on it: the vertex stage starts when the launch has ended.
// At most ENTRIES_GRID_MAX = 256 workgroups are launched: ONE SWEEP of the grid covers ENTRIES_SWEEP = 524288 slots, a
// longer chunk makes workgroups take a second ticket (a grid that covers every tile takes one ticket per workgroup and
// leaves, like keygen's).
// BOUNDS: slots >= n are never loaded or stored; kept entries go to draw_list[< number of kept entries <= n], skipped ones
// (TAIL only) to tail[< number of skipped entries <= n]; both buffers hold n records (ensure_entries).
#include <hip/hip_runtime.h>

#include "entries_math.h"
#include "kernels.h"
#include "lookback.h"

namespace bgs {

static_assert(ENTRIES_TILE == KEYGEN_TILE, "the rasteriser's clean-up zeroes one chain word per KEYGEN_TILE splats");

namespace {

__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

}  // namespace

// TAIL: the skipped entries are written too, in list order, to `tail` (RasterizeMode::Depth reads entries 1 and n - 1 of
// [drawn] ++ [skipped]: frame_color_inputs, render_kernels.hip), their index made safe to dereference (entry_parked_index).
template <bool TAIL>
__global__ __launch_bounds__(ENTRIES_THREADS) void entries_compact_kernel(FrameParams fp, const uint2* __restrict__ entries,
                                                                           uint2* __restrict__ draw_list, uint2* __restrict__ tail,
                                                                           Control* ctl, uint32_t* part_status, uint32_t ticket_slot,
                                                                           FrameParams* fp_out, uint32_t* zero_word) {
    __shared__ uint32_t s_cnt[ENTRIES_ROWS];   // kept entries of each row ...
    __shared__ uint32_t s_off[ENTRIES_ROWS];   // ... and of the rows before it
    __shared__ uint32_t s_base, s_tile;
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = tid >> 6;
    // the frame's first kernel leaves its parameters in device memory for the kernels behind it (as keygen does)
    if (fp_out && blockIdx.x == 0 && tid < (uint32_t)(sizeof(FrameParams) / 4u))
        reinterpret_cast<uint32_t*>(fp_out)[tid] = reinterpret_cast<const uint32_t*>(&fp)[tid];
    if (zero_word && blockIdx.x == 0 && tid == 0) *zero_word = 0u;
    const uint32_t n = fp.n;
    const uint32_t num_tiles = entries_tiles(n);
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const bool single_shot = gridDim.x >= num_tiles;

    for (;;) {
        if (tid == 0) s_tile = atomicAdd(&ctl->ticket[ticket_slot][0], 1u);
        __syncthreads();
        const uint32_t tile = s_tile;
        if (tile >= num_tiles) break;
        uint2 e[ENTRIES_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < ENTRIES_ITEMS; ++k) {
            const uint64_t slot = entries_slot(tile, k, tid);
            e[k] = slot < n ? entries[slot] : make_uint2(0xFFFFFFFFu, 0u);   // (past the chunk: never kept, never stored)
        }
        uint32_t below[ENTRIES_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < ENTRIES_ITEMS; ++k) {
            const bool keep = entries_slot(tile, k, tid) < n && entry_kept(e[k].x, e[k].y, n);
            const unsigned long long b = __ballot(keep);
            below[k] = (uint32_t)__popcll(b & lanes_below);
            if (lane == 0) s_cnt[entries_row(k, wave)] = (uint32_t)__popcll(b);
        }
        __syncthreads();
        if (wave == 0) {
            // one wave: exclusive scan of the 32 row counts, then the tile's place in the chunk from the chain
            const uint32_t c = (uint32_t)lane < ENTRIES_ROWS ? s_cnt[lane] : 0u;
            const uint32_t inc = wave_inclusive_scan_u32(c, lane);
            if ((uint32_t)lane < ENTRIES_ROWS) s_off[lane] = inc - c;
            const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
            uint32_t* const my_status = part_status + tile;
            uint32_t excl = 0u;
            if (tile > 0u) {
                if (lane == 0) __hip_atomic_store(my_status, STATUS_AGGREGATE | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                excl = lookback_wave(part_status, tile, lane, &ctl->error, 8u);
            }
            if (lane == 0) {
                __hip_atomic_store(my_status, STATUS_PREFIX | ((excl + total) & STATUS_VALUE_MASK), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_base = excl;
                if (tile == num_tiles - 1u) {
                    ctl->draw_count = excl + total;
                    ctl->splat_count = n;
                }
            }
        }
        __syncthreads();
        const uint32_t tile_excl = s_base;
#pragma unroll
        for (uint32_t k = 0; k < ENTRIES_ITEMS; ++k) {
            const uint64_t slot = entries_slot(tile, k, tid);
            if (slot < n) {
                const uint32_t before = entries_kept_dst(tile_excl, s_off[entries_row(k, wave)], below[k]);   // kept entries before this slot
                if (entry_kept(e[k].x, e[k].y, n)) draw_list[before] = e[k];
                else if constexpr (TAIL) tail[entries_skipped_dst(slot, before)] = make_uint2(e[k].x, entry_parked_index(e[k].y, n));
            }
        }
        if (single_shot) break;
        __syncthreads();   // s_tile, s_cnt, s_off and s_base are read above: the next ticket overwrites them
    }
}

bool EntriesLaunch::prepare(uint32_t max_blocks) {
    if (fp.n == 0) return false;
    func = tail ? reinterpret_cast<const void*>(&entries_compact_kernel<true>) : reinterpret_cast<const void*>(&entries_compact_kernel<false>);
    blocks = entries_blocks(fp.n);
    if (max_blocks && blocks > max_blocks) blocks = max_blocks;
    threads = ENTRIES_THREADS;
    per_tile = ENTRIES_TILE;
    argv[0] = &fp; argv[1] = &entries; argv[2] = &draw_list; argv[3] = &tail; argv[4] = &ctl;
    argv[5] = &part_status; argv[6] = &ticket_slot; argv[7] = &fp_out; argv[8] = &zero_word;
    return true;
}

hipError_t EntriesLaunch::launch(hipStream_t stream) {
    return hipLaunchKernel(func, dim3(blocks), dim3(threads), argv, 0, stream);
}

hipError_t EntriesLaunch::update_node(hipGraphExec_t exec, hipGraphNode_t node) {
    hipKernelNodeParams np{};
    np.func = const_cast<void*>(func);
    np.gridDim = dim3(blocks);
    np.blockDim = dim3(threads);
    np.sharedMemBytes = 0;
    np.kernelParams = argv;
    np.extra = nullptr;
    return hipGraphExecKernelNodeSetParams(exec, node, &np);
}

}  // namespace bgs
