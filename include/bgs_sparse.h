/* bgs_sparse.h — sparse-splat selection on the device: the C ABI of libbgs_sparse.so.
 *
 * The reference's third query (src/query/sparse.rs): SparseSelect { radius: 0.05, neighbor_threshold: 3 } selects every
 * splat that has fewer than neighbor_threshold splats within radius of it, itself included — the floaters of a trained
 * asset; inverted, it drops them. Like libbgs_query this is a separate small library. It links the HIP runtime only, not
 * libbgs and not libbgs_query, and declares nothing of their headers. It works on device memory the caller owns:
 *   - points:  n x 4 floats in the `position_visibility` layout (x, y, z read; the fourth lane ignored), 16-byte aligned;
 *   - counts:  n x uint32, written;
 *   - entries: a chunk of `bgs_sort_entry` { uint32 key; uint32 index; } as bgs_view.entries_device_ptr names one.
 * bgs_device_alloc / bgs_upload / bgs_download serve such memory.
 *
 * What is computed: counts[i] = the number of points j in [0, n), i included, with
 *   ((0 + dx*dx) + dy*dy) + dz*dz < radius*radius     (f32, every operation rounded once, strict)
 * clamped to `cap` when cap != 0. The arithmetic contract, with the line of it that is not pinned to the kd-tree crate's
 * source, is bevy_gaussian_splatting_amd/csrc_sparse/sparse_math.h. A point with a NaN or infinite lane has count 0 and
 * is counted by nobody. A uniform grid finds the candidates; the counts are those of all n x n pairs for every input.
 *
 * ORDERING. bgss_neighbor_counts and bgss_entries_keep only ENQUEUE on the stream they are given: they never block, and
 * they touch no other stream. What they read must be complete on that stream (or earlier), and what they write is
 * complete once the stream reaches that point. A grid's scratch belongs to the call that was enqueued last: use one grid
 * on one stream at a time. With libbgs the rule a host follows is:
 *   1. bgs_sort(ctx, cloud, &view, &settings, ..) with view.entries_device_ptr = the chunk   (blocking: the chunk is written)
 *   2. bgss_neighbor_counts / bgss_entries_keep on bgs_stream(ctx)
 *   3. bgs_synchronize(ctx)
 *   4. bgs_render(ctx, ..) with the chunk: an entry whose key is 0xFFFFFFFF is skipped wherever it stands.
 * The chunk must stay unwritten while frames in flight read it (the existing rule of bgs_view.entries_device_ptr), so a
 * host with async frames completes them (bgs_synchronize) before step 2 as well.
 *
 * bgss_grid_create and bgss_grid_free block (device allocation); they may be called while frames are in flight.
 * Not thread-safe per grid. Status codes mirror bgs_status. */
#ifndef BGS_SPARSE_H
#define BGS_SPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGSS_VERSION_MAJOR 0
#define BGSS_VERSION_MINOR 1

#define BGSS_OK 0
#define BGSS_EINVAL (-1) /* bad argument; bgss_last_error() names it */
#define BGSS_ENOMEM (-2) /* host or device allocation failed */
#define BGSS_EHIP (-3)   /* a HIP call failed, or no usable device */

#define BGSS_KEEP_SPARSE 0u /* the reference's selection: keep the splats with fewer than neighbor_threshold neighbours */
#define BGSS_KEEP_DENSE 1u  /* its Select::invert: the floaters are removed */

typedef struct bgss_grid bgss_grid; /* the scratch of the counting stages, on one device */

/* (major << 16) | minor */
uint32_t bgss_version(void);
/* Message of the calling thread's last failed call; "" if none. Valid until that thread's next call. */
const char* bgss_last_error(void);

/* Allocates, once, everything the counting stages need for clouds of up to max_points: the table of cells, the cursor,
 * the scattered points and their indices (20 bytes a point), and a table of 8-byte slots, between 2 and 4 a point, at
 * least 64 and at most 2^26 of them. Nothing is allocated per call. max_points == 0 is legal: such a grid serves n == 0. */
int bgss_grid_create(int hip_device, uint32_t max_points, bgss_grid** out);
void bgss_grid_free(bgss_grid* grid); /* NULL is fine */
uint32_t bgss_grid_capacity(const bgss_grid* grid);

/* counts[i], i < n, as above. cap == 0 counts everything; with cap != 0 a point stops looking once it has found cap
 * neighbours, which is what a selection with neighbor_threshold <= cap needs and costs far less in dense clouds.
 * BGSS_EINVAL names the offender: a radius that is not finite, not positive, or whose square is 0 or infinite in f32;
 * with n > 0 a NULL or misaligned pointer (16 bytes for points, 4 for counts); a NULL grid; n above the grid's capacity.
 * n == 0 enqueues nothing. */
int bgss_neighbor_counts(bgss_grid* grid, void* hip_stream, const void* points_device_ptr, uint32_t n, float radius, uint32_t cap,
                         void* counts_device_ptr);

/* For every entry with index < n and key != 0xFFFFFFFF: key becomes 0xFFFFFFFF unless counts[index] < neighbor_threshold
 * — with BGSS_KEEP_DENSE, unless it is not. Everything else is left as it is; index is never written. hip_device is the
 * device the memory and the stream live on. Any other flag, or entries that are not 8-byte aligned, are BGSS_EINVAL.
 * Counts taken with a cap below neighbor_threshold make every point look sparse: that is the caller's error and is not
 * detected. */
int bgss_entries_keep(int hip_device, void* hip_stream, void* entries_device_ptr, uint32_t entry_count, const void* counts_device_ptr,
                      uint32_t n, uint32_t neighbor_threshold, uint32_t flags);

/* Test hook: forces a table of 2^bits slots, clamped to [1, what the grid allocated]. 0 = automatic: the smallest power
 * of two that is at least 2 n, at least 64. The counts do not depend on it. */
int bgss_debug_set_table_bits(bgss_grid* grid, uint32_t bits);

#ifdef __cplusplus
}
#endif

#endif /* BGS_SPARSE_H */
