// cloud_bounds_time.hip — times the reduction behind BGS_BOUNDS_CLOUD (csrc/bounds_kernels.hip, compiled into this program
// as it is) with HIP events on a stream of its own: warm-ups, then the median, minimum and maximum of the timed runs. The
// library has no entry point that runs the reduction alone (the seam is full: include/bgs.h), hence a program of its own;
// scripts/measure_cloud_bounds.py builds and runs it and sets the figure beside bgs_hbm_probe's.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off scripts/micro/cloud_bounds_time.hip -o scripts/micro/cloud_bounds_time
//   scripts/micro/cloud_bounds_time POINTS [RUNS [WARMUP]]
// Two timings a run: "reduce" the kernel alone (the words preset outside the events), "refresh" the two presets and the
// kernel, which is what the first flagged frame after a change of the cloud enqueues. One JSON line. The positions are a
// fixed pseudo-random plane, resident in as many copies as fill 640 MiB, and successive runs read successive copies: a run
// does not find its plane in the 256 MiB Infinity Cache (a 1 M plane is 16 MB, a 5 M plane 80 MB: alone they would stay
// there, and the figure would be the cache's). The six words are checked against the host fold of bounds_math.h after the last run.
#include "../../bevy_gaussian_splatting_amd/csrc/bounds_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1000000u;
    const int runs = argc > 2 ? std::atoi(argv[2]) : 30, warmup = argc > 3 ? std::atoi(argv[3]) : 5;
    if (n == 0u || n > (1u << 30) || runs < 1 || warmup < 0) { std::fprintf(stderr, "usage: cloud_bounds_time POINTS [RUNS [WARMUP]]\n"); return 2; }
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const uint32_t cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    std::vector<float> pv((size_t)n * 4u);
    uint32_t state = 12345u;
    for (float& v : pv) {
        state = state * 1664525u + 1013904223u;
        v = ((float)(state >> 8) / 16777216.0f - 0.5f) * 40.0f;
    }
    float4* d_pv = nullptr;
    uint32_t* d_words = nullptr;
    const size_t plane_bytes = pv.size() * sizeof(float);
    const uint32_t copies = (uint32_t)(((640ull << 20) + plane_bytes - 1u) / plane_bytes);
    CHECK(hipMalloc(&d_pv, plane_bytes * copies));
    CHECK(hipMalloc(&d_words, bgs::BOUNDS_WORDS * sizeof(uint32_t)));
    CHECK(hipMemcpy(d_pv, pv.data(), plane_bytes, hipMemcpyHostToDevice));
    for (uint32_t c = 1; c < copies; ++c) CHECK(hipMemcpy(d_pv + (size_t)c * n, d_pv, plane_bytes, hipMemcpyDeviceToDevice));
    uint32_t turn = 0;
    hipStream_t stream;
    CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    hipEvent_t start, stop;
    CHECK(hipEventCreate(&start));
    CHECK(hipEventCreate(&stop));
    const uint32_t grid = bgs::bounds_grid(n, cus, 0u);
    std::vector<float> reduce_ms, refresh_ms;
    for (int pass = 0; pass < 2; ++pass)          // 0: the kernel alone, 1: presets + kernel
        for (int run = 0; run < warmup + runs; ++run) {
            const float4* plane = d_pv + (size_t)(turn++ % copies) * n;
            if (pass == 0) {
                CHECK(hipMemsetAsync(d_words, 0xFF, 12, stream));
                CHECK(hipMemsetAsync(d_words + 3, 0, 12, stream));
            }
            CHECK(hipEventRecord(start, stream));
            if (pass == 0) {
                hipLaunchKernelGGL(bgs::cloud_bounds_kernel, dim3(grid), dim3(bgs::BOUNDS_THREADS), 0, stream, plane, n, d_words);
                CHECK(hipGetLastError());
            } else {
                CHECK(bgs::launch_cloud_bounds(stream, plane, n, d_words, cus, 0u));
            }
            CHECK(hipEventRecord(stop, stream));
            CHECK(hipEventSynchronize(stop));
            float ms = 0.0f;
            CHECK(hipEventElapsedTime(&ms, start, stop));
            if (run >= warmup) (pass == 0 ? reduce_ms : refresh_ms).push_back(ms);
        }
    uint32_t words[bgs::BOUNDS_WORDS];
    CHECK(hipMemcpy(words, d_words, sizeof words, hipMemcpyDeviceToHost));
    float got[6], want[6];
    bgs::bounds_decode(words, got, got + 3);
    bgs::bounds_fold_reference(pv.data(), n, want, want + 3);
    const bool same = std::memcmp(got, want, sizeof got) == 0;
    auto stats = [](std::vector<float> v, double out[3]) {
        std::sort(v.begin(), v.end());
        out[0] = v.size() % 2 ? v[v.size() / 2] : 0.5 * ((double)v[v.size() / 2 - 1] + v[v.size() / 2]);
        out[1] = v.front();
        out[2] = v.back();
    };
    double a[3], b[3];
    stats(reduce_ms, a);
    stats(refresh_ms, b);
    const double bytes = (double)n * 16.0;
    std::printf("{\"points\": %u, \"runs\": %d, \"warmup\": %d, \"compute_units\": %u, \"workgroups\": %u, \"resident_copies\": %u, \"bytes_read\": %.0f, "
                "\"reduce\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"max_ms\": %.6f, \"gb_per_s\": %.1f}, "
                "\"refresh\": {\"median_ms\": %.6f, \"min_ms\": %.6f, \"max_ms\": %.6f, \"gb_per_s\": %.1f}, \"equals_host_fold\": %s}\n",
                n, runs, warmup, cus, grid, copies, bytes, a[0], a[1], a[2], bytes / (a[0] * 1e-3) / 1e9, b[0], b[1], b[2],
                bytes / (b[0] * 1e-3) / 1e9, same ? "true" : "false");
    (void)hipEventDestroy(start);
    (void)hipEventDestroy(stop);
    (void)hipStreamDestroy(stream);
    (void)hipFree(d_words);
    (void)hipFree(d_pv);
    return same ? 0 : 3;
}
