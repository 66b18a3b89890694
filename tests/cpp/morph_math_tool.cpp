// morph_math_tool.cpp — TEST-ONLY stand-alone program over the product's morph arithmetic (csrc_morph/morph_math.h through
// tests/host_shim/morph_math_shim.cpp), built by tests/test_interpolate_host.py with the address and undefined-behaviour
// sanitizers and run as a process of its own.
//
//   morph_math_tool IN OUT
// IN:  u32 n, u32 planes a side (4: f32 layout, 3: precomputed-covariance layout), u32 settings; then `settings` times
//      (time, time_start, time_stop); then the lhs's planes and the rhs's, each n rows of f32.
// OUT: for every setting t, u and the output's planes.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../host_shim/morph_math_shim.cpp"

static void read_all(void* to, size_t size, size_t count, FILE* f) {
    if (count && fread(to, size, count, f) != count) {
        fprintf(stderr, "morph_math_tool: short read\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: morph_math_tool IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "morph_math_tool: cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    uint32_t head[3];
    read_all(head, sizeof(uint32_t), 3, in);
    const uint32_t n = head[0], per_side = head[1], settings = head[2];
    if (per_side != 3u && per_side != 4u) {
        fprintf(stderr, "morph_math_tool: %u planes a side\n", per_side);
        return 2;
    }
    static const size_t f32_widths[4] = {4, 48, 4, 4}, cov_widths[3] = {4, 48, 8};
    const size_t* widths = per_side == 4u ? f32_widths : cov_widths;
    std::vector<float> times(3 * (size_t)settings);
    read_all(times.data(), sizeof(float), times.size(), in);
    std::vector<std::vector<float>> side[2], result(per_side);
    for (int s = 0; s < 2; ++s)
        for (uint32_t p = 0; p < per_side; ++p) {
            side[s].emplace_back((size_t)n * widths[p]);
            read_all(side[s].back().data(), sizeof(float), side[s].back().size(), in);
        }
    for (uint32_t p = 0; p < per_side; ++p) result[p].assign((size_t)n * widths[p], -77.0f);
    for (uint32_t k = 0; k < settings; ++k) {
        const float time = times[3 * k], start = times[3 * k + 1], stop = times[3 * k + 2];
        float factor[2];
        shim_factor(time, start, stop, &factor[0], &factor[1]);
        fwrite(factor, sizeof(float), 2, out);
        const std::vector<std::vector<float>>&l = side[0], &r = side[1];
        if (per_side == 4u)
            shim_interpolate_f32(n, l[0].data(), l[1].data(), l[2].data(), l[3].data(), r[0].data(), r[1].data(), r[2].data(), r[3].data(), time,
                                 start, stop, result[0].data(), result[1].data(), result[2].data(), result[3].data());
        else
            shim_interpolate_cov3d_f32(n, l[0].data(), l[1].data(), l[2].data(), r[0].data(), r[1].data(), r[2].data(), time, start, stop,
                                       result[0].data(), result[1].data(), result[2].data());
        for (uint32_t p = 0; p < per_side; ++p)
            if (!result[p].empty()) fwrite(result[p].data(), sizeof(float), result[p].size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
