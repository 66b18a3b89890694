// bounds_shim.cpp — g++ build of csrc/bounds_math.h (the arithmetic of the device reduction behind BGS_BOUNDS_CLOUD) for
// tests/test_cloud_bounds_host.py: as a shared library for ctypes, and, with -DBOUNDS_SHIM_MAIN, as a stand-alone program
// that the test builds with -fsanitize=address,undefined and runs on the same inputs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bevy_gaussian_splatting_amd/csrc/bounds_math.h"

extern "C" {

// out[0..2] = min, out[3..5] = max: the contract as the reference writes it (one splat after the other, offset per splat)
void shim_bounds_reference(const float* position_visibility, uint32_t n, float* out) {
    bgs::bounds_fold_reference(position_visibility, n, out, out + 3);
}

// ... and as the device forms it: raw coordinates folded in `parts` interleaved partial results, merged as keys onto the
// preset words with integer min / max, decoded, offset applied once
void shim_bounds_device_order(const float* position_visibility, uint32_t n, uint32_t parts, float* out) {
    bgs::bounds_fold_device_order(position_visibility, n, parts, out, out + 3);
}

uint32_t shim_bounds_key(uint32_t bits) { return bgs::bounds_key(bits); }
uint32_t shim_bounds_key_bits(uint32_t key) { return bgs::bounds_key_bits(key); }
uint32_t shim_bounds_grid(uint32_t n, uint32_t compute_units, uint32_t grid_cap) { return bgs::bounds_grid(n, compute_units, grid_cap); }

void shim_bounds_decode(const uint32_t* words, float* out) { bgs::bounds_decode(words, out, out + 3); }

}  // extern "C"

#ifdef BOUNDS_SHIM_MAIN
// bounds_shim FILE PARTS: FILE holds n x 4 float32. Prints the twelve words (reference min, max; device-order min, max) in hex.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> pv;
    float rec[4];
    while (std::fread(rec, sizeof rec, 1, f) == 1) pv.insert(pv.end(), rec, rec + 4);
    std::fclose(f);
    const uint32_t n = (uint32_t)(pv.size() / 4u), parts = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    float out[12];
    shim_bounds_reference(pv.data(), n, out);
    shim_bounds_device_order(pv.data(), n, parts, out + 6);
    for (int i = 0; i < 12; ++i) {
        uint32_t bits;
        std::memcpy(&bits, &out[i], 4);
        std::printf("%08x%c", bits, i == 11 ? '\n' : ' ');
    }
    return 0;
}
#endif
