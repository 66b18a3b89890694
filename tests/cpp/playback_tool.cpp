// playback_tool — bgs::playback_update (include/bgs_host.hpp) on cases read from stdin, for tests/test_playback_host.py.
// A case is one line of seven words: the mode's number, then the bit patterns (hex) of time, time_scale, time_start,
// time_stop, delta_secs, elapsed_secs. The answer is one line a case: the bit pattern (hex) of the time afterwards.
// Built without libbgs: the header's other functions are inline and unused here.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "bgs_host.hpp"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

int main() {
    unsigned mode, w[6];
    while (std::scanf("%u %x %x %x %x %x %x", &mode, &w[0], &w[1], &w[2], &w[3], &w[4], &w[5]) == 7) {
        bgs::Playback s;
        s.playback_mode = static_cast<bgs::PlaybackMode>(mode);
        s.time = from_bits(w[0]);
        s.time_scale = from_bits(w[1]);
        s.time_start = from_bits(w[2]);
        s.time_stop = from_bits(w[3]);
        bgs::playback_update(s, from_bits(w[4]), from_bits(w[5]));
        uint32_t out;
        std::memcpy(&out, &s.time, 4);
        std::printf("%08x\n", out);
    }
    return 0;
}
