// Test driver for the particle behaviours of include/bgs.hpp / bgs_host.hpp (no GPU needed): tests/test_particles_host.py.
//   particle_tool layout                         sizeof and field offsets of bgs::ParticleBehavior and bgs_particle_behavior
//   particle_tool random <n> <seed> <out.bin>    random_particle_behaviors -> n records of 64 bytes
//   particle_tool validate <records.bin> <n>     validate_particle_behaviors for a cloud of n splats: "ok", or exit 1 + message
#include <cstddef>
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../include/bgs_host.hpp"

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    try {
        if (cmd == "layout") {
            std::printf("%zu %zu %zu %zu %zu\n", sizeof(bgs::ParticleBehavior), offsetof(bgs::ParticleBehavior, indicies),
                        offsetof(bgs::ParticleBehavior, velocity), offsetof(bgs::ParticleBehavior, acceleration),
                        offsetof(bgs::ParticleBehavior, jerk));
            std::printf("%zu %zu %zu %zu %zu\n", sizeof(bgs_particle_behavior), offsetof(bgs_particle_behavior, indicies),
                        offsetof(bgs_particle_behavior, velocity), offsetof(bgs_particle_behavior, acceleration),
                        offsetof(bgs_particle_behavior, jerk));
        } else if (cmd == "random" && argc == 5) {
            const auto r = bgs::random_particle_behaviors(std::stoul(argv[2]), std::stoull(argv[3]));
            std::ofstream f(argv[4], std::ios::binary);
            f.write((const char*)r.data(), (std::streamsize)(r.size() * sizeof(bgs::ParticleBehavior)));
        } else if (cmd == "validate" && argc == 4) {
            std::ifstream in(argv[2], std::ios::binary);
            const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            std::vector<bgs::ParticleBehavior> r(raw.size() / sizeof(bgs::ParticleBehavior));
            if (!r.empty()) std::memcpy(r.data(), raw.data(), r.size() * sizeof(bgs::ParticleBehavior));
            bgs::validate_particle_behaviors(r, (uint32_t)std::stoul(argv[3]));
            std::printf("ok\n");
        } else {
            std::fprintf(stderr, "usage: particle_tool layout | random <n> <seed> <out> | validate <records> <n>\n");
            return 2;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "particle_tool: %s\n", e.what());
        return 1;
    }
    return 0;
}
