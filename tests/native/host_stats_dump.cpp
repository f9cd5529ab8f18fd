// Test helper (tests/test_display_stats_cpu.py): the host layer's CPU
// restatements of the display statistics, without a GPU.
//   hist W H in.f32 NB   the counts of ipt::histogram, one per line
//   kth W H in.f32 K     the bit pattern of ipt::kth_smallest
//   tone W H in.f32 WHITE_BITS out.f32   ipt::tone_map(plane, white)
//   rank W H FRACTION    ipt::white_rank_for
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "ipt_host.h"

static ipt::GridRenderPlane read_plane(char** argv) {
    const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
    ipt::GridRenderPlane plane(w, h);
    std::ifstream in(argv[4], std::ios::binary);
    in.read(reinterpret_cast<char*>(plane.pixels.data()), (std::streamsize)(w * h * 4));
    return plane;
}

int main(int argc, char** argv) {
    if (argc >= 6 && std::strcmp(argv[1], "hist") == 0) {
        for (uint32_t c : ipt::histogram(read_plane(argv), std::atoi(argv[5]))) std::printf("%u\n", c);
        return 0;
    }
    if (argc >= 6 && std::strcmp(argv[1], "kth") == 0) {
        const float v = ipt::kth_smallest(read_plane(argv), std::strtoull(argv[5], nullptr, 10));
        uint32_t u;
        std::memcpy(&u, &v, 4);
        std::printf("%u\n", u);
        return 0;
    }
    if (argc >= 7 && std::strcmp(argv[1], "tone") == 0) {
        const uint32_t u = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        float white;
        std::memcpy(&white, &u, 4);
        const std::vector<float> t = ipt::tone_map(read_plane(argv), white);
        std::ofstream out(argv[6], std::ios::binary);
        out.write(reinterpret_cast<const char*>(t.data()), (std::streamsize)(t.size() * 4));
        return 0;
    }
    if (argc >= 5 && std::strcmp(argv[1], "rank") == 0) {
        std::printf("%llu\n", (unsigned long long)ipt::white_rank_for(std::strtoul(argv[2], nullptr, 10),
                                                                      std::strtoul(argv[3], nullptr, 10),
                                                                      std::atof(argv[4])));
        return 0;
    }
    std::fprintf(stderr, "usage: host_stats_dump hist|kth|tone|rank ...\n");
    return 2;
}
