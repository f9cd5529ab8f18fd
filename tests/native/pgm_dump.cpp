// Test helper (tests/test_pgm_cpu.py): the host layer's PGM writer, the
// restatement of main.cpp:225-235 and 297-309 that runs on the CPU.
//   nval in.f32 N MAX_BITS CONTRAST_BITS GAMMA_BITS   ipt::n_val of each value, one per line
//   pgm W H in.f32 MAX_BITS CONTRAST_BITS GAMMA_BITS out.pgm   ipt::write_pgm
//   bytes W H in.u8 out.pgm                           ipt::write_pgm_bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "ipt_host.h"

static float from_bits(const char* s) {
    const uint32_t u = (uint32_t)std::strtoul(s, nullptr, 10);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc >= 7 && std::strcmp(argv[1], "nval") == 0) {
        const size_t n = std::strtoul(argv[3], nullptr, 10);
        std::vector<float> v(n);
        std::ifstream in(argv[2], std::ios::binary);
        in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * 4));
        const float mx = from_bits(argv[4]), contrast = from_bits(argv[5]), gamma = from_bits(argv[6]);
        for (float x : v) std::printf("%d\n", ipt::n_val(x, mx, contrast, gamma));
        return 0;
    }
    if (argc >= 9 && std::strcmp(argv[1], "pgm") == 0) {
        const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
        ipt::GridRenderPlane plane(w, h);
        std::ifstream in(argv[4], std::ios::binary);
        in.read(reinterpret_cast<char*>(plane.pixels.data()), (std::streamsize)(w * h * 4));
        plane.max_value = from_bits(argv[5]);
        ipt::write_pgm(argv[8], plane, from_bits(argv[6]), from_bits(argv[7]));
        return 0;
    }
    if (argc >= 6 && std::strcmp(argv[1], "bytes") == 0) {
        const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
        std::vector<uint8_t> b(w * h);
        std::ifstream in(argv[4], std::ios::binary);
        in.read(reinterpret_cast<char*>(b.data()), (std::streamsize)(w * h));
        ipt::write_pgm_bytes(argv[5], w, h, b);
        return 0;
    }
    std::fprintf(stderr, "usage: pgm_dump nval|pgm|bytes ...\n");
    return 2;
}
