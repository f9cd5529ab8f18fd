// Test helper (tests/test_gui_plane_cpu.py): the host layer's CPU
// GuiRenderPlane without a GPU. "addray W H in.xyv out.bin" feeds the float
// triples (x, y, value) of in.xyv to GuiRenderPlane::addRay in order and
// writes W*H float pixels followed by W*H uint32 counters; "reset W H" fills
// a plane, calls resetImage() and prints the number of entries left non-zero.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "ipt_host.h"

int main(int argc, char** argv) {
    if (argc >= 6 && std::strcmp(argv[1], "addray") == 0) {
        const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
        std::ifstream in(argv[4], std::ios::binary | std::ios::ate);
        const size_t n = (size_t)in.tellg() / 12;
        in.seekg(0);
        std::vector<float> xyv(3 * n);
        in.read(reinterpret_cast<char*>(xyv.data()), (std::streamsize)(12 * n));
        ipt::GuiRenderPlane plane(w, h);
        for (size_t i = 0; i < n; ++i) plane.addRay(xyv[3 * i], xyv[3 * i + 1], xyv[3 * i + 2]);
        std::vector<uint32_t> cnt(plane.value_counter.begin(), plane.value_counter.end());
        std::ofstream out(argv[5], std::ios::binary);
        out.write(reinterpret_cast<const char*>(plane.pixels.data()), (std::streamsize)(4 * w * h));
        out.write(reinterpret_cast<const char*>(cnt.data()), (std::streamsize)(4 * w * h));
        return out ? 0 : 1;
    }
    if (argc >= 4 && std::strcmp(argv[1], "reset") == 0) {
        const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
        ipt::GuiRenderPlane plane(w, h);
        for (size_t i = 0; i < w * h; ++i) plane.addRay((float)(i % w) / (float)w, (float)(i / w) / (float)h, 1.0f + (float)i);
        plane.resetImage();
        size_t left = 0;
        for (float v : plane.pixels) left += v != 0.0f;
        for (size_t c : plane.value_counter) left += c != 0;
        std::printf("%zu\n", left);
        return 0;
    }
    std::fprintf(stderr, "usage: gui_plane_probe addray W H in.xyv out.bin | reset W H\n");
    return 2;
}
