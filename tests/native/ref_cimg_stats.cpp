// ref_cimg_stats — the reference's own CImg as the authority on the display
// statistics (tests/test_display_stats_cpu.py): for a fixed list of small
// images it records what Gui::updateDisplay's histogram call (gui.cpp:83-88)
// and the kth_smallest remedy noted beside normalize() (gui.cpp:13) return.
// Compiled against the reference tree's include/CImg.h, headless:
//
//   g++ -O2 -std=c++17 -Dcimg_display=0 -I<reference>/include \
//       tests/native/ref_cimg_stats.cpp -o ref_cimg_stats -lpthread
//   ref_cimg_stats tests/golden/ref_display_stats.bin
//
// File (little endian): u32 case count, then per case
//   i32 W, H, nb, 0; i64 k; f32 input[W*H]; u32 hist[nb]; f32 max; f32 kth
// with hist = get_histogram(nb, max/100000.0f, max), max = max() and kth =
// kth_smallest(k). Every image is free of NaN and of mixed -0/+0, where CImg's
// quickselect returns the one value any correct selection returns.
#include <CImg.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using cimg_library::CImg;

namespace {
uint64_t lcg_state = 0x9e3779b97f4a7c15ull;
float uniform() {  // [0, 1) on the 2^-24 grid
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(lcg_state >> 40) * (1.0f / 16777216.0f);
}

struct Case {
    int W, H, nb;
    int64_t k;
    std::vector<float> px;
};

template <class F>
Case make(int W, int H, int nb, int64_t k, F f) {
    Case c{W, H, nb, k, std::vector<float>((size_t)W * H)};
    for (size_t i = 0; i < c.px.size(); ++i) c.px[i] = f(i);
    return c;
}

template <class T>
void put(std::FILE* f, const T& v) {
    std::fwrite(&v, sizeof v, 1, f);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: ref_cimg_stats OUT.bin\n");
        return 2;
    }
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<Case> cases;
    // spread: uniform values, the Gui's 400 buckets, the reference's 0.95 rank
    cases.push_back(make(37, 23, 400, (int64_t)(37 * 23 * 0.95), [](size_t) { return uniform() * 3.0f; }));
    // percentile: a dim scene with the emitter in view (a few pixels 1000 times brighter)
    cases.push_back(make(64, 64, 400, (int64_t)(64 * 64 * 0.95), [](size_t i) {
        const float u = uniform();
        return i % 97 == 5 ? 900.0f + 100.0f * u : u * u * u * u * 2.0f;
    }));
    cases.push_back(make(5, 17, 7, 0, [](size_t) { return uniform() * 4.0f - 1.5f; }));  // mixed sign
    cases.push_back(make(1, 1, 1, 0, [](size_t) { return 2.5f; }));
    cases.push_back(make(16, 16, 400, 100, [](size_t) { return 0.3f; }));  // constant
    cases.push_back(make(16, 16, 400, 5, [](size_t) { return 0.0f; }));    // all zeros
    cases.push_back(make(8, 8, 16, 63, [](size_t) { return -0.25f - uniform(); }));  // negative maximum
    cases.push_back(make(32, 32, 400, 32 * 32, [inf](size_t i) { return i % 211 == 7 ? inf : uniform(); }));
    cases.push_back(make(1, 7, 400, 3, [](size_t i) {  // subnormal maximum: max / 100000.0f underflows
        uint32_t u = 0x00000400u * (uint32_t)(i + 1);
        float v;
        std::memcpy(&v, &u, 4);
        return v;
    }));
    cases.push_back(make(48, 48, 4096, 48 * 48 / 2, [](size_t) { return uniform() * uniform(); }));
    cases.push_back(make(31, 9, 2, 139, [](size_t i) { return i % 2 ? 1.0f : 4.0f; }));  // two values, 139 ones

    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 1;
    put(f, (uint32_t)cases.size());
    for (const Case& c : cases) {
        CImg<float> img(c.px.data(), (unsigned)c.W, (unsigned)c.H, 1, 1);
        const float mx = img.max();
        const auto hist = img.get_histogram((unsigned)c.nb, mx / 100000.0f, mx);
        const float kth = img.kth_smallest((unsigned long)c.k);
        put(f, (int32_t)c.W);
        put(f, (int32_t)c.H);
        put(f, (int32_t)c.nb);
        put(f, (int32_t)0);
        put(f, (int64_t)c.k);
        std::fwrite(c.px.data(), 4, c.px.size(), f);
        for (int b = 0; b < c.nb; ++b) put(f, (uint32_t)hist[b]);
        put(f, mx);
        put(f, kth);
    }
    std::fclose(f);
    return 0;
}
