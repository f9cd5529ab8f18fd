// display_bench — what one displayed frame of a progressive caller costs when
// its plane lives in device memory:
//   device route  ipt_display_device on the plane + 1 B per pixel to the host
//   host route    what the library offered before ipt_display_device: wait for
//                 the stream, download the plane (4 B per pixel), then
//                 ipt::to_gray8 on one CPU thread; with glare, ipt_glare
//                 (upload, three allocations, download) in between
// Both routes end with the 8-bit picture in host memory and must agree byte
// for byte. Cases: 1024 x 1024 without glare and 640 x 640 with the GUI's
// cutoff 1.01, each on a render of the box scene (the C2 workload's scene);
// that render has no pixel above 1.01, so a third case scales it until 1 % of
// its pixels are bright.
// Then the display statistics (ipt_display_stats_device) on 640 x 640 and
// 1024 x 1024, see run_stats_case.
// Wall times from std::chrono::steady_clock around the whole route (host
// work, queueing and the final stream wait included); the device route's
// kernels alone from HIP events. 3 warm-up runs, then the median and minimum
// of 15.
//
//   hipcc -O2 -std=c++17 -ffp-contract=off scripts/display_bench.cpp -Iipt_amd/host -Iinclude \
//         -Lipt_amd/lib -lipt_host -lipt_hip -Wl,-rpath,$PWD/ipt_amd/lib -o /tmp/display_bench
//   /tmp/display_bench        # one JSON line per case
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ipt_host.h"

#define HIPOK(expr)                                                                    \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));            \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)
#define IPTOK(ctx, expr)                                                               \
    do {                                                                               \
        if ((expr) != IPT_OK) {                                                        \
            std::fprintf(stderr, "%s: %s\n", #expr, ipt_last_error(ctx));              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

namespace {
constexpr int kWarm = 3, kReps = 15;

struct Stat {
    double median, min;
};
Stat stat(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return {v[v.size() / 2], v.front()};
}
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// bright_frac > 0: the rendered plane is scaled so that this fraction of its
// pixels lies above the cutoff (the box render itself has none above 1.01)
void run_case(ipt::GpuRenderer& gpu, int W, int H, int spp, float cutoff, double bright_frac = 0.0) {
    ipt_ctx* ctx = gpu.handle();
    ipt::GridRenderPlane plane((size_t)W, (size_t)H);
    ipt::RenderParams rp;
    rp.spp = spp;
    gpu.render(plane, rp);
    const size_t n = (size_t)W * H;
    if (bright_frac > 0.0) {
        std::vector<float> sorted = plane.pixels;
        std::sort(sorted.begin(), sorted.end());
        const float q = sorted[(size_t)((1.0 - bright_frac) * (double)(n - 1))];
        for (float& v : plane.pixels) v = v / q * cutoff;
    }
    size_t bright = 0;
    for (float v : plane.pixels) bright += !(v <= cutoff) && cutoff > 0.0f;

    hipStream_t st;
    HIPOK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    float* d_plane = nullptr;
    uint8_t *d_gray = nullptr, *h_gray = nullptr;
    HIPOK(hipMalloc(&d_plane, n * sizeof(float)));
    HIPOK(hipMalloc(&d_gray, n));
    HIPOK(hipHostMalloc(&h_gray, n));
    HIPOK(hipMemcpy(d_plane, plane.pixels.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIPOK(hipEventCreate(&e0));
    HIPOK(hipEventCreate(&e1));
    ipt_display_params dp{};
    dp.width = W;
    dp.height = H;
    dp.glare_cutoff = cutoff;

    std::vector<double> dev_wall, dev_kernels, host_wall;
    std::vector<uint8_t> host_bytes;
    ipt::GridRenderPlane back((size_t)W, (size_t)H);
    for (int r = 0; r < kWarm + kReps; ++r) {
        // device route
        double t0 = now_ms();
        HIPOK(hipEventRecord(e0, st));
        IPTOK(ctx, ipt_display_device(ctx, &dp, d_plane, nullptr, nullptr, d_gray, st));
        HIPOK(hipEventRecord(e1, st));
        HIPOK(hipMemcpyAsync(h_gray, d_gray, n, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        double t1 = now_ms();
        float k = 0.0f;
        HIPOK(hipEventElapsedTime(&k, e0, e1));
        // host route
        double t2 = now_ms();
        HIPOK(hipStreamSynchronize(st));
        HIPOK(hipMemcpy(back.pixels.data(), d_plane, n * sizeof(float), hipMemcpyDeviceToHost));
        if (cutoff > 0.0f) {
            ipt::GridRenderPlane g((size_t)W, (size_t)H);
            g.pixels = gpu.glare(back, cutoff);
            host_bytes = ipt::to_gray8(g);
        } else {
            host_bytes = ipt::to_gray8(back);
        }
        double t3 = now_ms();
        if (r >= kWarm) {
            dev_wall.push_back(t1 - t0);
            dev_kernels.push_back(k);
            host_wall.push_back(t3 - t2);
        }
    }
    const bool same = std::memcmp(host_bytes.data(), h_gray, n) == 0;
    const Stat a = stat(dev_wall), b = stat(dev_kernels), c = stat(host_wall);
    std::printf(
        "{\"case\": \"box %dx%d %d spp\", \"glare_cutoff\": %.2f, \"bright_pixels\": %zu, \"bytes_identical\": %s, "
        "\"clock\": \"steady_clock wall per frame; kernels: HIP events\", \"warmup\": %d, \"reps\": %d, "
        "\"device_route_ms\": {\"median\": %.4f, \"min\": %.4f}, "
        "\"device_route_kernels_ms\": {\"median\": %.4f, \"min\": %.4f}, "
        "\"host_route_ms\": {\"median\": %.4f, \"min\": %.4f}}\n",
        W, H, spp, cutoff, bright, same ? "true" : "false", kWarm, kReps, a.median, a.min, b.median, b.min, c.median,
        c.min);
    std::fflush(stdout);
    IPTOK(ctx, ipt_render_wait(ctx));
    HIPOK(hipFree(d_plane));
    HIPOK(hipFree(d_gray));
    HIPOK(hipHostFree(h_gray));
    HIPOK(hipEventDestroy(e0));
    HIPOK(hipEventDestroy(e1));
    HIPOK(hipStreamDestroy(st));
    if (!same) std::exit(3);
}

// The display statistics (ipt_display_stats_device: the Gui's 400-bucket
// histogram and the white point at rank 0.95) on a render of the box scene
// that stays in device memory, kernels alone from HIP events:
//   display      ipt_display_device, the existing entry point, in the same run
//   hist / rank / both   the stats call with only the counts, only the white
//                point (stats), and counts + white point + 8-bit picture
//   hist_constant        the counts of a constant image (every lane, one bucket)
//   host_route   what the call replaces: wait, download the plane, then
//                ipt::histogram and std::nth_element on one CPU thread
// hist and rank must equal the host route's results.
void run_stats_case(ipt::GpuRenderer& gpu, int W, int H, int spp) {
    ipt_ctx* ctx = gpu.handle();
    ipt::GridRenderPlane plane((size_t)W, (size_t)H);
    ipt::RenderParams rp;
    rp.spp = spp;
    gpu.render(plane, rp);
    const size_t n = (size_t)W * H;
    const int nb = 400;
    const int64_t rank = (int64_t)ipt::white_rank_for((size_t)W, (size_t)H, 0.95);

    hipStream_t st;
    HIPOK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    float *d_plane = nullptr, *d_const = nullptr, *d_stats = nullptr;
    uint8_t* d_gray = nullptr;
    uint32_t* d_hist = nullptr;
    HIPOK(hipMalloc(&d_plane, n * sizeof(float)));
    HIPOK(hipMalloc(&d_const, n * sizeof(float)));
    HIPOK(hipMalloc(&d_gray, n));
    HIPOK(hipMalloc(&d_hist, nb * sizeof(uint32_t)));
    HIPOK(hipMalloc(&d_stats, 4 * sizeof(float)));
    HIPOK(hipMemcpy(d_plane, plane.pixels.data(), n * sizeof(float), hipMemcpyHostToDevice));
    const std::vector<float> constant(n, 0.3f);
    HIPOK(hipMemcpy(d_const, constant.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIPOK(hipEventCreate(&e0));
    HIPOK(hipEventCreate(&e1));
    ipt_display_params dp{};
    dp.width = W;
    dp.height = H;
    ipt_display_stats_params sp{};
    sp.width = W;
    sp.height = H;

    enum { kDisplay, kHist, kRank, kBoth, kHistConst, kVariants };
    const char* names[kVariants] = {"display", "hist", "rank", "both", "hist_constant"};
    std::vector<double> ms[kVariants], host_wall;
    for (int r = 0; r < kWarm + kReps; ++r) {
        for (int v = 0; v < kVariants; ++v) {
            sp.hist_buckets = v == kRank ? 0 : nb;
            sp.white_rank = v == kHist || v == kHistConst ? -1 : rank;
            HIPOK(hipEventRecord(e0, st));
            if (v == kDisplay) IPTOK(ctx, ipt_display_device(ctx, &dp, d_plane, nullptr, nullptr, d_gray, st));
            else if (v == kBoth) IPTOK(ctx, ipt_display_stats_device(ctx, &sp, d_plane, nullptr, nullptr, d_gray, d_hist, d_stats, st));
            else if (v == kRank) IPTOK(ctx, ipt_display_stats_device(ctx, &sp, d_plane, nullptr, nullptr, nullptr, nullptr, d_stats, st));
            else IPTOK(ctx, ipt_display_stats_device(ctx, &sp, v == kHistConst ? d_const : d_plane, nullptr, nullptr, nullptr, d_hist, nullptr, st));
            HIPOK(hipEventRecord(e1, st));
            HIPOK(hipStreamSynchronize(st));
            float k = 0.0f;
            HIPOK(hipEventElapsedTime(&k, e0, e1));
            if (r >= kWarm) ms[v].push_back(k);
        }
    }
    // results of one more "both" call against the host route, which is timed too
    sp.hist_buckets = nb;
    sp.white_rank = rank;
    IPTOK(ctx, ipt_display_stats_device(ctx, &sp, d_plane, nullptr, nullptr, d_gray, d_hist, d_stats, st));
    HIPOK(hipStreamSynchronize(st));
    std::vector<uint32_t> dev_hist(nb), host_hist;
    float dev_stats[4];
    HIPOK(hipMemcpy(dev_hist.data(), d_hist, nb * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(dev_stats, d_stats, sizeof dev_stats, hipMemcpyDeviceToHost));
    ipt::GridRenderPlane back((size_t)W, (size_t)H);
    float host_white = 0.0f;
    for (int r = 0; r < kWarm + kReps; ++r) {
        const double t0 = now_ms();
        HIPOK(hipStreamSynchronize(st));
        HIPOK(hipMemcpy(back.pixels.data(), d_plane, n * sizeof(float), hipMemcpyDeviceToHost));
        host_hist = ipt::histogram(back, nb);
        std::vector<float> sel = back.pixels;
        std::nth_element(sel.begin(), sel.begin() + rank, sel.end());
        host_white = sel[(size_t)rank];
        const double t1 = now_ms();
        if (r >= kWarm) host_wall.push_back(t1 - t0);
    }
    const bool same = host_hist == dev_hist && std::memcmp(&host_white, &dev_stats[2], 4) == 0;
    if (!same)
        std::fprintf(stderr, "stats differ: histogram %s, white %.9g (device) / %.9g (host)\n",
                     host_hist == dev_hist ? "equal" : "differs", (double)dev_stats[2], (double)host_white);
    std::printf("{\"case\": \"stats box %dx%d %d spp\", \"buckets\": %d, \"rank\": %lld, \"results_identical\": %s, "
                "\"clock\": \"kernels: HIP events; host route: steady_clock\", \"warmup\": %d, \"reps\": %d",
                W, H, spp, nb, (long long)rank, same ? "true" : "false", kWarm, kReps);
    for (int v = 0; v < kVariants; ++v) {
        const Stat s = stat(ms[v]);
        std::vector<double> sorted = ms[v];
        std::sort(sorted.begin(), sorted.end());
        std::printf(", \"%s_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}", names[v], s.median, s.min, sorted.back());
    }
    const Stat h = stat(host_wall);
    std::printf(", \"host_route_ms\": {\"median\": %.4f, \"min\": %.4f}}\n", h.median, h.min);
    std::fflush(stdout);
    IPTOK(ctx, ipt_render_wait(ctx));
    for (void* p : {(void*)d_plane, (void*)d_const, (void*)d_gray, (void*)d_hist, (void*)d_stats}) HIPOK(hipFree(p));
    HIPOK(hipEventDestroy(e0));
    HIPOK(hipEventDestroy(e1));
    HIPOK(hipStreamDestroy(st));
    if (!same) std::exit(3);
}
}  // namespace

int main() {
    try {
        ipt::GpuRenderer gpu(0);
        gpu.upload(ipt::make_scene_box());
        run_case(gpu, 1024, 1024, 4, 0.0f);
        run_case(gpu, 640, 640, 16, 1.01f);
        run_case(gpu, 640, 640, 16, 1.01f, 0.01);
        run_stats_case(gpu, 640, 640, 16);
        run_stats_case(gpu, 1024, 1024, 4);
    } catch (const ipt::IptError& e) {
        std::fprintf(stderr, "display_bench: error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
