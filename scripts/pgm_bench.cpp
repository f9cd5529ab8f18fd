// pgm_bench — what main.cpp's written output (smooth(2) -> computeSmoothedMax(5)
// -> n_val, main.cpp:291-309) costs for a plane that lives in device memory
// (DESIGN.md §4.8 "PGM path"), in the manner of display_bench.cpp:
//   device route  ipt_pgm_device(smooth 2, max 5) on the plane + 1 B per pixel
//                 to the host
//   host route    what the library offered before ipt_pgm_device: wait for the
//                 stream, download the plane (4 B per pixel), ipt_smooth twice
//                 (each: three allocations, an upload, a download), then
//                 write_pgm's ipt::n_val loop on one CPU thread
// Both routes end with the PGM's numbers in host memory and must agree byte for
// byte. One case: 1024 x 1024, a render of the box scene (the C2 workload's).
// Wall times from std::chrono::steady_clock around the whole route; the device
// route's kernels alone from HIP events. 3 warm-up runs, then the median and
// minimum of 15.
//
//   hipcc -O2 -std=c++17 -ffp-contract=off scripts/pgm_bench.cpp -Iipt_amd/host -Iinclude \
//         -Lipt_amd/lib -lipt_host -lipt_hip -Wl,-rpath,$PWD/ipt_amd/lib -o /tmp/pgm_bench
//   /tmp/pgm_bench        # one JSON line
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

void run_case(ipt::GpuRenderer& gpu, int W, int H, int spp) {
    ipt_ctx* ctx = gpu.handle();
    ipt::GridRenderPlane plane((size_t)W, (size_t)H);
    ipt::RenderParams rp;
    rp.spp = spp;
    gpu.render(plane, rp);
    const size_t n = (size_t)W * H;

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
    ipt_pgm_params pp{};
    pp.width = W;
    pp.height = H;
    pp.smooth_side = 2;
    pp.max_side = 5;
    pp.contrast = 500.0f;
    pp.gamma = 0.6f;

    std::vector<double> dev_wall, dev_kernels, host_wall, host_nval;
    std::vector<uint8_t> host_bytes(n);
    ipt::GridRenderPlane back((size_t)W, (size_t)H);
    for (int r = 0; r < kWarm + kReps; ++r) {
        // device route
        const double t0 = now_ms();
        HIPOK(hipEventRecord(e0, st));
        IPTOK(ctx, ipt_pgm_device(ctx, &pp, d_plane, nullptr, nullptr, d_gray, nullptr, st));
        HIPOK(hipEventRecord(e1, st));
        HIPOK(hipMemcpyAsync(h_gray, d_gray, n, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        const double t1 = now_ms();
        float k = 0.0f;
        HIPOK(hipEventElapsedTime(&k, e0, e1));
        // host route
        const double t2 = now_ms();
        HIPOK(hipStreamSynchronize(st));
        HIPOK(hipMemcpy(back.pixels.data(), d_plane, n * sizeof(float), hipMemcpyDeviceToHost));
        gpu.smooth(back, 2);
        gpu.computeSmoothedMax(back, 5);
        const double t3 = now_ms();
        for (size_t i = 0; i < n; ++i) host_bytes[i] = (uint8_t)ipt::n_val(back.pixels[i], back.max_value, 500.0f, 0.6f);
        const double t4 = now_ms();
        if (r >= kWarm) {
            dev_wall.push_back(t1 - t0);
            dev_kernels.push_back(k);
            host_wall.push_back(t4 - t2);
            host_nval.push_back(t4 - t3);
        }
    }
    const bool same = std::memcmp(host_bytes.data(), h_gray, n) == 0;
    const Stat a = stat(dev_wall), b = stat(dev_kernels), c = stat(host_wall), d = stat(host_nval);
    std::printf(
        "{\"case\": \"pgm box %dx%d %d spp, smooth 2, smoothed max 5, contrast 500, gamma 0.6\", "
        "\"bytes_identical\": %s, \"clock\": \"steady_clock wall per frame; kernels: HIP events\", \"warmup\": %d, "
        "\"reps\": %d, \"device_route_ms\": {\"median\": %.4f, \"min\": %.4f}, "
        "\"device_route_kernels_ms\": {\"median\": %.4f, \"min\": %.4f}, "
        "\"host_route_ms\": {\"median\": %.4f, \"min\": %.4f}, "
        "\"host_route_n_val_loop_ms\": {\"median\": %.4f, \"min\": %.4f}}\n",
        W, H, spp, same ? "true" : "false", kWarm, kReps, a.median, a.min, b.median, b.min, c.median, c.min, d.median,
        d.min);
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
}  // namespace

int main() {
    try {
        ipt::GpuRenderer gpu(0);
        gpu.upload(ipt::make_scene_box());
        run_case(gpu, 1024, 1024, 4);
    } catch (const ipt::IptError& e) {
        std::fprintf(stderr, "pgm_bench: error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
