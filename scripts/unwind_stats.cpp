// Analysis tool (not product code): replays paths through the oracle and
// counts, per unwind of the path kernel's pop (pop_node in ipt_kernels.hip),
// how many levels finish at once -- the current node plus every suspended
// ancestor that was on its last iteration when it pushed. A pop that finishes
// four or more levels runs the loop `l = tdepth - 3 > stop` behind the two
// unrolled levels. The cases are those of tests/test_gpu_step_unwind.py (it
// links the C-ABI library only for the host layer's scene builder; no GPU):
//   g++ -O2 -std=c++17 -Iinclude -Iipt_amd/host scripts/unwind_stats.cpp ipt_amd/host/ipt_host.cpp \
//       -o /tmp/unwind_stats -lpthread -L ipt_amd/lib -lipt_hip -Wl,-rpath,$PWD/ipt_amd/lib
//   /tmp/unwind_stats
#include <cstdint>
#include <cstdio>
#include <vector>

struct Ev {
    int depth, i, n;
};
static thread_local std::vector<Ev>* g_evs = nullptr;
#define IPT_ORACLE_ITER_HOOK(depth, i, n, k, skip, pos) \
    do {                                                 \
        if (g_evs) g_evs->push_back(Ev{depth, i, n});    \
    } while (0)
#include "../oracle/ipt_oracle.cpp"
#include "ipt_host.h"

static void run(const char* scene, int W, int H, int spp, int spp_offset, int n_rays, int depth_max) {
    ipt::FlatScene f = ipt::flatten(ipt::make_scene_by_name(scene));
    ipt_params p{};
    p.width = W;
    p.height = H;
    p.spp = 1;
    p.n_rays = n_rays;
    p.depth_max = depth_max;
    p.seed = 20241223ULL;  // capi.make_params' default
    SceneO sc = make_scene(&f.scene);
    Mixture mix = build_mixture(sc);
    Ctx cx{&sc, &mix, p.depth_max};
    std::vector<Ev> evs;
    g_evs = &evs;
    uint64_t hist[10] = {}, pops = 0;
    for (int s = 0; s < spp; ++s)
        for (int iy = 0; iy < H; ++iy)
            for (int ix = 0; ix < W; ++ix) {
                evs.clear();
                p.spp_offset = spp_offset + s;
                int xo, yo;
                oracle_pixel(cx, &p, ix, iy, 0, &xo, &yo);
                // events arrive in DFS order: the nodes between an event's depth
                // and the next event's (or the path's end) finish in one pop
                for (size_t e = 0; e < evs.size(); ++e) {
                    const int next = e + 1 < evs.size() ? evs[e + 1].depth : -1;
                    if (next < evs[e].depth || (next == -1)) {
                        const int levels = evs[e].depth - next;
                        if (levels > 0) {
                            ++pops;
                            ++hist[levels < 9 ? levels : 9];
                        }
                    }
                }
            }
    g_evs = nullptr;
    std::printf("%-14s %2dx%-2d spp %d n_rays %2d depth_max %d: pops %8llu, levels finished at once:", scene, W, H, spp,
                n_rays, depth_max, (unsigned long long)pops);
    for (int l = 1; l < 10; ++l)
        if (hist[l]) std::printf(" %d:%llu", l, (unsigned long long)hist[l]);
    uint64_t loop = 0;
    for (int l = 4; l < 10; ++l) loop += hist[l];
    std::printf("  -> unwind loop entered %llu times\n", (unsigned long long)loop);
}

int main() {
    const char* scenes[] = {"box", "box_lights:4", "box_lights:16"};
    const int nr[] = {16, 1, 2, 17, 0};
    for (const char* s : scenes)
        for (int n : nr) run(s, 24, 20, 2, 5, n, 8);
    run("box", 4, 4, 1, 0, 64, 8);
    return 0;
}
