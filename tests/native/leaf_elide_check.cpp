// Host check of the path kernel's leaf elision: in a tree of
// n_rays = 2^K, a node at depth K (one iteration, whose ray has no children)
// that lies strictly behind the lights' plane -- (o.z - P.z) * n.z < 0, the
// kernel's own test -- is worth exactly +0 whatever it draws, and draws three
// words (a light or cosine pick) or one (the fall-through). The kernel's
// product FIXED = K instances rely on it to resolve such a child at its
// parent instead of pushing it.
//
// The oracle is replayed with its iteration hook; at every iteration of a
// depth-K node behind the plane the hook checks the draw count, traces the
// sampled direction against the lights (no hit allowed) and restates the
// node's value from the oracle's own functions (UnionDdf::value, ray_power of
// the childless ray, the finite test): its bits must be +0.
//
// usage: leaf_elide_check SCENE WIDTH PASSES   (WIDTH^2 * PASSES paths)
// One line: scene S paths N leaves L back B draws3 D3 draws1 D1 skips Z nan_rays R
//           light_hits H nonzero V bad_draws W     exit status 1 on a violation
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

struct LeafStats {
    unsigned long long leaves = 0, back = 0, draws3 = 0, draws1 = 0, skips = 0, nan_rays = 0, light_hits = 0,
                       nonzero = 0, bad_draws = 0;
};
static LeafStats g_st;
static int g_K = 0;
static float g_pz = 0.0f, g_nz = 0.0f;
template <class C, class S, class D, class V>
static void leaf_hook(const C& cx, const S& si, const D& sdf, const V& nd, int depth, int n, uint32_t k_at);
#define IPT_ORACLE_ITER_HOOK(depth, i, n, k, skip, pos) leaf_hook(cx, si, sdf, new_direction, depth, n, k)
#include "../../oracle/ipt_oracle.cpp"
#include "ipt_host.h"

template <class C, class S, class D, class V>
static void leaf_hook(const C& cx, const S& si, const D& sdf, const V& nd, int depth, int n, uint32_t k_at) {
    if (depth != g_K || n != 1) return;
    ++g_st.leaves;
    if (!((si.position.z - g_pz) * g_nz < 0.0f)) return;
    ++g_st.back;
    const uint32_t draws = g_rng->k - k_at;
    if (draws == 3u) ++g_st.draws3;
    else if (draws == 1u) ++g_st.draws1;
    else ++g_st.bad_draws;
    float res = 0.0f;
    if (nd == mk(0, 0, 0)) {
        ++g_st.skips;
    } else {
        if (draws != 3u) ++g_st.bad_draws;  // the fall-through samples no direction
        const SceneO& sc = *cx.sc;
        V3 lpos;
        float lpow;
        if (lighting_trace(sc, si.position, nd, &lpos, &lpow)) ++g_st.light_hits;
        // the iteration's term (main.cpp:165-176) and the node's value (main.cpp:181)
        const std::vector<float>& w = cx.mix->weights;
        const int nl = (int)sc.lights.size();
        float mix_val = 0.0f;
        for (int c = 0; c < nl; ++c) mix_val += w[c] * light_ddf_value(sc.lights[c], si.position, nd);
        mix_val += w[nl] * sdf.value(nd);
        const float sdf_val = sdf.value(nd);
        const float multiplier = sdf_val / mix_val;
        const uint32_t k_before = g_rng->k;
        const float rp = ray_power(cx, si.position, nd, depth + 1, n / 2);  // no children: draws nothing
        if (g_rng->k != k_before) ++g_st.bad_draws;
        if (rp != rp) ++g_st.nan_rays;
        res += multiplier * 1.0f * rp;
    }
    res = std::isfinite(res) ? res / n : 0.0f;
    uint32_t bits;
    std::memcpy(&bits, &res, 4);
    if (bits != 0u) ++g_st.nonzero;
}

int main(int argc, char** argv) {
    const std::string name = argc > 1 ? argv[1] : "box";
    const int W = argc > 2 ? std::atoi(argv[2]) : 128;
    const int passes = argc > 3 ? std::atoi(argv[3]) : 4;
    ipt::FlatScene f = ipt::flatten(ipt::make_scene_by_name(name));
    ipt_params p{};
    p.width = W;
    p.height = W;
    p.spp = 1;
    p.n_rays = 16;
    p.depth_max = 8;
    p.seed = 0x1234abcdULL;
    while ((p.n_rays >> (g_K + 1)) != 0) ++g_K;
    SceneO sc = make_scene(&f.scene);
    // the lights' shared plane (one light, or a coplanar lattice): P.z and the
    // z component of the normal AreaLight::traceRay uses
    g_pz = sc.lights[0].position.z;
    g_nz = normalize(cross(sc.lights[0].x_axis, sc.lights[0].y_axis)).z;
    for (const AreaLightO& l : sc.lights) {
        const V3 nn = normalize(cross(l.x_axis, l.y_axis));
        if (l.position.z != g_pz || nn.z != g_nz || nn.x != 0.0f || nn.y != 0.0f) {
            std::printf("scene %s: the lights do not share a z plane\n", name.c_str());
            return 2;
        }
    }
    Mixture mix = build_mixture(sc);
    Ctx cx{&sc, &mix, p.depth_max};
    unsigned long long paths = 0;
    for (int s = 0; s < passes; ++s)
        for (int iy = 0; iy < W; ++iy)
            for (int ix = 0; ix < W; ++ix) {
                p.spp_offset = s;
                int xo, yo;
                oracle_pixel(cx, &p, ix, iy, 0, &xo, &yo);
                ++paths;
            }
    std::printf("scene %s paths %llu leaves %llu back %llu draws3 %llu draws1 %llu skips %llu nan_rays %llu "
                "light_hits %llu nonzero %llu bad_draws %llu\n",
                name.c_str(), paths, g_st.leaves, g_st.back, g_st.draws3, g_st.draws1, g_st.skips, g_st.nan_rays,
                g_st.light_hits, g_st.nonzero, g_st.bad_draws);
    return (g_st.light_hits || g_st.nonzero || g_st.bad_draws) ? 1 : 0;
}
