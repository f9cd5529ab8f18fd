// ipt_scene_plan.h — everything ipt_upload_scene decides about a scene, with
// no HIP runtime call: validation, the host images of the scene's device
// buffers and every scene-dependent KParams scalar. ipt_upload_scene
// (ipt_kernels.hip) puts the plan on the device; a plain host program can run
// it too (tests/native/scene_plan_dump.cpp, under the host sanitizers).
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <vector>

#include "ipt_kparams.h"

namespace {

// The draw word w's u01(w) = (w >> 8) 2^-24 is below c exactly when w >> 8 <
// T = ceil(c 2^24) (both sides exact: an integer against c scaled by a power
// of two), i.e. when w < T << 8: T = 0 for c <= 0 or NaN (never), 2^24 for
// c >= 1 (always, as a 64-bit bound).
inline unsigned long long word_threshold(float c) {
    const double x = (double)c * 16777216.0;
    if (!(x > 0.0)) return 0ull;
    if (x >= 16777216.0) return 1ull << 32;
    return (unsigned long long)std::ceil(x) << 8;
}

// the creation-time settings of the context that the plan reads
struct PlanSettings {
    bool lnodes_lds;     // stage the light BVH in LDS (IPT_LNODES_LDS=0: global memory)
    bool light_grid_on;  // coplanar light lattices by cell lookup (IPT_LIGHT_GRID=0: the light BVH)
};

struct ScenePlan {
    // every KParams field that depends only on the scene and on PlanSettings;
    // every pointer null (ipt_upload_scene sets them), what the scene does not
    // use zero
    KParams kp{};
    // host images of the scene's device buffers; an empty vector: no buffer
    // (grid_c4: [items] centre/radius, then [items] original indices; cdf_lo:
    // none when a bucket is crowded)
    std::vector<LightDev> lights;  // max(n_lights, 1)
    std::vector<float> weights, cdf;  // n_lights + 1
    Frame wall[5];
    std::vector<float4> spheres, grid_c4;  // spheres: max(n_spheres, 1)
    std::vector<int> grid_start, lgrid, cdf_lo;
    std::vector<BvhSphere> grid_items, bvh_prims;
    std::vector<BvhNode> bvh_nodes, light_nodes;
    std::vector<LightAx> lax;
    // what selects the path-kernel instance and is no kernel parameter
    bool any_round_light = false;
    int light_axis = 0;     // axis_aligned_light() of a single AreaLight (kLightsOneA10/A01)
    int light_pattern = 0;  // LightGrid::pattern != 0: coplanar light lattice (kLightsGridA10/A01)
};

// IPT_OK, or the IPT_E_* code with its message in err (out is then unspecified)
inline int plan_scene(const ipt_scene* s, const PlanSettings& set, ScenePlan& out, std::string& err) {
    auto fail = [&err](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!s) return fail(IPT_E_INVALID, "scene is NULL");
    if (s->geometry_kind < IPT_GEOM_SPHERE_IN_BOX || s->geometry_kind > IPT_GEOM_SMALLPT)
        return fail(IPT_E_UNSUPPORTED, "unknown geometry_kind");
    if (s->n_lights < 0 || s->n_lights > kMaxLights || (s->n_lights > 0 && !s->lights))
        return fail(IPT_E_UNSUPPORTED, "n_lights out of range");
    if (s->n_spheres < 0 || (s->n_spheres > 0 && !s->spheres))
        return fail(IPT_E_INVALID, "bad sphere array");
    out = ScenePlan{};
    KParams& k = out.kp;
    const int nl = s->n_lights;
    std::vector<LightDev>& L = out.lights;
    L.resize(std::max(nl, 1));
    std::vector<float> powers(std::max(nl, 1));
    bool any_round = false;
    for (int i = 0; i < nl; ++i) {
        const ipt_area_light& a = s->lights[i];
        if (a.type < IPT_LIGHT_AREA_DIAMOND || a.type > IPT_LIGHT_OUTER_SPHERE)
            return fail(IPT_E_UNSUPPORTED, "unknown light type");
        if (a.type >= IPT_LIGHT_SPHERE) any_round = true;
        L[i] = make_light(v3(a.position[0], a.position[1], a.position[2]),
                          v3(a.x_axis[0], a.x_axis[1], a.x_axis[2]),
                          v3(a.y_axis[0], a.y_axis[1], a.y_axis[2]), a.power, a.type);
        powers[i] = a.power;
    }
    std::vector<float>& wts = out.weights;
    std::vector<float>& cdf = out.cdf;
    wts.resize(nl + 1);
    cdf.resize(nl + 1);
    mixture_weights(powers.data(), nl, wts.data());
    float acc = 0.0f;
    for (int i = 0; i <= nl; ++i) {
        acc += wts[i];  // UnionDdf::sample's running sum (ddf.cpp:145-146)
        cdf[i] = acc;
    }
    // plane frames, indexed by the plane primitive the geometry trace returns:
    // box: RotateDdf(CosineDdf, -plane) for planes {+x,+y,+z,-x,-z};
    // corner: RotateDdf(CosineDdf, n) for n = +x, +y, +z (GeometryCorner.cpp:16-28);
    // floor: its unrotated CosineDdf == make_frame((0,0,1)), which is exactly
    // the identity (axis falls back to +x, angle acos(1) = 0, sin 0 = 0, cos 0 = 1)
    const vec3 planes[5] = {v3(1, 0, 0), v3(0, 1, 0), v3(0, 0, 1), v3(-1, 0, 0), v3(0, 0, -1)};
    Frame* wall = out.wall;
    for (int i = 0; i < 5; ++i) wall[i] = make_frame(-planes[i]);
    if (s->geometry_kind == IPT_GEOM_CORNER)
        for (int i = 0; i < 3; ++i) wall[i] = make_frame(planes[i]);
    if (s->geometry_kind == IPT_GEOM_FLOOR) wall[0] = make_frame(v3(0, 0, 1));
    std::vector<float4>& sph = out.spheres;
    sph.resize(std::max(s->n_spheres, 1));
    for (int i = 0; i < s->n_spheres; ++i)
        sph[i] = make_float4(s->spheres[i].center[0], s->spheres[i].center[1], s->spheres[i].center[2], s->spheres[i].radius);
    // Bound of every surface point a ray can start from: the box [-1,1]^3 and
    // the spheres (ipt_bvh.h pads item boxes from it and the camera).
    float B = 1.0f;
    for (int i = 0; i < s->n_spheres; ++i)
        B = std::max(B, std::max(std::fabs(sph[i].x), std::max(std::fabs(sph[i].y), std::fabs(sph[i].z))) +
                            std::fabs(sph[i].w));
    const float cam[3] = {s->camera.position[0], s->camera.position[1], s->camera.position[2]};
    std::vector<BvhNode>& bnodes = out.bvh_nodes;
    std::vector<BvhSphere>& bprims = out.bvh_prims;
    int per_order = 0;
    float tmargin = 0.0f;
    // many spheres inside the box: a uniform grid; otherwise (and if the grid
    // cannot be built) the BVH
    SphereGrid grid;
    bool use_grid = s->geometry_kind == IPT_GEOM_SPHERES_IN_BOX && s->n_spheres > 256 &&
                    grid_build_spheres(reinterpret_cast<const float*>(sph.data()), s->n_spheres, cam, B, grid);
    if (!use_grid && (s->geometry_kind == IPT_GEOM_SPHERES_IN_BOX || s->geometry_kind == IPT_GEOM_SPHERES) &&
        s->n_spheres > 16)
        bvh_build_spheres(reinterpret_cast<const float*>(sph.data()), s->n_spheres, cam, B, bnodes, bprims,
                          &per_order, &tmargin);
    // light BVH: only for the global-memory light mode (n_lights > kLdsLights)
    std::vector<BvhNode>& lnodes = out.light_nodes;
    int n_lnodes = 0;
    if (nl > kLdsLights && !any_round) {  // the light BVH indexes AreaLights only
        std::vector<std::array<float, 3>> lp(nl), lx(nl), ly(nl);
        std::vector<std::array<float, 9>> li(nl);
        for (int i = 0; i < nl; ++i) {
            lp[i] = {L[i].P.x, L[i].P.y, L[i].P.z};
            lx[i] = {L[i].x.x, L[i].x.y, L[i].x.z};
            ly[i] = {L[i].y.x, L[i].y.y, L[i].y.z};
            for (int c = 0; c < 3; ++c) {
                li[i][3 * c + 0] = L[i].inv.c[c].x;
                li[i][3 * c + 1] = L[i].inv.c[c].y;
                li[i][3 * c + 2] = L[i].inv.c[c].z;
            }
        }
        if (!bvh_build_lights(nl, reinterpret_cast<const float(*)[3]>(lp.data()),
                              reinterpret_cast<const float(*)[3]>(lx.data()),
                              reinterpret_cast<const float(*)[3]>(ly.data()),
                              reinterpret_cast<const float(*)[9]>(li.data()), cam, B, lnodes, &n_lnodes)) {
            lnodes.clear();
            n_lnodes = 0;
        }
    }
    LightGrid lg;
    const bool use_lgrid = set.light_grid_on && nl > kLdsLights && !any_round &&
                           s->geometry_kind == IPT_GEOM_SPHERE_IN_BOX && light_grid_build(L.data(), nl, lg);
    // (the lattice instances take the range-free light arithmetic: every
    // light's ranges proven as for the single light)
    bool lg_inr = use_lgrid;
    for (int i = 0; lg_inr && i < nl; ++i) lg_inr = light_ranges_box(L[i], 2, cam);
    if (!use_lgrid || !lg_inr) lg = LightGrid{};
    // bucket starts of the pick's scan: lo[b] = first c with cdf[c] > b/256
    // (the float compare the scan makes; nl+1 if none); kept when no bucket
    // spans more than 8 entries
    std::vector<int>& cdf_lo = out.cdf_lo;
    cdf_lo.resize(kCdfBuckets);
    bool use_cdf_lo = nl > kLdsLights && !any_round;
    for (int b = 0; use_cdf_lo && b < kCdfBuckets; ++b) {
        const float start = (float)b / (float)kCdfBuckets;
        int c = 0;
        while (c <= nl && !(start < cdf[c])) ++c;
        cdf_lo[b] = c;
        const float end = (float)(b + 1) / (float)kCdfBuckets;
        int e = c;
        while (e <= nl && !(end < cdf[e])) ++e;
        if (e - c > 8) use_cdf_lo = false;
    }
    if (!use_cdf_lo) cdf_lo.clear();
    bool cdf_mono = true;
    for (int i = 0; i <= nl; ++i)
        if (!(cdf[i] == cdf[i]) || (i > 0 && !(cdf[i - 1] <= cdf[i]))) cdf_mono = false;
    if (use_grid) {
        out.grid_start = std::move(grid.start);
        out.grid_items = std::move(grid.items);
        // the wave walk's items: [items] centre/radius, then [items] original indices
        const size_t n_items = out.grid_items.size();
        out.grid_c4.resize(n_items + (n_items + 3) / 4);
        int* idx = reinterpret_cast<int*>(out.grid_c4.data() + n_items);
        for (size_t i = 0; i < n_items; ++i) {
            const BvhSphere& it = out.grid_items[i];
            out.grid_c4[i] = make_float4(it.c[0], it.c[1], it.c[2], it.r);
            idx[i] = it.index;
        }
    }
    if (lg.pattern) {
        out.lgrid = lg.cells;
        for (int i = 0; i < nl; ++i) out.lax.push_back(light_ax_record(L[i], lg.pattern, wts[i]));
    }
    k.geometry_kind = s->geometry_kind;
    k.n_lights = nl;
    const ipt_camera& c = s->camera;
    k.cam_pos = v3(c.position[0], c.position[1], c.position[2]);
    k.cam_dir = v3(c.direction[0], c.direction[1], c.direction[2]);
    k.cam_right = v3(c.right[0], c.right[1], c.right[2]);
    k.cam_up = v3(c.up[0], c.up[1], c.up[2]);
    k.n_spheres = s->n_spheres;
    if (use_grid) {
        k.n_grid = (int)(out.grid_start.size() - 1);
        k.bvh_tmargin = grid.tmargin;
        for (int a = 0; a < 3; ++a) {
            k.grid_g0[a] = grid.g0[a];
            k.grid_h[a] = grid.h[a];
            k.grid_inv_h[a] = grid.inv_h[a];
            k.grid_n[a] = grid.n[a];
            k.grid_g1[a] = grid.g0[a] + (float)grid.n[a] * grid.h[a];
        }
        k.grid_m = grid.m;
    }
    if (!bnodes.empty()) {
        k.n_nodes = per_order;  // nodes per octant order; buffer holds kBvhOrders of them
        k.bvh_tmargin = tmargin;
    }
    k.n_light_nodes = lnodes.empty() ? 0 : n_lnodes;
    // light BVH staged in LDS (IPT_LNODES_LDS=0 at ipt_create keeps it in
    // global memory): the resumable light walk runs at 3 workgroups/CU, which
    // the extra LDS keeps, and gains 10 % on C5 (43.8 vs 40.2 Mpaths/s)
    k.lnodes_lds = (set.lnodes_lds && k.n_light_nodes > 0 && k.n_light_nodes <= kLdsLightNodesMax) ? 1 : 0;
    out.light_pattern = lg.pattern;
    k.lg_nu = lg.nu;
    k.lg_nv = lg.nv;
    k.lg_u0 = lg.u0;
    k.lg_v0 = lg.v0;
    k.lg_icw = lg.icw;
    k.lg_ich = lg.ich;
    k.lg_e = lg.e;
    k.lg_pn = lg.pn;
    k.lg_nn = lg.nn;
    k.cdf_bsearch = cdf_mono ? 1 : 0;
    k.pk_u0 = word_threshold(cdf[0]);
    k.pk_u1 = word_threshold(nl >= 1 ? cdf[1] : 0.0f);
    // cdf[nl]'s threshold in every scene: the lattice instances' pre-skip
    // compares the next pick word with it in every step (pre_ft), also where
    // no leaf is taken (cdf_p2 == 0) -- there a taken word picks a light, below
    // cdf[nl - 1] <= cdf[nl], and must read as three draws
    k.cdf_end_t = (uint32_t)(word_threshold(cdf[nl]) >> 8);
    // nearly equal lights (e.g. 256 of one power: weights within rounding of
    // 0.5/256 = 2^-9): with w = 2^-e and every light's |cdf[i] - (i+1) w| <= d
    // < w/2 on a non-decreasing cdf, the first c with r < cdf[c] is ce - 1, ce
    // or ce + 1 for ce = floor(r/w) = floor(r 2^e) (exact: r = m 2^-24): cdf[ce-2]
    // <= (ce-1) w + d < ce w <= r and cdf[ce+1] >= (ce+2) w - d > r + w - d > r.
    // Past the lights (ce >= nl) the scan's answer is ce's clamp to nl - 1, then
    // cdf[nl]. The kernel reads cdf[ce-1] and cdf[ce] only.
    for (int e = 1; cdf_mono && nl > kLdsLights && !any_round && e <= 20 && !k.cdf_p2; ++e) {
        const double w = std::ldexp(1.0, -e);
        bool ok = (double)nl * w <= 1.0;
        for (int i = 0; ok && i < nl; ++i) ok = std::fabs((double)cdf[i] - (double)(i + 1) * w) < 0.25 * w;
        if (!ok) continue;
        k.cdf_p2 = 1;
        k.cdf_p2e = e;
        // exactly uniform on the draw's 24-bit integer: every light's
        // ceil(cdf[i] 2^24) is (i+1) 2^(24-e) (C5's 256 equal emitters),
        // so the integer pick reads no cdf entry at all (KParams::cdf_p2 2)
        bool exact = true;
        for (int i = 0; exact && i < nl; ++i)
            exact = (word_threshold(cdf[i]) >> 8) == ((unsigned long long)(i + 1) << (24 - e));
        if (exact) k.cdf_p2 = 2;
    }
    out.any_round_light = any_round;
    // the axis-aligned single-light instances also take the range-free roots
    // and quotients: only where their ranges are proven (sphere-in-box scenes)
    out.light_axis = (nl == 1 && !any_round) ? axis_aligned_light(L[0]) : 0;
    if (out.light_axis && !(s->geometry_kind == IPT_GEOM_SPHERE_IN_BOX && light_ranges_box(L[0], 2, cam)))
        out.light_axis = 0;
    // skip-ahead plane: one area light (or a lattice, whose lights share P.z
    // and n.z bit for bit) whose axes have zero z components, so that every
    // sampled point (x*u1 + y*u2) + P has z = P.z exactly, and whose normal is
    // (+-0, +-0, n.z): a light sample's cosinus then has the sign of
    // n.z * (o.z - P.z) whatever the draws (lighting.cpp:93-104, 125-134)
    {
        auto zero = [](float f) { return (f2u(f) & 0x7fffffffu) == 0u; };
        bool ok = nl >= 1 && !any_round && (nl == 1 || lg.pattern != 0);
        for (int i = 0; ok && i < nl; ++i)
            ok = (L[i].type == 0 || L[i].type == 1) && zero(L[i].x.z) && zero(L[i].y.z) && zero(L[i].n.x) &&
                 zero(L[i].n.y) && !zero(L[i].n.z) && std::isfinite(L[i].n.z) && std::fabs(L[i].P.z) >= 0x1p-32f &&
                 std::fabs(L[i].P.z) <= 0x1p32f &&
                 f2u(L[i].P.z) == f2u(L[0].P.z) && f2u(L[i].n.z) == f2u(L[0].n.z);
        float sa_cl = 0.0f;
        if (ok) {
            k.sa_on = 1;
            k.sa_pz = L[0].P.z;
            k.sa_nz = L[0].n.z;
            // UnionDdf::sample picks a light (c < nl) iff r < cdf[c] for some
            // c < nl, i.e. iff r < cdf[nl - 1] on a non-decreasing cdf
            sa_cl = (nl == 1 || cdf_mono) ? cdf[nl - 1] : 0.0f;
        }
        k.sa_u = word_threshold(sa_cl);
    }
    // the product FIXED = kTreeK instances' fact (select_path4): no draw word
    // falls through the pick
    k.no_fallthrough = word_threshold(cdf[nl]) == 1ull << 32 ? 1 : 0;
    // every ray origin (camera, surface points within B) inside 2^39: the box
    // planes may use the range-free division (box_plane_t<true>)
    const float lim = 549755813888.0f;  // 2^39
    k.box_inrange = B < lim && std::fabs(cam[0]) < lim && std::fabs(cam[1]) < lim && std::fabs(cam[2]) < lim;
    return IPT_OK;
}

}  // namespace
