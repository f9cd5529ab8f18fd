// ipt_select.h — which path_kernel<MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED>
// instance a launch takes. Host only, no HIP runtime call: the library's
// launch (launch_path, ipt_kernels.hip) passes a functor that launches the
// instance, tests/native/scene_plan_dump.cpp one that records its key.
#pragma once

#include <type_traits>

#include "ipt_kparams.h"

namespace {

// Number of suspended stack levels the DFS can need.
inline int needed_susp(const ipt_params* p) {
    // a node at depth d is pushed iff d < depth_max and (n_rays >> d) > 0
    int maxpush = -1;
    for (int d = 0; d < p->depth_max; ++d)
        if ((p->n_rays >> d) > 0) maxpush = d;
    return maxpush < 0 ? 0 : maxpush;  // suspended levels = depth of deepest pushed node
}

// dynamic LDS bytes of a path-kernel instance (the layout at the top of path_kernel)
template <int MAXSUSP, int LMODE, int GEOM>
size_t path_lds_bytes(const KParams& kp) {
    constexpr int kBlock = block_of(LMODE, GEOM);
    const size_t cells = (size_t)kp.lg_nu * kp.lg_nv;
    return ((size_t)MAXSUSP * kStackFields * kBlock + scene_lds_words(LMODE, GEOM) +
            (LMODE == kLightsGlobal ? global_light_lds_words(kp.n_lights, kp.lnodes_lds ? kp.n_light_nodes : 0) : 0) +
            (grid_lights(LMODE) ? global_light_lds_words(kp.n_lights, 0, true) +
                                      (lax_in_lds(LMODE) ? ((cells + 3) & ~(size_t)3) + 12 * (size_t)kp.n_lights : cells)
                                : 0)) *
           sizeof(float);
}

// What the selector reads: the launch's KParams (the scene's fields with
// n_rays and depth_max), its stack depth (needed_susp) and counting flag, the
// scene's facts that are no kernel parameter (ScenePlan, ipt_scene_plan.h) and
// the context's creation-time settings. (The FIXED = kTreeK instances'
// scene fact rides in kp.no_fallthrough, a field no kernel reads.)
struct SelectIn {
    const KParams& kp;
    int susp;
    bool count, any_round_light;
    int light_axis, light_pattern;
    bool box_generic, lattice_lds;  // IPT_BOX_GENERIC=1, IPT_LATTICE_LDS != 0
    size_t max_lds;                 // the device's LDS per workgroup
};
template <int V>
using int_c = std::integral_constant<int, V>;
template <bool V>
using bool_c = std::integral_constant<bool, V>;

// select_path(in, f) returns f(int_c<MAXSUSP>, bool_c<COUNT>, int_c<LMODE>,
// int_c<GEOM>, bool_c<BOXIN>, int_c<FIXED>) of the launch's instance; every
// call of f below names an instance of the build.

// the box instances' range form (path_kernel's BOXIN): in range unless the
// scene is not (box_inrange) or IPT_BOX_GENERIC=1 forces the generic instance;
// and, in range, the instance with the step's per-launch choices fixed (FIXED)
// where the launch has them: n_rays a power of two, a skip-ahead plane
template <int MAXSUSP, bool COUNT, int LMODE, int GEOM, class F>
int select_path4(const SelectIn& in, F&& f) {
    const KParams& kp = in.kp;
    constexpr int_c<MAXSUSP> ms{};
    constexpr bool_c<COUNT> cnt{};
    constexpr int_c<LMODE> lm{};
    constexpr int_c<GEOM> g{};
    if constexpr (GEOM == IPT_GEOM_SPHERE_IN_BOX) {
        if (kp.box_inrange && !in.box_generic) {
            if constexpr (step_fixed_mode(LMODE)) {
                const uint32_t nr = (uint32_t)kp.n_rays;
                if (kp.sa_on && nr != 0u && (nr & (nr - 1u)) == 0u) {
                    // the tree shape as well: n_rays == 2^K and depth_max > K + 1 (then
                    // the stack has K levels: the 4-level instances), and, in the
                    // instances compiled for it, no fall-through pick
                    // (kp.no_fallthrough, from plan_scene; one light: its pick
                    // threshold a 32-bit word as well, i.e. cdf[0] < 1)
                    if constexpr (MAXSUSP == kTreeK)
                        if (nr == (1u << kTreeK) && kp.depth_max > kTreeK + 1 &&
                            (!no_fallthrough_mode(LMODE) ||
                             (kp.no_fallthrough != 0 && (!one_light(LMODE) || (kp.pk_u0 >> 32) == 0ull))))
                            return f(ms, cnt, lm, g, bool_c<true>{}, int_c<kTreeK>{});
                    return f(ms, cnt, lm, g, bool_c<true>{}, int_c<kFixedPow2>{});
                }
            }
            return f(ms, cnt, lm, g, bool_c<true>{}, int_c<0>{});
        }
    }
    return f(ms, cnt, lm, g, bool_c<false>{}, int_c<0>{});
}
// -DIPT_AB_BUILD -DIPT_C2_ONLY=1: experiment builds (scripts/variants.sh)
// instantiate the sample_scenes[0] kernel alone (ipt_knobs.h); every other
// launch is IPT_E_UNSUPPORTED, and f is not called.
template <int MAXSUSP, bool COUNT, int LMODE, class F>
int select_path3(const SelectIn& in, F&& f) {
    const KParams& kp = in.kp;
    if constexpr (IPT_C2_ONLY != 0) {
        if (MAXSUSP != 4 || LMODE != IPT_C2_LMODE || kp.geometry_kind != IPT_GEOM_SPHERE_IN_BOX)
            return IPT_E_UNSUPPORTED;
        return select_path4<4, COUNT, IPT_C2_LMODE, IPT_GEOM_SPHERE_IN_BOX>(in, f);
    } else {
    switch (kp.geometry_kind) {
        case IPT_GEOM_SPHERES_IN_BOX: return select_path4<MAXSUSP, COUNT, LMODE, IPT_GEOM_SPHERES_IN_BOX>(in, f);
        case IPT_GEOM_FLOOR: return select_path4<MAXSUSP, COUNT, LMODE, IPT_GEOM_FLOOR>(in, f);
        case IPT_GEOM_CORNER: return select_path4<MAXSUSP, COUNT, LMODE, IPT_GEOM_CORNER>(in, f);
        case IPT_GEOM_SPHERES: return select_path4<MAXSUSP, COUNT, LMODE, IPT_GEOM_SPHERES>(in, f);
        case IPT_GEOM_SMALLPT: return select_path4<MAXSUSP, COUNT, LMODE, IPT_GEOM_SMALLPT>(in, f);
        default: return select_path4<MAXSUSP, COUNT, LMODE, IPT_GEOM_SPHERE_IN_BOX>(in, f);
    }
    }
}
template <int MAXSUSP, bool COUNT, class F>
int select_path2(const SelectIn& in, F&& f) {
    const KParams& kp = in.kp;
    if (in.any_round_light) return select_path3<MAXSUSP, COUNT, kLightsAny>(in, f);
    if (kp.n_lights == 1) {
        if (in.light_axis == 1) return select_path3<MAXSUSP, COUNT, kLightsOneA10>(in, f);
        if (in.light_axis == 2) return select_path3<MAXSUSP, COUNT, kLightsOneA01>(in, f);
        return select_path3<MAXSUSP, COUNT, kLightsOne>(in, f);
    }
    if (kp.n_lights <= kLdsLights) return select_path3<MAXSUSP, COUNT, kLightsLds>(in, f);
    if constexpr (IPT_C2_ONLY == 0) {
        // (the lattice is only built for sphere-in-box scenes)
        // the records-in-LDS instance wherever its LDS fits one workgroup per CU
        constexpr int G = IPT_GEOM_SPHERE_IN_BOX;
        if (in.light_pattern == 1 && kp.geometry_kind == G) {
            if (in.lattice_lds && path_lds_bytes<MAXSUSP, kLightsGridA10L, G>(kp) <= in.max_lds)
                return select_path4<MAXSUSP, COUNT, kLightsGridA10L, G>(in, f);
            return select_path4<MAXSUSP, COUNT, kLightsGridA10, G>(in, f);
        }
        if (in.light_pattern == 2 && kp.geometry_kind == G) {
            if (in.lattice_lds && path_lds_bytes<MAXSUSP, kLightsGridA01L, G>(kp) <= in.max_lds)
                return select_path4<MAXSUSP, COUNT, kLightsGridA01L, G>(in, f);
            return select_path4<MAXSUSP, COUNT, kLightsGridA01, G>(in, f);
        }
    }
    return select_path3<MAXSUSP, COUNT, kLightsGlobal>(in, f);
}
// the instances for the call's stack depth (4 or 8 suspended levels) and counting flag
template <class F>
int select_path(const SelectIn& in, F&& f) {
    if (in.susp <= 4) return in.count ? select_path2<4, true>(in, f) : select_path2<4, false>(in, f);
    return in.count ? select_path2<8, true>(in, f) : select_path2<8, false>(in, f);
}

}  // namespace
