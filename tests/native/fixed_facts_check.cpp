// The scene fact of the product FIXED = K box instances by the
// library's own host code, plan_scene (ipt_scene_plan.h) and select_path
// (ipt_select.h), with no device (tests/test_fixed_facts_host.py builds it with
// the host sanitizers and runs it).
//
//   plan NR DM LDS  the scene on stdin, LDS the lattice_lds setting: the plan's
//             no_fallthrough, whether pk_u0 is a 32-bit word, the bits of the
//             skip-ahead plane's n.z, how many of the 2^24 draw values fall
//             through the pick, the launch's LMODE and the selector's FIXED
//             for n_rays NR, depth_max DM without and with the counting flag;
//             then the same launch with the fact forced on and off and with
//             pk_u0 forced to 2^32: tree_on / tree_off / tree_wide are whether
//             FIXED is kTreeK then.
// Scene text as tests/native/scene_plan_dump.cpp reads it. Exit status 2 on bad
// input.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ipt_amd/csrc/ipt_scene_plan.h"
#include "../../ipt_amd/csrc/ipt_select.h"

static bool read_scene(ipt_scene& s, std::vector<ipt_area_light>& lights, std::vector<ipt_sphere>& spheres) {
    if (std::scanf("%d", &s.geometry_kind) != 1) return false;
    float* cam[4] = {s.camera.position, s.camera.direction, s.camera.right, s.camera.up};
    for (float* v : cam)
        for (int i = 0; i < 3; ++i)
            if (std::scanf("%f", &v[i]) != 1) return false;
    if (std::scanf("%d", &s.n_lights) != 1 || s.n_lights < 0 || s.n_lights > (1 << 20)) return false;
    lights.resize(s.n_lights);
    for (ipt_area_light& a : lights) {
        float v[11];
        for (float& f : v)
            if (std::scanf("%f", &f) != 1) return false;
        for (int i = 0; i < 3; ++i) {
            a.position[i] = v[i];
            a.x_axis[i] = v[3 + i];
            a.y_axis[i] = v[6 + i];
        }
        a.power = v[9];
        a.type = (int)v[10];
    }
    if (std::scanf("%d", &s.n_spheres) != 1 || s.n_spheres < 0 || s.n_spheres > (1 << 24)) return false;
    spheres.resize(s.n_spheres);
    for (ipt_sphere& q : spheres)
        if (std::scanf("%f %f %f %f", &q.center[0], &q.center[1], &q.center[2], &q.radius) != 4) return false;
    s.lights = lights.data();
    s.spheres = spheres.data();
    return true;
}

static int plan_mode(int n_rays, int depth_max, bool lattice_lds) {
    ipt_scene s{};
    std::vector<ipt_area_light> lights;
    std::vector<ipt_sphere> spheres;
    if (!read_scene(s, lights, spheres)) return 2;
    ScenePlan plan;
    std::string err;
    if (const int rc = plan_scene(&s, PlanSettings{true, true}, plan, err)) {
        std::printf("error %d %s\n", rc, err.c_str());
        return 2;
    }
    ipt_params p{};
    p.n_rays = n_rays;
    p.depth_max = depth_max;
    KParams kp = plan.kp;
    kp.n_rays = n_rays;
    kp.depth_max = depth_max;
    std::printf("no_fallthrough %d\npick32 %d\nsa_on %d\nn_lights %d\n", kp.no_fallthrough,
                (kp.pk_u0 >> 32) == 0ull ? 1 : 0, kp.sa_on, kp.n_lights);
    // the bits of the plane's n.z, and how many of the 2^24 draw values fall through the pick
    std::printf("sa_nz_bits %u\nfallthrough_values %u\n", f2u(kp.sa_nz), (1u << 24) - kp.cdf_end_t);
    int lmode = 0;
    auto fixed_of = [&](const KParams& k, bool count) {
        const SelectIn in{k, needed_susp(&p), count, plan.any_round_light, plan.light_axis, plan.light_pattern,
                          false, lattice_lds, (size_t)160 * 1024};
        int fixed = -99;
        const int rc = select_path(in, [&](auto, auto, auto lm, auto, auto, auto fx) {
            fixed = decltype(fx)::value;
            lmode = decltype(lm)::value;
            return IPT_OK;
        });
        return rc ? -98 : fixed;
    };
    std::printf("fixed0 %d\n", fixed_of(kp, false));
    std::printf("fixed1 %d\n", fixed_of(kp, true));
    std::printf("lmode %d\n", lmode);
    // the same launch with the fact forced on and off, and with a pick threshold of 2^32
    // (cdf[0] >= 1, a certain light pick); the counting flag must not change the answer
    KParams on = kp, off = kp, wide = kp;
    on.no_fallthrough = 1;
    on.pk_u0 &= 0xffffffffull;
    off.no_fallthrough = 0;
    wide.no_fallthrough = 1;
    wide.pk_u0 = 1ull << 32;
    const KParams* forced[3] = {&on, &off, &wide};
    const char* names[3] = {"tree_on", "tree_off", "tree_wide"};
    int differ = 0;
    for (int i = 0; i < 3; ++i) {
        const int f0 = fixed_of(*forced[i], false), f1 = fixed_of(*forced[i], true);
        differ += f0 != f1;
        std::printf("%s %d\n", names[i], f0 == kTreeK ? 1 : 0);
    }
    std::printf("count_differs %d\n", differ);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "plan"))
        return plan_mode(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) != 0);
    return 2;
}
