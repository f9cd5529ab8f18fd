// The library's host-only scene plan and instance selector on a scene given as
// text: plan_scene (ipt_scene_plan.h) and select_path (ipt_select.h), the code
// ipt_upload_scene and launch_path run, here without a device and without a
// HIP runtime call (tests/test_scene_plan_cpu.py builds it with the host
// sanitizers).
// stdin: geometry_kind; the camera's 12 floats (position, direction, right,
// up); n_lights, then per light "px py pz xx xy xz yx yy yz power type" (as
// light_grid_check.cpp reads them); n_spheres, then per sphere "cx cy cz r".
// argv: n_rays depth_max box_generic lattice_lds max_lds light_grid_on lnodes_lds.
// Prints "name value" pairs, inst0 / inst1 (the instance without and with
// IPT_FLAG_COUNTERS) as six integers each. A plan error prints
// "error <code> <message>" and exits with status 3; bad input exits with 2.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../ipt_amd/csrc/ipt_scene_plan.h"
#include "../../ipt_amd/csrc/ipt_select.h"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    ipt_params p{};
    p.n_rays = std::atoi(argv[1]);
    p.depth_max = std::atoi(argv[2]);
    const bool box_generic = std::atoi(argv[3]) != 0, lattice_lds = std::atoi(argv[4]) != 0;
    const size_t max_lds = (size_t)std::atoll(argv[5]);
    const PlanSettings set{std::atoi(argv[7]) != 0, std::atoi(argv[6]) != 0};

    ipt_scene s{};
    if (std::scanf("%d", &s.geometry_kind) != 1) return 2;
    float* cam[4] = {s.camera.position, s.camera.direction, s.camera.right, s.camera.up};
    for (float* v : cam)
        for (int i = 0; i < 3; ++i)
            if (std::scanf("%f", &v[i]) != 1) return 2;
    if (std::scanf("%d", &s.n_lights) != 1 || s.n_lights < 0 || s.n_lights > (1 << 20)) return 2;
    std::vector<ipt_area_light> lights(s.n_lights);
    for (ipt_area_light& a : lights) {
        float v[11];
        for (float& f : v)
            if (std::scanf("%f", &f) != 1) return 2;
        for (int i = 0; i < 3; ++i) {
            a.position[i] = v[i];
            a.x_axis[i] = v[3 + i];
            a.y_axis[i] = v[6 + i];
        }
        a.power = v[9];
        a.type = (int)v[10];
    }
    if (std::scanf("%d", &s.n_spheres) != 1 || s.n_spheres < 0 || s.n_spheres > (1 << 24)) return 2;
    std::vector<ipt_sphere> spheres(s.n_spheres);
    for (ipt_sphere& q : spheres)
        if (std::scanf("%f %f %f %f", &q.center[0], &q.center[1], &q.center[2], &q.radius) != 4) return 2;
    s.lights = lights.data();
    s.spheres = spheres.data();

    ScenePlan plan;
    std::string err;
    if (const int rc = plan_scene(&s, set, plan, err)) {
        std::printf("error %d %s\n", rc, err.c_str());
        return 3;
    }
    const KParams& k = plan.kp;
    std::printf("any_round %d\nlight_axis %d\nlight_pattern %d\nsa_on %d\nbox_inrange %d\n", plan.any_round_light ? 1 : 0,
                plan.light_axis, plan.light_pattern, k.sa_on, k.box_inrange);
    std::printf("n_grid %d\nn_nodes %d\nn_light_nodes %d\nlnodes_lds %d\nlg_nu %d\nlg_nv %d\n", k.n_grid, k.n_nodes,
                k.n_light_nodes, k.lnodes_lds, k.lg_nu, k.lg_nv);
    std::printf("cdf_p2 %d\ncdf_bsearch %d\nhas_cdf_lo %d\n", k.cdf_p2, k.cdf_bsearch, plan.cdf_lo.empty() ? 0 : 1);
    // the buffers ipt_upload_scene allocates: the non-empty images and the wall frames
    const size_t sizes[13] = {plan.lights.size(),     plan.weights.size(),   plan.cdf.size(),       plan.spheres.size(),
                              plan.grid_c4.size(),    plan.grid_start.size(), plan.lgrid.size(),     plan.cdf_lo.size(),
                              plan.grid_items.size(), plan.bvh_prims.size(), plan.bvh_nodes.size(), plan.light_nodes.size(),
                              plan.lax.size()};
    int n_bufs = 1;
    for (size_t n : sizes) n_bufs += n != 0;
    std::printf("n_bufs %d\n", n_bufs);

    KParams kp = k;  // the launch's: launch_params adds n_rays and depth_max to the scene's fields
    kp.n_rays = p.n_rays;
    kp.depth_max = p.depth_max;
    for (int count = 0; count < 2; ++count) {
        const SelectIn in{kp, needed_susp(&p), count != 0, plan.any_round_light, plan.light_axis, plan.light_pattern,
                          box_generic, lattice_lds, max_lds};
        int inst[6] = {0, 0, 0, 0, 0, 0};
        const int rc = select_path(in, [&](auto ms, auto cnt, auto lm, auto g, auto boxin, auto fixed) {
            const int key[6] = {decltype(ms)::value, decltype(cnt)::value ? 1 : 0,   decltype(lm)::value,
                                decltype(g)::value,  decltype(boxin)::value ? 1 : 0, decltype(fixed)::value};
            for (int i = 0; i < 6; ++i) inst[i] = key[i];
            return IPT_OK;
        });
        if (rc) return 2;
        std::printf("inst%d %d %d %d %d %d %d\n", count, inst[0], inst[1], inst[2], inst[3], inst[4], inst[5]);
    }
    return 0;
}
