// ipt_kparams.h — the kernels' parameter block (KParams) and the path-kernel
// instances' launch-shape and LDS-layout constants: what the host-only scene
// plan (ipt_scene_plan.h) and instance selector (ipt_select.h) share with the
// kernels of ipt_kernels.hip. No device code and no HIP runtime call: it
// compiles in a plain host program (tests/native/scene_plan_dump.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ipt_capi.h"
#include "ipt_bvh.h"
#include "ipt_path.h"
#include "ipt_knobs.h"
#include "ipt_diag.h"

using namespace ipt;

namespace {

constexpr int kBlock = IPT_BLOCK;  // threads per workgroup (4 waves; ipt_knobs.h)
constexpr int kStackFields = 6;   // pos3, res, mult, meta(i | kind<<8)

// Unread fields: the fields marked (unread) below lost their last reader when
// the build switches that selected their code were retired; the host leaves
// them zero. They keep their places because KParams' layout decides how the
// compiler groups the kernel-argument loads: taking any of them out regroups
// those loads in some kernel and changes its register assignment or its
// instruction count (DESIGN.md §9 has the counts per field group). Removing
// them is a change of device code, to be measured as one.
struct KParams {
    int W, H, spp, spp_offset, n_rays, depth_max;
    int meta_shift;  // a suspended level's meta word: ti | kind << meta_shift (8, or 16 for n_rays > 255)
    uint32_t key0, key1;
    int n_cand;              // candidate source rows
    const int* __restrict__ cand_rows;    // [n_cand] source row index
    int tile_rows, n_shards, shard_id;
    unsigned long long total_units;
    unsigned long long* unit_counter;
    // the launch's pool-drained flag (signal memory, hipStreamWaitValue64's
    // operand): the wave that takes the last chunk stores drain_seq there
    unsigned long long* drained;
    unsigned long long drain_seq;
#if IPT_RAYLOG
    RayLogRec* raylog;               // [raylog_cap]
    unsigned long long* raylog_n;    // finished traces seen
    unsigned long long raylog_cap;
    unsigned raylog_every;
#endif
    float* __restrict__ values;           // [spp][n_cand][W]
    uint8_t* __restrict__ codes;          // [spp][n_cand][W]
    uint8_t* __restrict__ flags;          // [H][W]
    unsigned long long* counters;
    int geometry_kind;
    int n_lights;
    const LightDev* __restrict__ lights;  // [n_lights]
    const float* __restrict__ weights;    // [n_lights+1]
    const float* __restrict__ cdf;        // [n_lights+1] sequential prefix sums of weights
    const Frame* __restrict__ wall_frames;  // [5]
    vec3 cam_pos, cam_dir, cam_right, cam_up;
    int n_spheres;
    const float4* __restrict__ spheres;   // (c.xyz, r)
    float bvh_tmargin;                    // sphere BVH / grid: additive pruning margin (1e-3 D, ipt_bvh.h)
    int n_grid;                           // > 0: uniform sphere grid (ipt_bvh.h SphereGrid) instead of the BVH
    float grid_g0[3], grid_h[3], grid_inv_h[3], grid_m;
    float grid_g1[3];                     // g0 + (float)n * h, the grid's far corner (host-computed)
    int grid_n[3];
    const int* __restrict__ grid_start;   // [cells + 1]
    // (unread: see the note on unread fields above KParams)
    const int* __restrict__ grid_packed;
    int grid_packed_words, grid_packed_nb;
    const void* __restrict__ grid_cells;
    const BvhSphere* __restrict__ grid_items;
    // the same items packed for the wave walk: centre and radius as one float4
    // per item (16-byte stride: a cell's items share lines), original indices
    // in a separate array
    const float4* __restrict__ grid_c4;
    const int* __restrict__ grid_idx;
    const BvhNode* __restrict__ bvh_nodes;     // n_nodes > 0: sphere BVH (ipt_bvh.h)
    const BvhSphere* __restrict__ bvh_prims;
    int n_nodes;
    const BvhNode* __restrict__ light_nodes;   // n_light_nodes > 0: light BVH over index ranges
    int n_light_nodes;
    int lnodes_lds;                       // light BVH staged in LDS (kLightsGlobal)
    // kLightsGridA10/A01: coplanar axis-aligned lights on a lattice (LightGrid)
    const int* __restrict__ lgrid;        // [lg_nu * lg_nv] light index per cell, -1 = none
    const float4* __restrict__ lax;       // [n_lights][3] LightAx records
    int lg_nu, lg_nv;
    float lg_u0, lg_v0, lg_icw, lg_ich;   // cell coordinates: (q - u0) * icw
    float lg_e;                           // candidate margin in cells (LightGrid::e)
    // skip-ahead (prologue): every light sample's point lies on the plane z =
    // sa_pz and the light normal is (+-0, +-0, sa_nz): light picks at nodes
    // with sa_nz * (sa_pz - z) >= 0 are certain skips (sa_on, host-checked)
    // u01(w) < c  <=>  w < (ceil(c 2^24) << 8) (clamped to [0, 2^32]) for the
    // draw word w: the single light's cdf[0], cdf[1] (pk_u0, pk_u1) and the
    // light-pick bound (sa_u: one light: cdf[0]; a lattice with a non-decreasing
    // cdf: cdf[nl - 1]; else 0, never) as word thresholds (host: word_threshold)
    unsigned long long pk_u0, pk_u1, sa_u;
    int sa_on;
    float sa_pz, sa_nz;
    float sa_cl;                          // (unread)
    float lg_pn, lg_nn;                   // the lights' shared plane: P[na], n[na]
    int cdf_bsearch;                      // cdf non-decreasing: pick by binary search
    // |cdf[i] - (i+1) 2^-e| < 2^-e/2 for every light i and a non-decreasing
    // cdf (host-checked): the pick is floor(r 2^e) - 1, + 0 or + 1 by two cdf
    // entries, then cdf[nl] decides past the lights. It is taken on the draw's
    // 24-bit integer g = w >> 8: floor(r 2^e) = g >> (24 - e) and r < c <=> g <
    // ceil(c 2^24); the staged cdf then holds those integer thresholds
    // (cdf_end_t: cdf[nl]'s)
    int cdf_p2;  // 1: near-uniform as above; 2: every threshold exact, no cdf read
    float cdf_p2s, cdf_end;               // (unread)
    int cdf_p2e;
    uint32_t cdf_end_t;
    // no_fallthrough: word_threshold(cdf[nl]) == 2^32, no draw word falls
    // through the pick (set by plan_scene, read by the selector alone: no kernel
    // reads it; it sits in an unread field's place, so the layout is the same);
    // lc_shift on: (unread)
    int no_fallthrough, lc_shift;
    float lc_x0, lc_y0, lc_dx, lc_dy, lc_ax, lc_ay;
    int ltr_calc, lg_ident;
    float lc_ix, lc_iy, lc_area, lc_spow;
    const int* __restrict__ cdf_lo;       // [kCdfBuckets] or null: first c with cdf[c] > b/256
    double inv_per_pass, inv_w;           // 1/(n_cand*W), 1/W (exact 32-bit unit decomposition)
    uint32_t per_pass32;                  // n_cand*W (< 2^32)
    int box_inrange;                      // camera and sphere list within 2^39 (box_plane_t<true>): the sphere-list
                                          // and preview kernels (the box path instances: BOXIN)
    const float* __restrict__ cos_a;      // [2^24] CosineDdf table by u1's 24 bits: sin(acos(sqrt(u1)))
    const float2* __restrict__ cos_b;     // (unread)
    const float2* __restrict__ frame_sc;  // frame_table_kernel: RotateDdf angle (sin, cos) by to.z
    const uint4* __restrict__ rg;         // [total_units][2] raygen_kernel records
    int count;                            // raygen_kernel: accumulate the drift counter
    int plane;                            // new_path_setup: kPlaneGrid / kPlaneGui (IPT_FLAG_GUI_PLANE)
    // new_path_setup: the caller's sample mask [H][W] by nominal destination
    // pixel, or null (ipt_render_masked_device). Appended: no other field moves,
    // and path_kernel, which never reads it, keeps its instructions
    const uint8_t* __restrict__ mask;
};
// The render plane's index map: GridRenderPlane::addRay's or Gui::addRay's.
enum { kPlaneGrid = 0, kPlaneGui = 1 };

// Scene data staged once per workgroup (never re-read from HBM/L2 inside the
// step loop): wall frames, lights (<= kLdsLights), mixture weights + CDF and
// the candidate-row table live in LDS after the DFS stack.
constexpr int kLdsLights = 16;
constexpr int kLightWords = (int)(sizeof(LightDev) / 4);
// LDS after the DFS stack: frames, [LMODE 2: lights, weights, cdf],
// [sharded: candidate rows], [LMODE 3: weights, cdf, light BVH].
// Frames live in LDS, [12][kFrameStride]: column tid is the lane's current
// sphere-node frame, columns kBlock..kBlock+4 the five wall frames.
// CosineDdf samples come from exact tables (cos_table_kernel).
// Column stride: single-light instances use kBlock + 64 words (a multiple of
// 64 dwords, so a column's 12 words pair into ds_read2st64/ds_write2st64;
// 2.7 KiB more, still 4 workgroups/CU); the others keep kBlock + 8 so that
// their light data fits 4 workgroups as well.
// Threads per workgroup of a path-kernel instance: kBlock, or one 1024-thread
// workgroup per CU for the light lattices with their records in LDS
// (kLightsGridA10L/A01L: the per-lane LDS is the same, the shared tables and
// records are held once per CU instead of once per 256-thread workgroup).
constexpr int kLatticeBlock = 1024;
// Sphere-list instances carry the resumable walk's state (their walks are
// bounded per step and resumed in later steps).
__host__ __device__ constexpr bool resumable_geom(int geom) {
    return geom == IPT_GEOM_SPHERES_IN_BOX || geom == IPT_GEOM_SPHERES;
}
// The sphere-list (resumable) instances run 64-thread workgroups: a persistent
// launch's tail frees a CU slot per finished wave instead of per finished
// 4-wave workgroup, so the next launch fills it sooner (C3 +2.2 %, 16-spp
// progressive calls 0.964 -> 0.985 of one call); C2 keeps 256 (its frame
// columns' ds_read2st64 stride, -1.2 % at 64).
__host__ __device__ constexpr int block_of(int lmode, int geom) {
    return (lmode == 9 || lmode == 10) ? kLatticeBlock : (resumable_geom(geom) ? IPT_RES_BLOCK : kBlock);
}
// the wave-spread grid walk's per-lane LDS: an 8-byte slot
__host__ __device__ constexpr int walk_lds_words(int lmode, int geom) {
    return resumable_geom(geom) ? 2 * block_of(lmode, geom) : 0;
}
__host__ __device__ constexpr int frame_stride(int lmode, int geom) {
    return ((lmode == 1 || lmode == 5 || lmode == 6) && walk_lds_words(lmode, geom) == 0 && block_of(lmode, geom) >= 256)
               ? block_of(lmode, geom) + 64
               : block_of(lmode, geom) + 8;
}
__host__ __device__ constexpr size_t scene_lds_words(int lmode, int geom) {
    return (size_t)walk_lds_words(lmode, geom) + 12 * (size_t)frame_stride(lmode, geom) +
           (lmode == 2 ? (size_t)kLdsLights * kLightWords + 2 * (kLdsLights + 1) : 0);
}
// kLightsGlobal: mixture weights + CDF (and, when small, the light BVH) are
// staged in LDS after the fixed layout: their global copies would be evicted
// from L2 by the CosineDdf gathers, and the pick / walk are chains of
// dependent loads.
constexpr int kLdsLightNodesMax = 512;
// [weights | cdf | cdf bucket starts (kCdfBuckets)] then the light BVH nodes or
// the lattice cells, 16-byte aligned
constexpr int kCdfBuckets = 256;
// The lattice instances leave the weights in global memory (read once per hit
// light) so that C5's 256 emitters fit 4 workgroups per CU: [cdf | buckets].
__host__ __device__ inline int global_light_prefix_words(int nl, bool grid = false) {
    return ((grid ? 1 : 2) * (nl + 1) + kCdfBuckets + 3) & ~3;
}
__host__ __device__ inline size_t global_light_lds_words(int nl, int n_nodes_lds, bool grid = false) {
    return (size_t)global_light_prefix_words(nl, grid) + 8 * (size_t)n_nodes_lds;
}

// Where the lights live during the step loop (compile time, so that no
// generic/flat pointer is ever formed: a flat load would make the compiler
// wait for every outstanding radiance store).
enum { kLightsOne = 1, kLightsLds = 2, kLightsGlobal = 3, kLightsAny = 4, kLightsOneA10 = 5, kLightsOneA01 = 6,
       kLightsGridA10 = 7, kLightsGridA01 = 8, kLightsGridA10L = 9, kLightsGridA01L = 10 };
// kLightsGridA10 / A01: many AreaLights, all axis-aligned with the same axis
// pattern, sharing their plane and lying on a lattice, one per cell
// (light_grid_build): a ray's lights are found by its plane point's cell(s)
// instead of the light BVH walk; weights and CDF staged as kLightsGlobal.
// kLightsGridA10L / A01L: the same with the 48-byte records in LDS, one
// 1024-thread workgroup per CU (block_of), chosen when the LDS fits (+5 % C5)
__host__ __device__ constexpr bool grid_lights(int lm) { return lm >= kLightsGridA10 && lm <= kLightsGridA01L; }
__host__ __device__ constexpr bool lattice_a10(int lm) { return lm == kLightsGridA10 || lm == kLightsGridA10L; }
// the box instances that exist with the step's per-launch choices fixed
// (path_kernel's FIXED): the axis-aligned single light (sample_scenes[0]'s
// instance, +0.8 % C2) and the light lattices (+1.1 % C5)
__host__ __device__ constexpr bool step_fixed_mode(int lm) {
    return lm == kLightsOneA10 || lm == kLightsOneA01 || grid_lights(lm);
}
// path_kernel's FIXED: 0, kFixedPow2, or the tree shape K = log2 n_rays (the
// one compiled K: n_rays 16, every configuration of bench.py but C3)
constexpr int kFixedPow2 = -1;
constexpr int kTreeK = 4;
// KParams::no_fallthrough, the scene fact that gates the FIXED = kTreeK product
// instances besides the tree shape (select_path4):
// word_threshold(cdf[nl]) == 2^32, so every draw word picks a light or the
// surface and UnionDdf's fall-through (one draw, a zero direction) cannot
// occur -- what those instances' pick, pre-skip and direction select are
// compiled for.
// The instances compiled for it (no_fallthrough_mode): the axis-aligned single
// light and the lattices with their records in LDS (bench.py's C2, C4 and C5).
// The lattices with global records keep the general pick in their FIXED =
// kTreeK instances, and the selector does not ask them for the fact: they are
// what a lattice too large for the LDS takes, and such a lattice's hundreds of
// weights rarely sum to 1 (the 17 x 18 census lattices leave 48 of the 2^24
// draw values past cdf[nl]).
__host__ __device__ constexpr bool no_fallthrough_mode(int lm) {
    return lm == kLightsOneA10 || lm == kLightsOneA01 || lm == kLightsGridA10L || lm == kLightsGridA01L;
}
__host__ __device__ constexpr bool lax_in_lds(int lm) { return lm == kLightsGridA10L || lm == kLightsGridA01L; }
__host__ __device__ constexpr bool global_lights(int lm) { return lm == kLightsGlobal || grid_lights(lm); }
// kLightsOneA10 / A01: the single light is an axis-aligned AreaLight
// (axis_aligned_light, ipt_path.h) with x_axis along y and y_axis along x
// (A10, sample_scenes[0]'s light) or along x and y (A01), normal along z
__host__ __device__ constexpr bool one_light(int lm) { return lm == kLightsOne || lm == kLightsOneA10 || lm == kLightsOneA01; }
// kLightsAny: global-memory lights of any type (sphere, point, outer lights
// present); the other modes are AreaLight-only.

}  // namespace
