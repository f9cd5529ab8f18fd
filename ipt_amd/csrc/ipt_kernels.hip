// ipt_kernels.hip — gfx950 kernels and the C-ABI (include/ipt_capi.h) of the
// ipt path-tracing inner loop.
//
// Kernels
//   path_kernel        persistent megakernel: one lane = one path (camera
//                      sample) at a time; the reference's recursive branching
//                      estimator (main.cpp:98-184) runs as an explicit DFS
//                      with the suspended ancestors in LDS and the current
//                      node in registers; lanes refill from a wave-local pool
//                      of work units fed by one global atomic per 256 units.
//                      Writes the per-sample radiance + GridRenderPlane drift
//                      code of every (pass, source pixel).
//   accumulate_kernel  one thread per destination pixel: replays
//                      GridRenderPlane::addRay (GridRenderPlane.cpp:61-75) for
//                      all passes in render_sample order — coalesced reads of
//                      the radiance buffer, HBM-bound. Its kPlaneGui instance
//                      replays Gui::addRay's row map instead (gui.cpp:165-182,
//                      IPT_FLAG_GUI_PLANE). Its ADAPT instances serve masked
//                      renders (ipt_render_masked_device): pixels the mask
//                      switched off are left alone and every added sample
//                      updates the second-moment plane m2.
// Build: see __graft_entry__.py (hipcc --offload-arch=gfx950 -O3
//        -ffp-contract=off, no fast-math).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/ipt_capi.h"
#include "ipt_bvh.h"
#include "ipt_internal.h"
#include "ipt_path.h"
#include "ipt_knobs.h"
#include "ipt_diag.h"
#include "ipt_kparams.h"     // KParams, the instances' launch shape and LDS layout
#include "ipt_scene_plan.h"  // plan_scene: what ipt_upload_scene decides (host only)
#include "ipt_select.h"      // select_path: which path_kernel instance a launch takes (host only)

using namespace ipt;

namespace {

template <typename T>
__device__ __forceinline__ void keep_alive(const T& v) {
    const float* p = reinterpret_cast<const float*>(&v);
    for (int i = 0; i < (int)(sizeof(T) / 4); ++i) asm volatile("" ::"v"(p[i]));
}
constexpr int kPoolChunk = 256;   // work units per global atomic
constexpr int kNumCounters = 15;

// floor(n / d) for 32-bit n, d >= 1 from a double reciprocal: the estimate's
// error is below (n/d) * 2^-51 < 1/d (n < 2^32), i.e. below the distance of a
// non-integer n/d from the next integer, so it truncates to the quotient or,
// when n/d is an integer approached from below, to one less (fixed up).
__host__ __device__ inline uint32_t udiv_exact(uint32_t n, uint32_t d, double inv_d) {
    uint32_t q = (uint32_t)((double)n * inv_d);
    if (n - q * d >= d) ++q;
    return q;
}
// length(a) > length(b) (glm length = sqrtf(dot), func_geometric.inl:8-14) for
// a, b with squares x, y: sqrtf is monotone, so x <= y gives false, and
// x > y(1+2^-20) (y normal) separates the two correctly rounded roots by more
// than their rounding; only the rare near-ties (or NaN/tiny) take the roots.
__device__ __forceinline__ bool longer_sq(float x, float y) {
    const bool far_gt = x > y * 1.000001907f && y >= 1e-30f;  // 1 + 2^-19
    const bool le = x <= y;
    const bool tie = !far_gt && !le;
    bool r = far_gt;
    if (__builtin_expect(__any(tie), 0))
        if (tie) r = sqrt_(x) > sqrt_(y);
    return r;
}
__device__ __forceinline__ bool longer(vec3 a, vec3 b) { return longer_sq(dot(a, a), dot(b, b)); }

// a float in LDS: 32-bit addresses and offsets (the stack's level addressing)
typedef __attribute__((address_space(3))) float lds_float;
// A uniform value kept in a VGPR (the asm output counts as divergent), so
// that its uses read it directly instead of from an SGPR spilled to a VGPR
// lane (v_readlane + hazard nops per use).
__device__ __forceinline__ void vgpr_hold(float& f) { asm volatile("" : "+v"(f)); }
__device__ __forceinline__ void vgpr_hold(vec3& v) { vgpr_hold(v.x); vgpr_hold(v.y); vgpr_hold(v.z); }
__device__ __forceinline__ void vgpr_hold(int& i) { asm volatile("" : "+v"(i)); }

// The RotateDdf angle's (sin, cos) are functions of to.z alone: an exact
// table over every float with |to.z| in [2^-8, 1] (frame_table_kernel, 1 GiB),
// entry ((bits(|z|) - bits(2^-8)) << 1 | sign); other z (|z| < 2^-8, NaN) are
// computed. Replaces the f64 acos + sincos of most frame builds by one gather.
constexpr uint32_t kFrameTabLo = 0x3b800000u;    // 2^-8
constexpr uint32_t kFrameTabSpan = 0x04000000u;  // bits(1.0) - bits(2^-8)
constexpr size_t kFrameTabEntries = 2 * ((size_t)kFrameTabSpan + 1);
__device__ __forceinline__ void frame_sc_lookup(const float2* __restrict__ tab, vec3 to, float& s, float& c) {
    const uint32_t u = f2u(to.z), m = u & 0x7fffffffu;
    const bool in = m - kFrameTabLo <= kFrameTabSpan;
    if (in) {
        const float2 e = tab[((m - kFrameTabLo) << 1) | (u >> 31)];
        s = e.x;
        c = e.y;
    }
    if (__builtin_expect(__any(!in), 0))
        if (!in) frame_angle_sc(to, &s, &c);
}

__device__ __forceinline__ bool owned_row(const KParams& kp, int yi) {
    if (kp.n_shards <= 1 || kp.tile_rows <= 0) return true;
    return ((yi / kp.tile_rows) % kp.n_shards) == kp.shard_id;
}

// 8-word RNG window (blocks blk and blk+1 of the path's Philox stream) in
// named registers; draws are picked with selects (a runtime-indexed array
// would be placed in scratch).
struct Win8 {
    uint32_t a0, a1, a2, a3, b0, b1, b2, b3;
};

// w_j, w_(j+1), w_(j+2) for j in [0,4) (the prologue shifts the window as soon
// as k leaves block blk, and a step consumes at most 3 draws): three 4-way
// selects on j's two bits instead of three 6-way chains
__device__ __forceinline__ uint32_t sel4(uint32_t j, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const bool b0 = (j & 1u) != 0u, b1 = (j & 2u) != 0u;
    const uint32_t lo = b0 ? x1 : x0, hi = b0 ? x3 : x2;
    return b1 ? hi : lo;
}

// ceil(c 2^24) clamped to [0, 2^24] (0 for c <= 0 or NaN): u01(w) < c <=>
// (w >> 8) < cdf_threshold24(c), both sides exact (host: word_threshold)
__device__ __forceinline__ uint32_t cdf_threshold24(float c) {
    const float x = c * 16777216.0f;
    return !(x > 0.0f) ? 0u : (x >= 16777216.0f ? 16777216u : (uint32_t)__builtin_ceilf(x));
}

__device__ __forceinline__ void philox_fill(uint32_t& d0, uint32_t& d1, uint32_t& d2, uint32_t& d3,
                                            uint32_t blk, uint32_t pass, uint32_t pix, uint32_t k0,
                                            uint32_t k1) {
    u32x4 o = philox4x32_10(blk, pass, pix, 0u, k0, k1);
    d0 = o.v[0];
    d1 = o.v[1];
    d2 = o.v[2];
    d3 = o.v[3];
}

// Conservative slab test (entry distance or +inf). Approximate reciprocals
// are fine here: only whether a subtree can contain the scan's winner is
// decided, with margins; the winner itself comes from the exact sphere_t().
__device__ __forceinline__ float bvh_box_entry(const BvhNode& b, vec3 o, vec3 inv) {
    const float tx0 = (b.bmin[0] - o.x) * inv.x, tx1 = (b.bmax[0] - o.x) * inv.x;
    const float ty0 = (b.bmin[1] - o.y) * inv.y, ty1 = (b.bmax[1] - o.y) * inv.y;
    const float tz0 = (b.bmin[2] - o.z) * inv.z, tz1 = (b.bmax[2] - o.z) * inv.z;
    const float tnear = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.0f));
    const float tfar = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
    return tnear <= tfar * 1.0001f + 1e-5f ? tnear : inf_();
}
__device__ __forceinline__ float safe_rcp(float d) {
    return d == 0.0f ? (f2u(d) >> 31 ? -1e30f : 1e30f) : __builtin_amdgcn_rcpf(d);
}

// Stackless walk of the sphere BVH (ipt_bvh.h) from node i for at most
// `budget` node visits; i == kp.n_nodes when the walk is complete. best/bidx
// carry the nearest accepted hit (FractalSpheres.cpp:75-84's rule: minimal t,
// lowest original index on ties, never replacing an equal plane hit).
template <bool COUNT>
__device__ __forceinline__ void sphere_bvh_walk(const KParams& kp, vec3 o, vec3 d, int& i, float& best, int& bidx,
                                                int budget, uint32_t& c_nodes, uint32_t& c_tests) {
    const vec3 inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    // near-child-first linearisation for this direction octant (ipt_bvh.h)
    const int oct = (int)(f2u(d.x) >> 31) | (int)(f2u(d.y) >> 31) << 1 | (int)(f2u(d.z) >> 31) << 2;
    const BvhNode* __restrict__ nodes = kp.bvh_nodes + (size_t)oct * kp.n_nodes;
    // while-while (Aila & Laine 2009): the inner loop only walks nodes until
    // each lane stands on an entered leaf (or is done), so the leaf's sphere
    // tests run with all such lanes together instead of once per wave-iteration
    while (i < kp.n_nodes && budget > 0) {
        int leaf = -1;
        while (i < kp.n_nodes && budget > 0) {
            --budget;
            const BvhNode nd = nodes[i];
            if (COUNT) ++c_nodes;
            const float te = bvh_box_entry(nd, o, inv);
            // te == inf is a miss; it must not pass when best is inf too (open floor)
            const bool enter = te != inf_() && te <= best * 1.0001f + 1e-5f + kp.bvh_tmargin;
            if (enter && nd.leaf >= 0) {
                leaf = nd.leaf;
                i = nd.skip;
                break;
            }
            i = enter ? i + 1 : nd.skip;
        }
        if (leaf >= 0) {
            const int first = leaf & 0xffffff, cnt = leaf >> 24;
            if (COUNT) c_tests += (uint32_t)cnt;
            for (int k2 = 0; k2 < cnt; ++k2) {
                const BvhSphere sp = kp.bvh_prims[first + k2];
                const float t = sphere_t(sp.r, o - v3(sp.c[0], sp.c[1], sp.c[2]), d);
                if (isfinite_(t) && gt_1em6(fabs_(t)) &&
                    (t < best || (t == best && bidx >= 0 && sp.index < bidx))) {
                    best = t;
                    bidx = sp.index;
                }
            }
        }
    }
}

// Uniform-grid walk (ipt_bvh.h SphereGrid; exactness argument there). The
// resumable state is the current cell (x | y << 8 | z << 16, -1 when done) and
// the t of the next cell boundary per axis.
__device__ __forceinline__ void sphere_grid_init(const KParams& kp, vec3 o, vec3 d, int& cell, vec3& tmx) {
    const vec3 inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    const float dv[3] = {d.x, d.y, d.z}, ov[3] = {o.x, o.y, o.z}, iv[3] = {inv.x, inv.y, inv.z};
    float tn = 0.0f, tf = inf_();
    for (int a = 0; a < 3; ++a) {
        const float g1 = kp.grid_g1[a];  // g0 + (float)n * h
        if (dv[a] == 0.0f) {
            if (ov[a] < kp.grid_g0[a] || ov[a] > g1) tf = -1.0f;  // parallel and outside
            continue;
        }
        const float t0 = (kp.grid_g0[a] - ov[a]) * iv[a], t1 = (g1 - ov[a]) * iv[a];
        tn = fmaxf(tn, fminf(t0, t1));
        tf = fminf(tf, fmaxf(t0, t1));
    }
    if (!(tn <= tf * 1.0001f + 1e-5f)) {
        cell = -1;
        return;
    }
    int ia[3];
    float tm[3];
    for (int a = 0; a < 3; ++a) {
        const float pa = ov[a] + dv[a] * tn;
        int c = (int)floorf((pa - kp.grid_g0[a]) * kp.grid_inv_h[a]);
        c = c < 0 ? 0 : (c >= kp.grid_n[a] ? kp.grid_n[a] - 1 : c);
        ia[a] = c;
        tm[a] = dv[a] > 0.0f   ? ((kp.grid_g0[a] + (float)(c + 1) * kp.grid_h[a]) - ov[a]) * iv[a]
                : dv[a] < 0.0f ? ((kp.grid_g0[a] + (float)c * kp.grid_h[a]) - ov[a]) * iv[a]
                               : inf_();
    }
    cell = ia[0] | ia[1] << 8 | ia[2] << 16;
    tmx = v3(tm[0], tm[1], tm[2]);
}
// the wave walk's items: centre and radius as one 16-byte record, the original
// index apart (read only on a tie and when the walk is done)
__device__ __forceinline__ float4 grid_item(const KParams& kp, int k) { return kp.grid_c4[k]; }
__device__ __forceinline__ int grid_item_index(const KParams& kp, int k) { return kp.grid_idx[k]; }
template <bool COUNT>
__device__ __forceinline__ void sphere_grid_walk(const KParams& kp, vec3 o, vec3 d, int& cell, vec3& tmx, float& best,
                                                 int& bidx, int budget, uint32_t& c_nodes,
                                                 uint32_t& c_tests) {
    const vec3 inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    while (cell >= 0 && budget-- > 0) {
        const int ix = cell & 0xff, iy = (cell >> 8) & 0xff, iz = cell >> 16;
        const int lin = ix + kp.grid_n[0] * (iy + kp.grid_n[1] * iz);
        const int s0 = kp.grid_start[lin], s1 = kp.grid_start[lin + 1];
        if (COUNT) {
            ++c_nodes;
            c_tests += (uint32_t)(s1 - s0);
        }
        for (int k2 = s0; k2 < s1; ++k2) {
            const BvhSphere sp = kp.grid_items[k2];
            const float t = sphere_t(sp.r, o - v3(sp.c[0], sp.c[1], sp.c[2]), d);
            if (isfinite_(t) && gt_1em6(fabs_(t)) && (t < best || (t == best && bidx >= 0 && sp.index < bidx))) {
                best = t;
                bidx = sp.index;
            }
        }
        const float texit = fminf(fminf(tmx.x, tmx.y), tmx.z);
        if (texit > (best * 1.0001f + 1e-5f + kp.bvh_tmargin + kp.grid_m) * 1.00001f + 1e-5f) {
            cell = -1;
            break;
        }
        // step across the nearest boundary (x, then y, then z on ties)
        if (tmx.x <= tmx.y && tmx.x <= tmx.z) {
            const int nx = d.x > 0.0f ? ix + 1 : ix - 1;
            if (nx < 0 || nx >= kp.grid_n[0]) { cell = -1; break; }
            cell = (cell & ~0xff) | nx;
            tmx.x = ((kp.grid_g0[0] + (float)(d.x > 0.0f ? nx + 1 : nx) * kp.grid_h[0]) - o.x) * inv.x;
        } else if (tmx.y <= tmx.z) {
            const int ny = d.y > 0.0f ? iy + 1 : iy - 1;
            if (ny < 0 || ny >= kp.grid_n[1]) { cell = -1; break; }
            cell = (cell & ~0xff00) | ny << 8;
            tmx.y = ((kp.grid_g0[1] + (float)(d.y > 0.0f ? ny + 1 : ny) * kp.grid_h[1]) - o.y) * inv.y;
        } else {
            const int nz = d.z > 0.0f ? iz + 1 : iz - 1;
            if (nz < 0 || nz >= kp.grid_n[2]) { cell = -1; break; }
            cell = (cell & 0xffff) | nz << 16;
            tmx.z = ((kp.grid_g0[2] + (float)(d.z > 0.0f ? nz + 1 : nz) * kp.grid_h[2]) - o.z) * inv.z;
        }
    }
}

// Wave-wide inclusive scans over the 64 lanes (DPP: row shifts within each
// 16-lane row, then rows 1/3 from lane 15 of the row before and rows 2/3 from
// lane 31). Called with every lane of the wave active.
__device__ __forceinline__ int wave_scan_add(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}
__device__ __forceinline__ int wave_scan_max(int v) {  // v >= 0
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
    return v;
}

// Orders one wave's LDS accesses across its lanes for the compiler (the
// hardware runs a wave's LDS instructions in order): without it a lane's load
// of a word it stored itself would be forwarded from that store, missing the
// other lanes' stores in between.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The resumable grid walk, with the item tests spread over the whole wave.
// Per wave iteration every walking lane steps one cell: the
// (lane, item) pairs of the cells the lanes stand on are numbered by a wave
// prefix sum and tested 64 at a time, one pair per lane (the lane that owns
// pair p is found by a ds_permute of the segment starts and a max-scan; its
// ray is read with ds_bpermute), and each accepted t goes to its owner's
// LDS slot as an atomic minimum of (t bits << 32 | item position). Within a
// cell the positions are in original-index order (grid_build_spheres fills
// each cell in index order) and accepted t are positive, so the slot ends as
// the cell's (t, index) minimum; the owner merges it with `accept`, the
// scan's rule (FractalSpheres.cpp:75-84: strict '<', lowest index on
// equal t, a plane never loses a tie). The tests run at full lane
// utilisation instead of once per lane per item slot. Same cells, same tests
// (sphere_t on the same operands), same exit decisions: the (t, index) minimum
// does not depend on the order of the tests. Every lane of the wave calls it.
template <bool COUNT>
__device__ __forceinline__ void sphere_grid_walk_wave(const KParams& kp, bool walking, vec3 o, vec3 d, int& cell,
                                                      vec3& tmx, float& best, int& bidx, int budget,
                                                      unsigned long long* slots, int lane,
                                                      uint32_t& c_nodes, uint32_t& c_tests IPT_DIAG_PARAMS) {
    const vec3 inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
    auto lin_of = [&](int c) {
        return (c & 0xff) + kp.grid_n[0] * (((c >> 8) & 0xff) + kp.grid_n[1] * (c >> 16));
    };
    bool act = walking && cell >= 0 && budget > 0;
    int s0 = 0, s1 = 0;
    if (act) {
        const int lin = lin_of(cell);
        s0 = kp.grid_start[lin];
        s1 = kp.grid_start[lin + 1];
    }
    for (;;) {
        const uint64_t am = __ballot(act);
        if (!am) break;
#if IPT_PROF
        // phase 6 (walk cell): one wave iteration, its walking lanes (every
        // lane of the wave runs this loop, so lane 0 counts)
        if (prof_w && lane == 0) {
            prof_w[6] += 1u;
            prof_l[6] += (uint32_t)__popcll(am);
        }
#endif
        // the next cell (from tmx alone) and its range, in flight during the tests
        int ncell = 0, n0 = 0, n1 = 0;
        vec3 ntm = tmx;
        bool nvalid = false;
        if (act) {
            const int ix = cell & 0xff, iy = (cell >> 8) & 0xff, iz = cell >> 16;
            if (tmx.x <= tmx.y && tmx.x <= tmx.z) {
                const int nx = d.x > 0.0f ? ix + 1 : ix - 1;
                nvalid = !(nx < 0 || nx >= kp.grid_n[0]);
                ncell = (cell & ~0xff) | (nx & 0xff);
                ntm.x = ((kp.grid_g0[0] + (float)(d.x > 0.0f ? nx + 1 : nx) * kp.grid_h[0]) - o.x) * inv.x;
            } else if (tmx.y <= tmx.z) {
                const int ny = d.y > 0.0f ? iy + 1 : iy - 1;
                nvalid = !(ny < 0 || ny >= kp.grid_n[1]);
                ncell = (cell & ~0xff00) | (ny & 0xff) << 8;
                ntm.y = ((kp.grid_g0[1] + (float)(d.y > 0.0f ? ny + 1 : ny) * kp.grid_h[1]) - o.y) * inv.y;
            } else {
                const int nz = d.z > 0.0f ? iz + 1 : iz - 1;
                nvalid = !(nz < 0 || nz >= kp.grid_n[2]);
                ncell = (cell & 0xffff) | (nz & 0xff) << 16;
                ntm.z = ((kp.grid_g0[2] + (float)(d.z > 0.0f ? nz + 1 : nz) * kp.grid_h[2]) - o.z) * inv.z;
            }
            ncell = nvalid ? ncell : -1;
            // (no next cell: cell 0's range, unused)
            const int nlin = nvalid ? lin_of(ncell) : 0;
            n0 = kp.grid_start[nlin];
            n1 = kp.grid_start[nlin + 1];
        }
        const int cnt = act ? s1 - s0 : 0;
        if (COUNT && act) {
            ++c_nodes;
            c_tests += (uint32_t)cnt;
        }
        const int incl = wave_scan_add(cnt);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        const int excl = incl - cnt;
        if (total > 0) {
            if (cnt > 0) slots[lane] = ~0ull;
            wave_lds_sync();  // the clears before any lane's atomic minimum
            const int dk = s0 - excl;  // pair p of this lane tests item p + dk
            // one round: pairs base .. base + 63 (owner, its ray, the item)
            struct Pair {
                vec3 o, d;
                float4 c4;
                int k, src;
                bool valid;
            };
            auto setup = [&](int base, Pair& q) {
                // the owner of pair base + lane, in one ds_permute (no LDS
                // round trip): every lane whose segment starts before the
                // round's end sends lane + 1 to its start (clamped to 0); of
                // lanes sharing a start only the highest-numbered can own
                // pairs (excl[L] == excl[L+1] means cnt[L] == 0), and the
                // highest-numbered source is the one ds_permute keeps. The
                // lanes starting beyond the round (a suffix: excl does not
                // decrease) send to position 63, which then takes the last
                // sender; a max-scan carries each start to the pairs after it.
                const bool snd = excl < base + 64;
                int r = __builtin_amdgcn_ds_permute((snd ? (excl > base ? excl - base : 0) : 63) << 2, lane + 1);
                const uint64_t sm = __ballot(snd);
                if (~sm && lane == 63) r = __popcll(sm);
                q.src = wave_scan_max(r) - 1;
                const int p = base + lane;
                q.valid = p < total;
                const int sl = q.valid ? q.src : lane;
                q.o = v3(__shfl(o.x, sl), __shfl(o.y, sl), __shfl(o.z, sl));
                q.d = v3(__shfl(d.x, sl), __shfl(d.y, sl), __shfl(d.z, sl));
                q.k = p + __shfl(dk, sl);
                q.c4 = grid_item(kp, q.valid ? q.k : 0);
            };
            auto test = [&](const Pair& q) {
                // every lane loads (item 0 for lanes without a pair) and the wave
                // waits for the item here, outside the branch: otherwise a load left
                // pending on the path that skips the test made the next round's load
                // wait for every outstanding load, the next cell's range prefetch
                // included (vmcnt(0))
                keep_alive(q.c4);
                if (q.valid) {
                    const float t = sphere_t(q.c4.w, q.o - v3(q.c4.x, q.c4.y, q.c4.z), q.d);
                    if (isfinite_(t) && gt_1em6(fabs_(t)))
                        __hip_atomic_fetch_min(slots + q.src,
                                               (unsigned long long)__float_as_uint(t) << 32 | (uint32_t)q.k,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                }
            };
            int base = 0;
            for (; base < total; base += 64) {
                Pair q;
                setup(base, q);
                test(q);
            }
            wave_lds_sync();
            if (cnt > 0) {
                const unsigned long long key = slots[lane];
                if (key != ~0ull) {
                    const float t = __uint_as_float((uint32_t)(key >> 32));
                    const int k2 = (int)(uint32_t)key;
                    if (t < best)
                        bidx = k2;
                    else if (t == best && bidx >= 0 && grid_item_index(kp, k2) < grid_item_index(kp, bidx))
                        bidx = k2;
                    best = t < best ? t : best;
                }
            }
        }
        if (act) {
            --budget;
            const float texit = fminf(fminf(tmx.x, tmx.y), tmx.z);
            if (texit > (best * 1.0001f + 1e-5f + kp.bvh_tmargin + kp.grid_m) * 1.00001f + 1e-5f || ncell < 0) {
                cell = -1;
                act = false;
            } else {
                cell = ncell;
                tmx = ntm;
                s0 = n0;
                s1 = n1;
                act = budget > 0;
            }
        }
    }
}

// Nearest geometry hit for both geometry kinds. prim: 0..4 plane, 5 the
// r=0.5 sphere, 6+i extra sphere i (original index), -1 miss.
// RANGE: the box planes' range form. In range, every ray origin (camera,
// wall/floor hits, listed spheres) lies within 2^39, so the planes' divisions
// take the range-free sequence. The path kernel's box instances fix the form at
// compile time (one copy of the trace per instance); kRangeRuntime selects on
// kp.box_inrange (the preview kernel).
enum { kRangeRuntime = -1, kRangeGeneric = 0, kRangeIn = 1 };
template <bool COUNT, int GEOM, bool NEAREST, int RANGE = kRangeRuntime>
__device__ __forceinline__ float trace_geometry(const KParams& kp, vec3 o, vec3 d, int* prim, vec3* hit,
                                                uint32_t& c_nodes, uint32_t& c_tests) {
    // (*hit: the box's hit point o + d*t where NEAREST, see resolve's kBoxHit)
    if (GEOM == IPT_GEOM_SPHERE_IN_BOX) {
        if constexpr (RANGE == kRangeIn) {
            if (NEAREST) return trace_box_hit<true>(o, d, prim, hit);
            return trace_box<true>(o, d, prim);
        } else if constexpr (RANGE == kRangeGeneric) {
            static_assert(!NEAREST || GEOM != IPT_GEOM_SPHERE_IN_BOX, "the generic box instances take the full form");
            return trace_box<false>(o, d, prim);
        } else {
            if (NEAREST)
                return kp.box_inrange ? trace_box_hit<true>(o, d, prim, hit) : trace_box_hit<false>(o, d, prim, hit);
            return kp.box_inrange ? trace_box<true>(o, d, prim) : trace_box<false>(o, d, prim);
        }
    }
    if (GEOM == IPT_GEOM_FLOOR) {  // GeometryFloor.cpp:11-13
        const float t = box_plane_t(o.z, d.z, -1.0f, o, d);
        *prim = t == inf_() ? -1 : 0;
        return t;
    }
    if (GEOM == IPT_GEOM_CORNER) {  // GeometryCorner.cpp:11-28: tx, then ty, tz with strict <
        float t = box_plane_t(o.x, d.x, -1.0f, o, d);
        int p = 0;
        const float ty = box_plane_t(o.y, d.y, -1.0f, o, d);
        if (ty < t) { t = ty; p = 1; }
        const float tz = box_plane_t(o.z, d.z, -1.0f, o, d);
        if (tz < t) { t = tz; p = 2; }
        *prim = t == inf_() ? -1 : p;
        return t;
    }
    if (GEOM == IPT_GEOM_SMALLPT) {  // GeometrySmallPt.cpp:14-47, double precision
        double min_t = (double)inf_();
        int mi = -1;
        for (int i = 0; i < kp.n_spheres; ++i) {
            const float4 sp = kp.spheres[i];
            const vec3 op = v3(sp.x, sp.y, sp.z) - o;  // p - ro (float)
            const double rad = (double)sp.w;
            const double b = (double)dot(op, d);
            double det = b * b - (double)dot(op, op) + rad * rad;
            double t = 0.0;
            if (!(det < 0.0)) {
                det = sqrtd_(det);
                t = b - det;
                if (!(t > 1e-4)) {
                    t = b + det;
                    if (!(t > 1e-4)) t = 0.0;
                }
            }
            if (COUNT) ++c_tests;
            if (t != 0.0 && t < min_t) {
                min_t = t;
                mi = i;
            }
        }
        *prim = mi >= 0 ? 6 + mi : -1;
        return mi >= 0 ? (float)min_t : inf_();
    }
    // planes as GeometrySphereInBox, then spheres with FractalSpheres' rule
    // (FractalSpheres.cpp:75-84): strict '<' in index order == minimal t,
    // lowest index among equal t, and a sphere never wins a tie with a plane.
    int p = -1;
    float best = inf_();  // FractalSpheres: no walls
    if (GEOM == IPT_GEOM_SPHERES_IN_BOX)
        best = kp.box_inrange ? trace_box_planes_only<true>(o, d, &p) : trace_box_planes_only<false>(o, d, &p);
    int bidx = -1;
    if (kp.n_grid > 0) {
        int cell;
        vec3 tmx;
        sphere_grid_init(kp, o, d, cell, tmx);
        sphere_grid_walk<COUNT>(kp, o, d, cell, tmx, best, bidx, 0x7fffffff, c_nodes, c_tests);
    } else if (kp.n_nodes > 0) {
        int i = 0;
        sphere_bvh_walk<COUNT>(kp, o, d, i, best, bidx, 0x7fffffff, c_nodes, c_tests);
    } else {
        if (COUNT) c_tests += (uint32_t)kp.n_spheres;
        for (int i = 0; i < kp.n_spheres; ++i) {
            float4 s = kp.spheres[i];
            vec3 c = v3(s.x, s.y, s.z);
            float t = sphere_t(s.w, o - c, d);
            if (isfinite_(t) && gt_1em6(fabs_(t)) && t < best) {
                best = t;
                bidx = i;
            }
        }
    }
    *prim = bidx >= 0 ? 6 + bidx : p;
    return best;
}

// the instances whose box trace takes the nearest-candidate planes
// (trace_box_planes_nearest): every in-range box instance (path_kernel's
// BOXIN), the lattice instances included since the range form is fixed per
// instance and the full form behind the vote is compiled once (+0.65 % C5,
// DESIGN.md 4.12; with both range forms in the step they lost 0.2 %, 4.10).
// The generic box instances keep the full form (kNearest), and so do the
// sphere-list instances' walls, which gain nothing measurable (4.10).
__host__ __device__ constexpr bool box_nearest(int geom) { return geom == IPT_GEOM_SPHERE_IN_BOX; }

template <int LMODE>
struct LightSet {
    const LightDev* lds;
    const LightDev* __restrict__ glob;
    const float* wl;  // weights in LDS
    const float* cl;  // cdf in LDS
    const float* __restrict__ wg;
    const float* __restrict__ cg;
    LightDev one;
    float w0, c0, c1;
    __device__ __forceinline__ const LightDev& light(int i) const {
        if (one_light(LMODE)) return one;
        if (LMODE == kLightsLds) return lds[i];
        return glob[i];  // kLightsGlobal, kLightsAny
    }
    __device__ __forceinline__ float weight(int i) const {
        if (one_light(LMODE)) return w0;
        if (grid_lights(LMODE)) return wg[i];
        if (LMODE == kLightsLds || global_lights(LMODE)) return wl[i];
        return wg[i];
    }
    __device__ __forceinline__ float cdf(int i) const {
        if (one_light(LMODE)) return i == 0 ? c0 : c1;
        if (LMODE == kLightsLds || global_lights(LMODE)) return cl[i];
        return cg[i];
    }
};

// GEOM (IPT_GEOM_*) is a template parameter so that the box instance carries
// neither the sphere-list code nor its pointers (SGPR pressure).
// Sphere-list instances carry the resumable walk's state (resumable_geom,
// ipt_kparams.h: their walks are bounded per step and resumed in later steps): they
// are given 3 waves per SIMD of registers (their LDS allows 3 workgroups).
// many-light instances without a sphere list resume their light-BVH walk the same way
__host__ __device__ constexpr bool resumable_lights(int lmode, int geom) {
    return lmode == 3 /* kLightsGlobal */ && !resumable_geom(geom);
}
__host__ __device__ constexpr int waves_per_simd(int geom, int lmode) {
    return resumable_geom(geom) ? IPT_RES_WAVES : (resumable_lights(lmode, geom) ? IPT_RESL_WAVES : IPT_WAVES_PER_SIMD);
}
// render_sample's per-sample work before ray_power (main.cpp:192-211) for
// work unit `unit` (pass-major, then candidate row, then column): the absolute
// pass and source pixel (the Philox counter), the two jitter draws, the
// render plane's drift code (GridRenderPlane's or, with kp.plane ==
// kPlaneGui, the Gui's; and the flags of drifted samples), the camera ray. A
// unit whose sample lands outside the image or in another shard's row gets
// its value (0) and code stored here and is not traced.
struct RayGen {
    vec3 rd;
    uint32_t a0, a1, a2, a3, rpass, rpix;
    bool valid, drift;
};
__device__ __forceinline__ RayGen new_path_setup(const KParams& kp, unsigned long long unit, bool sharded,
                                                 const int* cand_rows) {
    RayGen g;
    // 32-bit arithmetic with double reciprocals (udiv_exact; units < 2^32)
    const uint32_t u32 = (uint32_t)unit;
    const uint32_t s = udiv_exact(u32, kp.per_pass32, kp.inv_per_pass);
    const uint32_t rem = u32 - s * kp.per_pass32;
    const int cand = (int)udiv_exact(rem, (uint32_t)kp.W, kp.inv_w);
    const int ix = (int)(rem - (uint32_t)cand * (uint32_t)kp.W);
    const int iy = sharded ? cand_rows[cand] : cand;
    g.rpass = (uint32_t)(kp.spp_offset + (int)s);
    g.rpix = (uint32_t)(iy * kp.W + ix);
    philox_fill(g.a0, g.a1, g.a2, g.a3, 0u, g.rpass, g.rpix, kp.key0, kp.key1);
    const float x = jitter_coord(ix, u01(g.a0), kp.W);
    const float y = jitter_coord(iy, u01(g.a1), kp.H);
    int xi, yi, yn;
    if (kp.plane == kPlaneGui) {
        gui_index(x, y, kp.W, kp.H, &xi, &yi);
        yn = gui_nominal_row(iy, kp.H);
    } else {
        grid_index(x, y, kp.W, kp.H, &xi, &yi);
        yn = nominal_row(iy, kp.H);
    }
    const int dx = xi - ix, dy = yi - yn;
    uint8_t code = 0xff;
    if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 && xi < kp.W && yi < kp.H)
        code = (uint8_t)((dx + 1) | ((dy + 1) << 2));
    // the caller's mask, by the sample's nominal destination (ix, yn): byte 0
    // means the sample is not traced -- no flags, no drift count, value 0 and
    // code 0xfe, which the replay's code-checking branch skips
    const bool masked = kp.mask && kp.mask[(size_t)yn * kp.W + ix] == 0;
    g.drift = code != 0x05 && code != 0xff && !masked;
    if (g.drift) {
        kp.flags[(size_t)yn * kp.W + ix] = 1;
        kp.flags[(size_t)yi * kp.W + xi] = 1;
    }
    g.valid = !(code == 0xff || masked || !owned_row(kp, yi));
    g.rd = v3(0, 0, 0);
    if (!g.valid) {
        // not ours (halo row of another shard), out of range or masked
        kp.values[unit] = 0.0f;
        kp.codes[unit] = (code == 0xff && !masked) ? code : (uint8_t)0xfe;
    } else {
        kp.codes[unit] = code;
        g.rd = camera_dir(kp.cam_right, kp.cam_up, kp.cam_dir, x, y);
    }
    return g;
}

// One thread per work unit of the launch: new_path_setup at full lane
// utilisation (inside the persistent path kernel a refill serves ~2 lanes of a
// wave), written as two 16-byte records {rd.xyz, valid} {a2, a3, pass, pixel}
// that the path kernel's refill reads.
__global__ __launch_bounds__(256) void raygen_kernel(const KParams kp) {
    const unsigned long long unit = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= kp.total_units) return;
    const bool sharded = !(kp.n_shards <= 1 || kp.tile_rows <= 0);
    const RayGen g = new_path_setup(kp, unit, sharded, kp.cand_rows);
    uint4* out = const_cast<uint4*>(kp.rg) + 2 * unit;
    out[0] = make_uint4(__float_as_uint(g.rd.x), __float_as_uint(g.rd.y), __float_as_uint(g.rd.z), g.valid ? 1u : 0u);
    out[1] = make_uint4(g.a2, g.a3, g.rpass, g.rpix);
    if (kp.count) {
        const uint64_t m = __ballot(g.drift);
        if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
            atomicAdd(&kp.counters[10], (unsigned long long)__popcll(m));
    }
}

// ------------------------------------------------ unit compaction (IPT_FLAG_COMPACT)
// A compacting launch takes raygen_kernel's place with four
// kernels on the slot stream, and runs one more after the path kernel:
//   compact_classify_kernel  new_path_setup once per dense unit that is not
//                            masked (codes, the invalid units' values, flags
//                            and the drift count, all as raygen_kernel leaves
//                            them; a masked unit gets its value and code from
//                            its mask byte alone) and each block's count of
//                            valid units;
//   compact_scan_kernel      (one workgroup) the counts -> exclusive offsets in
//                            place, the total n_active behind them;
//   compact_scatter_kernel   valid unit number j in ascending dense order gets
//                            the compact index c = total_units - n_active + j:
//                            its two records go to rg[2c], rg[2c+1], its dense
//                            unit to src[c]; the pad [start, total_units -
//                            n_active) gets valid = 0 records, start being the
//                            compact range's begin rounded down to kPoolChunk;
//   compact_preset_kernel    (one thread) the unit counter starts at `start`, so
//                            the unchanged path_kernel hands out [start,
//                            total_units) alone; {start, n_active} go to the
//                            launch's ring entry (ipt_last_units);
//   compact_expand_kernel    values[src[c]] = cvalues[c] for the compact range
//                            (the path kernel's kp.values is cvalues).
// Nothing crosses to the host: n_active is read from blocks[nblk] by the
// kernels that need it. A block is 256 consecutive dense units throughout.
struct CompactBufs {
    unsigned int* blocks;       // [nblk + 1]: counts, then exclusive offsets; [nblk] = n_active
    uint32_t* src;              // [total_units] dense unit of a compact index
    float* cvalues;             // [total_units] the path kernel's values, by compact index
    float* values;              // [total_units] the launch's dense values
    unsigned long long* ring;   // {start, n_active} of this launch
};

__global__ __launch_bounds__(256) void compact_classify_kernel(const KParams kp, unsigned int* __restrict__ blocks) {
    __shared__ unsigned int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const unsigned long long unit = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false, drift = false;
    if (unit < kp.total_units) {
        const bool sharded = !(kp.n_shards <= 1 || kp.tile_rows <= 0);
        // a masked unit is known from its nominal pixel alone: new_path_setup
        // leaves it value 0 and code 0xfe whatever its draws are, no flag and
        // no drift count, so its Philox block and jitter are not computed here
        bool masked = false;
        if (kp.mask) {
            const uint32_t u32 = (uint32_t)unit;
            const uint32_t rem = u32 - udiv_exact(u32, kp.per_pass32, kp.inv_per_pass) * kp.per_pass32;
            const int cand = (int)udiv_exact(rem, (uint32_t)kp.W, kp.inv_w);
            const int ix = (int)(rem - (uint32_t)cand * (uint32_t)kp.W);
            const int iy = sharded ? kp.cand_rows[cand] : cand;
            const int yn = kp.plane == kPlaneGui ? gui_nominal_row(iy, kp.H) : nominal_row(iy, kp.H);
            masked = kp.mask[(size_t)yn * kp.W + ix] == 0;
        }
        if (masked) {
            kp.values[unit] = 0.0f;
            kp.codes[unit] = (uint8_t)0xfe;
        } else {
            const RayGen g = new_path_setup(kp, unit, sharded, kp.cand_rows);
            valid = g.valid;
            drift = g.drift;
        }
    }
    if (kp.count) {
        const uint64_t m = __ballot(drift);
        if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
            atomicAdd(&kp.counters[10], (unsigned long long)__popcll(m));
    }
    const unsigned int c = (unsigned int)__popcll(__ballot(valid));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) blocks[blockIdx.x] = total;
}

// one workgroup: blocks[0..nblk) -> exclusive offsets in place, total -> blocks[nblk]
__global__ __launch_bounds__(256) void compact_scan_kernel(unsigned int* __restrict__ blocks, unsigned int nblk) {
    __shared__ unsigned int part[256];
    const unsigned int per = (nblk + 255u) / 256u;
    const unsigned int lo = min(threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    unsigned int s = 0;
    for (unsigned int i = lo; i < hi; ++i) s += blocks[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int acc = 0;
        for (int t = 0; t < 256; ++t) {
            const unsigned int v = part[t];
            part[t] = acc;
            acc += v;
        }
        blocks[nblk] = acc;
    }
    __syncthreads();
    unsigned int off = part[threadIdx.x];
    for (unsigned int i = lo; i < hi; ++i) {
        const unsigned int v = blocks[i];
        blocks[i] = off;
        off += v;
    }
}

// new_path_setup's record of a unit it found valid, without its stores: the
// same draws, jitter and camera ray (the build contracts no operations, so the
// ray's bits are raygen_kernel's)
__device__ __forceinline__ void compact_record(const KParams& kp, uint32_t u32, bool sharded, uint4& r0, uint4& r1) {
    const uint32_t s = udiv_exact(u32, kp.per_pass32, kp.inv_per_pass);
    const uint32_t rem = u32 - s * kp.per_pass32;
    const int cand = (int)udiv_exact(rem, (uint32_t)kp.W, kp.inv_w);
    const int ix = (int)(rem - (uint32_t)cand * (uint32_t)kp.W);
    const int iy = sharded ? kp.cand_rows[cand] : cand;
    const uint32_t rpass = (uint32_t)(kp.spp_offset + (int)s);
    const uint32_t rpix = (uint32_t)(iy * kp.W + ix);
    uint32_t a0, a1, a2, a3;
    philox_fill(a0, a1, a2, a3, 0u, rpass, rpix, kp.key0, kp.key1);
    const float x = jitter_coord(ix, u01(a0), kp.W);
    const float y = jitter_coord(iy, u01(a1), kp.H);
    const vec3 rd = camera_dir(kp.cam_right, kp.cam_up, kp.cam_dir, x, y);
    r0 = make_uint4(__float_as_uint(rd.x), __float_as_uint(rd.y), __float_as_uint(rd.z), 1u);
    r1 = make_uint4(a2, a3, rpass, rpix);
}

__global__ __launch_bounds__(256) void compact_scatter_kernel(const KParams kp, const unsigned int* __restrict__ blocks,
                                                              uint32_t* __restrict__ src) {
    __shared__ unsigned int wave_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long unit = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = unit < kp.total_units;
    const unsigned long long first = kp.total_units - blocks[gridDim.x];  // the compact range's begin
    const unsigned long long start = first / kPoolChunk * kPoolChunk;
    // (compact_classify_kernel's code: an invalid unit has 0xfe or 0xff)
    const bool valid = in && kp.codes[unit] < (uint8_t)0xfe;
    const unsigned long long mask = __ballot(valid);
    if (lane == 0) wave_cnt[wave] = (unsigned int)__popcll(mask);
    __syncthreads();
    unsigned int before = 0;
    for (int w = 0; w < 4; ++w) before += w < wave ? wave_cnt[w] : 0u;
    uint4* rg = const_cast<uint4*>(kp.rg);
    // the pad: records of the slot's earlier launches lie there, and one with
    // valid = 1 would be traced and stored
    if (in && unit >= start && unit < first) {
        rg[2 * unit] = make_uint4(0u, 0u, 0u, 0u);
        rg[2 * unit + 1] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (valid) {
        const unsigned long long c =
            first + blocks[blockIdx.x] + before + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
        const bool sharded = !(kp.n_shards <= 1 || kp.tile_rows <= 0);
        uint4 r0, r1;
        compact_record(kp, (uint32_t)unit, sharded, r0, r1);
        if (c < kp.total_units) {
            rg[2 * c] = r0;
            rg[2 * c + 1] = r1;
            src[c] = (uint32_t)unit;
        }
    }
}

__global__ void compact_preset_kernel(const unsigned int* __restrict__ blocks, unsigned int nblk,
                                      unsigned long long total_units, unsigned long long* __restrict__ unit_counter,
                                      unsigned long long* __restrict__ ring) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long n_active = blocks[nblk];
    const unsigned long long start = (total_units - n_active) / kPoolChunk * kPoolChunk;
    *unit_counter = start;
    ring[0] = start;
    ring[1] = n_active;
}

__global__ __launch_bounds__(256) void compact_expand_kernel(const CompactBufs cb, unsigned int nblk,
                                                             unsigned long long total_units) {
    const unsigned long long c = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= total_units || c < total_units - cb.blocks[nblk]) return;
    cb.values[cb.src[c]] = cb.cvalues[c];
}

// BOXIN (sphere-in-box instances; false in the others, which do not read it):
// the box planes' range form, a property of the scene (box_inrange, set at
// upload). true compiles the in-range trace alone, false the generic full-form
// trace alone, correct for every input.
// FIXED (step_fixed_mode's in-range box instances): two more choices of the
// launch that the step otherwise makes once per step -- n_rays is a power of
// two (the pop's unwind keeps its exact scaling form alone) and the lights'
// skip-ahead plane exists (kp.sa_on: the skip-ahead and the pre-skip lose
// their guard). Both are read from the launch's parameters by the dispatch
// (select_path4, ipt_select.h), so a launch without them takes the FIXED = 0 instance.
// FIXED = K > 0 (kTreeK; the 4-level instances): the tree's shape is the
// launch's as well -- n_rays == 2^K, hence meta_shift, and depth_max > K + 1:
// no node deeper than K is pushed (n_rays >> d == 0 beyond), so no ray has
// rdepth > K + 1 and every ray is traced. The step then reads neither
// kp.n_rays, kp.meta_shift nor kp.depth_max. kFixedPow2 is the form above
// (any power of two, any depth_max).
template <int MAXSUSP, bool COUNT, int LMODE, int GEOM, bool BOXIN, int FIXED>
__global__ __launch_bounds__(block_of(LMODE, GEOM), waves_per_simd(GEOM, LMODE)) void path_kernel(const KParams kp) {
    static_assert(!BOXIN || GEOM == IPT_GEOM_SPHERE_IN_BOX, "BOXIN is the box instances' parameter");
    static_assert(!FIXED || (BOXIN && step_fixed_mode(LMODE)), "FIXED: in-range box instances with a skip-ahead plane");
    static_assert(FIXED >= kFixedPow2 && FIXED <= MAXSUSP, "FIXED = K: K suspended levels");
    constexpr bool kFixed = FIXED != 0;
    constexpr int kK = FIXED > 0 ? FIXED : 0;
    // the launch's tree shape, constants in the FIXED = K instances (written as
    // conditional expressions on kK at each use: the other instances keep
    // their code, and their register assignment, as it was)
    constexpr int kTreeRays = 1 << kK, kTreeMetaShift = kTreeRays > 255 ? 16 : 8;
    // the product FIXED = K instances also take a fact of the scene's lights as
    // the launch's (kp.no_fallthrough, checked by select_path4; DESIGN.md
    // 4.19): no draw word falls through the pick (cdf[nl] >= 1),
    // so a pick is a light or the surface and every pick word stands for three
    // draws. The counting instances keep the general code, and so do the
    // lattices with global records (no_fallthrough_mode, ipt_kparams.h).
    constexpr bool kFactPick = kK > 0 && !COUNT && no_fallthrough_mode(LMODE);
    constexpr int kRange = GEOM == IPT_GEOM_SPHERE_IN_BOX ? (BOXIN ? kRangeIn : kRangeGeneric) : kRangeRuntime;
    // the generic box instances keep the full-form trace (small, rarely run)
    constexpr bool kNearest = box_nearest(GEOM) && kRange != kRangeGeneric;
    constexpr int kBlock = block_of(LMODE, GEOM);  // this instance's workgroup size
    extern __shared__ float lds[];
    // resumable sphere-list instances: the wave walk's 64-bit test slot per
    // lane in front of the stack
    unsigned long long* wslots = reinterpret_cast<unsigned long long*>(lds);
    float* stk = lds + walk_lds_words(LMODE, GEOM);           // [MAXSUSP][F][kBlock]
    constexpr int kFrameStride = frame_stride(LMODE, GEOM);
    float* lfr = stk + MAXSUSP * kStackFields * kBlock;       // [12][kFrameStride] lane + wall frames
    LightDev* lights_lds = reinterpret_cast<LightDev*>(lfr + 12 * kFrameStride);
    float* weights_lds = reinterpret_cast<float*>(lights_lds) + kLdsLights * kLightWords;
    float* cdf_lds = weights_lds + (kLdsLights + 1);
    // kLightsGlobal: [weights | cdf | light BVH nodes] after the frames
    float* gl_lds = reinterpret_cast<float*>(lights_lds) +
                    (LMODE == kLightsLds ? kLdsLights * kLightWords + 2 * (kLdsLights + 1) : 0);
    constexpr bool kGridL = grid_lights(LMODE);
    BvhNode* lnodes_lds = reinterpret_cast<BvhNode*>(gl_lds + global_light_prefix_words(kp.n_lights, kGridL));
    float* cdf_gl = gl_lds + (kGridL ? 0 : kp.n_lights + 1);
    // kLightsGridA10L/A01L: the lattice lights' records after the cells (16-byte aligned)
    constexpr bool kLaxLds = lax_in_lds(LMODE);
    float4* lax_lds = reinterpret_cast<float4*>(reinterpret_cast<int*>(lnodes_lds) + ((kp.lg_nu * kp.lg_nv + 3) & ~3));
    int* cdf_lo_lds = reinterpret_cast<int*>(cdf_gl + kp.n_lights + 1);
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    if (tid < 60) lfr[(tid % 12) * kFrameStride + kBlock + tid / 12] = reinterpret_cast<const float*>(kp.wall_frames)[tid];
    if (LMODE == kLightsLds) {
        const float* src = reinterpret_cast<const float*>(kp.lights);
        float* dst = reinterpret_cast<float*>(lights_lds);
        for (int i = tid; i < kp.n_lights * kLightWords; i += kBlock) dst[i] = src[i];
        for (int i = tid; i <= kp.n_lights; i += kBlock) {
            weights_lds[i] = kp.weights[i];
            cdf_lds[i] = kp.cdf[i];
        }
    }
    if (global_lights(LMODE)) {
        const bool int_cdf = kp.cdf_p2;
        for (int i = tid; i <= kp.n_lights; i += kBlock) {
            if (!kGridL) gl_lds[i] = kp.weights[i];
            cdf_gl[i] = int_cdf ? __uint_as_float(cdf_threshold24(kp.cdf[i])) : kp.cdf[i];
        }
        if (kp.cdf_lo)
            for (int i = tid; i < kCdfBuckets; i += kBlock) cdf_lo_lds[i] = kp.cdf_lo[i];
        if (grid_lights(LMODE))
            for (int i = tid; i < kp.lg_nu * kp.lg_nv; i += kBlock) reinterpret_cast<int*>(lnodes_lds)[i] = kp.lgrid[i];
        if (kLaxLds)
            for (int i = tid; i < 3 * kp.n_lights; i += kBlock) lax_lds[i] = kp.lax[i];
        if (LMODE == kLightsGlobal && kp.lnodes_lds) {
            const float4* src = reinterpret_cast<const float4*>(kp.light_nodes);
            float4* dst = reinterpret_cast<float4*>(lnodes_lds);
            for (int i = tid; i < 2 * kp.n_light_nodes; i += kBlock) dst[i] = src[i];
        }
    }
    __syncthreads();
    LightSet<LMODE> LS;
    LS.lds = lights_lds;
    LS.glob = kp.lights;
    LS.wl = global_lights(LMODE) ? gl_lds : weights_lds;
    LS.cl = global_lights(LMODE) ? cdf_gl : cdf_lds;
    LS.wg = kp.weights;
    LS.cg = kp.cdf;
    if (one_light(LMODE)) {
        LS.one = kp.lights[0];
        // held in VGPRs by the non-resumable instances (+3.5 % C2; area and spow
        // stay uniform; the sphere-list instances need the registers at 4 waves)
        if (!resumable_geom(GEOM)) {
            vgpr_hold(LS.one.P); vgpr_hold(LS.one.x); vgpr_hold(LS.one.y);
            vgpr_hold(LS.one.n); vgpr_hold(LS.one.inv.c[0]); vgpr_hold(LS.one.inv.c[1]); vgpr_hold(LS.one.inv.c[2]);
        }
        LS.w0 = kp.weights[0];
        LS.c0 = kp.cdf[0];
        LS.c1 = kp.cdf[1];
    }

    // this instance's light functions (axis-aligned single light: the reduced
    // forms of ipt_path.h, exact where observed)
    auto ltrace = [&](const LightDev& L, vec3 o, vec3 d, vec3* hp, vec3* hn) -> bool {
        if constexpr (LMODE == kLightsOneA10) return light_trace_ax<1, 0, true>(L, o, d, hp, hn);
        else if constexpr (LMODE == kLightsOneA01) return light_trace_ax<0, 1, true>(L, o, d, hp, hn);
        else if constexpr (grid_lights(LMODE) && lattice_a10(LMODE)) return light_trace_ax<1, 0, true>(L, o, d, hp, hn);
        else if constexpr (grid_lights(LMODE)) return light_trace_ax<0, 1, true>(L, o, d, hp, hn);
        else return light_trace<LMODE == kLightsAny>(L, o, d, hp, hn);
    };
    auto lpdf = [&](const LightDev& L, vec3 o, bool h, vec3 hp, vec3 hn) -> float {
        if constexpr (LMODE == kLightsOneA10 || LMODE == kLightsOneA01) return light_pdf_ax<2, true>(L, o, h, hp, hn);
        else if constexpr (grid_lights(LMODE)) return light_pdf_ax<2, true>(L, o, h, hp, hn);
        else return light_pdf(L, o, h, hp, hn);
    };
    auto lsample = [&](const LightDev& L, vec3 o, float a, float b) -> vec3 {
        if constexpr (LMODE == kLightsOneA10) return light_sample_dir_ax<1, 0, true>(L, o, a, b);
        else if constexpr (LMODE == kLightsOneA01) return light_sample_dir_ax<0, 1, true>(L, o, a, b);
        else if constexpr (grid_lights(LMODE) && lattice_a10(LMODE)) return light_sample_dir_ax<1, 0, true>(L, o, a, b);
        else if constexpr (grid_lights(LMODE)) return light_sample_dir_ax<0, 1, true>(L, o, a, b);
        else return light_sample_dir<LMODE == kLightsAny>(L, o, a, b);
    };

    const int lane = tid & 63;
    const uint64_t lanemask_lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int nl = one_light(LMODE) ? 1 : kp.n_lights;  // a compile-time 1 for one light
    const float w_sdf = kp.weights[nl];
    const unsigned long long per_pass = (unsigned long long)kp.n_cand * (unsigned long long)kp.W;

    // the setup's vector loads (the single light, weights) complete here, so
    // the step loop's waits never drain them (a conservative vmcnt(0) inside
    // the loop would also drain the step's young table gathers)
    __builtin_amdgcn_s_waitcnt(0);

    // wave-local unit pool (uniform)
    unsigned long long pool_next = 0, pool_end = 0;

    // lane state. The current node lives in registers; suspended ancestors in
    // LDS as {pos.xyz, res, pending multiplier, meta = i | kind<<8}. Frames are
    // never stored: walls load theirs from the LDS table, sphere nodes rebuild
    // theirs (make_frame) in the frame phase of the step after a push or pop.
    bool active = true, has_path = false, fresh = false, need_frame = false, need_b = false;
    // the iteration's pick and draws (prologue) and CosineDdf factors (gathers)
    int pick = -1;
    float u1 = 0.0f, u2 = 0.0f, tr = 0.0f, cs_c = 0.0f, cs_s = 0.0f;
    // kFramePf: the frame-table entry (sin, cos) of the node the lane
    // builds a frame for in the next step, gathered at the end of this step,
    // with its `to` (pfok: `to` inside the table's range)
    float pfs = 0.0f, pfc = 0.0f;
    vec3 pto = v3(0, 0, 0);
    bool pfok = false;
    uint32_t unit = 0;  // < 2^32 per launch (checked by the host)
    uint32_t rpass = 0, rpix = 0, k = 0, blk = 0;
    Win8 w;
    vec3 tpos = v3(0, 0, 0);
    int fdepth = -1;  // depth of the sphere node whose frame is in the lane's column
    uint32_t finm = 0;  // bit l = the node suspended at level l has run all its iterations
    // Resumable sphere-BVH walks (sphere-list scenes): a lane whose walk is not
    // done within IPT_WALK_BUDGET node visits keeps its ray and light results
    // and resumes the walk in the next steps (doing nothing else meanwhile), so
    // a step costs the budget, not the longest walk of the workgroup.
    constexpr bool kRes = resumable_geom(GEOM);
    constexpr bool kResL = resumable_lights(LMODE, GEOM);
    // the box instances' direct trace hands its hit point to resolve (box_hitp)
    constexpr bool kBoxHit = !kRes && !kResL && GEOM == IPT_GEOM_SPHERE_IN_BOX && kNearest;
    // the frame-entry prefetch pays where every lane iterates every step; in the
    // resumable instances (lanes parked in walks) it measured -5 % on C5
    constexpr bool kFramePf = !(kRes || kResL);
    // certain light-sample skips taken within the step (the prologue below):
    // the axis-aligned single-light instances, whose ranges are proven
    constexpr bool kSkipAhead = (one_light(LMODE) || grid_lights(LMODE)) && !kResL;
    // ... and the next iteration's certain skip taken at the end of the step,
    // before its pop (the instances that pop at the end of the step)
    constexpr bool kPreSkip = kSkipAhead && kFramePf;
    bool tracing = false;  // a resumable walk (sphere list or light BVH) is in progress
    float xlmix = 0.0f;    // light walk: the running UnionDdf light sum
    vec3 xro = v3(0, 0, 0), xrd = v3(0, 0, 0), xli_pos = v3(0, 0, 0);
    int xrdepth = 0, xi = 0, xbidx = -1;
    // sphere-list walks (kRes) keep |li_pos - origin|^2 instead of li_pos
    // (resolve's only use of it), and neither the origin nor the depth: the
    // lane's node does not change while it walks, so they are (is_iter ?
    // tpos : camera) and (is_iter ? tdepth + 1 : 0); the plane hit rides in
    // xbidx as -2 - plane (-1: none), negative until a sphere wins (-7 VGPRs:
    // the C3 instance fits 128 without spills)
    float xli_y = 0.0f;
    bool xis_iter = false, xhas_li = false;
    float xmult = 0.0f, xli_pow = 0.0f, xbest = 0.0f;
    vec3 xtm = v3(0, 0, 0);  // grid walk: t of the next cell boundaries
    float tres = 0.0f;
    int ti = 0, tdepth = 0, tkind = 0;  // kind: 0..4 wall plane, 5 box sphere, 6+i extra sphere i
    uint32_t c_paths = 0, c_traced = 0, c_surf = 0, c_light = 0, c_exp = 0, c_iter = 0,
             c_lsamp = 0, c_skip = 0, c_sframe = 0, c_ltr = 0, c_drift = 0, c_nodes = 0, c_tests = 0,
             c_lnode = 0, c_ltest = 0;
    IPT_DIAG_STATE  // diagnostic builds only (ipt_diag.h)

    for (;;) {
        IPT_STAMP_AT(0);  // previous step's tail (resolve, push, stores)
        // -------------------------------------------------- unit refill
        const bool need = active && !has_path;
        const uint64_t needmask = __ballot(need);
        if (needmask) {
            const int cnt = __popcll(needmask);
            const int rank = __popcll(needmask & lanemask_lt);
            unsigned long long avail = pool_end - pool_next;
            unsigned long long my = 0;
            if ((unsigned long long)cnt > avail) {
                unsigned long long base = 0;
                if (lane == __ffsll((long long)needmask) - 1) {
                    base = atomicAdd(kp.unit_counter, (unsigned long long)kPoolChunk);
                    // every unit handed out: release the successor launch's
                    // gate (a plain vector store of this launch's sequence
                    // number; every wave that gets here stores the same value)
                    if (kp.drained && base + kPoolChunk >= kp.total_units)
                        __hip_atomic_store(kp.drained, kp.drain_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                base = __shfl(base, __ffsll((long long)needmask) - 1);
                if ((unsigned long long)rank < avail)
                    my = pool_next + rank;
                else
                    my = base + (rank - avail);
                pool_next = base + (cnt - avail);
                pool_end = base + kPoolChunk;
            } else {
                my = pool_next + rank;
                pool_next += cnt;
            }
            if (need) {
                if (my >= kp.total_units) {
                    active = false;
                } else {
                    unit = (uint32_t)my;
                    has_path = true;
                    fresh = true;
                }
            }
        }

        IPT_STAMP_AT(1);  // refill
        if (active) { IPT_PHASE(0); }
        // ------------------------------- phase 1: finalize + pop (main.cpp:177-183)
        // (kFramePf: at the end of the previous step instead -- the
        // same operations on the same state, nothing changes it in between but
        // the refill of lanes without a path)
        auto pop_node = [&]() {
        // (a lane with a path is active, and a path is fresh only between the
        // refill and the new-path phase of one step: at the end-of-step pop
        // neither flag has to be read)
        if (has_path && (kFramePf || !fresh) && !((kRes || kResL) && tracing) && ti >= ((kK > 0 ? kTreeRays : kp.n_rays) >> tdepth)) {
            // the node is done: unwind every suspended level whose node has run
            // all its iterations too (finm, set at push) in one pass -- only
            // their res/multiplier are read -- then resume the first level
            // with iterations left (or store the path's value)
            IPT_PHASE(1);
            const uint32_t m = ~finm & ((1u << tdepth) - 1u);
            const int stop = m ? 31 - (int)__clz(m) : -1;
            // every LDS read of the unwind issued before the first use -- the
            // resumed level's six fields and the res/multiplier of the first
            // two finished levels (addresses clamped to level 0 where a level
            // does not exist; those values are not used) -- so that their
            // latencies overlap instead of forming a chain; the finished
            // levels' outcomes as selects so that their loads have
            // unconditional consumers
            // (32-bit level offsets: LDS addresses, one v_mad_u32_u24 each)
            constexpr int kLevelWords = kStackFields * kBlock;
            const lds_float* sb = (const lds_float*)(stk + tid);
            auto lvl = [&](int l) { return sb + __umul24((uint32_t)(l < 0 ? 0 : l), (uint32_t)kLevelWords); };
            const lds_float* bs = lvl(stop);
            const float s0 = bs[0 * kBlock], s1 = bs[1 * kBlock], s2 = bs[2 * kBlock];
            const float s3 = bs[3 * kBlock], s4 = bs[4 * kBlock], s5 = bs[5 * kBlock];
            const lds_float* b1 = lvl(tdepth - 1);
            const float r1 = b1[3 * kBlock], m1 = b1[4 * kBlock];
            const lds_float* b2 = lvl(tdepth - 2);
            const float r2 = b2[3 * kBlock], m2 = b2[4 * kBlock];
            // the finished levels' values, one instance of the code per form of
            // res/n (a wave-uniform choice made once, not once per level).
            // n at every depth is n_rays >> d; when n_rays is a power of two,
            // res/n == res * 2^-(log2 n_rays - d) exactly (both round the same
            // exact quotient), with the factor's bits built directly: level
            // d's exponent field is 127 - log2 n_rays + d, the next level up
            // one less -- the very float ldexpf(1, d - log2 n_rays) returns (a
            // pushed node has n_rays >> d != 0, i.e. d <= log2 n_rays <= 30,
            // and d >= -2 here: the field stays within 95 .. 127), hence the
            // same product. The choice and the exponent come from n_rays
            // inside the step (scalar instructions): as loop invariants they
            // sat in spilled scalar registers, a v_readlane per use.
            // (FIXED = K: the exponent is a constant)
            uint32_t nr = kK > 0 ? 1u << kK : (uint32_t)kp.n_rays;
            if constexpr (kK == 0) asm volatile("" : "+s"(nr));
            const bool n_pow2 = kFixed || (nr != 0u && (nr & (nr - 1u)) == 0u);
            const uint32_t p2_exp = 96u + (uint32_t)__clz((int)nr);  // 127 - log2 n_rays
            float v;
            auto unwind = [&](auto p2) {
                constexpr bool kP2 = decltype(p2)::value;
                const uint32_t sc0 = (p2_exp + (uint32_t)tdepth) << 23;
                auto fin_s = [&](float r, int d, uint32_t sc) {
                    const float q = kP2 ? r * __uint_as_float(sc) : r / (float)(kp.n_rays >> (d < 0 ? 0 : d));
                    return isfinite_(r) ? q : 0.0f;
                };
                v = fin_s(tres, tdepth, sc0);
                const float v1 = fin_s(r1 + (m1 * 1.0f) * v, tdepth - 1, sc0 - (1u << 23));
                v = tdepth - 1 > stop ? v1 : v;
                const float v2 = fin_s(r2 + (m2 * 1.0f) * v, tdepth - 2, sc0 - (2u << 23));
                v = tdepth - 2 > stop ? v2 : v;
                uint32_t sc = sc0 - (3u << 23);
#pragma unroll 1
                for (int l = tdepth - 3; l > stop; --l, sc -= 1u << 23) {
                    const lds_float* b = lvl(l);
                    const float r = b[3 * kBlock] + (b[4 * kBlock] * 1.0f) * v;
                    v = 0.0f;
                    if (isfinite_(r)) v = kP2 ? r * __uint_as_float(sc) : r / (float)(kp.n_rays >> l);
                }
            };
            if constexpr (kFixed)
                unwind(std::true_type{});
            else if (n_pow2)
                unwind(std::true_type{});
            else
                unwind(std::false_type{});
            if (stop >= 0) {
                const int meta = __float_as_int(s5);
                tpos = v3(s0, s1, s2);
                tres = s3 + (s4 * 1.0f) * v;  // res += multiplier*albedo*ray_power
                // (unsigned: with n_rays > 255 a kind of 6 + sphere index >= 32768
                // sets bit 31 of the word, which must not sign-extend)
                tkind = (int)((uint32_t)meta >> (kK > 0 ? kTreeMetaShift : kp.meta_shift));
                ti = (int)__builtin_amdgcn_ubfe((uint32_t)meta, 0u, (uint32_t)(kK > 0 ? kTreeMetaShift : kp.meta_shift));  // meta_shift <= 31
                need_frame = tkind >= 5 && fdepth != stop;
                tdepth = stop;
                // (the resumed node's position and depth land in the lane's
                // registers here: no merge moves on the path-end side)
                vgpr_hold(tpos);
                vgpr_hold(tdepth);
            } else {
                kp.values[unit] = v >= 0.0f ? v : 0.0f;  // main.cpp:214
                has_path = false;
            }
        }
        };
        if (!kFramePf) pop_node();

        IPT_STAMP_AT(2);  // finalize + pop
        // the current node's frame normal (frame build below)
        auto frame_normal = [&]() -> vec3 {
            vec3 nrm;
            if (GEOM == IPT_GEOM_SPHERE_IN_BOX || tkind == 5) {
                nrm = tpos;  // normalize(position), GeometrySphereInBox.cpp:67
            } else {
                const float4 sp = kp.spheres[tkind - 6];
                nrm = tpos - v3(sp.x, sp.y, sp.z);  // FractalSpheres.cpp:91
                // GeometrySmallPt.cpp:41: -normalize(v) for the room spheres;
                // normalize(-v) is the same bits (negation is exact)
                if (GEOM == IPT_GEOM_SMALLPT && !((double)sp.w < 100.0)) nrm = -nrm;
            }
            return nrm;
        };
        constexpr bool kFrameInrange = GEOM == IPT_GEOM_SPHERE_IN_BOX;  // range-free frame roots / quotients (+1.4 % C2)
        const bool fneed = need_frame && has_path && !fresh && !((kRes || kResL) && tracing);
        IPT_STAMP_AT(3);  // (new path: later in the step)
        // iteration prologue: RNG window, UnionDdf pick (ddf.cpp:142-153) and,
        // for a cosine pick, the CosineDdf table gathers (running it one step
        // ahead, right after the direction phase, measured -2.7 %: DESIGN.md 4.3)
        const bool iter_lane = has_path && !fresh && !((kRes || kResL) && tracing);
        if constexpr (kRes) {
            // the iteration's pick, draws and CosineDdf factors live within the
            // step (set by the prologue / gathers, used by the direction phase):
            // overwritten here, they are not carried across the step loop's back
            // edge (-13 VGPRs: the sphere-list instances fit 4 waves per SIMD;
            // the others measured 1 % slower this way)
            pick = -1;
            u1 = u2 = tr = cs_c = cs_s = 0.0f;
        }
        // the cosine pick's table indices; the gathers are issued by the whole
        // wave after the prologue (index 0 for the other lanes) so that the
        // number of loads between a gather and its wait is the same on every
        // path and the compiler's waits drain only what they wait for
        uint32_t gi_a = 0, gi_b = 0;
        bool gcos = false;
        // kPreSkip: the word after the iteration's draws (the next pick) and
        // whether the end of the step may take it (set by the prologue)
        // (pre_w is read only behind pre_ok: left uninitialised, no per-step moves)
        uint32_t pre_w;
        bool pre_ok = false;
        // product FIXED = K: pre_w picks the fall-through (one draw, not three);
        // read by the pre-skip's leaf rule, only behind pre_ok as well
        bool pre_ft;
        // lattice instances: the picked light's sample fields are
        // gathered with the CosineDdf gathers (whole wave, index 0 for lanes
        // without a light pick) instead of read in the direction phase
        vec3 lpP = v3(0, 0, 0);
        float lpx = 0.0f, lpy = 0.0f, lpn = 0.0f;
        int lptype = 0;
        // (`ran`: the lane ran the prologue in this step. In the resumable
        // instances a lane keeps its prepared iteration while its walk goes on,
        // so there the gathers stay per lane.)
        auto gathers = [&](bool ran) {
            if constexpr (kRes || kResL) {
                if (ran && gcos) {
                    tr = kp.cos_a[gi_a];
                    float sp, cp;
                    sincosf_small_(two_pi_times_u24(gi_b), &sp, &cp);
                    cs_c = cp;
                    cs_s = sp;
                }
            } else {
                if constexpr (grid_lights(LMODE)) {
                    // the compact record's first 16 bytes: P.xy, x[XA], y[YA]
                    // (P.z, n.z: the lattice plane; lattice lights are diamonds)
                    const int pk = (ran && pick >= 0 && pick < nl) ? pick : 0;
                    const float4 a = kLaxLds ? lax_lds[3 * pk] : kp.lax[3 * pk];
                    lpP = v3(a.x, a.y, kp.lg_pn);
                    lpx = a.z;
                    lpy = a.w;
                    lpn = kp.lg_nn;
                    lptype = 0;
                }
                // (cos phi, sin phi) computed (the table kernel's own code): one
                // table line per cosine sample instead of two (computing r as
                // well, or non-temporal gathers, measured slower: DESIGN.md 4.3)
                tr = kp.cos_a[gcos ? gi_a : 0u];
                float sp, cp;
                sincosf_small_(two_pi_times_u24(gi_b), &sp, &cp);
                cs_c = cp;
                cs_s = sp;
            }
        };
        auto prologue = [&]() {
            if ((k >> 2) != blk) {
                w.a0 = w.b0; w.a1 = w.b1; w.a2 = w.b2; w.a3 = w.b3;
                ++blk;
                need_b = true;
            }
            if (need_b) {
                IPT_PHASE(4);
                philox_fill(w.b0, w.b1, w.b2, w.b3, blk + 1, rpass, rpix, kp.key0, kp.key1);
                need_b = false;
            }
            // j = k - 4*blk: the window was shifted above. kPreSkip: a step that
            // took the next pick's skip may end 9 words past blk, so after the
            // one shift j <= 5 (words j .. j+2 are still in the window)
            const uint32_t j = kPreSkip ? k - 4u * blk : k & 3u;
            const uint32_t rw = kPreSkip && j >= 4u ? (j & 1u ? w.b1 : w.b0) : sel4(j & 3u, w.a0, w.a1, w.a2, w.a3);
            const float r = u01(rw);
            // the single light's pick on the raw word: r < cdf[c] as w < pk_u (host-exact)
            // (kFactPick: no word falls through and pk_u0 < 2^32, select_path4:
            // one 32-bit compare)
            auto pick_w = [&](uint32_t wd) {
                if constexpr (kFactPick) return wd < (uint32_t)kp.pk_u0 ? 0 : 1;
                return (unsigned long long)wd < kp.pk_u0 ? 0 : ((unsigned long long)wd < kp.pk_u1 ? 1 : 2);
            };
            constexpr bool kPickInt = one_light(LMODE);
            // UnionDdf::sample's component: the first c with r < cdf[c] (ddf.cpp:142-153)
            auto pick_of = [&](float r) {
                int c = 0;
                if (global_lights(LMODE) && kp.cdf_lo) {
                    // the scan from the first index whose cdf exceeds r's bucket
                    // start floor(256 r)/256 (host table): every earlier entry is
                    // <= that start <= r, so the scan would pass it; a bucket holds
                    // at most 8 entries (else the table is not built)
                    c = cdf_lo_lds[(int)(r * 256.0f)];
                    if (kp.cdf_bsearch) {
                        // non-decreasing cdf: the answer is c plus the number of
                        // the entries from c on that r does not undercut, a
                        // prefix; the first three are read at once (C5: two
                        // lights per bucket), the scan past them is a rare branch
                        const float f0 = LS.cdf(min(c, nl)), f1 = LS.cdf(min(c + 1, nl)), f2 = LS.cdf(min(c + 2, nl));
                        const int n0 = (c <= nl && !(r < f0)) ? 1 : 0;
                        const int n1 = (c + 1 <= nl && !(r < f1)) ? 1 : 0;
                        const int n2 = (c + 2 <= nl && !(r < f2)) ? 1 : 0;
                        const bool more = n2 != 0;
                        c += n0 + n1 + n2;
                        if (__builtin_expect(__any(more), 0))
                            if (more) while (c <= nl && !(r < LS.cdf(c))) ++c;
                    } else {
                        while (c <= nl && !(r < LS.cdf(c))) ++c;
                    }
                } else if ((global_lights(LMODE) || LMODE == kLightsAny) && kp.cdf_bsearch) {
                    // first c with r < cdf[c] (else nl+1): the scan's answer on a
                    // non-decreasing cdf (checked at upload)
                    int hi = nl + 1;
                    while (c < hi) {
                        const int mid = (c + hi) >> 1;
                        if (r < LS.cdf(mid)) hi = mid; else c = mid + 1;
                    }
                } else {
                    while (c <= nl && !(r < LS.cdf(c))) ++c;
                }
                return c;
            };
            // the near-uniform many-light pick on the draw's 24-bit integer
            // (the staged cdf holds ceil(cdf 2^24), KParams::cdf_p2e)
            auto pick_p2w = [&](uint32_t wd) {
                const uint32_t g = wd >> 8;
                const int ce = min((int)(g >> (24 - kp.cdf_p2e)), nl);
                // (kFactPick: g < cdf_end_t = 2^24 always, no fall-through)
                if (kp.cdf_p2 == 2) {
                    // every light's threshold is exactly (i+1) 2^(24-e)
                    // (host-checked): the first i with g < T[i] is ce itself
                    if constexpr (kFactPick) return ce;  // (clamped to nl above)
                    return ce < nl ? ce : (g < kp.cdf_end_t ? nl : nl + 1);
                }
                const uint32_t fa = __float_as_uint(LS.cdf(max(ce - 1, 0))), fb = __float_as_uint(LS.cdf(ce));
                int c = (ce >= 1 && g < fa) ? ce - 1 : (g < fb ? ce : ce + 1);
                if constexpr (kFactPick) return min(c, nl);
                if (c >= nl) c = g < kp.cdf_end_t ? nl : nl + 1;
                return c;
            };
            constexpr bool kPickIntCdf = global_lights(LMODE);
            auto pick_word = [&](uint32_t wd) {
                if constexpr (kPickInt) return pick_w(wd);
                if constexpr (kPickIntCdf)
                    if (kp.cdf_p2) return pick_p2w(wd);
                return pick_of(u01(wd));
            };
            int c = (kPickInt || kPickIntCdf) ? pick_word(rw) : pick_of(r);
            uint32_t jj = j;  // the window offset of the iteration's pick (skip-ahead: j + 3)
            if constexpr (kSkipAhead) {
                // A light pick at a node on the lights' back side is a certain
                // skip: DdfFromLight::sample returns vec3() when cosinus < 1e-5
                // (lighting.cpp:125-134), and for these axis-aligned lights (one,
                // or a coplanar lattice) the sampled point's normal-axis
                // coordinate is P[2] whatever the two draws, so cosinus = n[2] *
                // -RN(RN(P[2] - o[2]) * s) (+ signed zeros, generic light code;
                // s = 1/|pos - o| >= 0: pos.z != o.z and |P[2]| >= 2^-32, so
                // |pos - o|^2 >= 2^-112 does not underflow; an overflow gives
                // s = 0 and cosinus = +-0) is <= 0 whenever n[2] * (P[2] - o[2])
                // > 0 (sa_on: host-checked). Such an iteration does nothing but
                // consume its three draws and count (main.cpp:149-163), so the
                // lane takes the next iteration's pick (word j + 3) in the same
                // step -- when the node has an iteration left and that pick's
                // draws are in the window without a shift (j <= 1: words j+3 ..
                // j+5 <= 6, and k ends below 4*(blk+2)). Same draws, same order,
                // same results; a lane on the back side of the lights spends one
                // step instead of two on the pair. (The draws below are then
                // selected at offset jj = j + 3: one pick computation serves
                // both cases.) (j = 2 as well -- words 5 .. 7, and the next
                // step reading its pick at j = 4 after one shift -- measured
                // +0.2 % on C2, -0.4 % on C5 and C3: not taken.)
                // (o.z - P.z) * n.z < 0: the rounded difference keeps its sign
                // and is zero only when o.z == P.z; an underflowed product is
                // +-0, i.e. not taken (conservative)
                const bool back = (tpos.z - kp.sa_pz) * kp.sa_nz < 0.0f;
                if ((kFixed || kp.sa_on) && c < nl && back && j <= 1u && ti + 1 < ((kK > 0 ? kTreeRays : kp.n_rays) >> tdepth)) {
                    ++ti;
                    if (COUNT) { ++c_iter; ++c_lsamp; ++c_skip; }
                    k += 3;
                    jj = j + 3u;
                    c = pick_word(j == 0u ? w.a3 : w.b0);  // word j + 3
                }
            }
            pick = c;
            // (kFactPick: c <= nl always -- the scan's last entry cdf[nl] >= 1
            // exceeds every draw)
            if (kFactPick || c <= nl) {
                // words jj+1, jj+2 (jj <= 4 in the skip-ahead instances, <= 5
                // with kPreSkip, else <= 3)
                uint32_t r1, r2;
                if constexpr (kPreSkip) {
                    // words jj+1 .. jj+3 (the last: the next pick's word, taken
                    // only at jj <= 3: the step then ends at most 9 words past
                    // blk) from one rotation of the window instead of three
                    // select trees: the four words 2h+1 .. 2h+4 of the pair h =
                    // jj >> 1 (0 .. 2), then one select each on jj's low bit.
                    // (Word 8 does not exist: at jj >= 4 the third result is
                    // another word than before, and as before not read.)
                    const bool odd = (jj & 1u) != 0u, h0 = jj < 2u, h2 = jj >= 4u;
                    auto sel3 = [&](uint32_t x0, uint32_t x1, uint32_t x2) {
                        const uint32_t t = h0 ? x0 : x1;
                        return h2 ? x2 : t;
                    };
                    const uint32_t e1 = sel3(w.a1, w.a3, w.b1), e2 = sel3(w.a2, w.b0, w.b2);
                    const uint32_t e3 = sel3(w.a3, w.b1, w.b3), e4 = h0 ? w.b0 : w.b2;
                    r1 = odd ? e2 : e1;
                    r2 = odd ? e3 : e2;
                    pre_w = odd ? e4 : e3;
                    pre_ok = jj <= 3u && (kFixed || kp.sa_on);
                    // (lattices: pick_p2w's own last test -- with cdf_p2 a pick
                    // below nl has g < T[pick] <= T[nl] on the non-decreasing cdf
                    // that cdf_p2 requires; without cdf_p2 the leaf rule is off,
                    // the whole pick_word here measured -0.9 % on C5)
                    if constexpr (kK > 0 && !COUNT && !kFactPick)
                        pre_ft = kPickIntCdf ? (pre_w >> 8) >= kp.cdf_end_t : pick_word(pre_w) > nl;
                } else {
                    const bool hi = kSkipAhead && jj >= 4u;
                    r1 = hi ? w.b1 : sel4(jj & 3u, w.a1, w.a2, w.a3, w.b0);
                    r2 = hi ? w.b2 : sel4(jj & 3u, w.a2, w.a3, w.b0, w.b1);
                }
                u1 = u01(r1);
                u2 = u01(r2);
                if (c == nl) {
                    // CosineDdf::sample (ddf.cpp:223-231) of (u1, u2): (cos_alpha, r) x
                    // (cos phi, sin phi) looked up by the draws' 24 bits
                    // (a non-temporal hint measured slower on C2 and C5)
                    // (cos_alpha = sqrtf(u1) is recomputed in the direction phase)
                    gi_a = r1 >> 8;
                    gi_b = r2 >> 8;
                    gcos = true;
                }
                k += 3;
            } else {
                k += 1;  // fall-through: defined as vec3() (reference UB, ddf.cpp:139)
            }
        };
        if (iter_lane) {
            IPT_PHASE(3);
            prologue();
        }
        gathers(iter_lane);
        // (the frame build sits between the table gathers' issue and their use)
        // ------------- phase 3: the current node's RotateDdf frame when it is a sphere node without one
        // (after a push, or a pop past a sphere descendant): built by the lane
        // itself into its LDS column. Waves share no LDS after the setup, so they
        // run without barriers (a pooled workgroup frame pass with two barriers
        // per step measured 5-13 % slower).
        if (fneed) {
            const vec3 nrm = frame_normal();
            IPT_PHASE(5);
            Frame f;
            // the sphere-in-box node's normal comes from a point on the r = 0.5
            // sphere: every root and quotient of the frame is in the range-free
            // sequences' range (make_frame<true>)
            if (GEOM == IPT_GEOM_SPHERE_IN_BOX) {
                // (sphere-list scenes: measured slower with the table's
                // gathers in their latency-bound walks)
                vec3 to;
                float fs = 0.0f, fc = 0.0f;
                if (kFramePf) {
                    // `to` and its frame-table entry, prepared at the end of
                    // the previous step (pfok: `to` inside the table's range)
                    // (the rare branch writes the prefetch's own variables --
                    // nothing reads them again before the next prefetch -- so
                    // the common path copies nothing)
                    if (__builtin_expect(__any(!pfok), 0))
                        if (!pfok) {
                            pto = kFrameInrange ? normalize_inrange_(nrm) : normalize(nrm);
                            frame_sc_lookup(kp.frame_sc, pto, pfs, pfc);
                            keep_alive(pfs);  // its wait stays in this rare branch
                            keep_alive(pfc);
                        }
                    to = pto;
                    fs = pfs;
                    fc = pfc;
                    pfok = false;
                } else {
                    to = kFrameInrange ? normalize_inrange_(nrm) : normalize(nrm);
                    frame_sc_lookup(kp.frame_sc, to, fs, fc);
                }
                if (kFrameInrange) {
                    // without the zero terms; the rare lanes where a term
                    // could decide a zero's sign take the exact build
                    bool ok;
                    f = make_frame_sc_fast(to, fs, fc, ok);
                    if (__builtin_expect(__any(!ok), 0))
                        if (!ok) f = make_frame_sc<kFrameInrange>(to, fs, fc);
                } else {
                    f = make_frame_sc<kFrameInrange>(to, fs, fc);
                }
            } else if (kFrameInrange) {
                f = make_frame<true>(normalize_inrange_(nrm));
            } else {
                // sphere-list scenes: the f64 angle, then the fast build
                // (its own range checks; a normalized `to`), exact fallback
                const vec3 to = normalize(nrm);
                float fs, fc;
                frame_angle_sc(to, &fs, &fc);
                bool ok;
                f = make_frame_sc_fast(to, fs, fc, ok);
                if (__builtin_expect(__any(!ok), 0))
                    if (!ok) f = make_frame_sc<false>(to, fs, fc);
            }
            float* c = lfr + tid;
            c[0 * kFrameStride] = f.m0.x; c[1 * kFrameStride] = f.m0.y; c[2 * kFrameStride] = f.m0.z;
            c[3 * kFrameStride] = f.m1.x; c[4 * kFrameStride] = f.m1.y; c[5 * kFrameStride] = f.m1.z;
            c[6 * kFrameStride] = f.m2.x; c[7 * kFrameStride] = f.m2.y; c[8 * kFrameStride] = f.m2.z;
            c[9 * kFrameStride] = f.iz.x; c[10 * kFrameStride] = f.iz.y; c[11 * kFrameStride] = f.iz.z;
            need_frame = false;
            fdepth = tdepth;
        }
        if (IPT_PROF && wave == 0) { IPT_PHASE(11); }  // workgroup steps (one wave counts)
        IPT_STAMP_AT(4);  // task posting, iteration prologue, Philox
        // the wave's exit test (waves are independent after the setup barrier)
        if (!__ballot(active)) break;
        IPT_STAMP_AT(5);
        // the current node's frame: its wall column or the lane's own column
        const float* frc = lfr + (tkind < 5 ? kBlock + tkind : tid);

        bool have_ray = false, is_iter = false;
        // (written by the new-path or the direction phase wherever have_ray is
        // set and read only then: left uninitialised, no per-step moves)
        // The ray's origin is the lane's node position: an iteration's ray
        // starts there, and a new path parks the camera position in tpos (no
        // node of its own yet: nothing reads tpos as a node before the
        // camera ray's push overwrites it), so no origin is copied per step.
        vec3 rd;
        int rdepth;
        // ------------- phase 2: new path (render_sample body, main.cpp:192-211), after
        // barrier B so that its camera ray is not live across the worker pass
        if (has_path && fresh) {
            IPT_PHASE(2);
            // raygen_kernel ran render_sample's per-sample work for this
            // unit (jitter, drift code and flags, camera ray, Philox block 0)
            // both records load together and are consumed here: no load of
            // this (divergent) phase is left in flight for later waits
            uint4 r0 = kp.rg[2 * unit], r1 = kp.rg[2 * unit + 1];
            keep_alive(r0);
            keep_alive(r1);
            if (r0.w == 0u) {
                has_path = false;  // not ours / out of range: already stored
            } else {
                tpos = kp.cam_pos;
                rd = v3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
                w.a2 = r1.x;
                w.a3 = r1.y;
                rpass = r1.z;
                rpix = r1.w;
                blk = 0;
                need_b = true;  // block 1 is produced by the window refill of the next iteration
                k = 2;
                rdepth = 0;
                have_ray = true;
                if (COUNT) ++c_paths;
            }
        }
        // (a fresh lane has a path, so the phase above ran for it: cleared for
        // every lane, the flag is not carried over the loop's back edge)
        fresh = false;

        // ------------------------- phase 3b: the iteration's direction (main.cpp:149-163)
        // kLightsOne: both candidate directions are computed by every lane and
        // one is selected (a mixed wave runs both anyway), so the CosineDdf
        // gathers have an unconditional consumer and stay unconditional loads
        vec3 dir_bf = v3(0, 0, 0);
        // kFactPick, one light: the light sample returned the zero vector (a
        // certain skip; dir_bf then holds the unused direction)
        bool lskip = false;
        // (the lattice instances measured 3 % slower this way: their light sample
        // reads the picked light's record, and both directions cost more there)
        constexpr bool kDirBf = one_light(LMODE);
        if constexpr (kDirBf) {
            Frame fm;
            fm.m0 = v3(frc[0 * kFrameStride], frc[1 * kFrameStride], frc[2 * kFrameStride]);
            fm.m1 = v3(frc[3 * kFrameStride], frc[4 * kFrameStride], frc[5 * kFrameStride]);
            fm.m2 = v3(frc[6 * kFrameStride], frc[7 * kFrameStride], frc[8 * kFrameStride]);
            const vec3 cdir = frame_apply(fm, v3(tr * cs_c, tr * cs_s, sqrt_inrange_(u1)));
            const vec3 zero = v3(0, 0, 0);
            if constexpr (LMODE == kLightsOneA10 || LMODE == kLightsOneA01) {
                // the light sample's own zero vector (cosinus < 1e-5) folded
                // into the pick's select: two selects per component, not three
                bool lok;
                const vec3 ldir = LMODE == kLightsOneA10
                                      ? light_sample_dir_ax_ok<1, 0, true>(LS.one, tpos, u1, u2, &lok)
                                      : light_sample_dir_ax_ok<0, 1, true>(LS.one, tpos, u1, u2, &lok);
                if constexpr (kFactPick) {
                    // the pick is a light or the surface: one select per
                    // component; the light sample's zero vector (!lok) is the
                    // skip flag below, not a third value
                    dir_bf = pick < nl ? ldir : cdir;
                    lskip = pick < nl && !lok;
                } else {
                const vec3 other = pick == nl ? cdir : zero;
                dir_bf = pick < nl && lok ? ldir : other;
                }
            } else {
                const vec3 ldir = lsample(LS.one, tpos, u1, u2);
                dir_bf = pick < nl ? ldir : (pick == nl ? cdir : zero);
            }
        }
        if (iter_lane) {
            vec3 dir = v3(0, 0, 0);
            if (kDirBf) {
                dir = dir_bf;
                if (COUNT && pick < nl) ++c_lsamp;
            } else if (pick < nl) {
                IPT_PHASE(7);
                if constexpr (grid_lights(LMODE)) {
                    // the gathered fields are all light_sample_dir_ax reads
                    constexpr int XA = lattice_a10(LMODE) ? 1 : 0, YA = 1 - XA;
                    dir = light_sample_dir_axf<XA, YA, true>(lpP, lpx, lpy, lpn, lptype, tpos, u1, u2);
                } else
                dir = lsample(LS.light(pick), tpos, u1, u2);
                if (COUNT) ++c_lsamp;
            } else if (pick == nl) {
                Frame fm;
                fm.m0 = v3(frc[0 * kFrameStride], frc[1 * kFrameStride], frc[2 * kFrameStride]);
                fm.m1 = v3(frc[3 * kFrameStride], frc[4 * kFrameStride], frc[5 * kFrameStride]);
                fm.m2 = v3(frc[6 * kFrameStride], frc[7 * kFrameStride], frc[8 * kFrameStride]);
                // cosine_sample_local from the tables: (r cos phi, r sin phi, cos_alpha)
                // with u2 = r and cos_alpha = sqrtf(u1)
                // u1 is 0 or in [2^-24, 1): the range-free root is sqrtf there
                // (math probe 13 is exhaustive on [2^-96, 2^126); sqrt_inrange_(0) = +0)
                dir = frame_apply(fm, v3(tr * cs_c, tr * cs_s, sqrt_inrange_(u1)));
            }
            ++ti;
            if (COUNT) ++c_iter;
            if (lskip || is_zero(dir)) {
                if (COUNT) ++c_skip;
            } else {
                rd = dir;
                rdepth = tdepth + 1;
                have_ray = true;
                is_iter = true;
            }
        }
        const vec3 ro = tpos;
        IPT_STAMP_AT(8);  // direction
        // --------------------------------------------- phase 4: trace + resolve
        // the child's value (main.cpp:100-143) from its traces, then push it,
        // add it to the current node's sum, or finish the path
        // kBoxHit: the trace already holds the winner's point box_hitp = o + d*t
        // wherever prim >= 0, the only place si_pos is observed (uninitialised
        // like the ray: no merge moves)
        vec3 box_hitp;
        auto resolve = [&](bool traced, float t, int prim, vec3 o, vec3 d, int depth, bool iter, float mult,
                           bool has_li, float li_y, float li_pow) {
            float cv = 0.0f;
            bool push = false;
            vec3 si_pos = v3(0, 0, 0);
            {
                // the reference's hit / light / expand decision (main.cpp:100-143)
                // as selects (the branches only cost exec-mask bookkeeping in
                // waves that mix outcomes: +1 %)
                const bool has_si = prim >= 0;
                if (COUNT && traced) {
                    ++c_traced;
                    c_surf += has_si ? 1u : 0u;
                    c_light += has_li ? 1u : 0u;
                }
                if constexpr (kBoxHit)  // (no capture of box_hitp in the other instances)
                    si_pos = box_hitp;
                else
                    si_pos = o + d * t;
                // y = |li_pos - o|^2, computed by the caller
                const vec3 ea = si_pos - o;
                const float x = dot(ea, ea), y = li_y;
                // longer(si_pos - o, li_pos - o), asked only where both hits exist
                const bool need = has_li && has_si;
                bool lg = x > y * 1.000001907f && y >= 1e-30f;
                const bool tie = need && (!lg && !(x <= y));
                if (__builtin_expect(__any(tie), 0))
                    if (tie) lg = sqrt_(x) > sqrt_(y);
                const bool li_wins = has_li && (!has_si || lg);
                const int nchild = (kK > 0 ? kTreeRays : kp.n_rays) >> depth;
                const float zero = 0.0f;
                // 0/0 for an expanded node without children: the NaN that
                // poisons the parent (main.cpp:181)
                const float cv_exp = nchild == 0 ? zero / (float)nchild : 0.0f;
                cv = li_wins ? (isfinite_(li_pow) ? li_pow : 1.0f) : (has_si ? cv_exp : 0.0f);
                cv = traced ? cv : 0.0f;
                push = traced && !li_wins && has_si && nchild != 0;
                if (COUNT && traced && !li_wins && has_si) ++c_exp;
            }
            if (push) {
                IPT_PHASE(10);
                if (iter) {
                    const uint32_t lbit = 1u << tdepth;
                    finm = (finm & ~lbit) | (ti >= ((kK > 0 ? kTreeRays : kp.n_rays) >> tdepth) ? lbit : 0u);
                    lds_float* b = (lds_float*)(stk + tid) + __umul24((uint32_t)tdepth, (uint32_t)(kStackFields * kBlock));  // (32-bit LDS address)
                    b[0 * kBlock] = tpos.x;
                    b[1 * kBlock] = tpos.y;
                    b[2 * kBlock] = tpos.z;
                    b[3 * kBlock] = tres;
                    b[4 * kBlock] = mult;
                    b[5 * kBlock] = __uint_as_float((uint32_t)ti | ((uint32_t)tkind << (kK > 0 ? kTreeMetaShift : kp.meta_shift)));
                }
                tpos = si_pos;
                tkind = prim;
                if (prim >= 5) {
                    need_frame = true;  // built by the frame pass of the next step
                    if (COUNT) ++c_sframe;
                }
                tres = 0.0f;
                ti = 0;
                tdepth = depth;
            } else if (iter) {
                tres = tres + (mult * 1.0f) * cv;
            } else {
                // the camera ray itself ended (light, miss, depth_max or n_rays==0)
                kp.values[unit] = cv >= 0.0f ? cv : 0.0f;
                has_path = false;
            }
        };
        if constexpr (kResL) {
            // many lights: the light-BVH walk (same order and arithmetic as the
            // full walk below) is bounded per step and resumed; then the mixture
            // value, the geometry trace and resolve, as below
            if (have_ray) {
                IPT_PHASE(8);
                if (COUNT) c_ltr += (uint32_t)nl * ((is_iter ? 1u : 0u) + ((rdepth < kp.depth_max) ? 1u : 0u));
                xro = ro;
                xrd = rd;
                xrdepth = rdepth;
                xis_iter = is_iter;
                xlmix = 0.0f;
                xhas_li = false;
                xli_pos = v3(0, 0, 0);
                xli_pow = 0.0f;
                xi = 0;
                tracing = true;
            }
            if (tracing) {
                if (kp.n_light_nodes > 0) {
                    const vec3 inv = v3(safe_rcp(xrd.x), safe_rcp(xrd.y), safe_rcp(xrd.z));
                    auto walk = [&](const BvhNode* __restrict__ lnodes) {
                    int budget = IPT_LWALK_BUDGET;
                    while (xi < kp.n_light_nodes && budget > 0) {
                        int leaf = -1;
                        while (xi < kp.n_light_nodes && budget > 0) {
                            --budget;
                            const BvhNode nd = lnodes[xi];
                            if (COUNT) ++c_lnode;
                            const bool enter = bvh_box_entry(nd, xro, inv) != inf_();
                            if (enter && nd.leaf >= 0) {
                                leaf = nd.leaf;
                                xi = nd.skip;
                                break;
                            }
                            xi = enter ? xi + 1 : nd.skip;
                        }
                        if (leaf >= 0) {
                            const int first = leaf & 0xffffff, cnt = leaf >> 24;
                            for (int l = first; l < first + cnt; ++l) {
                                const LightDev& L = LS.light(l);
                                vec3 hp, hn;
                                const bool h = light_trace<false>(L, xro, xrd, &hp, &hn);
                                if (COUNT) ++c_ltest;
                                if (xis_iter) xlmix += LS.weight(l) * light_pdf(L, xro, h, hp, hn);
                                if (h && (!xhas_li || longer(xli_pos - xro, hp - xro))) {
                                    xhas_li = true;
                                    xli_pos = hp;
                                    xli_pow = L.spow;
                                }
                            }
                        }
                    }
                    };
                    if (kp.lnodes_lds)
                        walk(lnodes_lds);
                    else
                        walk(kp.light_nodes);
                } else {
                    for (int l = 0; l < nl; ++l) {
                        const LightDev& L = LS.light(l);
                        vec3 hp, hn;
                        const bool h = light_trace<false>(L, xro, xrd, &hp, &hn);
                        if (COUNT) ++c_ltest;
                        if (xis_iter) xlmix += LS.weight(l) * light_pdf(L, xro, h, hp, hn);
                        if (h && (!xhas_li || longer(xli_pos - xro, hp - xro))) {
                            xhas_li = true;
                            xli_pos = hp;
                            xli_pow = L.spow;
                        }
                    }
                    xi = kp.n_light_nodes;
                }
                if (xi >= kp.n_light_nodes) {
                    tracing = false;
                    float mult = 0.0f;
                    if (xis_iter) {
                        const float* fc = lfr + (tkind < 5 ? kBlock + tkind : tid);
                        Frame fz;
                        fz.iz = v3(fc[9 * kFrameStride], fc[10 * kFrameStride], fc[11 * kFrameStride]);
                        const float sdf_val = frame_cosine_value(fz, xrd);
                        const float mix = xlmix + w_sdf * sdf_val;
                        mult = div_(sdf_val, mix);
                    }
                    int prim = -1;
                    float t = inf_();
                    if (xrdepth < kp.depth_max) {
                        IPT_PHASE(9);
                        vec3 hitp;
                        t = trace_geometry<COUNT, GEOM, kNearest, kRange>(kp, xro, xrd, &prim, &hitp, c_nodes, c_tests);
                    }
                    const vec3 eb = xli_pos - xro;
                    resolve(xrdepth < kp.depth_max, t, prim, xro, xrd, xrdepth, xis_iter, mult, xhas_li, dot(eb, eb),
                            xli_pow);
                }
            }
        } else {
        if (have_ray) {
            IPT_PHASE(8);
            // lights: per-light traces feed both UnionDdf::value (ddf.cpp:157-162)
            // and the child's CollectionLighting::traceRayToLight
            float lmix = 0.0f;
            bool has_li = false;
            vec3 li_pos = v3(0, 0, 0);
            float li_pow = 0.0f;
            // coplanar lattice: the lights' shared n[2]*d[2] and plane quotient,
            // computed once by the lookup below with light_trace_ax's operations
            float lg_ndir = 0.0f, lg_t = 0.0f;
            vec3 lg_q = v3(0, 0, 0);
            auto light_step_with = [&](const LightDev& L, float wl) {
                vec3 hp, hn;
                bool h;
                if constexpr (grid_lights(LMODE)) {
                    constexpr int XA = lattice_a10(LMODE) ? 1 : 0, YA = 1 - XA;
                    h = light_trace_ax_q<XA, YA>(L, lg_ndir, lg_t, lg_q, &hp, &hn);
                } else {
                    h = ltrace(L, ro, rd, &hp, &hn);
                }
                if (COUNT) ++c_ltest;
                if (is_iter) lmix += wl * lpdf(L, ro, h, hp, hn);
                if constexpr (LMODE == kLightsOneA10 || LMODE == kLightsOneA01) {
                    // the only light: a hit is the nearest one, and its point
                    // (always written by light_trace_ax) and power are read
                    // only behind has_li (resolve): taken without selects
                    has_li = h;
                    li_pos = hp;
                    li_pow = L.spow;
                } else
                if (h && (!has_li || longer(li_pos - ro, hp - ro))) {
                    has_li = true;
                    li_pos = hp;
                    li_pow = L.spow;
                }
            };
            auto light_step = [&](int l) {
                if constexpr (grid_lights(LMODE)) {
                    // the lattice light from its 48-byte record: exactly the
                    // fields light_trace_ax / light_pdf_ax read (ipt_path.h LightAx)
                    constexpr int XA = lattice_a10(LMODE) ? 1 : 0, YA = 1 - XA;
                    float4 a, b, c;
                    // (a plain `if` on the constant: the lambda then captures lax_lds in
                    // every lattice instance, which keeps their register assignment)
                    if (kLaxLds) {
                        a = lax_lds[3 * l]; b = lax_lds[3 * l + 1]; c = lax_lds[3 * l + 2];
                    } else {
                        const float4* r = kp.lax + 3 * l;
                        a = r[0]; b = r[1]; c = r[2];
                    }
                    LightDev L;
                    L.P = v3(a.x, a.y, kp.lg_pn);
                    L.x = XA == 0 ? v3(a.z, 0.0f, 0.0f) : v3(0.0f, a.z, 0.0f);
                    L.y = YA == 0 ? v3(a.w, 0.0f, 0.0f) : v3(0.0f, a.w, 0.0f);
                    L.n = v3(0.0f, 0.0f, kp.lg_nn);
                    L.inv.c[XA] = v3(b.x, 0.0f, 0.0f);
                    L.inv.c[YA] = v3(0.0f, b.y, 0.0f);
                    L.inv.c[2] = v3(0.0f, 0.0f, 0.0f);
                    L.area = b.z;
                    L.spow = b.w;
                    L.type = 0;
                    L.pad = 0;
                    light_step_with(L, c.x);
                } else {
                    light_step_with(LS.light(l), LS.weight(l));
                }
            };
            // the reference's event count: every light traced once for the
            // pdf (iterations) and once for traceRayToLight (depth < max)
            if (COUNT) c_ltr += (uint32_t)nl * ((is_iter ? 1u : 0u) + ((kK > 0 || rdepth < kp.depth_max) ? 1u : 0u));
            if constexpr (grid_lights(LMODE)) {
                // the ray's point on the lights' plane and its cell(s): every
                // light whose exact test can pass lies in a cell within
                // kp.lg_e cells of that point (LightGrid::e, derived per
                // lattice by light_grid_build in ipt_path.h from the lattice's
                // tolerance and the rounding of u, v; as small as 2^-14 -- it
                // holds because the light tests below take the same plane
                // point q as this lookup), so the lights of those <= 4 cells,
                // in index order, are the scan's hits (a light that is not hit
                // adds +0 to lmix and is never nearest)
                constexpr int XA = lattice_a10(LMODE) ? 1 : 0, YA = 1 - XA;
                // (the lattice's ranges are proven like the single light's,
                // light_ranges_box: the range-free quotient of light_trace_ax,
                // shared with the light tests below)
                const float n_dir = kp.lg_nn * comp<2>(rd);
                const float num = kp.lg_nn * (kp.lg_pn - comp<2>(ro));
                const float t = div_inrange_(num, n_dir);
                lg_ndir = n_dir;
                lg_t = t;
                lg_q = ro + rd * t;
                const float u = (comp<XA>(lg_q) - kp.lg_u0) * kp.lg_icw;
                const float v = (comp<YA>(lg_q) - kp.lg_v0) * kp.lg_ich;
                int cand[4] = {-1, -1, -1, -1};
                const float e = kp.lg_e;
                if (u > -1.0f && u < (float)kp.lg_nu + 1.0f && v > -1.0f && v < (float)kp.lg_nv + 1.0f) {
                    const int i0 = (int)floorf(u - e), i1 = (int)floorf(u + e);
                    const int j0 = (int)floorf(v - e), j1 = (int)floorf(v + e);
                    const int* cells = reinterpret_cast<const int*>(lnodes_lds);
                    auto cell = [&](int i, int j) {
                        const bool in = i >= 0 && i < kp.lg_nu && j >= 0 && j < kp.lg_nv;
                        return in ? cells[i + kp.lg_nu * j] : -1;
                    };
                    cand[0] = cell(i0, j0);
                    cand[1] = i1 != i0 ? cell(i1, j0) : -1;
                    cand[2] = j1 != j0 ? cell(i0, j1) : -1;
                    cand[3] = (i1 != i0 && j1 != j0) ? cell(i1, j1) : -1;
                }
                // ascending index order (-1 = none sorts last as 0xffffffff);
                // with the per-lattice margin a second candidate cell is rare
                // (C5: ~1 lookup in 8 000), so the sorting network runs only in
                // waves where some lane has one
                uint32_t c0 = (uint32_t)cand[0], c1 = (uint32_t)cand[1], c2 = (uint32_t)cand[2], c3 = (uint32_t)cand[3];
                auto cs = [](uint32_t& a, uint32_t& b) { const uint32_t lo = a < b ? a : b; b = a < b ? b : a; a = lo; };
                if (__builtin_expect(__any((c1 & c2 & c3) != 0xffffffffu), 0)) {
                    cs(c0, c1); cs(c2, c3); cs(c0, c2); cs(c1, c3); cs(c1, c2);
                }
                if (c0 != 0xffffffffu) light_step((int)c0);
                if (c1 != 0xffffffffu) light_step((int)c1);
                if (c2 != 0xffffffffu) light_step((int)c2);
                if (c3 != 0xffffffffu) light_step((int)c3);
            } else if (LMODE == kLightsGlobal && kp.n_light_nodes > 0) {
                // index-ordered light BVH (ipt_bvh.h): lights met in scan order;
                // a skipped light would add +0 to lmix and never be nearest
                const vec3 inv = v3(safe_rcp(rd.x), safe_rcp(rd.y), safe_rcp(rd.z));
                auto walk = [&](const BvhNode* __restrict__ lnodes) {
                int i = 0;
                // while-while: walk to the next entered leaf, then run the
                // leaf's light steps with every lane that stands on one
                while (i < kp.n_light_nodes) {
                    int leaf = -1;
                    while (i < kp.n_light_nodes) {
                        const BvhNode nd = lnodes[i];
                        if (COUNT) ++c_lnode;
                        const bool enter = bvh_box_entry(nd, ro, inv) != inf_();
                        if (enter && nd.leaf >= 0) {
                            leaf = nd.leaf;
                            i = nd.skip;
                            break;
                        }
                        i = enter ? i + 1 : nd.skip;
                    }
                    if (leaf >= 0) {
                        const int first = leaf & 0xffffff, cnt = leaf >> 24;
                        for (int l = first; l < first + cnt; ++l) light_step(l);
                    }
                }
                };
                if (kp.lnodes_lds)
                    walk(lnodes_lds);
                else
                    walk(kp.light_nodes);
            } else {
                for (int l = 0; l < nl; ++l) light_step(l);
            }
            IPT_STAMP_AT(9);  // light traces + pdf
            float mult = 0.0f;
            if (is_iter) {
                Frame fz;
                fz.iz = v3(frc[9 * kFrameStride], frc[10 * kFrameStride], frc[11 * kFrameStride]);
                const float sdf_val = frame_cosine_value(fz, rd);
                const float mix = lmix + w_sdf * sdf_val;
                mult = div_(sdf_val, mix);
            }
            // child ray_power (main.cpp:100-143): the geometry trace, then resolve
            if (kRes && rdepth < kp.depth_max && (kp.n_nodes > 0 || kp.n_grid > 0)) {
                // resumable walk: keep the ray and the light results, planes now
                xrd = rd;
                xis_iter = is_iter;
                xmult = mult;
                xhas_li = has_li;
                {
                    const vec3 eb = li_pos - ro;
                    xli_y = dot(eb, eb);
                }
                xli_pow = li_pow;
                int xp = -1;
                xi = 0;
                xbest = inf_();
                if (GEOM == IPT_GEOM_SPHERES_IN_BOX)
                    xbest = kp.box_inrange ? trace_box_planes_only<true>(ro, rd, &xp)
                                           : trace_box_planes_only<false>(ro, rd, &xp);
                xbidx = -2 - xp;
                if (kp.n_grid > 0) sphere_grid_init(kp, ro, rd, xi, xtm);
                tracing = true;
            } else {
                int prim = -1;
                float t = inf_();
                if (kK > 0 || rdepth < kp.depth_max) {
                    IPT_PHASE(9);
                    t = trace_geometry<COUNT, GEOM, kNearest, kRange>(kp, ro, rd, &prim, &box_hitp, c_nodes, c_tests);
                    IPT_STAMP_AT(10);  // mixture value + geometry trace
                }
                const vec3 eb = li_pos - ro;
                resolve(kK > 0 || rdepth < kp.depth_max, t, prim, ro, rd, rdepth, is_iter, mult, has_li, dot(eb, eb), li_pow);
            }
        }
        IPT_STAMP_AT(11);  // resolve + push
        // (kRes) the walking ray's origin: the lane's node or the camera
        const vec3 xo = xis_iter ? tpos : kp.cam_pos;
        if (kRes && kp.n_grid > 0) {
            // the whole wave walks (the item tests are spread over its lanes)
            if (__ballot(tracing))
                sphere_grid_walk_wave<COUNT>(kp, tracing, xo, xrd, xi, xtm, xbest, xbidx, IPT_GRID_BUDGET,
                                             wslots + (tid & ~63), lane, c_nodes, c_tests IPT_DIAG_ARGS);
            if (tracing && xi < 0) {
                tracing = false;
                if (xbidx >= 0) xbidx = grid_item_index(kp, xbidx);  // item position -> original index
#if IPT_RAYLOG
                if (!COUNT && kp.raylog) {
                    const unsigned long long k = atomicAdd(kp.raylog_n, 1ull);
                    if (k % kp.raylog_every == 0 && k / kp.raylog_every < kp.raylog_cap) {
                        RayLogRec r;
                        r.o[0] = xo.x; r.o[1] = xo.y; r.o[2] = xo.z; r.t = xbest;
                        r.d[0] = xrd.x; r.d[1] = xrd.y; r.d[2] = xrd.z; r.hit = xbidx;
                        kp.raylog[k / kp.raylog_every] = r;
                    }
                }
#endif
                resolve(true, xbest, xbidx >= 0 ? 6 + xbidx : -2 - xbidx, xo, xrd, xis_iter ? tdepth + 1 : 0, xis_iter,
                        xmult, xhas_li, xli_y, xli_pow);
            }
        } else if (kRes && tracing) {  // no grid: the sphere BVH
            IPT_PHASE(9);
            sphere_bvh_walk<COUNT>(kp, xo, xrd, xi, xbest, xbidx, IPT_WALK_BUDGET, c_nodes, c_tests);
            if (xi >= kp.n_nodes) {
                tracing = false;
                resolve(true, xbest, xbidx >= 0 ? 6 + xbidx : -2 - xbidx, xo, xrd, xis_iter ? tdepth + 1 : 0, xis_iter,
                        xmult, xhas_li, xli_y, xli_pow);
            }
        }
        }  // !kResL
        if constexpr (kPreSkip) {
            // The next iteration of the lane's node -- the same node's next one,
            // or the first of the child pushed in this step -- is a certain skip
            // when its pick word (read by the prologue: word jj+3) picks a light
            // and the node lies behind the lights' plane (the prologue's
            // skip-ahead argument). It does nothing but consume its three draws
            // and count (main.cpp:149-163), so it is taken here: a node whose
            // last iteration it was is then done and popped below in this step
            // (instead of a step of its own for the skip). Same draws in the
            // same order, same counts.
            // (as selects: no exec-mask branch)
            const bool back = (tpos.z - kp.sa_pz) * kp.sa_nz < 0.0f;
            const bool lpick = (unsigned long long)pre_w < kp.sa_u;
            // Product FIXED = K: the leaf behind the plane. A
            // node at depth K has one iteration, whose ray (rdepth K + 1, no
            // children) returns the light's power, 0/0 on a surface or 0 on a
            // miss. Strictly behind the plane that ray reaches no light
            // whatever the pick: in light_trace_ax num = n.z (P.z - o.z) has
            // n.z's sign (or is +-0), a hit needs n_dir < 0, so t = num / n_dir
            // is negative or a zero and lt_1em6 rejects it (the lattice's shared
            // quotient is the same expression). The node's sum is then 0 +
            // mult {NaN, +-0}, NaN or +0, and fin_s returns +0: its value does
            // not depend on what it draws, and its draw count is its pick
            // word's class, three words (pick <= nl) or one (the fall-through,
            // pre_ft). So the child just pushed at depth K (ti == 0 there)
            // takes its iteration here whatever pre_w picks, and the pop below
            // unwinds it in this step with the pop's own arithmetic: the child
            // costs no lane-step, and its frame is never built. The counting
            // instances run the iteration: the oracle counts its events.
            // (lattices: where the pick word's class is one compare, cdf_p2)
            const bool leaf = kK > 0 && !COUNT && tdepth == kK && (!global_lights(LMODE) || kp.cdf_p2 != 0);
            const bool take = iter_lane && pre_ok && back && ti < ((kK > 0 ? kTreeRays : kp.n_rays) >> tdepth) &&
                              (kK > 0 && !COUNT ? lpick || leaf : lpick);
            ti += take ? 1 : 0;
            // (a light pick is not the fall-through: pre_ft is true only on a leaf's take)
            // (kFactPick: no fall-through, every pick word stands for three draws)
            if constexpr (kFactPick)
                k += take ? 3u : 0u;
            else
            k += take ? (kK > 0 && !COUNT ? (pre_ft ? 1u : 3u) : 3u) : 0u;
            if (COUNT) {
                c_iter += take ? 1u : 0u;
                c_lsamp += take ? 1u : 0u;
                c_skip += take ? 1u : 0u;
            }
        }
        if constexpr (kFramePf) {
            pop_node();
            IPT_STAMP_AT(6);  // pop (end of step)
            if constexpr (kFrameInrange) {
                // the frame the lane builds in the next step (a sphere node
                // pushed in this step, or popped back to with its column
                // overwritten): `to` and the table gather now, consumed there
                if (need_frame && has_path) {
                    const vec3 to = normalize_inrange_(tpos);
                    const uint32_t u = f2u(to.z), mz = u & 0x7fffffffu;
                    pfok = mz - kFrameTabLo <= kFrameTabSpan;
                    if (pfok) {
                        const float2 e = kp.frame_sc[((mz - kFrameTabLo) << 1) | (u >> 31)];
                        pfs = e.x;
                        pfc = e.y;
                        pto = to;
                    }
                }
            }
            IPT_STAMP_AT(7);  // next frame's `to` + table gather
        }
    }

    IPT_DIAG_FLUSH(kp.counters, kNumCounters)
    if (COUNT) {
        atomicAdd(&kp.counters[0], (unsigned long long)c_paths);
        atomicAdd(&kp.counters[1], (unsigned long long)c_traced);
        atomicAdd(&kp.counters[2], (unsigned long long)c_surf);
        atomicAdd(&kp.counters[3], (unsigned long long)c_light);
        atomicAdd(&kp.counters[4], (unsigned long long)c_exp);
        atomicAdd(&kp.counters[5], (unsigned long long)c_iter);
        atomicAdd(&kp.counters[6], (unsigned long long)c_lsamp);
        atomicAdd(&kp.counters[7], (unsigned long long)c_skip);
        atomicAdd(&kp.counters[8], (unsigned long long)c_sframe);
        atomicAdd(&kp.counters[9], (unsigned long long)c_ltr);
        atomicAdd(&kp.counters[10], (unsigned long long)c_drift);
        atomicAdd(&kp.counters[11], (unsigned long long)c_nodes);
        atomicAdd(&kp.counters[12], (unsigned long long)c_tests);
        atomicAdd(&kp.counters[13], (unsigned long long)c_lnode);
        atomicAdd(&kp.counters[14], (unsigned long long)c_ltest);
    }
}

// ------------------------------------------------------------------ preview
// ray_power_preview (main.cpp:55-92) in place of ray_power_recursive
// (IPT_FLAG_PREVIEW): one geometry trace and one traceRayToLight per camera
// ray, 1 for a visible light, 0 for a miss, dot(normal, -direction) /
// length(direction) for a surface. One thread per work unit, raygen, trace and
// shade fused: no unit pool, no DFS stack, no raygen records, no LDS, and
// neither sampling table is read.
// ipt_preview_values' per-sample outputs (FULL instances; either may be null)
struct PreviewOut {
    uint8_t* kinds;  // [units] outcome | si << 2 | li << 3, 0xff untraced
    float* hits;     // [units][6] position, normal
};
// surface_intersection::normal of the hit primitive, as geometry_trace's
// callers see it: -planes[i] of GeometrySphereInBox.cpp:13-17 (the negated
// zeros included), GeometryFloor / GeometryCorner's constants,
// normalize(position [- centre]) and GeometrySmallPt.cpp:41's flip (the path
// kernel's frame_normal, normalized)
template <int GEOM>
__device__ __forceinline__ vec3 preview_normal(const KParams& kp, int prim, vec3 pos) {
    if (GEOM == IPT_GEOM_FLOOR) return v3(0.0f, 0.0f, 1.0f);
    if (GEOM == IPT_GEOM_CORNER) return v3(prim == 0 ? 1.0f : 0.0f, prim == 1 ? 1.0f : 0.0f, prim == 2 ? 1.0f : 0.0f);
    if (prim < 5) {
        const float one = prim >= 3 ? 1.0f : -1.0f;
        return v3(prim == 0 || prim == 3 ? one : -0.0f, prim == 1 ? one : -0.0f, prim == 2 || prim == 4 ? one : -0.0f);
    }
    if (GEOM == IPT_GEOM_SPHERE_IN_BOX) return normalize(pos);
    const float4 sp = kp.spheres[prim - 6];
    const vec3 v = normalize(pos - v3(sp.x, sp.y, sp.z));
    if (GEOM == IPT_GEOM_SMALLPT && !((double)sp.w < 100.0)) return -v;
    return v;
}
// FULL: the counting / AOV instance (IPT_FLAG_COUNTERS, ipt_preview_values);
// the displayed path's instance carries neither the counters nor the stores.
template <bool FULL, int GEOM>
__global__ __launch_bounds__(256) void preview_kernel(const KParams kp, const PreviewOut po) {
    const unsigned long long unit = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    // (every lane stays to the end: the FULL instances' wave sums)
    const bool in = unit < kp.total_units;
    uint32_t c_nodes = 0, c_tests = 0, c_lnode = 0, c_ltest = 0;
    bool drift = false, valid = false, has_si = false, has_li = false;
    if (in) {
        const bool sharded = !(kp.n_shards <= 1 || kp.tile_rows <= 0);
        const RayGen g = new_path_setup(kp, unit, sharded, kp.cand_rows);
        drift = g.drift;
        valid = g.valid;
        uint8_t kind = 0xff;
        vec3 hpos = v3(0, 0, 0), hnrm = v3(0, 0, 0);
        if (valid) {
            const vec3 o = kp.cam_pos, d = g.rd;
            // CollectionLighting::traceRayToLight (CollectionLighting.cpp:23-34):
            // the running compare in index order. More than kLdsLights
            // AreaLights: the index-ordered light BVH (a skipped light is
            // never hit); otherwise the scan itself, lights of any type
            vec3 li_pos = v3(0, 0, 0);
            auto light_step = [&](int l) {
                vec3 hp, hn;
                const bool h = light_trace<true>(kp.lights[l], o, d, &hp, &hn);
                if (FULL) ++c_ltest;
                if (h && (!has_li || longer(li_pos - o, hp - o))) {
                    has_li = true;
                    li_pos = hp;
                }
            };
            if (kp.n_light_nodes > 0) {
                const vec3 inv = v3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z));
                int i = 0;
                while (i < kp.n_light_nodes) {
                    const BvhNode nd = kp.light_nodes[i];
                    if (FULL) ++c_lnode;
                    const bool enter = bvh_box_entry(nd, o, inv) != inf_();
                    if (enter && nd.leaf >= 0) {
                        const int first = nd.leaf & 0xffffff, cnt = nd.leaf >> 24;
                        for (int l = first; l < first + cnt; ++l) light_step(l);
                    }
                    i = (enter && nd.leaf < 0) ? i + 1 : nd.skip;
                }
            } else {
                for (int l = 0; l < kp.n_lights; ++l) light_step(l);
            }
            int prim = -1;
            vec3 unused;
            const float t = trace_geometry<FULL, GEOM, false>(kp, o, d, &prim, &unused, c_nodes, c_tests);
            has_si = prim >= 0;
            const vec3 si_pos = o + d * t;
            // main.cpp:64-66 (the path kernel's depth-0 comparison)
            const bool li_wins = has_li && (!has_si || longer(si_pos - o, li_pos - o));
            float v = li_wins ? 1.0f : 0.0f;
            if (!li_wins && has_si) {
                hnrm = preview_normal<GEOM>(kp, prim, si_pos);
                hpos = si_pos;
                v = div_(dot(hnrm, -d), length(d));  // main.cpp:88
            }
            kp.values[unit] = v >= 0.0f ? v : 0.0f;  // main.cpp:214
            if (li_wins) hpos = li_pos;
            kind = (uint8_t)((li_wins ? 2 : (has_si ? 1 : 0)) | (has_si ? 4 : 0) | (has_li ? 8 : 0));
        }
        if (FULL) {
            if (po.kinds) po.kinds[unit] = kind;
            if (po.hits) {
                float* h = po.hits + 6 * unit;
                h[0] = hpos.x; h[1] = hpos.y; h[2] = hpos.z;
                h[3] = hnrm.x; h[4] = hnrm.y; h[5] = hnrm.z;
            }
        }
    }
    if (FULL && kp.count) {
        // the reference restatement's events: a path and a traced ray per
        // valid sample, every light traced once by traceRayToLight
        const uint32_t nl = valid ? (uint32_t)kp.n_lights : 0u;
        const uint32_t vals[10] = {valid ? 1u : 0u, valid ? 1u : 0u, has_si ? 1u : 0u, has_li ? 1u : 0u, nl,
                                   drift ? 1u : 0u, c_nodes, c_tests, c_lnode, c_ltest};
        const int slot[10] = {0, 1, 2, 3, 9, 10, 11, 12, 13, 14};
        for (int k = 0; k < 10; ++k) {
            const int s = wave_scan_add((int)vals[k]);  // (< 2^31 per wave)
            if ((threadIdx.x & 63) == 63 && s) atomicAdd(&kp.counters[slot[k]], (unsigned long long)(uint32_t)s);
        }
    }
}

struct AParams {
    int W, H, spp, n_cand;
    const int* cand_of_row;  // [H] candidate index or -1
    const float* values;
    const uint8_t* codes;
    const uint8_t* flags;
    int tile_rows, n_shards, shard_id;
    float* pixels;
    uint32_t* counters;
    float* sums;
    float* pixel_max;
    // [2]: the launch's first block start and last block end on the 100 MHz
    // wall clock (atomic min / max; the host presets them), for its duration
    unsigned long long* clk;
};
// The ADAPT instances' parameters (ipt_render_masked_device): AParams and,
// appended after clk, the caller's mask [H][W] and second-moment plane [H][W],
// either may be null. A type of its own, so that the unmasked instances keep
// AParams' size and with it the offsets of the kernel's hidden arguments: they
// stay the parent's instruction for instruction, immediates included.
struct AParamsAdapt : AParams {
    const uint8_t* mask;
    float* m2;
};
template <bool ADAPT>
using AParamsOf = std::conditional_t<ADAPT, AParamsAdapt, AParams>;

__device__ __forceinline__ void add_ray(float v, float& p, uint32_t& c, float& s, float& m) {
    // GridRenderPlane::addRay (GridRenderPlane.cpp:68-73)
    p = (p * (float)c + v) / (float)(c + 1u);
    ++c;
    s += v;
    if (p > m) m = p;
}

// add_ray and, in the ADAPT instances, Welford's second moment of the sample
// against the running mean before and after it: sub, sub, mul, add in f32
template <bool ADAPT>
__device__ __forceinline__ void add_ray_m2(float v, float& p, uint32_t& c, float& s, float& m, float& m2) {
    if (ADAPT) {
        const float p_old = p;
        add_ray(v, p, c, s, m);
        m2 += (v - p_old) * (v - p);
    } else {
        add_ray(v, p, c, s, m);
    }
}

// PLANE: kPlaneGrid replays GridRenderPlane::addRay's row map (source rows
// H-2 and H-1 both land in row 0), kPlaneGui Gui::addRay's (source row s lands
// in row H-1-s); the running mean is the same.
// ADAPT (a launch with a mask or an m2 plane): a pixel without a flag whose
// mask byte is 0 has no sample this launch and returns at once (the unflagged
// branches read `values` without looking at codes and would add the 0 stored
// for a masked sample); every added sample also updates m2. The ADAPT = false
// instances are the unmasked replay, instruction for instruction.
template <int PLANE, bool ADAPT>
__device__ __forceinline__ void accumulate_pixel(const AParamsOf<ADAPT>& ap, int xi, int yi);
template <int PLANE, bool ADAPT>
__global__ __launch_bounds__(256) void accumulate_kernel(AParamsOf<ADAPT> ap) {
    const int xi = blockIdx.x * blockDim.x + threadIdx.x;
    const int yi = blockIdx.y;
    if (threadIdx.x == 0) atomicMin(&ap.clk[0], (unsigned long long)wall_clock64());
    if (xi < ap.W && (ap.n_shards <= 1 || ap.tile_rows <= 0 || ((yi / ap.tile_rows) % ap.n_shards) == ap.shard_id))
        accumulate_pixel<PLANE, ADAPT>(ap, xi, yi);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&ap.clk[1], (unsigned long long)wall_clock64());
}
template <int PLANE, bool ADAPT>
__device__ __forceinline__ void accumulate_pixel(const AParamsOf<ADAPT>& ap, int xi, int yi) {
    const size_t d = (size_t)yi * ap.W + xi;
    float m2 = 0.0f;
    if constexpr (ADAPT) {
        if (ap.mask && ap.flags[d] == 0 && ap.mask[d] == 0) return;
        if (ap.m2) m2 = ap.m2[d];
    }
    float p = ap.pixels[d];
    uint32_t c = ap.counters[d];
    float s = ap.sums ? ap.sums[d] : 0.0f;
    float m = ap.pixel_max ? ap.pixel_max[d] : 0.0f;
    const size_t pass_stride = (size_t)ap.n_cand * ap.W;
    const int H = ap.H;
    if (PLANE == kPlaneGui && ap.flags[d] == 0) {
        // the one nominal source: row H-1-yi (in [0, H) for every yi). Loads
        // of 8 passes, then their 8 updates, as below
        const int c0 = ap.cand_of_row[H - 1 - yi];
        if (c0 >= 0) {
            const float* v0p = ap.values + (size_t)c0 * ap.W + xi;
            int sp = 0;
            for (; sp + 8 <= ap.spp; sp += 8) {
                float a0[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) a0[q] = v0p[(size_t)(sp + q) * pass_stride];
#pragma unroll
                for (int q = 0; q < 8; ++q) add_ray_m2<ADAPT>(a0[q], p, c, s, m, m2);
            }
            for (; sp < ap.spp; ++sp) add_ray_m2<ADAPT>(v0p[(size_t)sp * pass_stride], p, c, s, m, m2);
        }
    } else if (PLANE == kPlaneGui) {
        // source rows whose nominal row H-1-iy is yi+1, yi, yi-1: ascending
        // (raster order of render_sample). A sample the min() clamped has
        // code 0x5 (row H-1 is source row 0's nominal row): no special case
        for (int sp = 0; sp < ap.spp; ++sp) {
            const size_t base = (size_t)sp * pass_stride;
            for (int iy = H - 2 - yi; iy <= H - yi; ++iy) {
                if (iy < 0 || iy >= H) continue;
                const int ci = ap.cand_of_row[iy];
                if (ci < 0) continue;
                const int yn = H - 1 - iy;
                for (int ix = xi - 1; ix <= xi + 1; ++ix) {
                    if (ix < 0 || ix >= ap.W) continue;
                    const size_t idx = base + (size_t)ci * ap.W + ix;
                    const uint8_t code = ap.codes[idx];
                    if (code >= 0x10) continue;
                    const int dx = (code & 3) - 1, dy = ((code >> 2) & 3) - 1;
                    if (ix + dx == xi && yn + dy == yi) add_ray_m2<ADAPT>(ap.values[idx], p, c, s, m, m2);
                }
            }
        }
    } else if (ap.flags[d] == 0) {
        // nominal sources only: source row H-2-yi (and H-1 for yi == 0)
        int r0 = H - 2 - yi;
        const int c0 = r0 >= 0 ? ap.cand_of_row[r0] : -1;
        const int c1 = (yi == 0 && H >= 1) ? ap.cand_of_row[H - 1] : -1;
        // the samples' loads issued 8 passes at a time, then the 8 running-mean
        // updates in the same order: one load latency per 8 passes instead of
        // one per pass (the updates are a serial chain per pixel)
        const bool t0 = c0 >= 0, t1 = c1 >= 0 && c1 != c0;
        const float* v0p = ap.values + (size_t)(t0 ? c0 : 0) * ap.W + xi;
        const float* v1p = ap.values + (size_t)(t1 ? c1 : 0) * ap.W + xi;
        int sp = 0;
        for (; sp + 8 <= ap.spp; sp += 8) {
            float a0[8], a1[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const size_t base = (size_t)(sp + q) * pass_stride;
                a0[q] = t0 ? v0p[base] : 0.0f;
                a1[q] = t1 ? v1p[base] : 0.0f;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (t0) add_ray_m2<ADAPT>(a0[q], p, c, s, m, m2);
                if (t1) add_ray_m2<ADAPT>(a1[q], p, c, s, m, m2);
            }
        }
        for (; sp < ap.spp; ++sp) {
            const size_t base = (size_t)sp * pass_stride;
            if (t0) add_ray_m2<ADAPT>(v0p[base], p, c, s, m, m2);
            if (t1) add_ray_m2<ADAPT>(v1p[base], p, c, s, m, m2);
        }
    } else {
        int rows[4];
        int nr = 0;
        const int cand_rows[4] = {H - 3 - yi, H - 2 - yi, H - 1 - yi, yi <= 1 ? H - 1 : -1};
        for (int q = 0; q < 4; ++q) {
            const int r = cand_rows[q];
            if (r < 0 || r >= H) continue;
            bool dup = false;
            for (int e = 0; e < nr; ++e) dup |= rows[e] == r;
            if (!dup) rows[nr++] = r;
        }
        // ascending row order (raster order of render_sample)
        for (int a = 0; a < nr; ++a)
            for (int b2 = a + 1; b2 < nr; ++b2)
                if (rows[b2] < rows[a]) { int t = rows[a]; rows[a] = rows[b2]; rows[b2] = t; }
        for (int sp = 0; sp < ap.spp; ++sp) {
            const size_t base = (size_t)sp * pass_stride;
            for (int a = 0; a < nr; ++a) {
                const int iy = rows[a];
                const int ci = ap.cand_of_row[iy];
                if (ci < 0) continue;
                const int yn = H - 2 - iy > 0 ? H - 2 - iy : 0;
                for (int ix = xi - 1; ix <= xi + 1; ++ix) {
                    if (ix < 0 || ix >= ap.W) continue;
                    const size_t idx = base + (size_t)ci * ap.W + ix;
                    const uint8_t code = ap.codes[idx];
                    if (code >= 0x10) continue;
                    const int dx = (code & 3) - 1, dy = ((code >> 2) & 3) - 1;
                    if (ix + dx == xi && yn + dy == yi) add_ray_m2<ADAPT>(ap.values[idx], p, c, s, m, m2);
                }
            }
        }
    }
    ap.pixels[d] = p;
    ap.counters[d] = c;
    if (ap.sums) ap.sums[d] = s;
    if (ap.pixel_max) ap.pixel_max[d] = m;
    if constexpr (ADAPT) {
        if (ap.m2) ap.m2[d] = m2;
    }
}

// ipt_replay_samples' sample source: the caller's whole-frame samples
// [spp][H][W] of this launch's passes, on the device.
struct ReplaySrc {
    const float* values;
    const uint8_t* codes;
};
// One thread per work unit, in raygen_kernel's place (and no path kernel): what
// new_path_setup does with a code, restated for a code that is given instead
// of computed -- the sample goes to its unit of the candidate layout, a code
// other than 0x05 flags its nominal pixel and its destination, a destination
// row of another shard leaves value 0 and code 0xfe. The host has checked
// every code (ipt_replay_samples): its destination lies inside the frame.
__global__ __launch_bounds__(256) void replay_mark_kernel(const KParams kp, const ReplaySrc src) {
    const unsigned long long unit = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (unit >= kp.total_units) return;
    const bool sharded = !(kp.n_shards <= 1 || kp.tile_rows <= 0);
    const uint32_t u32 = (uint32_t)unit;
    const uint32_t s = udiv_exact(u32, kp.per_pass32, kp.inv_per_pass);
    const uint32_t rem = u32 - s * kp.per_pass32;
    const int cand = (int)udiv_exact(rem, (uint32_t)kp.W, kp.inv_w);
    const int ix = (int)(rem - (uint32_t)cand * (uint32_t)kp.W);
    const int iy = sharded ? kp.cand_rows[cand] : cand;
    const size_t at = ((size_t)s * kp.H + iy) * kp.W + ix;
    const uint8_t code = src.codes[at];
    const int yn = kp.plane == kPlaneGui ? gui_nominal_row(iy, kp.H) : nominal_row(iy, kp.H);
    const int xi = ix + (code & 3) - 1, yi = yn + ((code >> 2) & 3) - 1;
    if (code != 0x05) {
        kp.flags[(size_t)yn * kp.W + ix] = 1;
        kp.flags[(size_t)yi * kp.W + xi] = 1;
    }
    const bool mine = owned_row(kp, yi);
    kp.values[unit] = mine ? src.values[at] : 0.0f;
    kp.codes[unit] = mine ? code : (uint8_t)0xfe;
}

// ----------------------------------------------------------- math probes
// Division pairs for the fast-division proof (fn 9): every 32-bit pattern b
// maps to a numerator with b's sign and mantissa and a biased exponent in
// [87, 167] (or +-0 when b's exponent field is 0) and a hashed denominator in
// the same range, so every wave of the self-check takes div_'s fast path.
__device__ __host__ inline float div_pair_a(uint32_t b) {
    const uint32_t e = (b >> 23) & 0xffu;
    if (e == 0u) return u2f(b & 0x80000000u);
    return u2f((b & 0x807fffffu) | ((87u + e % 81u) << 23));
}
__device__ __host__ inline float div_pair_b(uint32_t b) {
    uint32_t h = b * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA77u;
    h ^= h >> 13;
    return u2f((h & 0x807fffffu) | ((87u + ((h >> 23) & 0xffu) % 81u) << 23));
}

// fn 20: divisors whose significands are all ones or within 2^12 ulps of it
// (the hard case of one-correction division), hashed exponents as above
__device__ __host__ inline float div_pair_b_ones(uint32_t b) {
    uint32_t h = b * 0x85EBCA77u;
    h ^= h >> 13;
    const uint32_t m = 0x007fffffu - (h & 0xfffu);
    return u2f((h & 0x80000000u) | ((87u + ((h >> 12) & 0xffu) % 81u) << 23) | m);
}

// fn 11 / 12 probes: a 32-bit pattern b seeds a pair.
//  11: x = |b| as a float, y = x moved by a hashed -64..63 ulps (every 16th
//      pair: an unrelated hashed float) -> longer_sq(x, y) as 0/1;
//  12: n = b, d = a hashed divisor of hashed magnitude -> udiv_exact(n, d).
__device__ __host__ inline uint32_t probe_hash(uint32_t b) {
    uint32_t h = b * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA77u;
    h ^= h >> 13;
    return h;
}
__device__ __host__ inline void longer_pair(uint32_t b, float* x, float* y) {
    const uint32_t h = probe_hash(b);
    const uint32_t xb = b & 0x7fffffffu;
    *x = u2f(xb);
    *y = (h & 15u) == 0u ? u2f(probe_hash(h) & 0x7fffffffu) : u2f(xb + ((h >> 4) & 127u) - 64u);
}
__device__ __host__ inline uint32_t udiv_pair_d(uint32_t b) {
    const uint32_t h = probe_hash(b ^ 0x5bd1e995u);
    return (h >> (h & 31u)) | 1u;
}
__device__ __host__ inline float math_fn(int fn, float x) {
    switch (fn) {
        case 10: return div_inrange_(div_pair_a(f2u(x)), div_pair_b(f2u(x)));
        case 11: {
            float a, b;
            longer_pair(f2u(x), &a, &b);
#if defined(__HIP_DEVICE_COMPILE__)
            return longer_sq(a, b) ? 1.0f : 0.0f;
#else
            return sqrt_(a) > sqrt_(b) ? 1.0f : 0.0f;
#endif
        }
        case 12: {
            const uint32_t d = udiv_pair_d(f2u(x));
            return u2f(udiv_exact(f2u(x), d, 1.0 / (double)d));
        }
        case 13:  // the range-free root on its range +0, [2^-96, 2^126); sqrtf elsewhere
            return (f2u(x) == 0u || (x >= 0x1p-96f && x < 0x1p126f)) ? sqrt_inrange_(x) : sqrt_(x);
        case 14:
        case 15: {  // the RotateDdf angle's sin / cos for to.z = x
            float sv, cv;
            frame_angle_sc(v3(0.6f, 0.8f, x), &sv, &cv);
            return fn == 14 ? sv : cv;
        }
        case 17: return rcp_newton_<1>(x);
        case 18: return rcp_newton_<2>(x);
        case 19: return div_inrange_(div_pair_a(f2u(x)), div_pair_b(f2u(x)));
        case 20: return div_inrange_(div_pair_a(f2u(x)), div_pair_b_ones(f2u(x)));
        case 0: return acosf_(x);
        case 1: return sinf_(x);
        case 2: return cosf_(x);
        case 3: return acos_f64_to_f32(x);
        case 4: { float s, c; sincosf_(x, &s, &c); return s; }
        case 5: { float s, c; sincosf_(x, &s, &c); return c; }
        case 6: return sqrt_(x);
        case 7: return div_pi_to_f32(x);
        case 8: return two_pi_times(x);
        case 9: return div_(div_pair_a(f2u(x)), div_pair_b(f2u(x)));
        default: return 0.0f;
    }
}
// Philox blocks for the known-answer tests (ipt_philox): the key arrives as
// kernel arguments, i.e. uniform, as in the path kernel
__global__ void philox_kernel(uint32_t k0, uint32_t k1, const uint4* __restrict__ ctr, uint4* __restrict__ out,
                              long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 c = ctr[i];
    const u32x4 o = philox4x32_10(c.x, c.y, c.z, c.w, k0, k1);
    out[i] = make_uint4(o.v[0], o.v[1], o.v[2], o.v[3]);
}
__global__ void math_kernel(int fn, const float* in, float* out, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = math_fn(fn, in[i]);
}

// DDF samplers / values exactly as the path kernel evaluates them, for the
// sampler checks (ipt_ddf_sample / ipt_ddf_value; tests/test_ddf_samplers.py).
// kind 0: RotateDdf(CosineDdf, to=params[0..2]); kind 1: DdfFromLight of light
// params[3] at origin params[0..2]; kind 2: the UnionDdf of every light and
// RotateDdf(CosineDdf, normal=params[3..5]) at origin params[0..2].
__global__ void ddf_kernel(int value_mode, int kind, const float* __restrict__ params, const LightDev* __restrict__ lights,
                           const float* __restrict__ weights, const float* __restrict__ cdf, int nl,
                           const float* __restrict__ in, long long n, float* __restrict__ out,
                           const float* __restrict__ cos_a, const float2* __restrict__ cos_b) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vec3 o = v3(params[0], params[1], params[2]);
    if (kind == 3) kind = value_mode ? 0 : kind;  // table sampler: same DDF value
    if (!value_mode) {
        const float pick = in[3 * i], u1 = in[3 * i + 1], u2 = in[3 * i + 2];
        vec3 v = v3(0.0f, 0.0f, 0.0f);
        if (kind == 0) {
            v = frame_apply(make_frame(o), cosine_sample_local(u1, u2));
        } else if (kind == 3) {
            // the path kernel's table lookup (u on the RNG's 2^-24 grid, checked by the caller)
            const float tr = cos_a[(uint32_t)(u1 * 16777216.0f)];
            const float2 tb = cos_b[(uint32_t)(u2 * 16777216.0f)];
            v = frame_apply(make_frame(o), v3(tr * tb.x, tr * tb.y, sqrt_(u1)));
        } else if (kind == 1) {
            v = light_sample_dir(lights[(int)params[3]], o, u1, u2);
        } else {
            int c = 0;
            while (c <= nl && !(pick < cdf[c])) ++c;
            if (c < nl) v = light_sample_dir(lights[c], o, u1, u2);
            else if (c == nl) v = frame_apply(make_frame(v3(params[3], params[4], params[5])), cosine_sample_local(u1, u2));
        }
        out[3 * i] = v.x;
        out[3 * i + 1] = v.y;
        out[3 * i + 2] = v.z;
    } else {
        const vec3 d = v3(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
        float v;
        if (kind == 0) {
            v = frame_cosine_value(make_frame(o), d);
        } else if (kind == 1) {
            const LightDev& L = lights[(int)params[3]];
            vec3 hp, hn;
            const bool h = light_trace(L, o, d, &hp, &hn);
            v = light_pdf(L, o, h, hp, hn);
        } else {
            float lmix = 0.0f;
            for (int l = 0; l < nl; ++l) {
                vec3 hp, hn;
                const bool h = light_trace(lights[l], o, d, &hp, &hn);
                lmix += weights[l] * light_pdf(lights[l], o, h, hp, hn);
            }
            v = lmix + weights[nl] * frame_cosine_value(make_frame(v3(params[3], params[4], params[5])), d);
        }
        out[i] = v;
    }
}

// Exact CosineDdf tables (ddf.cpp:223-231) over the 2^24 values a draw can
// take (u = i * 2^-24, ipt_math.h u01): a[i] = sinf(acosf(sqrtf(u))) (64 MiB),
// b[i] = sincosf((float)(2*M_PI*u)) as (cos, sin) (128 MiB).
// cosine_sample_local(u1, u2) == (a[i1]*b[i2].x, a[i1]*b[i2].y, sqrtf(u1)) bit
// for bit (same functions, same products).
__global__ void cos_table_kernel(float* __restrict__ a, float2* __restrict__ b) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << 24)) return;
    const float u = u01(i << 8);
    const float cos_alpha = sqrt_(u);
    const float r = sinf_small_(acosf_(cos_alpha));
    float sp, cp;
    sincosf_small_(two_pi_times(u), &sp, &cp);
    a[i] = r;
    b[i] = make_float2(cp, sp);
}

// frame_sc table (frame_sc_lookup): entry i is frame_angle_sc of to.z = the
// float with |bits| = kFrameTabLo + (i >> 1) and sign i & 1 (dot((0,0,1), to)
// is to.z for finite to.x, to.y and to.z != 0).
__global__ void frame_table_kernel(float2* __restrict__ t) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kFrameTabEntries) return;
    const float z = u2f((kFrameTabLo + (uint32_t)(i >> 1)) | ((uint32_t)(i & 1) << 31));
    float sv, cv;
    frame_angle_sc(v3(0.0f, 0.0f, z), &sv, &cv);
    t[i] = make_float2(sv, cv);
}

// Exact restatement of math_fn (differs only where the device uses a fast
// path, i.e. fn 3): the reference for ipt_math_selfcheck.
__device__ float math_fn_exact(int fn, float x) {
    if (fn == 3) return acos_f64_to_f32_exact(x);
    if (fn == 6) return __builtin_sqrtf(x);                                      // IEEE (compiler sequence)
    if (fn == 9 || fn == 10) return div_pair_a(f2u(x)) / div_pair_b(f2u(x));   // IEEE (compiler sequence)
    if (fn == 11) {
        float a, b;
        longer_pair(f2u(x), &a, &b);
        return sqrt_(a) > sqrt_(b) ? 1.0f : 0.0f;  // glm length comparison as written
    }
    if (fn == 12) return u2f(f2u(x) / udiv_pair_d(f2u(x)));
    if (fn == 13) return __builtin_sqrtf(x);  // IEEE (compiler sequence)
    if (fn == 17 || fn == 18) {  // the round-4 reciprocal: one Newton step, two quotient residual steps
        float y = __builtin_amdgcn_rcpf(x);
        y = __builtin_fmaf(__builtin_fmaf(-x, y, 1.0f), y, y);
        const float q1 = __builtin_fmaf(__builtin_fmaf(-x, y, 1.0f), y, y);
        return __builtin_fmaf(__builtin_fmaf(-x, q1, 1.0f), y, q1);
    }
    if (fn == 19) return div_pair_a(f2u(x)) / div_pair_b(f2u(x));       // IEEE (compiler sequence)
    if (fn == 20) return div_pair_a(f2u(x)) / div_pair_b_ones(f2u(x));  // IEEE (compiler sequence)
    return math_fn(fn, x);
}

// Self-check 16: a sphere-in-box-like normal from the bit pattern b (hashed
// coordinates with |nrm| around 0.5, plus the edge cases the fast frame must
// hand to the exact build: zero or tiny x / y, both tiny, z = +-1 directions,
// x = +-y) -> to = normalize(nrm); true when the fast frame says ok and any of
// its 12 floats differs from make_frame_sc<true>'s bits.
__device__ bool frame_fast_mismatch(uint32_t b) {
    const uint32_t h1 = probe_hash(b), h2 = probe_hash(h1 ^ 0x9e3779b9u), h3 = probe_hash(h2 + 0x7f4a7c15u);
    float x = (float)(int)(h1 >> 8) * 0x1p-24f - 0.5f;  // [-0.5, 0.5)
    float y = (float)(int)(h2 >> 8) * 0x1p-24f - 0.5f;
    float z = (float)(int)(h3 >> 8) * 0x1p-24f - 0.5f;
    switch (b & 15u) {
        case 0: x = 0.0f; break;
        case 1: y = 0.0f; break;
        case 2: x = u2f(h1 & 0x0fffffffu) * (h2 & 1 ? 1.0f : -1.0f); break;           // tiny x
        case 3: x = u2f(h1 & 0x0fffffffu); y = -u2f(h2 & 0x0fffffffu); break;        // tiny x and y
        case 4: x = -0.0f; y = u2f(h3 & 0x1fffffffu); break;
        case 5: y = x; break;
        case 6: y = -x; break;
        case 7: x = u2f(h1 & 0x33ffffffu); y = u2f(h2 & 0x33ffffffu); break;         // |x|, |y| ~ 1e-7
        default: break;
    }
    if (!(z != 0.0f)) z = 0.25f;
    const vec3 to = normalize_inrange_(v3(x, y, z));
    float s, c;
    frame_angle_sc(to, &s, &c);
    bool ok;
    const Frame f = make_frame_sc_fast(to, s, c, ok);
    if (!ok) return false;
    const Frame e = make_frame_sc<true>(to, s, c);
    const float* pf = &f.m0.x;
    const float* pe = &e.m0.x;
    bool diff = false;
    for (int k = 0; k < 12; ++k) diff |= f2u(pf[k]) != f2u(pe[k]);
    return diff;
}

// fn 21: the range-free division over EVERY pair of significands, a and b in
// [1, 2) (index i: a = 1 + (i >> 23) 2^-23, b = 1 + (i & (2^23 - 1)) 2^-23,
// 2^46 pairs), against IEEE a/b. With fn 22 (the reciprocal scales exactly)
// this extends to every in-range operand: the remaining operations (the
// Newton fma, a*y, the residual fma, the correction fma) are IEEE operations
// and commute with scaling by powers of two while nothing over- or
// underflows, which the callers' range [2^-40, 2^41) guarantees; RN is
// symmetric, so signs follow too. Mismatches counted; `first` = the lowest a
// significand index (i >> 23) with one.
__global__ void divcheck_kernel(unsigned long long lo, unsigned long long n, unsigned long long* bad,
                                unsigned int* first) {
    unsigned long long local = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned long long k = lo + i;
        const float a = u2f(0x3f800000u | (uint32_t)(k >> 23));
        const float b = u2f(0x3f800000u | (uint32_t)(k & 0x7fffffu));
        float bv = b;
        asm volatile("" : "+v"(bv));  // no constant folding of the IEEE sequence
        if (f2u(div_inrange_(a, bv)) != f2u(a / bv)) {
            ++local;
            atomicMin(first, (unsigned int)(k >> 23));
        }
    }
    if (local) atomicAdd(bad, local);
}
// fn 22: the reciprocal scales exactly: for every float b with |b| in
// [2^-40, 2^41), rcp_newton_<1>(b) == sign(b) 2^-e rcp_newton_<1>(m) for b =
// sign(b) m 2^e, m in [1, 2) (other patterns: not counted)
__device__ bool rcp_scale_mismatch(uint32_t bb) {
    const uint32_t e = (bb >> 23) & 0xffu;
    if (e < 127u - 40u || e >= 127u + 41u) return false;
    const float b = u2f(bb);
    const float m = u2f(0x3f800000u | (bb & 0x7fffffu));
    const float ym = rcp_newton_<1>(m);
    const float want = __builtin_amdgcn_ldexpf(ym, 127 - (int)e);
    const float y = rcp_newton_<1>(b);
    return f2u(y) != (f2u(want) ^ (bb & 0x80000000u));
}

__global__ void selfcheck_kernel(int fn, unsigned long long lo, unsigned long long n,
                                 unsigned long long* bad, unsigned int* first, const float2* __restrict__ ftab) {
    unsigned long long local = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t b = (uint32_t)(lo + i);
        const float x = u2f(b);
        if (fn == 16 || fn == 22) {  // 16: make_frame_sc_fast == make_frame_sc<true> wherever it reports ok
            if (fn == 16 ? frame_fast_mismatch(b) : rcp_scale_mismatch(b)) {
                ++local;
                atomicMin(first, b);
            }
            continue;
        }
        float a = math_fn(fn, x);
        const float e = math_fn_exact(fn, x);
        if (fn == 14 || fn == 15) {  // the path kernel's table lookup (frame_sc_lookup)
            float sv = 0.0f, cv = 0.0f;
            frame_sc_lookup(ftab, v3(0.6f, 0.8f, x), sv, cv);
            a = fn == 14 ? sv : cv;
        }
        // fn 10 / 19 / 20: a zero quotient's sign is not observed by the callers
        if (!(f2u(a) == f2u(e) || (a != a && e != e) || ((fn == 10 || fn >= 19) && a == 0.0f && e == 0.0f))) {
            ++local;
            atomicMin(first, b);
        }
    }
    if (local) atomicAdd(bad, local);
}

// ---------------------------------------------------------------- context
std::mutex g_err_mu;
std::string g_err_global;

}  // namespace

// One set of per-launch work buffers (radiance, drift codes, raygen records,
// drifted-pixel flags, the shard's candidate rows, the work-unit counter) with
// its own stream for raygen + path kernel. Consecutive launches -- chunks of
// one call and consecutive calls alike -- alternate between two slots, so a
// launch's workgroups take the CUs its predecessor's tail leaves idle (lanes
// out of paths while the longest trees finish); the
// GridRenderPlane replays run on the caller's stream in call order, each after
// its own path kernel (an event), so the image is accumulated exactly as by
// sequential calls.
struct WorkSlot {
    float* d_values = nullptr;
    uint8_t* d_codes = nullptr;
    uint4* d_rg = nullptr;  // raygen_kernel records, 2 x 16 B per element
    size_t work_cap = 0;    // elements
    size_t rg_cap = 0;      // elements of d_rg (full-estimator launches only)
    uint8_t* d_kinds = nullptr;  // ipt_preview_values' per-sample outputs
    float* d_hits = nullptr;
    size_t kinds_cap = 0, hits_cap = 0;
    uint8_t* d_flags = nullptr;
    size_t flags_cap = 0;
    int* d_cand_rows = nullptr;
    int* d_cand_of_row = nullptr;
    size_t cand_cap_rows = 0, cand_cap_h = 0;
    int plan[5] = {-1, -1, -1, -1, -1};  // (H, tile_rows, n_shards, shard_id, plane) whose rows are on the device
    unsigned long long* d_unit = nullptr;
    // a compacting launch's buffers (IPT_FLAG_COMPACT), allocated on the slot's
    // first such launch: the path kernel's values by compact index, the compact
    // indices' dense units, the scan's block counts (compact_cap / 256 + 2)
    float* d_cvalues = nullptr;
    uint32_t* d_src = nullptr;
    unsigned int* d_cblk = nullptr;
    size_t compact_cap = 0;  // elements
    // pool-drained flag in signal memory (hipExtMallocWithFlags(hipMallocSignalMemory),
    // the memory hipStreamWaitValue64 is specified for) and the sequence
    // number of the slot's last queued launch (the value it stores there)
    unsigned long long* d_drained = nullptr;
    unsigned long long seq = 0;
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;  // after the last reader of the slot's buffers (accumulate or host copies)
    hipEvent_t path_end = nullptr;  // after its last path kernel
    hipEvent_t mask_ready = nullptr;  // a masked call's point on the caller's stream (created on first use)
    unsigned long long total = 0;   // work units of its last launch
    bool used = false;
    bool idle = true;  // its last launch is known complete (a drain since): nothing to wait for
    // everything the slot owns (after a drain: nothing queued uses it)
    void release() {
        for (void* b : {(void*)d_values, (void*)d_codes, (void*)d_rg, (void*)d_kinds, (void*)d_hits, (void*)d_flags,
                        (void*)d_cand_rows, (void*)d_cand_of_row, (void*)d_unit, (void*)d_drained, (void*)d_cvalues,
                        (void*)d_src, (void*)d_cblk})
            if (b) hipFree(b);
        for (hipEvent_t e : {done, path_end, mask_ready})
            if (e) hipEventDestroy(e);
        if (st) hipStreamDestroy(st);
        *this = WorkSlot{};
    }
};
#if IPT_RAYLOG
// IPT_RAYLOG's buffer (scripts/probes/walk_split.hip arms it)
static RayLogRec* g_raylog = nullptr;
static unsigned long long* g_raylog_n = nullptr;
static unsigned long long g_raylog_cap = 0;
static unsigned g_raylog_every = 1;
#endif

// ipt_compact_plan: the first launch's plan, read back after compact_preset_kernel
struct CompactProbe {
    uint32_t* host_src;
    unsigned long long cap;
    unsigned long long n_active = 0, start = 0;
    int rc = 0;
};

// What a C-API entry point asks of render_chunks: each fills what it uses.
struct LaunchRequest {
    ipt_image* img = nullptr;   // device planes the samples are accumulated into, or null
    hipStream_t st = nullptr;   // the caller's stream
    // [spp][H][W] host outputs (whole frames), each null or given
    float* host_values = nullptr;
    uint8_t* host_codes = nullptr;
    uint8_t* host_kinds = nullptr;  // (the preview's, as host_hits)
    float* host_hits = nullptr;
    bool preview = false;  // ray_power_preview's launches whatever IPT_FLAG_PREVIEW says (ipt_preview_values, guides)
    ReplaySrc replay{nullptr, nullptr};  // ipt_replay_samples: the call's passes [spp][H][W], on the device
    // ipt_render_masked_device: sample mask and second-moment plane, [H][W] on the device, each or null
    const uint8_t* mask = nullptr;
    float* m2 = nullptr;
    CompactProbe* probe = nullptr;  // ipt_compact_plan
    ipt_guide* guides = nullptr;    // ipt_guides_device: the guide plane, on the device
};

// A call's mode, derived once from its flags and request (render_chunks).
struct LaunchMode {
    bool preview;  // the preview estimator's launches
    bool replay;   // the caller's samples
    bool traced;   // neither: the full estimator's (raygen + path kernel)
    bool compact;  // IPT_FLAG_COMPACT or the probe: the pool holds the valid units alone (traced launches only)
    bool adapt;    // a mask or an m2 plane: accumulate_kernel's ADAPT instances
    bool want_kinds, want_hits;  // the FULL preview instance's per-sample outputs (host copies or guides)
    bool count;    // IPT_FLAG_COUNTERS
    int susp;      // the DFS's suspended levels, <= 8 (validate)
};

// What the launches of one render_chunks call share.
struct Call {
    const ipt_params* p;
    const LaunchRequest& rq;
    LaunchMode m;
    std::vector<int> rows, of_row;  // candidate_rows
    int n_cand = 0;
    size_t per_pass = 0;  // units of one pass: n_cand * W
    int chunk = 1;        // passes per launch
    bool mask_waited[2] = {false, false};  // the slot stream waits for the caller's mask once per call
};

struct ChunkTiming {
    hipEvent_t t0 = nullptr, t1 = nullptr;  // raygen start, path-kernel end (slot stream)
    hipEvent_t a0 = nullptr, a1 = nullptr;  // accumulate (caller stream; null without an image)
    int clk = -1;           // the accumulate's wall-clock pair in ctx->d_clk (ring entry)
    unsigned long long units = 0;  // a full-estimator launch's total_units (ipt_last_units)
    int uring = -1;         // a compacting launch's {start, n_active} in ctx->d_uring (ring entry)
    bool recorded = false;  // every event of the launch was recorded (its queueing succeeded)
};
constexpr int kClkRing = 32;  // > the launches settle_oldest lets queue up (8) plus the last settled one

// ipt_render's device-resident GridRenderPlane: the caller's host image is
// the truth, the device keeps a copy of its OWNED rows (all rows unsharded,
// the shard's tiles otherwise) across calls, and a host shadow holds those
// rows as the previous call returned them. A call uploads only the owned row
// runs whose host bytes differ from the shadow (none when the caller left the
// plane alone between calls, e.g. progressive rendering), renders, and
// downloads only the owned rows: 16 B per owned pixel per call (pixels,
// counters, and sums / per-pixel max when the image has them) instead of the
// whole plane both ways.
struct ResidentPlane {
    int W = 0, H = 0;
    bool has_sums = false, has_pmax = false;
    int plan[3] = {-1, -1, -1};  // (tile_rows, n_shards, shard_id) of `runs`
    float* d_pixels = nullptr;
    uint32_t* d_counters = nullptr;
    float* d_sums = nullptr;
    float* d_pmax = nullptr;
    std::vector<std::pair<int, int>> runs;  // owned rows [y0, y1)
    size_t owned_px = 0;
    std::vector<uint8_t> shadow;  // per field, the owned runs' bytes as last returned
    bool shadow_ok = false;
    unsigned long long h2d = 0, d2h = 0;  // bytes moved by the last ipt_render
    void release() {
        for (void* b : {(void*)d_pixels, (void*)d_counters, (void*)d_sums, (void*)d_pmax})
            if (b) hipFree(b);
        *this = ResidentPlane{};
    }
};

using ipt_internal::DevBuf;
// The uploaded scene, kept once. ipt_upload_scene builds a fresh record from
// the scene's plan (ScenePlan, ipt_scene_plan.h) and swaps it in only after every upload succeeded; the record it replaces frees
// its buffers as it goes.
struct Scene {
    // Every KParams field that depends only on the scene and on the context's
    // creation-time settings: each launch starts from a copy (launch_params).
    // What a scene does not use stays zero. The host reads the scene's values
    // here as well (geometry_kind, n_lights, sa_on, box_inrange, ...): no second copy.
    KParams kp{};
    // the device buffers kp points into (grid_c4: [items] centre/radius, then
    // [items] original indices; cdf_lo: none when a bucket is crowded)
    struct Bufs {
        DevBuf<LightDev> lights;
        DevBuf<float> weights, cdf;
        DevBuf<Frame> wall;
        DevBuf<float4> spheres, grid_c4;
        DevBuf<BvhNode> bvh_nodes, light_nodes;
        DevBuf<BvhSphere> bvh_prims, grid_items;
        DevBuf<int> grid_start, lgrid, cdf_lo;
        DevBuf<LightAx> lax;
    } bufs;
    // what selects the path-kernel instance and is no kernel parameter
    bool any_round_light = false;
    int light_axis = 0;     // axis_aligned_light() of a single AreaLight (kLightsOneA10/A01)
    int light_pattern = 0;  // LightGrid::pattern != 0: coplanar light lattice (kLightsGridA10/A01)
};

struct ipt_ctx {
    int device = 0;
    ResidentPlane rp;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    std::string err;
    bool has_scene = false;
    Scene scene;
    int bpc_override = 0;
    int lnodes_lds = 1;  // stage the light BVH in LDS (IPT_LNODES_LDS=0: global memory)
    int light_grid_on = 1;  // coplanar light lattices by cell lookup (IPT_LIGHT_GRID=0: the light BVH)
    // work buffers: two slots, used by consecutive launches in turn (WorkSlot)
    WorkSlot slot[2];
    unsigned next_slot = 0;
    // a launch starts once its predecessor's work pool is drained (its unit
    // counter reached its total: hipStreamWaitValue64 on that counter, in
    // device memory); without stream value waits (or IPT_NO_TAIL_OVERLAP=1)
    // once the predecessor has finished (an event)
    bool gate_on_pool = false;
    size_t chunk_cap_test = 0;  // IPT_TEST_CHUNK_UNITS: at most this many units per launch (tests)
    // timing of the launches queued since the last drain (event sets from ev_pool)
    std::vector<ChunkTiming> pending;
    ChunkTiming prev{};  // the last processed launch (its path-end event bounds the next one's start)
    std::vector<hipEvent_t> ev_pool;
    float run_path_ms = 0.0f, run_acc_ms = 0.0f;
    // accumulate_kernel's start / end wall-clock stamps, a ring of kClkRing
    // pairs (HIP events on the caller's stream are stamped when its wait for
    // the path kernel is queued, not when it is released)
    unsigned long long* d_clk = nullptr;
    unsigned long long* d_clk_dummy = nullptr;  // (2 words: stamps of an untimed launch)
    unsigned next_clk = 0;
    // compacting launches' {start, n_active}, a ring as d_clk is (compact_preset_kernel
    // writes an entry, settle_oldest reads it), and ipt_last_units' sums
    unsigned long long* d_uring = nullptr;
    unsigned next_uring = 0;
    unsigned long long run_units[3] = {0, 0, 0}, last_units[3] = {0, 0, 0};
    double clk_khz = 100000.0;
    unsigned long long* d_counters = nullptr;
    float* d_cos_a = nullptr;   // CosineDdf tables (cos_table_kernel): r 64 MiB,
                                // (cos phi, sin phi) 128 MiB
    float2* d_cos_b = nullptr;
    float2* d_frame_sc = nullptr;  // frame_table_kernel, 1 GiB
    float last_path_ms = 0.0f, last_acc_ms = 0.0f;
    int blocks_per_cu = 0;      // of the last path-kernel launch
    // its template arguments {MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED} (ipt_last_instance; MAXSUSP 0: none yet)
    int32_t last_instance[6] = {0, 0, 0, 0, 0, 0};
    bool box_generic = false;   // IPT_BOX_GENERIC=1: the box instances' generic range form (tests)
    bool lattice_lds = true;    // IPT_LATTICE_LDS=0: the lattice instances with global records (tests)
    size_t max_lds = 160 * 1024;  // the device's LDS per workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock)
    ipt_internal::PostScratch post;  // the queued post-processing calls' scratch and completion event (ipt_post.hip)
};

namespace {

int fail(ipt_ctx* ctx, int code, const std::string& msg) {
    if (ctx) {
        ctx->err = msg;
    } else {
        std::lock_guard<std::mutex> g(g_err_mu);
        g_err_global = msg;
    }
    return code;
}
#define HIPCHECK(ctx, expr)                                                             \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(ctx, e_ == hipErrorOutOfMemory ? IPT_E_OOM : IPT_E_DEVICE,      \
                        std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// The exact sampling tables are built once per context. Each is published in
// the context only after its allocation, its build kernel and that kernel's
// completion all succeeded, so a failure leaves no half-built table behind.
int ensure_cos_tables(ipt_ctx* ctx, hipStream_t st) {
    if (ctx->d_cos_a && ctx->d_cos_b) return IPT_OK;
    const size_t n = (size_t)1 << 24;
    DevBuf<float> a;
    DevBuf<float2> b;
    HIPCHECK(ctx, hipMalloc(&a.p, n * sizeof(float)));
    HIPCHECK(ctx, hipMalloc(&b.p, n * sizeof(float2)));
    hipLaunchKernelGGL(cos_table_kernel, dim3((unsigned)(n / 256)), dim3(256), 0, st, a.p, b.p);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(st));
    ctx->d_cos_a = a.release();
    ctx->d_cos_b = b.release();
    return IPT_OK;
}

// the geometries whose sphere-node frames read the frame-angle table
constexpr bool frame_table_user(int geom) {
    return geom == IPT_GEOM_SPHERE_IN_BOX;
}
int ensure_frame_table(ipt_ctx* ctx, hipStream_t st) {
    if (ctx->d_frame_sc) return IPT_OK;
    DevBuf<float2> t;
    HIPCHECK(ctx, hipMalloc(&t.p, kFrameTabEntries * sizeof(float2)));
    hipLaunchKernelGGL(frame_table_kernel, dim3((unsigned)((kFrameTabEntries + 255) / 256)), dim3(256), 0, st, t.p);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(st));
    ctx->d_frame_sc = t.release();
    return IPT_OK;
}

// Work buffers grow on demand, a group of buffers under one capacity: the
// group's buffers and its capacity are dropped together and the capacity is
// published only once every buffer of the group is allocated, so a failed
// regrowth never leaves a capacity over a missing buffer (what it did
// allocate is freed by the next regrowth or by WorkSlot::release). busy: the
// event after the last reader of the buffers, waited for before they go.
struct GrowBuf {
    void** p;
    size_t bytes;
};
template <class T>
GrowBuf grow_buf(T*& p, size_t bytes) {
    return {reinterpret_cast<void**>(&p), bytes};
}
int regrow(ipt_ctx* ctx, hipEvent_t busy, size_t& cap, size_t want, std::initializer_list<GrowBuf> bufs) {
    if (want <= cap) return IPT_OK;
    if (busy) HIPCHECK(ctx, hipEventSynchronize(busy));
    for (const GrowBuf& b : bufs) {
        if (*b.p) hipFree(*b.p);
        *b.p = nullptr;
    }
    cap = 0;
    for (const GrowBuf& b : bufs) HIPCHECK(ctx, hipMalloc(b.p, b.bytes));
    cap = want;
    return IPT_OK;
}

// The slot's buffer groups at the sizes a launch of the call needs. rg: the
// raygen records (none for a preview or replay launch: 5 B per unit instead of
// 37); kinds / hits: the FULL preview instance's outputs; compact: a compacting
// launch's buffers. (A used slot's buffers go only after its last launch's readers.)
int ensure_work(ipt_ctx* ctx, WorkSlot& S, const Call& c) {
    const size_t elems = (size_t)c.chunk * c.per_pass, npix = (size_t)c.p->width * c.p->height;
    const size_t rows = (size_t)c.n_cand, h = (size_t)c.p->height;
    const size_t rg = c.m.traced ? elems : 0, compact = c.m.compact ? elems : 0;
    const size_t kinds = c.m.want_kinds ? elems : 0, hits = c.m.want_hits ? elems : 0;
    const hipEvent_t busy = S.used ? S.done : nullptr;
    int rc = regrow(ctx, busy, S.work_cap, elems, {grow_buf(S.d_values, elems * sizeof(float)), grow_buf(S.d_codes, elems)});
    if (!rc) rc = regrow(ctx, busy, S.rg_cap, rg, {grow_buf(S.d_rg, rg * 2 * sizeof(uint4))});
    if (!rc)
        rc = regrow(ctx, busy, S.compact_cap, compact,
                    {grow_buf(S.d_cvalues, compact * sizeof(float)), grow_buf(S.d_src, compact * sizeof(uint32_t)),
                     grow_buf(S.d_cblk, (compact / 256 + 2) * sizeof(unsigned int))});
    if (!rc) rc = regrow(ctx, busy, S.kinds_cap, kinds, {grow_buf(S.d_kinds, kinds)});
    if (!rc) rc = regrow(ctx, busy, S.hits_cap, hits, {grow_buf(S.d_hits, hits * 6 * sizeof(float))});
    if (!rc) rc = regrow(ctx, busy, S.flags_cap, npix, {grow_buf(S.d_flags, npix)});
    // the shard's row maps: new buffers hold no plan
    if (rows > S.cand_cap_rows || h > S.cand_cap_h) S.plan[0] = -1;
    if (!rc) rc = regrow(ctx, busy, S.cand_cap_rows, rows, {grow_buf(S.d_cand_rows, rows * sizeof(int))});
    if (!rc) rc = regrow(ctx, busy, S.cand_cap_h, h, {grow_buf(S.d_cand_of_row, h * sizeof(int))});
    return rc;
}

hipEvent_t pool_event(ipt_ctx* ctx) {
    if (!ctx->ev_pool.empty()) {
        hipEvent_t e = ctx->ev_pool.back();
        ctx->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
void pool_return(ipt_ctx* ctx, ChunkTiming& c) {
    for (hipEvent_t e : {c.t0, c.t1, c.a0, c.a1})
        if (e) ctx->ev_pool.push_back(e);
    c = ChunkTiming{};
}

// Adds the oldest pending launch's times to the running sums (waiting for
// it): its path time counts from its own start or from its predecessor's end,
// whichever is later, so overlapped launches sum to their span; then the
// accumulate kernel's time.
// A launch whose queueing failed part-way (`recorded` false: its end events
// were never recorded) is dropped without timing: its events go back to the
// pool and the caller keeps the error message of the failure itself.
int settle_oldest(ipt_ctx* ctx) {
    ChunkTiming c = ctx->pending.front();
    ctx->pending.erase(ctx->pending.begin());
    if (!c.recorded) {
        pool_return(ctx, c);
        return IPT_OK;
    }
    const hipError_t e = hipEventSynchronize(c.a1 ? c.a1 : c.t1);
    float path = 0.0f, d = 0.0f, acc = 0.0f;
    if (e != hipSuccess || hipEventElapsedTime(&path, c.t0, c.t1) != hipSuccess ||
        (c.a1 && hipEventElapsedTime(&acc, c.a0, c.a1) != hipSuccess)) {
        pool_return(ctx, c);
        return fail(ctx, IPT_E_DEVICE, std::string("render launch failed: ") + hipGetErrorString(e != hipSuccess ? e : hipGetLastError()));
    }
    // the accumulate kernel's own duration from its wall-clock stamps (the
    // events bracket the caller stream's wait for the path kernel as well)
    if (c.a1 && c.clk >= 0 && ctx->d_clk) {
        unsigned long long h[2] = {~0ull, 0ull};
        if (hipMemcpy(h, ctx->d_clk + 2 * c.clk, sizeof h, hipMemcpyDeviceToHost) == hipSuccess && h[0] != ~0ull &&
            h[1] >= h[0])
            acc = (float)((double)(h[1] - h[0]) / ctx->clk_khz);
    }
    if (ctx->prev.t1 && hipEventElapsedTime(&d, c.t0, ctx->prev.t1) == hipSuccess && d > 0.0f)
        path = std::max(0.0f, path - d);
    ctx->run_path_ms += path;
    ctx->run_acc_ms += acc;
    if (c.units) {
        // (an uncompacted launch's pool hands out every dense unit)
        unsigned long long h[2] = {0ull, c.units};
        if (c.uring >= 0 &&
            hipMemcpy(h, ctx->d_uring + 2 * c.uring, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) {
            pool_return(ctx, c);
            return fail(ctx, IPT_E_DEVICE, "reading a compacting launch's unit counts failed");
        }
        ctx->run_units[0] += c.units;
        ctx->run_units[1] += c.units - h[0];
        ctx->run_units[2] += h[1];
    }
    pool_return(ctx, ctx->prev);
    ctx->prev = c;
    return IPT_OK;
}

// Waits for every queued launch and its readers; the launches' times since
// the previous drain become ipt_last_kernel_ms's.
int drain(ipt_ctx* ctx) {
    int rc = IPT_OK;
    for (WorkSlot& S : ctx->slot) {
        if (S.st && hipStreamSynchronize(S.st) != hipSuccess) rc = fail(ctx, IPT_E_DEVICE, "slot stream failed");
        if (S.used && S.done && hipEventSynchronize(S.done) != hipSuccess) rc = fail(ctx, IPT_E_DEVICE, "slot readers failed");
        S.idle = true;  // (synchronous calls therefore queue no stream value waits)
    }
    if (const int r = ipt_internal::post_wait(ctx)) rc = r;  // queued ipt_display_device work
    while (!ctx->pending.empty()) {
        const int r = settle_oldest(ctx);
        if (r && !rc) rc = r;
    }
    pool_return(ctx, ctx->prev);
    if (ctx->run_path_ms > 0.0f || ctx->run_acc_ms > 0.0f) {
        ctx->last_path_ms = ctx->run_path_ms;
        ctx->last_acc_ms = ctx->run_acc_ms;
    }
    ctx->run_path_ms = ctx->run_acc_ms = 0.0f;
    if (ctx->run_units[0]) std::copy(ctx->run_units, ctx->run_units + 3, ctx->last_units);
    ctx->run_units[0] = ctx->run_units[1] = ctx->run_units[2] = 0;
    return rc;
}

bool owned_host(const ipt_params* p, int yi) {
    if (p->n_shards <= 1 || p->tile_rows <= 0) return true;
    return ((yi / p->tile_rows) % p->n_shards) == p->shard_id;
}

int plane_of(const ipt_params* p) { return (p->flags & IPT_FLAG_GUI_PLANE) ? kPlaneGui : kPlaneGrid; }

// Source rows whose samples can land in an owned destination row: nominal
// row within +-1 of an owned row, H-2-iy (0 for iy=H-1) under
// GridRenderPlane's map, H-1-iy under the Gui's.
void candidate_rows(const ipt_params* p, std::vector<int>& rows, std::vector<int>& of_row) {
    const int H = p->height;
    const bool gui = plane_of(p) == kPlaneGui;
    rows.clear();
    of_row.assign(H, -1);
    for (int iy = 0; iy < H; ++iy) {
        const int yn = gui ? ipt::gui_nominal_row(iy, H) : ipt::nominal_row(iy, H);
        bool c = false;
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = yn + dy;
            if (y >= 0 && y < H && owned_host(p, y)) c = true;
        }
        if (c) {
            of_row[iy] = (int)rows.size();
            rows.push_back(iy);
        }
    }
}

int validate(ipt_ctx* ctx, const ipt_params* p, bool preview = false) {
    if (!ctx) return IPT_E_INVALID;
    if (!p) return fail(ctx, IPT_E_INVALID, "params is NULL");
    if (!ctx->has_scene) return fail(ctx, IPT_E_NOSCENE, "no scene uploaded");
    if (p->width <= 0 || p->height <= 0 || p->width > 65536 || p->height > 65536)
        return fail(ctx, IPT_E_INVALID, "width/height out of range");
    if ((int64_t)p->width * p->height > (int64_t)1 << 31)
        return fail(ctx, IPT_E_INVALID, "frame larger than 2^31 pixels");
    if (p->spp < 0 || p->spp_offset < 0) return fail(ctx, IPT_E_INVALID, "negative spp");
    const bool bad_shard = p->n_shards > 1 && (p->shard_id < 0 || p->shard_id >= p->n_shards);
    // the preview estimator reads neither n_rays nor depth_max (main.cpp:55's
    // unnamed parameters): any values are accepted
    if (preview || (p->flags & IPT_FLAG_PREVIEW))
        return bad_shard ? fail(ctx, IPT_E_INVALID, "shard_id out of range") : IPT_OK;
    // a suspended level stores its iteration count in the low bits of its meta
    // word (ti | kind << s, ti <= n_rays): s = 8 for n_rays < 256, else 16,
    // which leaves 16 bits for the node kind (6 + sphere index)
    if (p->n_rays < 0 || p->n_rays > 65535) return fail(ctx, IPT_E_UNSUPPORTED, "n_rays must be in [0,65535]");
    if (p->n_rays > 255 && ctx->scene.kp.n_spheres > 65535 - 6)
        return fail(ctx, IPT_E_UNSUPPORTED, "n_rays > 255 with more than 65529 spheres");
    if (p->depth_max < 0 || p->depth_max > 64) return fail(ctx, IPT_E_INVALID, "depth_max out of range");
    // the deepest pushed node: n_rays < 256 bounds it by 7 (a node at depth d
    // has n_rays >> d children) whatever depth_max; larger n_rays need
    // depth_max <= 9 (the MAXSUSP = 8 instances)
    if (needed_susp(p) > 8)
        return fail(ctx, IPT_E_UNSUPPORTED, "n_rays > 255 with depth_max > 9: more than 8 suspended levels");
    if (bad_shard) return fail(ctx, IPT_E_INVALID, "shard_id out of range");
    return IPT_OK;
}

template <int MAXSUSP, bool COUNT, int LMODE, int GEOM, bool BOXIN, int FIXED>
int launch_path5(ipt_ctx* ctx, const KParams& kp, hipStream_t st) {
    constexpr int kBlock = block_of(LMODE, GEOM);
    const size_t lds = path_lds_bytes<MAXSUSP, LMODE, GEOM>(kp);
    const void* fn = (const void*)path_kernel<MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED>;
    HIPCHECK(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // persistent grid: every block the CUs can hold at once (a work queue, no
    // inter-block waits, so an over-reported residency only queues blocks)
    int bpc = 0;
    HIPCHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, fn, kBlock, lds));
    bpc = std::max(1, std::min(bpc, 2048 / kBlock));  // (at most 32 waves per CU)
    if (ctx->bpc_override > 0) bpc = std::min(bpc, ctx->bpc_override);  // IPT_BLOCKS_PER_CU (profiling)
    ctx->blocks_per_cu = bpc;
    const int32_t inst[6] = {MAXSUSP, COUNT ? 1 : 0, LMODE, GEOM, BOXIN ? 1 : 0, FIXED};
    std::copy(inst, inst + 6, ctx->last_instance);
    dim3 grid(ctx->n_cu * bpc), block(kBlock);
    hipLaunchKernelGGL((path_kernel<MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED>), grid, block, lds, st, kp);
    HIPCHECK(ctx, hipGetLastError());
    return IPT_OK;
}
// The launch's instance by select_path (ipt_select.h), launched by launch_path5.
int launch_path(ipt_ctx* ctx, const KParams& kp, hipStream_t st, const LaunchMode& m) {
    const Scene& sc = ctx->scene;
    const SelectIn in{kp, m.susp, m.count, sc.any_round_light, sc.light_axis, sc.light_pattern,
                      ctx->box_generic, ctx->lattice_lds, ctx->max_lds};
    bool launched = false;
    const int rc = select_path(in, [&](auto ms, auto cnt, auto lm, auto g, auto boxin, auto fixed) {
        launched = true;
        return launch_path5<decltype(ms)::value, decltype(cnt)::value, decltype(lm)::value, decltype(g)::value,
                            decltype(boxin)::value, decltype(fixed)::value>(ctx, kp, st);
    });
    return launched ? rc : fail(ctx, rc, "IPT_C2_ONLY experiment build");
}

template <bool FULL>
int launch_preview(ipt_ctx* ctx, const KParams& kp, const PreviewOut& po, hipStream_t st) {
    const dim3 grid((unsigned)((kp.total_units + 255) / 256)), block(256);
    switch (kp.geometry_kind) {
#define IPT_PREVIEW_CASE(G) \
    case G: hipLaunchKernelGGL((preview_kernel<FULL, G>), grid, block, 0, st, kp, po); break;
        IPT_PREVIEW_CASE(IPT_GEOM_SPHERES_IN_BOX)
        IPT_PREVIEW_CASE(IPT_GEOM_FLOOR)
        IPT_PREVIEW_CASE(IPT_GEOM_CORNER)
        IPT_PREVIEW_CASE(IPT_GEOM_SPHERES)
        IPT_PREVIEW_CASE(IPT_GEOM_SMALLPT)
#undef IPT_PREVIEW_CASE
        default: hipLaunchKernelGGL((preview_kernel<FULL, IPT_GEOM_SPHERE_IN_BOX>), grid, block, 0, st, kp, po); break;
    }
    HIPCHECK(ctx, hipGetLastError());
    return IPT_OK;
}

LaunchMode mode_of(const ipt_params* p, const LaunchRequest& rq) {
    LaunchMode m{};
    m.preview = rq.preview || (p->flags & IPT_FLAG_PREVIEW) != 0;
    m.replay = rq.replay.values != nullptr;
    m.traced = !m.preview && !m.replay;
    // (the preview has no pool: the flag has no effect there)
    m.compact = m.traced && ((p->flags & IPT_FLAG_COMPACT) != 0 || rq.probe);
    m.adapt = rq.mask || rq.m2;
    // (guides: the kinds and hits stay on the device, where the scatter reads them)
    m.want_kinds = rq.host_kinds || rq.guides;
    m.want_hits = rq.host_hits || rq.guides;
    m.count = (p->flags & IPT_FLAG_COUNTERS) != 0;
    m.susp = m.traced ? needed_susp(p) : 0;
    return m;
}

// Passes per launch, so that the work buffers stay bounded: at most 2^29 units
// (37 B each: 2 GiB of radiance + 512 MiB of codes + 16 GiB of raygen
// records, of 288 GB), and at most 3/4 of the device memory this context
// can still obtain (hipMemGetInfo's free memory plus its own work buffers,
// less the sampling tables not yet built), so that contexts sharing a
// device split their passes into more launches instead of failing with
// IPT_E_OOM. Equal chunks: each launch ends with a tail in which lanes run
// out of work (the longest paths finish alone; 7 % of a 32-spp C2 launch),
// so few large launches beat many small ones (C2 1024^2 x 256 spp is a
// single launch).
int chunk_passes(ipt_ctx* ctx, const Call& c) {
    const LaunchMode& m = c.m;
    // (a preview unit is its value and code, 5 B, plus ipt_preview_values'
    // outputs; it has no raygen record and its launches read no table)
    constexpr size_t kRgBytes = 2 * sizeof(uint4);
    // (a compacting launch adds its compact values and dense-unit list, 8 B)
    constexpr size_t kCompactBytes = sizeof(float) + sizeof(uint32_t);
    const size_t unit_bytes = sizeof(float) + 1 +
                              (!m.traced ? (m.want_kinds ? 1 : 0) + (m.want_hits ? 6 * sizeof(float) : 0) : kRgBytes) +
                              (m.compact ? kCompactBytes : 0);
    size_t budget = (size_t)1 << 29;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const WorkSlot* S = ctx->slot;
        size_t avail = free_b + (S[0].work_cap + S[1].work_cap) * (sizeof(float) + 1) +
                       (!m.traced ? 0 : (S[0].rg_cap + S[1].rg_cap) * kRgBytes) +
                       (!m.compact ? 0 : (S[0].compact_cap + S[1].compact_cap) * kCompactBytes);
        const size_t tables = !m.traced ? 0 :
                              (ctx->d_cos_a ? 0 : ((size_t)3 << 26)) +
                              (ctx->d_frame_sc || !frame_table_user(ctx->scene.kp.geometry_kind)
                                   ? 0 : kFrameTabEntries * sizeof(float2));
        avail = avail > tables ? avail - tables : 0;
        // (two slots: consecutive launches hold a chunk each)
        budget = std::min(budget, std::max<size_t>(c.per_pass, avail / 8 * 3 / unit_bytes));
    }
    if (ctx->chunk_cap_test) budget = std::min(budget, std::max<size_t>(c.per_pass, ctx->chunk_cap_test));
    const size_t n_chunks = std::max<size_t>(1, ((size_t)c.p->spp * c.per_pass + budget - 1) / budget);
    int chunk = (int)std::max<size_t>(1, ((size_t)c.p->spp + n_chunks - 1) / n_chunks);
    while (chunk > 1 && (size_t)chunk * c.per_pass > budget) --chunk;
    return chunk;
}

// The next launch's slot. Its previous launch and that launch's readers
// (accumulate, host copies) must be done before its buffers are regrown or
// rewritten: the slot stream waits for them on the device, the host only where
// it rewrites device memory itself. Then the slot stream takes the gate on the
// other slot's launch, its predecessor.
int take_slot(ipt_ctx* ctx, const Call& c, WorkSlot*& out) {
    const ipt_params* p = c.p;
    WorkSlot& S = ctx->slot[ctx->next_slot];
    WorkSlot& P = ctx->slot[ctx->next_slot ^ 1u];
    ctx->next_slot ^= 1u;
    out = &S;
    if (const int rc = ensure_work(ctx, S, c)) return rc;
    const int plan[5] = {p->height, p->tile_rows, p->n_shards, p->shard_id, plane_of(p)};
    const bool replan = !std::equal(plan, plan + 5, S.plan);
    if (c.m.compact && !ctx->d_uring) HIPCHECK(ctx, hipMalloc(&ctx->d_uring, sizeof(unsigned long long) * 2 * kClkRing));
    if (replan) {
        if (S.used) HIPCHECK(ctx, hipEventSynchronize(S.done));
        // (synchronous copies: the host vectors do not outlive the call)
        HIPCHECK(ctx, hipMemcpy(S.d_cand_rows, c.rows.data(), sizeof(int) * c.n_cand, hipMemcpyHostToDevice));
        HIPCHECK(ctx, hipMemcpy(S.d_cand_of_row, c.of_row.data(), sizeof(int) * p->height, hipMemcpyHostToDevice));
        std::copy(plan, plan + 5, S.plan);
    }
    if (S.used) HIPCHECK(ctx, hipStreamWaitEvent(S.st, S.done, 0));
    // start in the predecessor's tail: once its pool is drained (or, without
    // stream value waits, once it has finished)
    // (P's counter is reset only by P's next launch, which waits for this
    // launch's pool in turn, so this wait cannot miss its value)
    // (a preview or replay launch has no tail to overlap and takes no gate;
    // such a predecessor leaves P.seq at that of P's last full launch, which
    // precedes it in P's stream)
    if (c.m.traced && P.used && !P.idle) {
        if (ctx->gate_on_pool)
            HIPCHECK(ctx, hipStreamWaitValue64(S.st, P.d_drained, P.seq, hipStreamWaitValueGte, ~0ull));
        else
            HIPCHECK(ctx, hipStreamWaitEvent(S.st, P.path_end, 0));
    }
    return IPT_OK;
}

// A launch's kernel parameters: the scene's template and what the call and
// this launch (passes [s0, s0 + ns) on slot S) add.
KParams launch_params(ipt_ctx* ctx, const Call& c, const WorkSlot& S, int s0, int ns) {
    const ipt_params* p = c.p;
    KParams kp = ctx->scene.kp;
    kp.W = p->width;
    kp.H = p->height;
    kp.spp = ns;
    kp.spp_offset = p->spp_offset + s0;
    kp.n_rays = p->n_rays;
    kp.meta_shift = p->n_rays > 255 ? 16 : 8;
    kp.depth_max = p->depth_max;
    kp.key0 = (uint32_t)p->seed;
    kp.key1 = (uint32_t)(p->seed >> 32);
    kp.n_cand = c.n_cand;
    kp.cand_rows = S.d_cand_rows;
    kp.tile_rows = p->tile_rows;
    kp.n_shards = p->n_shards;
    kp.shard_id = p->shard_id;
    kp.total_units = (unsigned long long)ns * c.per_pass;
    kp.per_pass32 = (uint32_t)c.per_pass;
    kp.inv_per_pass = 1.0 / (double)c.per_pass;
    kp.inv_w = 1.0 / (double)p->width;
    kp.unit_counter = S.d_unit;
    kp.drained = ctx->gate_on_pool ? S.d_drained : nullptr;
    kp.drain_seq = S.seq + 1;
#if IPT_RAYLOG
    kp.raylog = g_raylog;
    kp.raylog_n = g_raylog_n;
    kp.raylog_cap = g_raylog_cap;
    kp.raylog_every = g_raylog_every;
#endif
    kp.values = S.d_values;
    kp.codes = S.d_codes;
    kp.flags = S.d_flags;
    kp.rg = S.d_rg;
    kp.counters = ctx->d_counters;
    kp.cos_a = ctx->d_cos_a;  // (built before the call's first traced launch)
    kp.frame_sc = ctx->d_frame_sc;
    kp.count = c.m.count ? 1 : 0;
    kp.plane = plane_of(p);
    kp.mask = c.rq.mask;
    return kp;
}

// Queues the source of the launch's samples on the slot stream, between its
// t0 and t1 events: the caller's samples (replay_mark_kernel in the place of
// the raygen and path launches: no table, no raygen record), the preview
// kernel, or raygen + path kernel -- compacted or not.
int queue_samples(ipt_ctx* ctx, const Call& c, WorkSlot& S, const KParams& kp, int s0, ChunkTiming& tm) {
    const hipStream_t ss = S.st;
    const unsigned nblk = (unsigned)((kp.total_units + 255) / 256);
    if (c.m.replay) {
        const size_t off = (size_t)s0 * kp.W * kp.H;
        const ReplaySrc src{c.rq.replay.values + off, c.rq.replay.codes + off};
        hipLaunchKernelGGL(replay_mark_kernel, dim3(nblk), dim3(256), 0, ss, kp, src);
        HIPCHECK(ctx, hipGetLastError());
        return IPT_OK;
    }
    if (c.m.preview) {
        // one fused kernel; the counting / AOV instance only where asked
        const PreviewOut po{c.m.want_kinds ? S.d_kinds : nullptr, c.m.want_hits ? S.d_hits : nullptr};
        return (c.m.count || po.kinds || po.hits) ? launch_preview<true>(ctx, kp, po, ss)
                                                  : launch_preview<false>(ctx, kp, po, ss);
    }
    if (!c.m.compact) {
        hipLaunchKernelGGL(raygen_kernel, dim3(nblk), dim3(256), 0, ss, kp);
        HIPCHECK(ctx, hipGetLastError());
        if (const int rc = launch_path(ctx, kp, ss, c.m)) return rc;
        S.seq = kp.drain_seq;
        tm.units = kp.total_units;
        return IPT_OK;
    }
    // classify / scan / scatter / preset in raygen_kernel's place, the path
    // kernel over the compact range of the same records with the compact
    // values as its output, then the values back to their dense places:
    // everything after reads the launch as an uncompacted one leaves it
    CompactProbe* probe = c.rq.probe;
    tm.uring = (int)(ctx->next_uring++ % kClkRing);
    const CompactBufs cb{S.d_cblk, S.d_src, S.d_cvalues, S.d_values, ctx->d_uring + 2 * tm.uring};
    KParams kc = kp;
    if (probe) kc.count = 0;
    hipLaunchKernelGGL(compact_classify_kernel, dim3(nblk), dim3(256), 0, ss, kc, cb.blocks);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(256), 0, ss, cb.blocks, nblk);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nblk), dim3(256), 0, ss, kc, (const unsigned int*)cb.blocks, cb.src);
    hipLaunchKernelGGL(compact_preset_kernel, dim3(1), dim3(64), 0, ss, (const unsigned int*)cb.blocks, nblk,
                       kp.total_units, S.d_unit, cb.ring);
    HIPCHECK(ctx, hipGetLastError());
    if (probe) {
        // ipt_compact_plan: the plan of the call's first launch, no path kernel
        unsigned long long h[2] = {0, 0};
        HIPCHECK(ctx, hipStreamSynchronize(ss));
        HIPCHECK(ctx, hipMemcpy(h, cb.ring, sizeof h, hipMemcpyDeviceToHost));
        probe->start = h[0];
        probe->n_active = h[1];
        if (h[1] > kp.total_units || h[1] > probe->cap)
            probe->rc = fail(ctx, IPT_E_INVALID, "ipt_compact_plan: host_src holds fewer than n_active entries");
        else if (h[1])
            HIPCHECK(ctx, hipMemcpy(probe->host_src, cb.src + (kp.total_units - h[1]), h[1] * sizeof(uint32_t),
                                    hipMemcpyDeviceToHost));
        return IPT_OK;
    }
    kc.values = cb.cvalues;
    if (const int rc = launch_path(ctx, kc, ss, c.m)) return rc;
    S.seq = kp.drain_seq;
    hipLaunchKernelGGL(compact_expand_kernel, dim3(nblk), dim3(256), 0, ss, cb, nblk, kp.total_units);
    HIPCHECK(ctx, hipGetLastError());
    tm.units = kp.total_units;
    return IPT_OK;
}

// The call's host outputs of passes [s0, s0 + ns), [spp][H][W] (whole frames:
// per_pass == W * H), copied on the slot stream after the samples.
int queue_host_copies(ipt_ctx* ctx, const Call& c, const WorkSlot& S, int s0, int ns) {
    const LaunchRequest& rq = c.rq;
    const size_t off = (size_t)s0 * c.per_pass, n = (size_t)ns * c.per_pass;
    const hipStream_t ss = S.st;
    if (rq.host_values) {
        HIPCHECK(ctx, hipMemcpyAsync(rq.host_values + off, S.d_values, sizeof(float) * n, hipMemcpyDeviceToHost, ss));
        HIPCHECK(ctx, hipMemcpyAsync(rq.host_codes + off, S.d_codes, n, hipMemcpyDeviceToHost, ss));
    }
    if (rq.host_kinds) HIPCHECK(ctx, hipMemcpyAsync(rq.host_kinds + off, S.d_kinds, n, hipMemcpyDeviceToHost, ss));
    if (rq.host_hits)
        HIPCHECK(ctx, hipMemcpyAsync(rq.host_hits + off * 6, S.d_hits, sizeof(float) * 6 * n, hipMemcpyDeviceToHost, ss));
    return IPT_OK;
}

// ipt_guides_device (one pass, whole frame: unit = iy * W + ix): the scatter
// runs on the caller's stream, in call order, after the preview kernel; the
// slot's buffers are free again once it has run.
int queue_guide_scatter(ipt_ctx* ctx, const Call& c, WorkSlot& S, const ChunkTiming& tm) {
    const hipStream_t st = c.rq.st;
    HIPCHECK(ctx, hipStreamWaitEvent(st, tm.t1, 0));
    HIPCHECK(ctx, ipt_internal::launch_guide_scatter(st, S.d_kinds, S.d_hits, c.rq.guides, c.p->width, c.p->height,
                                                     plane_of(c.p) == kPlaneGui));
    HIPCHECK(ctx, hipEventRecord(S.done, st));
    return IPT_OK;
}

// The render plane's replay of the launch's ns passes: on the caller's stream,
// in call order, after this launch's path kernel.
int queue_accumulate(ipt_ctx* ctx, const Call& c, WorkSlot& S, int ns, ChunkTiming& tm) {
    const ipt_params* p = c.p;
    const LaunchRequest& rq = c.rq;
    const hipStream_t st = rq.st;
    HIPCHECK(ctx, hipStreamWaitEvent(st, tm.t1, 0));
    HIPCHECK(ctx, hipEventRecord(tm.a0, st));
    unsigned long long* clk = nullptr;
    if (ctx->d_clk) {
        tm.clk = (int)(ctx->next_clk++ % kClkRing);
        clk = ctx->d_clk + 2 * tm.clk;
        HIPCHECK(ctx, hipMemsetAsync(clk, 0xff, sizeof(unsigned long long), st));
        HIPCHECK(ctx, hipMemsetAsync(clk + 1, 0, sizeof(unsigned long long), st));
    }
    // (AParams' members in their order, then the ADAPT instances' two)
    const ipt_image& img = *rq.img;
    const AParamsAdapt aa{{p->width, p->height, ns, c.n_cand, S.d_cand_of_row, S.d_values, S.d_codes, S.d_flags,
                           p->tile_rows, p->n_shards, p->shard_id, img.pixels, img.counters, img.sums, img.pixel_max,
                           clk ? clk : ctx->d_clk_dummy},
                          rq.mask, rq.m2};
    const AParams& ap = aa;
    const dim3 grid((p->width + 255) / 256, p->height), block(256);
    const bool gui = plane_of(p) == kPlaneGui;
    if (c.m.adapt) {
        if (gui)
            hipLaunchKernelGGL((accumulate_kernel<kPlaneGui, true>), grid, block, 0, st, aa);
        else
            hipLaunchKernelGGL((accumulate_kernel<kPlaneGrid, true>), grid, block, 0, st, aa);
    } else if (gui)
        hipLaunchKernelGGL((accumulate_kernel<kPlaneGui, false>), grid, block, 0, st, ap);
    else
        hipLaunchKernelGGL((accumulate_kernel<kPlaneGrid, false>), grid, block, 0, st, ap);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipEventRecord(tm.a1, st));
    HIPCHECK(ctx, hipEventRecord(S.done, st));
    return IPT_OK;
}

// One launch: passes [s0, s0 + ns) of the call on the next slot.
int queue_launch(ipt_ctx* ctx, Call& c, int s0, int ns) {
    const LaunchRequest& rq = c.rq;
    WorkSlot* slot = nullptr;
    int rc = take_slot(ctx, c, slot);
    if (rc) return rc;
    WorkSlot& S = *slot;
    const unsigned sidx = (unsigned)(slot - ctx->slot);
    const KParams kp = launch_params(ctx, c, S, s0, ns);
    if (kp.total_units >= (1ull << 32)) return fail(ctx, IPT_E_INVALID, "more than 2^32 work units in one launch");
    // bounded timing backlog: settle launches far behind (they are done or
    // nearly so; the queue of launches ahead is untouched)
    while (ctx->pending.size() >= 8) {
        rc = settle_oldest(ctx);
        if (rc) return rc;
    }
    ChunkTiming ev;
    ev.t0 = pool_event(ctx);
    ev.t1 = pool_event(ctx);
    if (rq.img) {
        ev.a0 = pool_event(ctx);
        ev.a1 = pool_event(ctx);
    }
    if (!ev.t0 || !ev.t1 || (rq.img && (!ev.a0 || !ev.a1))) {
        pool_return(ctx, ev);
        return fail(ctx, IPT_E_DEVICE, "hipEventCreate failed");
    }
    // pushed before the first fallible call: drain settles it also on an error
    // below (unrecorded, untimed)
    ctx->pending.push_back(ev);
    ChunkTiming& tm = ctx->pending.back();
    S.used = true;
    S.idle = false;
    S.total = 0;  // (until its kernel is queued: a successor must not wait on a launch that failed)
    // the slot stream: t0..t1 is the path's per-sample work, raygen_kernel
    // (render_sample's jitter, camera ray, Philox block 0; ~0.2 % of a C2
    // launch) and path_kernel
    const hipStream_t ss = S.st;
    if (kp.mask && !c.mask_waited[sidx]) {
        // raygen reads caller memory: this slot stream's launches of the
        // call run after what the caller's stream holds at the call
        if (!S.mask_ready) HIPCHECK(ctx, hipEventCreateWithFlags(&S.mask_ready, hipEventDisableTiming));
        HIPCHECK(ctx, hipEventRecord(S.mask_ready, rq.st));
        HIPCHECK(ctx, hipStreamWaitEvent(ss, S.mask_ready, 0));
        c.mask_waited[sidx] = true;
    }
    // (a compacting launch's counter is set by compact_preset_kernel)
    if (!c.m.compact) HIPCHECK(ctx, hipMemsetAsync(S.d_unit, 0, sizeof(unsigned long long), ss));
    HIPCHECK(ctx, hipMemsetAsync(S.d_flags, 0, (size_t)kp.W * kp.H, ss));
    HIPCHECK(ctx, hipEventRecord(tm.t0, ss));
    rc = queue_samples(ctx, c, S, kp, s0, tm);
    if (rc) return rc;
    S.total = kp.total_units;
    HIPCHECK(ctx, hipEventRecord(tm.t1, ss));
    HIPCHECK(ctx, hipEventRecord(S.path_end, ss));
    rc = queue_host_copies(ctx, c, S, s0, ns);
    if (rc) return rc;
    // S.done: after the slot's last reader, the guide scatter, the accumulate or the host copies
    if (rq.guides)
        rc = queue_guide_scatter(ctx, c, S, tm);
    else if (!rq.img)
        HIPCHECK(ctx, hipEventRecord(S.done, ss));
    if (!rc && rq.img) rc = queue_accumulate(ctx, c, S, ns, tm);
    if (rc) return rc;
    tm.recorded = true;
    return IPT_OK;
}

// Queues the call's passes as launches of equal chunks, each on the next work
// slot (WorkSlot): the samples on the slot's stream, their readers -- the
// plane's replay or the guide scatter on the caller's stream, the host copies
// on the slot's -- after them. With a mask, each slot stream the call uses
// first waits for the caller's stream as it stands at the call (the mask is
// caller memory, written there). The probe's call ends after its first launch.
int render_chunks(ipt_ctx* ctx, const ipt_params* p, const LaunchRequest& rq) {
    Call c{p, rq, mode_of(p, rq)};
    candidate_rows(p, c.rows, c.of_row);
    c.n_cand = (int)c.rows.size();
    c.per_pass = (size_t)c.n_cand * p->width;
    if (c.per_pass == 0 || p->spp == 0) return IPT_OK;
    c.chunk = chunk_passes(ctx, c);
    // (the preview and the replay read neither table: a context that only
    // renders previews never builds them)
    if (c.m.traced) {
        int rc = ensure_cos_tables(ctx, rq.st);
        if (!rc && frame_table_user(ctx->scene.kp.geometry_kind)) rc = ensure_frame_table(ctx, rq.st);  // path_kernel's frame builds
        if (rc) return rc;
    }
    for (int s0 = 0; s0 < p->spp; s0 += c.chunk) {
        const int rc = queue_launch(ctx, c, s0, std::min(c.chunk, p->spp - s0));
        if (rc) return rc;
        if (rq.probe) return rq.probe->rc;
    }
    return IPT_OK;
}

}  // namespace

// Hooks for the library's other translation units (ipt_internal.h).
namespace ipt_internal {
int ctx_fail(ipt_ctx* ctx, int code, const std::string& msg) { return fail(ctx, code, msg); }
hipStream_t ctx_stream(ipt_ctx* ctx) { return ctx->stream; }
int ctx_device(ipt_ctx* ctx) { return ctx->device; }
int ctx_cus(ipt_ctx* ctx) { return ctx->n_cu; }
PostScratch& ctx_post(ipt_ctx* ctx) { return ctx->post; }
}  // namespace ipt_internal

extern "C" {

int ipt_abi_version(void) { return IPT_ABI_VERSION; }

const char* ipt_last_error(ipt_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> g(g_err_mu);
    return g_err_global.c_str();
}

int ipt_create(int hip_device, ipt_ctx** out) {
    if (!out) return fail(nullptr, IPT_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, IPT_E_DEVICE, "no HIP device available (the path tracer has no CPU fallback)");
    if (hip_device < 0 || hip_device >= n) return fail(nullptr, IPT_E_INVALID, "bad device index");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess)
        return fail(nullptr, IPT_E_DEVICE, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, IPT_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    ipt_ctx* ctx = new ipt_ctx();
    ctx->device = hip_device;
    ctx->n_cu = prop.multiProcessorCount;
    {
        // the records-in-LDS lattice instances are chosen against the device's
        // own limit (160 KiB on gfx950), so a smaller one falls back to the
        // global-record instances instead of failing the launch
        // (the larger of the per-block limit and its opt-in value)
        int lds = 0, optin = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, hip_device) != hipSuccess) lds = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, hip_device) != hipSuccess) optin = 0;
        if (std::max(lds, optin) > 0) ctx->max_lds = (size_t)std::max(lds, optin);
        (void)hipGetLastError();  // an unsupported attribute must not leave a sticky error behind
    }
    if (const char* e = std::getenv("IPT_BLOCKS_PER_CU")) ctx->bpc_override = std::atoi(e);  // profiling only
    if (const char* e = std::getenv("IPT_LNODES_LDS")) ctx->lnodes_lds = std::atoi(e) != 0;
    if (const char* e = std::getenv("IPT_LIGHT_GRID")) ctx->light_grid_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("IPT_LATTICE_LDS")) ctx->lattice_lds = std::atoi(e) != 0;
    if (const char* e = std::getenv("IPT_BOX_GENERIC")) ctx->box_generic = std::atoi(e) != 0;
    if (hipSetDevice(hip_device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return fail(nullptr, IPT_E_DEVICE, "stream creation failed");
    }
    if (const char* e = std::getenv("IPT_TEST_CHUNK_UNITS")) ctx->chunk_cap_test = (size_t)std::atoll(e);  // tests
    {
        // (round 4 measured hipStreamWaitValue64 on hipMalloc memory releasing
        // the waiting stream ~0.6 us after a kernel's atomicAdd reached the
        // value, scripts/probes/waitvalue_probe.hip; since round 6 the wait is
        // on a signal-memory flag, the memory the API specifies). A tool that serialises the
        // dispatches to collect counters or traces (rocprofv3 --pmc / --att,
        // which export ROCPROF_COUNTER_COLLECTION / ROCPROF_ADVANCED_THREAD_TRACE
        // to the profiled process) never released such a wait queued behind a
        // serialised dispatch, and the wait has no timeout: then
        // every launch is gated on its predecessor's path-end event instead
        // (the same images; consecutive launches lose their tail overlap).
        auto env_on = [](const char* n) {
            const char* v = std::getenv(n);
            return v && *v && std::strcmp(v, "0") != 0 && strcasecmp(v, "false") != 0 && strcasecmp(v, "off") != 0;
        };
        // (IPT_FORCE_POOL_GATE=1: keep the pool gate under such a tool --
        // diagnostics of that hang only)
        const bool serialising_tool = (env_on("ROCPROF_COUNTER_COLLECTION") || env_on("ROCPROF_ADVANCED_THREAD_TRACE")) &&
                                      !env_on("IPT_FORCE_POOL_GATE");
        int wv = 0;
        ctx->gate_on_pool = !env_on("IPT_NO_TAIL_OVERLAP") && !serialising_tool &&
                            hipDeviceGetAttribute(&wv, hipDeviceAttributeCanUseStreamWaitValue, hip_device) ==
                                hipSuccess &&
                            wv;
        (void)hipGetLastError();  // (an unsupported query leaves no sticky error for the caller's runtime)
    }
    for (WorkSlot& S : ctx->slot) {
        if (hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&S.done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&S.path_end, hipEventDisableTiming) != hipSuccess ||
            hipMalloc(&S.d_unit, sizeof(unsigned long long)) != hipSuccess) {
            ipt_destroy(ctx);
            return fail(nullptr, IPT_E_DEVICE, "work-slot stream / event / counter creation failed");
        }
        // the pool-drained flag: signal memory, set to 0 by a stream write
        // (without it -- allocation refused -- launches gate on events)
        if (ctx->gate_on_pool) {
            void* sig = nullptr;
            if (hipExtMallocWithFlags(&sig, sizeof(unsigned long long), hipMallocSignalMemory) != hipSuccess ||
                hipStreamWriteValue64(S.st, sig, 0ull, 0) != hipSuccess || hipStreamSynchronize(S.st) != hipSuccess) {
                if (sig) hipFree(sig);
                sig = nullptr;
                ctx->gate_on_pool = false;
                (void)hipGetLastError();
            }
            S.d_drained = reinterpret_cast<unsigned long long*>(sig);
        }
    }
    if (!ctx->gate_on_pool)
        for (WorkSlot& S : ctx->slot) {
            if (S.d_drained) hipFree(S.d_drained);
            S.d_drained = nullptr;
        }
    if (hipMalloc(&ctx->d_counters, sizeof(unsigned long long) * (kNumCounters + 2 * kProfPhases + kStamps)) != hipSuccess) {
        ipt_destroy(ctx);
        return fail(nullptr, IPT_E_OOM, "hipMalloc failed");
    }
    hipMemset(ctx->d_counters, 0, sizeof(unsigned long long) * (kNumCounters + 2 * kProfPhases + kStamps));
    if (hipMalloc(&ctx->d_clk, sizeof(unsigned long long) * 2 * (kClkRing + 1)) != hipSuccess) {
        ipt_destroy(ctx);
        return fail(nullptr, IPT_E_OOM, "hipMalloc failed");
    }
    ctx->d_clk_dummy = ctx->d_clk + 2 * kClkRing;
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, hip_device) == hipSuccess && khz > 0)
            ctx->clk_khz = (double)khz;
        (void)hipGetLastError();
    }
    *out = ctx;
    return IPT_OK;
}

void ipt_destroy(ipt_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    (void)drain(ctx);  // nothing queued may still use the buffers
    ipt_internal::post_release(ctx);
    // the context's own tables and rings (the scene's buffers go with its record)
    for (void* b : {(void*)ctx->d_counters, (void*)ctx->d_cos_a, (void*)ctx->d_cos_b, (void*)ctx->d_clk,
                    (void*)ctx->d_uring, (void*)ctx->d_frame_sc})
        if (b) hipFree(b);
    for (WorkSlot& S : ctx->slot) S.release();
    for (hipEvent_t e : ctx->ev_pool) hipEventDestroy(e);
    ctx->rp.release();
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int ipt_upload_scene(ipt_ctx* ctx, const ipt_scene* s) {
    if (!ctx) return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    {
        const int rc = drain(ctx);  // queued launches read the scene being replaced
        if (rc) return rc;
    }
    ctx->has_scene = false;  // any failure below leaves no scene (ipt_capi.h)
    ScenePlan plan;  // everything the scene decides, on the host (ipt_scene_plan.h)
    {
        std::string err;
        const int rc = plan_scene(s, PlanSettings{ctx->lnodes_lds != 0, ctx->light_grid_on != 0}, plan, err);
        if (rc) return fail(ctx, rc, err);
    }
    // Device phase, transactional: the new scene is built in a fresh record,
    // every buffer allocated and filled there first. Until all of them
    // succeeded the context has no scene (renders fail with IPT_E_NOSCENE,
    // never launch on a half-built one); on success the record is swapped in
    // and the old one frees its buffers. IPT_TEST_FAIL_UPLOAD_ALLOC=k makes the
    // k-th allocation of an upload fail (tests/test_gpu_parity.py exercises
    // the failure path).
    int n_alloc = 0, fail_at = 0;
    if (const char* e = std::getenv("IPT_TEST_FAIL_UPLOAD_ALLOC")) fail_at = std::atoi(e);
    auto upload = [&](auto& buf, const auto* src, size_t count) -> int {
        using T = std::remove_pointer_t<decltype(buf.p)>;
        if (++n_alloc == fail_at) return fail(ctx, IPT_E_OOM, "injected allocation failure (IPT_TEST_FAIL_UPLOAD_ALLOC)");
        HIPCHECK(ctx, hipMalloc(&buf.p, sizeof(T) * std::max<size_t>(count, 1)));
        if (count) HIPCHECK(ctx, hipMemcpy(buf.p, src, sizeof(T) * count, hipMemcpyHostToDevice));
        return IPT_OK;
    };
    auto upload_v = [&](auto& buf, const auto& v) { return upload(buf, v.data(), v.size()); };
    Scene sc;
    Scene::Bufs& b = sc.bufs;
    const bool use_grid = plan.kp.n_grid > 0, use_bvh = !plan.bvh_nodes.empty(), lattice = plan.light_pattern != 0;
    int rc = IPT_OK;
    if (use_grid && !rc) rc = upload_v(b.grid_start, plan.grid_start);
    if (use_grid && !rc) rc = upload_v(b.grid_items, plan.grid_items);
    if (use_grid && !rc) rc = upload_v(b.grid_c4, plan.grid_c4);
    if (!plan.light_nodes.empty() && !rc) rc = upload_v(b.light_nodes, plan.light_nodes);
    if (lattice && !rc) rc = upload_v(b.lgrid, plan.lgrid);
    if (lattice && !rc) rc = upload_v(b.lax, plan.lax);
    if (!plan.cdf_lo.empty() && !rc) rc = upload_v(b.cdf_lo, plan.cdf_lo);
    if (use_bvh && !rc) rc = upload_v(b.bvh_nodes, plan.bvh_nodes);
    if (use_bvh && !rc) rc = upload_v(b.bvh_prims, plan.bvh_prims);
    if (!rc) rc = upload_v(b.lights, plan.lights);
    if (!rc) rc = upload_v(b.weights, plan.weights);
    if (!rc) rc = upload_v(b.cdf, plan.cdf);
    if (!rc) rc = upload(b.wall, plan.wall, 5);
    if (!rc) rc = upload_v(b.spheres, plan.spheres);
    if (rc) return rc;  // the record frees what it holds; the context keeps no scene
    // (kp's scalars from the plan: what this scene does not set is zero and no kernel reads it -- DESIGN.md 5)
    KParams& k = sc.kp = plan.kp;
    k.lights = b.lights.p;
    k.weights = b.weights.p;
    k.cdf = b.cdf.p;
    k.wall_frames = b.wall.p;
    k.spheres = b.spheres.p;
    k.grid_start = b.grid_start.p;
    k.grid_items = b.grid_items.p;
    k.grid_c4 = b.grid_c4.p;
    if (use_grid) k.grid_idx = reinterpret_cast<const int*>(b.grid_c4.p + plan.grid_items.size());
    k.bvh_nodes = b.bvh_nodes.p;
    k.bvh_prims = b.bvh_prims.p;
    k.light_nodes = b.light_nodes.p;
    k.lgrid = b.lgrid.p;
    k.lax = reinterpret_cast<const float4*>(b.lax.p);
    k.cdf_lo = b.cdf_lo.p;
    sc.any_round_light = plan.any_round_light;
    sc.light_axis = plan.light_axis;
    sc.light_pattern = plan.light_pattern;
    std::swap(ctx->scene, sc);  // (sc, now the previous scene, frees its buffers on return)
    ctx->has_scene = true;
    return IPT_OK;
}

int ipt_render_device_async(ipt_ctx* ctx, const ipt_params* p, ipt_image* img, void* hip_stream) {
    return ipt_render_masked_device_async(ctx, p, img, nullptr, nullptr, hip_stream);  // (the unmasked launches)
}

int ipt_render_masked_device_async(ipt_ctx* ctx, const ipt_params* p, ipt_image* img, const uint8_t* dev_mask,
                                   float* dev_m2, void* hip_stream) {
    if (const int rc = validate(ctx, p)) return rc;
    if (!img || !img->pixels || !img->counters) return fail(ctx, IPT_E_INVALID, "image pixels/counters are NULL");
    {
        // the mask and m2 may not share a byte with an image buffer (or each other)
        const size_t n = (size_t)p->width * p->height;
        const void* buf[6] = {dev_mask, dev_m2, img->pixels, img->counters, img->sums, img->pixel_max};
        const size_t len[6] = {n, n * 4, n * 4, n * 4, n * 4, n * 4};
        for (int a = 0; a < 2; ++a)
            for (int b = a + 1; b < 6; ++b) {
                const uintptr_t x = (uintptr_t)buf[a], y = (uintptr_t)buf[b];
                if (buf[a] && buf[b] && x < y + len[b] && y < x + len[a])
                    return fail(ctx, IPT_E_INVALID, "ipt_render_masked_device: the mask or m2 overlaps another buffer");
            }
    }
    hipSetDevice(ctx->device);
    LaunchRequest rq;
    rq.img = img;
    rq.st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    rq.mask = dev_mask;
    rq.m2 = dev_m2;
    return render_chunks(ctx, p, rq);
}

int ipt_render_masked_device(ipt_ctx* ctx, const ipt_params* p, ipt_image* img, const uint8_t* dev_mask, float* dev_m2,
                             void* hip_stream) {
    const int rc = ipt_render_masked_device_async(ctx, p, img, dev_mask, dev_m2, hip_stream);
    const int rw = ctx ? drain(ctx) : IPT_OK;
    return rc ? rc : rw;
}

int ipt_render_adaptive(ipt_ctx* ctx, const ipt_params* p, const ipt_adapt_params* ap, int32_t round_spp,
                        ipt_image* himg, float* host_m2, uint8_t* host_mask, uint32_t* stats) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!ap || !stats || round_spp < 1) return fail(ctx, IPT_E_INVALID, "ipt_render_adaptive: ap/stats NULL or round_spp < 1");
    if (!himg || !himg->pixels || !himg->counters) return fail(ctx, IPT_E_INVALID, "image pixels/counters are NULL");
    if (ap->width != p->width || ap->height != p->height ||
        ((ap->flags ^ p->flags) & (uint32_t)IPT_FLAG_GUI_PLANE) != 0)
        return fail(ctx, IPT_E_INVALID, "ipt_render_adaptive: ap's size and plane flag must be p's");
    if (p->n_shards > 1) return fail(ctx, IPT_E_UNSUPPORTED, "ipt_render_adaptive renders whole frames on one device");
    hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)p->width * p->height;
    DevBuf<float> dpx, dsum, dmax, dm2;
    DevBuf<uint32_t> dcnt, dstats;
    DevBuf<uint8_t> dmask;
    HIPCHECK(ctx, hipMalloc(&dpx.p, n * 4));
    HIPCHECK(ctx, hipMalloc(&dcnt.p, n * 4));
    if (himg->sums) HIPCHECK(ctx, hipMalloc(&dsum.p, n * 4));
    if (himg->pixel_max) HIPCHECK(ctx, hipMalloc(&dmax.p, n * 4));
    HIPCHECK(ctx, hipMalloc(&dm2.p, n * 4));
    HIPCHECK(ctx, hipMalloc(&dmask.p, n));
    HIPCHECK(ctx, hipMalloc(&dstats.p, 4 * sizeof(uint32_t)));
    HIPCHECK(ctx, hipMemcpy(dpx.p, himg->pixels, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(ctx, hipMemcpy(dcnt.p, himg->counters, n * 4, hipMemcpyHostToDevice));
    if (himg->sums) HIPCHECK(ctx, hipMemcpy(dsum.p, himg->sums, n * 4, hipMemcpyHostToDevice));
    if (himg->pixel_max) HIPCHECK(ctx, hipMemcpy(dmax.p, himg->pixel_max, n * 4, hipMemcpyHostToDevice));
    if (host_m2)
        HIPCHECK(ctx, hipMemcpy(dm2.p, host_m2, n * 4, hipMemcpyHostToDevice));
    else
        HIPCHECK(ctx, hipMemset(dm2.p, 0, n * 4));
    HIPCHECK(ctx, hipMemset(dmask.p, 1, n));
    ipt_image dimg{dpx.p, dcnt.p, dsum.p, dmax.p};
    uint32_t hs[4] = {0, 0, 0, 0};
    int done = 0;
    // (an error below returns after the drain: the buffers are freed on return)
    for (int round = 0; done < p->spp && rc == IPT_OK; ++round) {
        ipt_params q = *p;
        q.spp = std::min<int>(round_spp, p->spp - done);
        q.spp_offset = p->spp_offset + done;
        rc = ipt_render_masked_device_async(ctx, &q, &dimg, round ? dmask.p : nullptr, dm2.p, st);
        if (!rc) rc = ipt_adapt_device(ctx, ap, dpx.p, dcnt.p, dm2.p, dmask.p, dstats.p, st);
        if (!rc && hipMemcpyAsync(hs, dstats.p, sizeof hs, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = fail(ctx, IPT_E_DEVICE, "ipt_render_adaptive: stats copy failed");
        if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(ctx, IPT_E_DEVICE, "ipt_render_adaptive: round failed");
        if (rc) break;
        done += q.spp;
        if (hs[0] == 0) break;
    }
    const int rw = drain(ctx);
    if (rc) return rc;
    if (rw) return rw;
    HIPCHECK(ctx, hipMemcpy(himg->pixels, dpx.p, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(ctx, hipMemcpy(himg->counters, dcnt.p, n * 4, hipMemcpyDeviceToHost));
    if (himg->sums) HIPCHECK(ctx, hipMemcpy(himg->sums, dsum.p, n * 4, hipMemcpyDeviceToHost));
    if (himg->pixel_max) HIPCHECK(ctx, hipMemcpy(himg->pixel_max, dmax.p, n * 4, hipMemcpyDeviceToHost));
    if (host_m2) HIPCHECK(ctx, hipMemcpy(host_m2, dm2.p, n * 4, hipMemcpyDeviceToHost));
    if (host_mask) HIPCHECK(ctx, hipMemcpy(host_mask, dmask.p, n, hipMemcpyDeviceToHost));
    stats[0] = hs[0];
    stats[1] = hs[1];
    stats[2] = hs[2];
    stats[3] = (uint32_t)done;
    return IPT_OK;
}

int ipt_render_wait(ipt_ctx* ctx) {
    if (!ctx) return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    return drain(ctx);
}

int ipt_render_device(ipt_ctx* ctx, const ipt_params* p, ipt_image* img, void* hip_stream) {
    return ipt_render_masked_device(ctx, p, img, nullptr, nullptr, hip_stream);
}

int ipt_render(ipt_ctx* ctx, const ipt_params* p, ipt_image* himg) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!himg || !himg->pixels || !himg->counters) return fail(ctx, IPT_E_INVALID, "image pixels/counters are NULL");
    hipSetDevice(ctx->device);
    ResidentPlane& R = ctx->rp;
    R.h2d = R.d2h = 0;
    const int W = p->width, H = p->height;
    const bool has_sums = himg->sums != nullptr, has_pmax = himg->pixel_max != nullptr;
    if (R.W != W || R.H != H || R.has_sums != has_sums || R.has_pmax != has_pmax || !R.d_pixels) {
        R.release();
        const size_t npix = (size_t)W * H;
        HIPCHECK(ctx, hipMalloc(&R.d_pixels, npix * 4));
        HIPCHECK(ctx, hipMalloc(&R.d_counters, npix * 4));
        if (has_sums) HIPCHECK(ctx, hipMalloc(&R.d_sums, npix * 4));
        if (has_pmax) HIPCHECK(ctx, hipMalloc(&R.d_pmax, npix * 4));
        R.W = W;
        R.H = H;
        R.has_sums = has_sums;
        R.has_pmax = has_pmax;
    }
    const bool sharded = p->n_shards > 1 && p->tile_rows > 0;
    const int plan[3] = {sharded ? p->tile_rows : 0, sharded ? p->n_shards : 1, sharded ? p->shard_id : 0};
    if (!std::equal(plan, plan + 3, R.plan)) {
        R.runs.clear();
        R.owned_px = 0;
        for (int y = 0; y < H;) {
            if (!owned_host(p, y)) { ++y; continue; }
            int y1 = y + 1;
            while (y1 < H && owned_host(p, y1)) ++y1;
            R.runs.emplace_back(y, y1);
            R.owned_px += (size_t)(y1 - y) * W;
            y = y1;
        }
        std::copy(plan, plan + 3, R.plan);
        R.shadow_ok = false;
    }
    // (host field, device field) in shadow order
    struct Field { uint8_t* h; uint8_t* d; };
    std::vector<Field> fields = {{reinterpret_cast<uint8_t*>(himg->pixels), reinterpret_cast<uint8_t*>(R.d_pixels)},
                                 {reinterpret_cast<uint8_t*>(himg->counters), reinterpret_cast<uint8_t*>(R.d_counters)}};
    if (has_sums) fields.push_back({reinterpret_cast<uint8_t*>(himg->sums), reinterpret_cast<uint8_t*>(R.d_sums)});
    if (has_pmax) fields.push_back({reinterpret_cast<uint8_t*>(himg->pixel_max), reinterpret_cast<uint8_t*>(R.d_pmax)});
    const size_t field_bytes = R.owned_px * 4;
    if (R.shadow.size() != fields.size() * field_bytes) {
        R.shadow.assign(fields.size() * field_bytes, 0);
        R.shadow_ok = false;
    }
    hipStream_t st = ctx->stream;
    // upload the owned runs the caller changed since the last call (all of
    // them when the shadow is not valid)
    for (size_t f = 0; f < fields.size(); ++f) {
        size_t off = f * field_bytes;
        for (const auto& r : R.runs) {
            const size_t b0 = (size_t)r.first * W * 4, len = (size_t)(r.second - r.first) * W * 4;
            if (!R.shadow_ok || std::memcmp(fields[f].h + b0, R.shadow.data() + off, len) != 0) {
                HIPCHECK(ctx, hipMemcpyAsync(fields[f].d + b0, fields[f].h + b0, len, hipMemcpyHostToDevice, st));
                R.h2d += len;
            }
            off += len;
        }
    }
    R.shadow_ok = false;  // (valid again only once this call's rows are back)
    ipt_image d{R.d_pixels, R.d_counters, R.d_sums, R.d_pmax};
    LaunchRequest rq;
    rq.img = &d;
    rq.st = st;
    rc = render_chunks(ctx, p, rq);
    if (rc) {
        (void)drain(ctx);  // nothing queued may still use the buffers
        (void)hipStreamSynchronize(st);
        return rc;
    }
    for (size_t f = 0; f < fields.size(); ++f)
        for (const auto& r : R.runs) {
            const size_t b0 = (size_t)r.first * W * 4, len = (size_t)(r.second - r.first) * W * 4;
            HIPCHECK(ctx, hipMemcpyAsync(fields[f].h + b0, fields[f].d + b0, len, hipMemcpyDeviceToHost, st));
            R.d2h += len;
        }
    HIPCHECK(ctx, hipStreamSynchronize(st));
    rc = drain(ctx);
    if (rc) return rc;
    for (size_t f = 0; f < fields.size(); ++f) {
        size_t off = f * field_bytes;
        for (const auto& r : R.runs) {
            const size_t b0 = (size_t)r.first * W * 4, len = (size_t)(r.second - r.first) * W * 4;
            std::memcpy(R.shadow.data() + off, fields[f].h + b0, len);
            off += len;
        }
    }
    R.shadow_ok = true;
    return IPT_OK;
}

int ipt_transfer_bytes(ipt_ctx* ctx, uint64_t* host_to_device, uint64_t* device_to_host) {
    if (!ctx || !host_to_device || !device_to_host) return IPT_E_INVALID;
    *host_to_device = ctx->rp.h2d;
    *device_to_host = ctx->rp.d2h;
    return IPT_OK;
}

// A call with host outputs: queued on the context's stream, then waited for.
static int render_to_host(ipt_ctx* ctx, const ipt_params* p, LaunchRequest rq) {
    rq.st = ctx->stream;
    const int rc = render_chunks(ctx, p, rq);
    const int rw = drain(ctx);  // the host copies run on the slot streams
    if (rc) return rc;
    if (rw) return rw;
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    return IPT_OK;
}

int ipt_render_values(ipt_ctx* ctx, const ipt_params* p, float* values, uint8_t* codes) {
    if (const int rc = validate(ctx, p)) return rc;
    if (!values || !codes) return fail(ctx, IPT_E_INVALID, "values/codes are NULL");
    if (p->n_shards > 1) return fail(ctx, IPT_E_UNSUPPORTED, "ipt_render_values renders whole frames");
    hipSetDevice(ctx->device);
    LaunchRequest rq;
    rq.host_values = values;
    rq.host_codes = codes;
    return render_to_host(ctx, p, rq);
}

int ipt_preview_values(ipt_ctx* ctx, const ipt_params* p, float* values, uint8_t* codes, uint8_t* kinds, float* hits) {
    if (const int rc = validate(ctx, p, true)) return rc;
    if (!values || !codes) return fail(ctx, IPT_E_INVALID, "values/codes are NULL");
    if (p->n_shards > 1) return fail(ctx, IPT_E_UNSUPPORTED, "ipt_preview_values renders whole frames");
    hipSetDevice(ctx->device);
    LaunchRequest rq;
    rq.host_values = values;
    rq.host_codes = codes;
    rq.host_kinds = kinds;
    rq.host_hits = hits;
    rq.preview = true;
    return render_to_host(ctx, p, rq);
}

int ipt_guides_device(ipt_ctx* ctx, const ipt_params* p, ipt_guide* dev_guides, void* hip_stream) {
    if (const int rc = validate(ctx, p, true)) return rc;
    if (!dev_guides) return fail(ctx, IPT_E_INVALID, "ipt_guides_device: dev_guides is NULL");
    if (p->spp != 1) return fail(ctx, IPT_E_INVALID, "ipt_guides_device: spp must be 1 (one sample per pixel)");
    if (p->n_shards > 1) return fail(ctx, IPT_E_UNSUPPORTED, "ipt_guides_device writes whole frames");
    if (p->flags & ~(uint32_t)(IPT_FLAG_GUI_PLANE | IPT_FLAG_PREVIEW))
        return fail(ctx, IPT_E_UNSUPPORTED, "ipt_guides_device takes IPT_FLAG_GUI_PLANE and IPT_FLAG_PREVIEW alone");
    hipSetDevice(ctx->device);
    // (tile_rows without shards: the call owns the whole frame)
    LaunchRequest rq;
    rq.st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    rq.preview = true;
    rq.guides = dev_guides;
    return render_chunks(ctx, p, rq);
}

int ipt_guides(ipt_ctx* ctx, const ipt_params* p, ipt_guide* guides) {
    if (!ctx) return IPT_E_INVALID;
    if (!guides) return fail(ctx, IPT_E_INVALID, "ipt_guides: guides is NULL");
    if (!p || p->width <= 0 || p->height <= 0) return fail(ctx, IPT_E_INVALID, "ipt_guides: bad arguments");
    hipSetDevice(ctx->device);
    const size_t bytes = (size_t)p->width * (size_t)p->height * sizeof(ipt_guide);
    DevBuf<ipt_guide> dg;
    HIPCHECK(ctx, hipMalloc(&dg.p, bytes));
    const int rc = ipt_guides_device(ctx, p, dg.p, ctx->stream);
    const int rw = drain(ctx);
    if (rc) return rc;
    if (rw) return rw;
    HIPCHECK(ctx, hipMemcpyAsync(guides, dg.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    return IPT_OK;
}

int ipt_replay_samples(ipt_ctx* ctx, const ipt_params* p, const float* values, const uint8_t* codes,
                       ipt_image* img, void* hip_stream) {
    // everything is refused here, on the host, before a device buffer is
    // touched: replay_mark_kernel writes flags at a code's destination
    if (!ctx) return IPT_E_INVALID;
    if (!p) return fail(ctx, IPT_E_INVALID, "params is NULL");
    if (!values || !codes) return fail(ctx, IPT_E_INVALID, "values/codes are NULL");
    if (!img || !img->pixels || !img->counters) return fail(ctx, IPT_E_INVALID, "image pixels/counters are NULL");
    if (p->width <= 0 || p->height <= 0 || p->width > 65536 || p->height > 65536)
        return fail(ctx, IPT_E_INVALID, "width/height out of range");
    if (p->spp < 0) return fail(ctx, IPT_E_INVALID, "negative spp");
    if (p->n_shards > 1 && (p->shard_id < 0 || p->shard_id >= p->n_shards))
        return fail(ctx, IPT_E_INVALID, "shard_id out of range");
    if (p->flags & ~(uint32_t)IPT_FLAG_GUI_PLANE)
        return fail(ctx, IPT_E_UNSUPPORTED, "ipt_replay_samples takes IPT_FLAG_GUI_PLANE alone");
    const int W = p->width, H = p->height;
    const int64_t n = (int64_t)p->spp * W * H;  // (< 2^63: 2^31 * 2^16 * 2^16)
    if (n > (int64_t)IPT_REPLAY_MAX_SAMPLES)
        return fail(ctx, IPT_E_UNSUPPORTED, "more than IPT_REPLAY_MAX_SAMPLES samples in one call");
    if (n == 0) return IPT_OK;
    const bool gui = plane_of(p) == kPlaneGui;
    for (int s = 0; s < p->spp; ++s)
        for (int iy = 0; iy < H; ++iy) {
            const int yn = gui ? ipt::gui_nominal_row(iy, H) : ipt::nominal_row(iy, H);
            const uint8_t* row = codes + ((size_t)s * H + iy) * W;
            for (int ix = 0; ix < W; ++ix) {
                const uint8_t c = row[ix];
                const int fx = c & 3, fy = (c >> 2) & 3;
                if (c >= 0x10 || fx == 3 || fy == 3)
                    return fail(ctx, IPT_E_INVALID, "not a drift code (0xfe and 0xff are the library's own)");
                const int xi = ix + fx - 1, yi = yn + fy - 1;
                if (xi < 0 || xi >= W || yi < 0 || yi >= H)
                    return fail(ctx, IPT_E_INVALID, "a code's destination lies outside the frame");
            }
        }
    hipSetDevice(ctx->device);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    DevBuf<float> dv;
    DevBuf<uint8_t> dc;
    HIPCHECK(ctx, hipMalloc(&dv.p, (size_t)n * sizeof(float)));
    HIPCHECK(ctx, hipMalloc(&dc.p, (size_t)n));
    HIPCHECK(ctx, hipMemcpy(dv.p, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(ctx, hipMemcpy(dc.p, codes, (size_t)n, hipMemcpyHostToDevice));
    LaunchRequest rq;
    rq.img = img;
    rq.st = st;
    rq.replay = ReplaySrc{dv.p, dc.p};
    const int rc = render_chunks(ctx, p, rq);
    // (nothing queued may still read the source when it is freed)
    const int rw = drain(ctx);
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return rc;
    if (rw) return rw;
    HIPCHECK(ctx, e);
    return IPT_OK;
}

int ipt_shard_plan(const ipt_params* p, uint8_t* owned_rows, int32_t* cand_rows, int32_t* n_cand) {
    if (!p || !owned_rows || !cand_rows || !n_cand || p->height <= 0) return IPT_E_INVALID;
    std::vector<int> rows, of_row;
    candidate_rows(p, rows, of_row);
    for (int y = 0; y < p->height; ++y) owned_rows[y] = owned_host(p, y) ? 1 : 0;
    for (size_t i = 0; i < rows.size(); ++i) cand_rows[i] = rows[i];
    *n_cand = (int32_t)rows.size();
    return IPT_OK;
}

int ipt_get_counters(ipt_ctx* ctx, ipt_counters* out) {
    if (!ctx || !out) return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    if (const int rc = drain(ctx)) return rc;
    unsigned long long h[kNumCounters];
    HIPCHECK(ctx, hipMemcpy(h, ctx->d_counters, sizeof h, hipMemcpyDeviceToHost));
    out->paths = h[0];
    out->traced_rays = h[1];
    out->surface_hits = h[2];
    out->light_hits = h[3];
    out->expanded_nodes = h[4];
    out->iterations = h[5];
    out->light_samples = h[6];
    out->skipped = h[7];
    out->sphere_frames = h[8];
    out->light_traces = h[9];
    out->drifted = h[10];
    out->bvh_nodes = h[11];
    out->sphere_tests = h[12];
    out->light_nodes = h[13];
    out->light_tests = h[14];
    return IPT_OK;
}

int ipt_get_profile(ipt_ctx* ctx, uint64_t* out, int n) {
    if (!ctx || !out || n < 0) return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    if (const int rc = drain(ctx)) return rc;
    unsigned long long h[2 * kProfPhases + kStamps];
    HIPCHECK(ctx, hipMemcpy(h, ctx->d_counters + kNumCounters, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < n && i < 2 * kProfPhases + kStamps; ++i) out[i] = h[i];
    return IPT_OK;
}

int ipt_reset_counters(ipt_ctx* ctx) {
    if (!ctx) return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    if (const int rc = drain(ctx)) return rc;
    HIPCHECK(ctx, hipMemset(ctx->d_counters, 0, sizeof(unsigned long long) * (kNumCounters + 2 * kProfPhases + kStamps)));
    return IPT_OK;
}

int ipt_last_kernel_ms(ipt_ctx* ctx, float* path_ms, float* accumulate_ms) {
    if (!ctx) return IPT_E_INVALID;
    if (path_ms) *path_ms = ctx->last_path_ms;
    if (accumulate_ms) *accumulate_ms = ctx->last_acc_ms;
    return IPT_OK;
}

int ipt_last_units(ipt_ctx* ctx, uint64_t out[3]) {
    if (!ctx || !out) return IPT_E_INVALID;
    for (int i = 0; i < 3; ++i) out[i] = ctx->last_units[i];
    return IPT_OK;
}

int ipt_last_instance(ipt_ctx* ctx, int32_t out[6]) {
    if (!ctx || !out) return IPT_E_INVALID;
    if (ctx->last_instance[0] == 0) return fail(ctx, IPT_E_INVALID, "ipt_last_instance: no path-kernel launch yet");
    std::copy(ctx->last_instance, ctx->last_instance + 6, out);
    return IPT_OK;
}

int ipt_compact_plan(ipt_ctx* ctx, const ipt_params* p, const uint8_t* dev_mask, uint32_t* host_src, uint64_t cap,
                     uint64_t* n_active, uint64_t* start) {
    int rc = validate(ctx, p);
    if (rc) return rc;
    if (!n_active || !start || (cap && !host_src)) return fail(ctx, IPT_E_INVALID, "ipt_compact_plan: NULL output");
    if (p->flags & IPT_FLAG_PREVIEW) return fail(ctx, IPT_E_UNSUPPORTED, "ipt_compact_plan: the preview has no unit pool");
    hipSetDevice(ctx->device);
    rc = drain(ctx);
    if (rc) return rc;
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the mask is the caller's, written on any stream before the call)
    CompactProbe probe{host_src, cap};
    LaunchRequest rq;
    rq.st = ctx->stream;
    rq.mask = dev_mask;
    rq.probe = &probe;
    rc = render_chunks(ctx, p, rq);
    const int rw = drain(ctx);
    *n_active = probe.n_active;
    *start = probe.start;
    return rc ? rc : rw;
}

int ipt_math_host(int fn, const float* in, float* out, int64_t n) {
    if (!in || !out || n < 0 || fn < 0 || fn > 15) return IPT_E_INVALID;
    const int nt = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([=]() {
            for (int64_t i = t; i < n; i += nt) out[i] = math_fn(fn, in[i]);
        });
    for (auto& x : th) x.join();
    return IPT_OK;
}

int ipt_math_device(ipt_ctx* ctx, int fn, const float* in, float* out, int64_t n) {
    if (!ctx || !in || !out || n < 0 || fn < 0 || fn > 15) return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    DevBuf<float> din, dout;
    HIPCHECK(ctx, hipMalloc(&din.p, std::max<int64_t>(n, 1) * 4));
    HIPCHECK(ctx, hipMalloc(&dout.p, std::max<int64_t>(n, 1) * 4));
    HIPCHECK(ctx, hipMemcpy(din.p, in, n * 4, hipMemcpyHostToDevice));
    const long long blocks = (n + 255) / 256;
    if (blocks > 0)
        hipLaunchKernelGGL(math_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, fn, din.p, dout.p, (long long)n);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHECK(ctx, hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return IPT_OK;
}

int ipt_philox(ipt_ctx* ctx, uint32_t key0, uint32_t key1, const uint32_t* ctr, uint32_t* out, int64_t n) {
    if (!ctr || !out || n < 0) return ctx ? fail(ctx, IPT_E_INVALID, "ipt_philox: bad arguments") : IPT_E_INVALID;
    if (!ctx) {
        for (int64_t i = 0; i < n; ++i) {
            const u32x4 o = philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key0, key1);
            for (int q = 0; q < 4; ++q) out[4 * i + q] = o.v[q];
        }
        return IPT_OK;
    }
    hipSetDevice(ctx->device);
    DevBuf<uint4> din, dout;
    HIPCHECK(ctx, hipMalloc(&din.p, std::max<int64_t>(n, 1) * sizeof(uint4)));
    HIPCHECK(ctx, hipMalloc(&dout.p, std::max<int64_t>(n, 1) * sizeof(uint4)));
    HIPCHECK(ctx, hipMemcpy(din.p, ctr, n * sizeof(uint4), hipMemcpyHostToDevice));
    if (n > 0)
        hipLaunchKernelGGL(philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, key0, key1,
                           din.p, dout.p, (long long)n);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHECK(ctx, hipMemcpy(out, dout.p, n * sizeof(uint4), hipMemcpyDeviceToHost));
    return IPT_OK;
}

static int ddf_call(ipt_ctx* ctx, int value_mode, int kind, const float* params, const float* in, int64_t n,
                    float* out) {
    if (!ctx) return IPT_E_INVALID;
    if (!params || !in || !out || n < 0 || kind < 0 || kind > 3) return fail(ctx, IPT_E_INVALID, "ipt_ddf: bad arguments");
    if (kind == 3 && !value_mode)
        for (int64_t i = 0; i < n; ++i)
            for (int c = 1; c < 3; ++c) {
                const float u = in[3 * i + c];
                if (!(u >= 0.0f && u < 1.0f) || u * 16777216.0f != (float)(uint32_t)(u * 16777216.0f))
                    return fail(ctx, IPT_E_INVALID, "ipt_ddf: table sampler needs u on the 2^-24 grid");
            }
    if (kind == 3) {
        const int rc = ensure_cos_tables(ctx, ctx->stream);
        if (rc) return rc;
    }
    if (!ctx->has_scene) return fail(ctx, IPT_E_INVALID, "ipt_ddf: no scene uploaded");
    const KParams& scene = ctx->scene.kp;
    if (kind == 1 && (params[3] < 0.0f || params[3] >= (float)scene.n_lights || params[3] != (float)(int)params[3]))
        return fail(ctx, IPT_E_INVALID, "ipt_ddf: light index out of range");
    hipSetDevice(ctx->device);
    const size_t in_w = 3, out_w = value_mode ? 1 : 3;
    DevBuf<float> dp, din, dout;
    HIPCHECK(ctx, hipMalloc(&dp.p, 8 * sizeof(float)));
    HIPCHECK(ctx, hipMalloc(&din.p, std::max<int64_t>(n, 1) * in_w * sizeof(float)));
    HIPCHECK(ctx, hipMalloc(&dout.p, std::max<int64_t>(n, 1) * out_w * sizeof(float)));
    float hp[8] = {0};
    for (int k = 0; k < (kind == 0 || kind == 3 ? 3 : (kind == 1 ? 4 : 6)); ++k) hp[k] = params[k];
    HIPCHECK(ctx, hipMemcpy(dp.p, hp, sizeof hp, hipMemcpyHostToDevice));
    HIPCHECK(ctx, hipMemcpy(din.p, in, n * in_w * sizeof(float), hipMemcpyHostToDevice));
    if (n > 0)
        hipLaunchKernelGGL(ddf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, value_mode, kind,
                           dp.p, scene.lights, scene.weights, scene.cdf, scene.n_lights, din.p, (long long)n, dout.p,
                           ctx->d_cos_a, ctx->d_cos_b);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHECK(ctx, hipMemcpy(out, dout.p, n * out_w * sizeof(float), hipMemcpyDeviceToHost));
    return IPT_OK;
}

int ipt_ddf_sample(ipt_ctx* ctx, int kind, const float* params, const float* u, int64_t n, float* dirs) {
    return ddf_call(ctx, 0, kind, params, u, n, dirs);
}

int ipt_ddf_value(ipt_ctx* ctx, int kind, const float* params, const float* dirs, int64_t n, float* values) {
    return ddf_call(ctx, 1, kind, params, dirs, n, values);
}

int ipt_math_selfcheck(ipt_ctx* ctx, int fn, uint64_t lo_bits, uint64_t hi_bits, uint64_t* mismatches,
                       uint32_t* first_bad) {
    if (!ctx || !mismatches || !first_bad || fn < 0 || fn > 22 || hi_bits > (1ull << (fn == 21 ? 46 : 32)) ||
        lo_bits > hi_bits)
        return IPT_E_INVALID;
    hipSetDevice(ctx->device);
    if (fn == 14 || fn == 15) {
        const int rc = ensure_frame_table(ctx, ctx->stream);
        if (rc) return rc;
    }
    DevBuf<unsigned long long> d_bad;
    DevBuf<unsigned int> d_first;
    HIPCHECK(ctx, hipMalloc(&d_bad.p, sizeof(unsigned long long)));
    HIPCHECK(ctx, hipMalloc(&d_first.p, sizeof(unsigned int)));
    HIPCHECK(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(unsigned long long), ctx->stream));
    HIPCHECK(ctx, hipMemsetAsync(d_first.p, 0xff, sizeof(unsigned int), ctx->stream));
    const unsigned long long n = hi_bits - lo_bits;
    if (n > 0 && fn == 21)
        hipLaunchKernelGGL(divcheck_kernel, dim3(ctx->n_cu * 64), dim3(256), 0, ctx->stream,
                           (unsigned long long)lo_bits, n, d_bad.p, d_first.p);
    else if (n > 0)
        hipLaunchKernelGGL(selfcheck_kernel, dim3(ctx->n_cu * 8), dim3(256), 0, ctx->stream, fn,
                           (unsigned long long)lo_bits, n, d_bad.p, d_first.p, ctx->d_frame_sc);
    HIPCHECK(ctx, hipGetLastError());
    unsigned long long hb = 0;
    unsigned int hf = 0;
    HIPCHECK(ctx, hipMemcpyAsync(&hb, d_bad.p, sizeof hb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipMemcpyAsync(&hf, d_first.p, sizeof hf, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    *mismatches = hb;
    *first_bad = hf;
    return IPT_OK;
}

}  // extern "C"
