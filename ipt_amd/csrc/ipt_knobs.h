// ipt_knobs.h — the path kernel's build-time parameters: the numeric values
// that sweeps still vary (the defaults are the measured best)
// and the experiment-build pair. The on/off switches that used to live here
// are retired: the source carries the measured winner of each alone
// (DESIGN.md §9 lists them with the result that decided each). A build that
// overrides a parameter must say so with -DIPT_AB_BUILD (A/B measurement
// builds, scripts/variants*.sh), so that a stray -D cannot slip into the
// product library unnoticed; no test builds or runs a non-default value.
#pragma once

#if !defined(IPT_AB_BUILD) &&                                                                    \
    (defined(IPT_BLOCK) || defined(IPT_RES_BLOCK) || defined(IPT_WAVES_PER_SIMD) ||              \
     defined(IPT_RES_WAVES) || defined(IPT_RESL_WAVES) || defined(IPT_GRID_BUDGET) ||            \
     defined(IPT_WALK_BUDGET) || defined(IPT_LWALK_BUDGET) || defined(IPT_BVH_LEAF) ||           \
     defined(IPT_LBVH_LEAF) || defined(IPT_GRID_CELLS_PER_SPHERE) || defined(IPT_C2_ONLY) ||     \
     defined(IPT_C2_LMODE))
#error "an ipt_knobs.h parameter is overridden: A/B builds must define IPT_AB_BUILD"
#endif

// ---- launch shape
#ifndef IPT_BLOCK
#define IPT_BLOCK 256  // threads per workgroup (4 waves; 128 / 512 measured -2 % / -7 %)
#endif
#ifndef IPT_RES_BLOCK
#define IPT_RES_BLOCK 64  // threads per workgroup of the sphere-list instances (C3: 64 / 128 / 256 -> 15.13 / 14.90 / 14.80)
#endif
#ifndef IPT_WAVES_PER_SIMD
#define IPT_WAVES_PER_SIMD 4  // __launch_bounds__ occupancy of the non-resumable instances
#endif
#ifndef IPT_RES_WAVES
#define IPT_RES_WAVES 4  // ... of the resumable sphere-list instances (C3: 3 -> 4 waves +12 %)
#endif
#ifndef IPT_RESL_WAVES
#define IPT_RESL_WAVES 3  // ... of the resumable many-light (light BVH) instances
#endif

// ---- walk budgets and acceleration-structure parameters
#ifndef IPT_GRID_BUDGET
#define IPT_GRID_BUDGET 8  // grid cells per lane per step of the resumable (wave) walk (6-32 measured)
#endif
#ifndef IPT_WALK_BUDGET
#define IPT_WALK_BUDGET 48  // sphere-BVH node visits per lane per step of a resumable walk
#endif
#ifndef IPT_LWALK_BUDGET
#define IPT_LWALK_BUDGET 16  // light-BVH nodes per lane per step of a resumable walk
#endif
#ifndef IPT_BVH_LEAF
#define IPT_BVH_LEAF 16  // sphere BVH: median split down to this many spheres (ipt_bvh.h)
#endif
#ifndef IPT_LBVH_LEAF
#define IPT_LBVH_LEAF 2  // light BVH leaf size
#endif
#ifndef IPT_GRID_CELLS_PER_SPHERE
#define IPT_GRID_CELLS_PER_SPHERE 1.5  // C3 sweep: 0.75-12, best 1.5
#endif

// ---- experiment builds: -DIPT_AB_BUILD -DIPT_C2_ONLY=1 instantiates the
// sample_scenes[0] kernel alone (seconds to compile); other scenes fail loudly
#ifndef IPT_C2_ONLY
#define IPT_C2_ONLY 0
#endif
#ifndef IPT_C2_LMODE
#define IPT_C2_LMODE kLightsOneA10
#endif
