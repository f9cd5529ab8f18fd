/* ipt_capi.h — C-ABI of the MI355X path-tracing inner loop (libipt_hip.so).
 *
 * This is the drop-in boundary for dimalit/ipt's hot path. The reference has
 * no FFI; its boundary is a set of C++ virtual interfaces called per ray
 * (reference src/tracer_interfaces.h:26-54) driven by
 *   render_sample(const Scene&, RenderPlane&, StatsNode*)   src/main.cpp:186-223
 *   ray_power_recursive(...)                                 src/main.cpp:98-184
 * Per-ray virtual calls cannot cross to a GPU, so this ABI works at frame
 * granularity: the caller flattens a Scene (camera + geometry + lights) into
 * the POD structs below once, then asks for whole sample passes.
 *
 * Conventions: plain pointers and sizes, no exceptions, every call returns
 * IPT_OK (0) or a negative IPT_E_* code, the message of the last failure is
 * available from ipt_last_error(). Calls are synchronous unless they take a
 * stream argument and say otherwise (ipt_render_device_async,
 * ipt_render_masked_device_async, ipt_adapt_device, ipt_display_device,
 * ipt_display_stats_device, ipt_smooth_device, ipt_pgm_device,
 * ipt_guides_device and ipt_denoise_device return once their work is queued). One context per HIP device; contexts are independent, a
 * single context is not reentrant. There is NO CPU fallback: without a usable
 * gfx950 device every rendering call fails with IPT_E_DEVICE.
 */
#ifndef IPT_CAPI_H
#define IPT_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPT_ABI_VERSION 7

enum {
    IPT_OK = 0,
    IPT_E_INVALID = -1,     /* bad argument / size / pointer */
    IPT_E_DEVICE = -2,      /* HIP runtime or device failure, no gfx950 device */
    IPT_E_UNSUPPORTED = -3, /* scene or parameter outside what the kernels implement */
    IPT_E_NOSCENE = -4,     /* ipt_render before ipt_upload_scene */
    IPT_E_OOM = -5
};

/* Geometry kinds (reference src/geometry/). */
enum {
    /* GeometrySphereInBox (GeometrySphereInBox.cpp:10-81): planes
       {+x,+y,+z,-x,-z} of the cube [-1,1]^3 (no -y wall) then a sphere of
       radius 0.5 at the origin. The sample_scenes[0] geometry. */
    IPT_GEOM_SPHERE_IN_BOX = 0,
    /* The same five box planes followed by N extra spheres scanned in order
       with FractalSpheres' acceptance rule (FractalSpheres.cpp:75-84); the
       10k-primitive stress configuration of BASELINE.json configs[2]. */
    IPT_GEOM_SPHERES_IN_BOX = 1,
    /* GeometryFloor (GeometryFloor.cpp:10-23): the z = -1 face of the cube
       ([-1,1]^2 through intersection_with_box_plane), unrotated CosineDdf.
       sample_scenes' make_scene_square_lit_by_square. */
    IPT_GEOM_FLOOR = 2,
    /* GeometryCorner (GeometryCorner.cpp:10-42): the x = -1, y = -1, z = -1
       faces, strict-< nearest in that order, RotateDdf(CosineDdf, normal).
       sample_scenes' make_scene_lit_corner. */
    IPT_GEOM_CORNER = 3,
    /* FractalSpheres (FractalSpheres.cpp:69-97): the sphere list alone, no
       walls, with the same acceptance rule as IPT_GEOM_SPHERES_IN_BOX.
       sample_scenes' make_scene_fractal. */
    IPT_GEOM_SPHERES = 4,
    /* GeometrySmallPt (GeometrySmallPt.cpp:11-58): the sphere list (smallpt's
       room: pass its 7 spheres) intersected in double precision
       (Sphere::intersect, eps 1e-4), strict-< nearest, normal flipped for
       radius >= 100. sample_scenes' make_scene_smallpt. */
    IPT_GEOM_SMALLPT = 5
};

/* Light kinds (reference src/lighting/lighting.h). Round lights use the
   ipt_area_light record with position = centre and x_axis[0] = radius
   (y_axis unused): SphereLight(centre, radius, power) (lighting.h:44-54),
   PointLight(position, virtual_radius, power) (radius unused, lighting.h:
   31-42), InvertedSphereLight(centre, radius, power) (addOuterLight,
   lighting.h:57-72). */
enum {
    IPT_LIGHT_AREA_DIAMOND = 0,
    IPT_LIGHT_AREA_TRIANGLE = 1,
    IPT_LIGHT_SPHERE = 2,
    IPT_LIGHT_POINT = 3,
    IPT_LIGHT_OUTER_SPHERE = 4
};

/* AreaLight constructor arguments (lighting.cpp:79-90); derived fields
   (area, normal, inverse_matrix, surface power) are computed by
   ipt_upload_scene with the constructor's own float operation order. */
typedef struct ipt_area_light {
    float position[3]; /* Light::position, the corner */
    float x_axis[3];
    float y_axis[3];
    float power;
    int32_t type; /* IPT_LIGHT_AREA_* */
} ipt_area_light;

/* SimpleCamera public fields after construction (SimpleCamera.h:11-13). */
typedef struct ipt_camera {
    float position[3];
    float direction[3];
    float right[3];
    float up[3];
} ipt_camera;

typedef struct ipt_sphere {
    float center[3];
    float radius;
} ipt_sphere;

typedef struct ipt_scene {
    int32_t geometry_kind;     /* IPT_GEOM_* */
    int32_t n_lights;          /* CollectionLighting::lights, insertion order */
    const ipt_area_light* lights;
    int32_t n_spheres;         /* extra spheres for IPT_GEOM_SPHERES_IN_BOX */
    const ipt_sphere* spheres;
    ipt_camera camera;
} ipt_scene;

typedef struct ipt_params {
    int32_t width, height;  /* render plane size; render_sample hardcodes 640x640 */
    int32_t spp;            /* number of render_sample passes in this call */
    int32_t spp_offset;     /* absolute index of the first pass (RNG counter) */
    int32_t n_rays;         /* branching factor of the root node (main.cpp:94), 0..65535
                               (above 255: at most 8 suspended levels, i.e. depth_max <= 9
                               once n_rays >= 512, and at most 65529 spheres) */
    int32_t depth_max;      /* main.cpp:95 */
    uint64_t seed;          /* Philox key */
    /* Destination-row sharding across devices: rows are cut into tiles of
       tile_rows rows, tile t belongs to shard t % n_shards. n_shards <= 1 or
       tile_rows <= 0 means this call owns the whole frame. */
    int32_t tile_rows;
    int32_t n_shards;
    int32_t shard_id;
    uint32_t flags;         /* IPT_FLAG_* */
} ipt_params;

enum {
    IPT_FLAG_COUNTERS = 1u, /* accumulate ipt_counters during the call */
    /* ABI 7: the render plane is the Gui's (gui.cpp:165-182), the plane the
       reference program renders into, displays and saves (main.cpp:250-289),
       instead of GridRenderPlane. Gui::addRay maps a sample to
         ix = min(size_t(x*W), W-1)   iy = min(size_t(H - y*H), H-1)
       (its 640 and 639 generalised to W, H and W-1, H-1): a plain vertical
       flip, source row s lands in row H-1-s, where GridRenderPlane::addRay's
       size_t(H - y*H - 1) folds source rows H-2 and H-1 into row 0. The
       running mean (gui.cpp:174-178) is addRay's, operation for operation.
       With the flag, ipt_render, ipt_render_device, ipt_render_device_async,
       ipt_render_values (codes relative to the nominal destination
       (ix, H-1-iy)), ipt_shard_plan and ipt_counters.drifted use this
       mapping; everything else of the ipt_image contract holds as written
       (preloaded planes, optional sums and pixel_max, the uint32 counter
       limit -- one sample per pixel and pass plus those that drift in --
       and accumulation across calls with increasing spp_offset). Which kind
       of plane an image holds is the caller's business: calls with and
       without the flag into one image mix the two mappings. Without the flag
       nothing changes. */
    IPT_FLAG_GUI_PLANE = 2u,
    /* ABI 7 addition: the estimator is ray_power_preview (main.cpp:55-92)
       instead of ray_power_recursive -- the frame a viewer shows while the
       camera moves. Everything else of render_sample (main.cpp:189-216) is
       unchanged: the two jitter draws (draws 0 and 1 of the same Philox
       stream), the camera ray, the clamp value >= 0 ? value : 0, the render
       plane's index math and drift codes. With si = Geometry::traceRay and li
       = Lighting::traceRayToLight of the camera ray (the nearest hits the full
       estimator computes at depth 0), a sample's value is
         1.0f  where li exists and (si is absent or
               length(si.position - origin) > length(li.position - origin)),
         0.0f  otherwise where si is absent,
         dot(si.normal, -direction) / length(direction), clamped, otherwise.
       n_rays and depth_max are not read (the reference's parameters are
       unnamed): any values are accepted and give the same frame; every other
       parameter is validated as without the flag. Composes with ipt_render,
       ipt_render_device, ipt_render_device_async, ipt_render_values,
       IPT_FLAG_GUI_PLANE, sharding, preloaded planes, sums / pixel_max,
       spp_offset, chunked launches and IPT_FLAG_COUNTERS (paths, traced_rays,
       surface_hits, light_hits, light_traces and drifted count the preview's
       events, the acceleration-structure counters what the kernel ran, the
       others stay 0). One fused kernel per launch, one thread per sample: no
       sampling table is read or built (a context that only renders previews
       never allocates them) and a sample takes 5 B of work buffer. Preview
       launches take no tail-overlap gate and stay ordered with queued
       full-estimator launches into the same image on the same stream. Which
       estimator's samples a plane holds is the caller's business. Without the
       flag nothing changes. */
    IPT_FLAG_PREVIEW = 4u,
    /* ABI 7 addition: unit compaction. The path kernel's work pool holds only
       the samples that are traced: masked samples (ipt_render_masked_device,
       ipt_render_adaptive), samples the render plane maps outside the frame
       and samples of other shards' rows are taken out before the path kernel
       starts, on the device (without the flag each of them is a unit the
       path kernel loads and drops).
       Every output is bit-identical to the same call without the flag:
       planes, m2, counters, ipt_render_values' values and codes. Honoured by
       every full-estimator launch (ipt_render, ipt_render_device[_async],
       ipt_render_masked_device[_async], ipt_render_values,
       ipt_render_adaptive); accepted and without effect with
       IPT_FLAG_PREVIEW, whose kernel has no pool; refused by
       ipt_replay_samples like every flag but IPT_FLAG_GUI_PLANE. A compacting
       launch runs three more passes over its samples (two before the path
       kernel, one after). Measured the pool shrinks with the
       active share and the launch time does not: even on contiguous masks,
       slower on scattered ones, so nothing sets the flag by itself. Without
       the flag nothing changes. */
    IPT_FLAG_COMPACT = 8u
};

/* Caller-owned GridRenderPlane state (GridRenderPlane.h:9-12), width*height
   row-major each. ipt_render ACCUMULATES into it with GridRenderPlane::addRay's
   running-mean update (GridRenderPlane.cpp:61-75), sample passes in order and
   each pass in render_sample's raster order, so repeated calls with increasing
   spp_offset continue the same image bit-for-bit. Zero-initialise before the
   first call. `sums` (sequential per-pixel sum in the same order) and
   `pixel_max` (per-pixel running maximum; GridRenderPlane::max_value is its
   maximum over the frame) may be NULL.
   A plane that is not zero may be passed in (a saved render, another
   renderer's plane): any counters, and pixels, sums and pixel_max of any
   value, infinities and NaNs included, are continued exactly as addRay would.
   The one limit: a counter must stay below 0xffffffff after the call's
   samples (one per pixel and pass, two in row 0, plus those that drift in
   from its neighbours). The reference counts in size_t where this plane
   counts in uint32_t, so from 0xffffffff on the next mean divides by
   (float)0 here and by 2^32 there. */
typedef struct ipt_image {
    float* pixels;
    uint32_t* counters;
    float* sums;
    float* pixel_max;
} ipt_image;

/* Event counters (SURVEY.md Appendix C vocabulary), summed over the call. */
typedef struct ipt_counters {
    uint64_t paths;           /* root ray_power calls */
    uint64_t traced_rays;     /* Geometry::traceRay calls */
    uint64_t surface_hits;    /* Geometry::traceRay calls that hit */
    uint64_t light_hits;      /* Lighting::traceRayToLight calls that hit */
    uint64_t expanded_nodes;  /* distributionInPoint calls (surface nodes) */
    uint64_t iterations;      /* UnionDdf::sample calls */
    uint64_t light_samples;   /* iterations that sampled a light component */
    uint64_t skipped;         /* iterations that returned vec3() */
    uint64_t sphere_frames;   /* RotateDdf builds at non-wall normals */
    uint64_t light_traces;    /* AreaLight::traceRay calls */
    uint64_t drifted;         /* samples the render plane maps off their nominal pixel */
    uint64_t bvh_nodes;       /* sphere-BVH nodes visited (IPT_GEOM_SPHERES_IN_BOX) */
    uint64_t sphere_tests;    /* intersection_with_sphere evaluations on the sphere list */
    uint64_t light_nodes;     /* light-BVH nodes visited (many-light scenes) */
    uint64_t light_tests;     /* AreaLight::traceRay evaluations actually run */
} ipt_counters;

typedef struct ipt_ctx ipt_ctx;

int ipt_abi_version(void);
const char* ipt_last_error(ipt_ctx* ctx); /* ctx may be NULL (creation errors) */

/* A context owns its stream and device buffers. The first render allocates its
 * exact sampling tables once: CosineDdf 192 MiB and, for sphere-in-box scenes,
 * the RotateDdf frame-angle table 1 GiB (freed by ipt_destroy); a render with
 * IPT_FLAG_PREVIEW reads neither and does not allocate them. Work buffers
 * grow to the largest render: 37 B per sample (radiance, drift code, raygen
 * record; 5 B for a preview sample, which has no record; 45 B with
 * IPT_FLAG_COMPACT, whose two buffers a context allocates on its first such
 * launch) in equal chunks of at most 2^29 samples (18.5 GiB) and at most 3/4
 * of the device memory free at the call (plus the context's own work
 * buffers), so a context's footprint is <= ~20 GiB and contexts sharing a
 * device get smaller chunks rather than IPT_E_OOM; a call renders all its
 * passes in as few path-kernel launches as that allows (each launch ends in
 * a tail where lanes have run out of paths, so batch passes per call).
 * Environment read here (diagnostics): IPT_LNODES_LDS=0 keeps the light BVH in
 * global memory, IPT_LIGHT_GRID=0 disables the light-lattice lookup (the light
 * BVH is used instead), IPT_LATTICE_LDS=0 keeps the lattice lights' records
 * in global memory (256-thread workgroups instead of one 1024-thread
 * workgroup per CU), IPT_BOX_GENERIC=1 launches the box scenes' generic
 * path-kernel instance (the box planes' range form for origins beyond 2^39)
 * whatever the scene's range, IPT_BLOCKS_PER_CU caps the path kernel's
 * residency. */
int ipt_create(int hip_device, ipt_ctx** out);
void ipt_destroy(ipt_ctx* ctx);

/* Copies the scene (caller keeps ownership of its arrays). Transactional: on
   any failure (IPT_E_OOM, IPT_E_DEVICE, ...) the context is left with NO
   scene, so a later render returns IPT_E_NOSCENE instead of rendering a
   half-uploaded one; upload again to recover. */
int ipt_upload_scene(ipt_ctx* ctx, const ipt_scene* scene);

/* Host buffers (the caller's GridRenderPlane state): renders p->spp passes
   into them. Device-resident: the context keeps the rows this call
   accumulates -- every row, or with p->n_shards > 1 the shard's owned tiles
   (ipt_shard_plan) -- on its device across calls, uploads only the owned rows
   whose host bytes changed since it last returned them (none in a
   progressive loop that leaves the plane alone between calls) and downloads
   only the owned rows: 16 B per owned pixel per call with sums and per-pixel
   max, 8 B without. Rows it does not own are neither read nor written, so the
   contexts of a multi-device render can share one host plane (one thread per
   context). Results are identical to copying the whole image each way. */
int ipt_render(ipt_ctx* ctx, const ipt_params* p, ipt_image* host_img);
/* Bytes the last ipt_render moved host -> device and device -> host. */
int ipt_transfer_bytes(ipt_ctx* ctx, uint64_t* host_to_device, uint64_t* device_to_host);

/* Device buffers (hipMalloc'd or torch CUDA tensors). The GridRenderPlane
   replays run on `hip_stream` (NULL = the context's own stream) after the work
   already queued there, in call order; the per-sample work (raygen + path
   kernel) runs on the context's two work-slot streams, consecutive launches
   alternating, so a launch fills the CUs its predecessor's tail leaves idle.
   Synchronous: the call returns when the image is complete (it waits for the
   path and accumulate kernels of every chunk and of every call queued before
   it; ipt_last_kernel_ms then holds their times). */
int ipt_render_device(ipt_ctx* ctx, const ipt_params* p, ipt_image* dev_img, void* hip_stream);

/* The same, returning once the launches are queued (the progressive loop of
   main.cpp:256-285 without a host wait per pass): the image is complete when
   `hip_stream` reaches the point after the call, or after ipt_render_wait.
   NULL is NOT the HIP null stream here but the context's own non-blocking
   stream, which the caller's kernels are not ordered with: a caller that
   passes NULL (torch's default-stream handle is 0) must call ipt_render_wait
   before reading the image. The image buffers must stay valid until then.
   Calls into the same image on the same stream accumulate exactly as
   sequential synchronous calls (bit-identical). ipt_upload_scene, the counter
   calls and ipt_destroy wait for queued work first.
   Consecutive launches (the chunks of one call, or queued calls) start in
   their predecessor's tail: a launch's stream waits (hipStreamWaitValue64) for
   the predecessor's work pool to drain. Under a tool that serialises
   dispatches for counter collection or thread trace (rocprofv3 --pmc / --att,
   detected at ipt_create from ROCPROF_COUNTER_COLLECTION /
   ROCPROF_ADVANCED_THREAD_TRACE), or with IPT_NO_TAIL_OVERLAP=1, a launch
   waits for its predecessor's end instead (same images). */
int ipt_render_device_async(ipt_ctx* ctx, const ipt_params* p, ipt_image* dev_img, void* hip_stream);
/* ---- adaptive sampling (ABI 7 additions) ---------------------------------------
   Masked renders, a second-moment plane and the kernel that turns both into
   the next mask, so that a progressive loop stops spending paths where the
   picture has converged (entry points and one struct added; no layout change).
   Without a mask and without an m2 plane every launch is
   ipt_render_device_async's.

   ipt_render_masked_device_async: ipt_render_device_async with
     dev_mask  [H][W] bytes, may be NULL (all active). Indexed by a sample's
               NOMINAL destination pixel (ix, yn), yn = max(H-2-iy, 0), or
               H-1-iy with IPT_FLAG_GUI_PLANE; under the Grid map mask[0][ix]
               therefore governs source rows H-2 and H-1 alike. Byte 0: the
               source sample is not traced (value 0, code 0xfe, no drift flag,
               counted neither in ipt_counters.paths nor .drifted). Any other
               byte: the sample is exactly the unmasked render's -- the pass
               index stays spp_offset + s whatever the mask. A traced sample
               that drifts is added where it lands, whatever the mask says
               there, as addRay would. Always the whole frame, also with
               n_shards > 1.
     dev_m2    [H][W] floats, may be NULL: the caller-owned second-moment
               plane, zero-initialised together with the image. For every
               sample v the replay adds to a pixel, in the replay's order, in
               f32 and with no contraction:
                 p_old = pixel;  addRay (unchanged);
                 m2 += (v - p_old) * (v - p_new)      (sub, sub, mul, add)
   The path kernel is untouched: a masked sample is a work unit that raygen
   marks invalid and the path kernel drops at its refill; nothing is compacted.
   Ordering: raygen reads the mask, caller memory, so before its first launch
   on each work-slot stream the call makes that stream wait for `hip_stream`
   as it stands at the call; the mask may be overwritten by work queued on
   `hip_stream` after the call. A masked call thereby gives up the tail overlap
   with what is queued before it on that stream (its launches start after it,
   not in its predecessor's tail); calls without a mask take no new wait.
   Composes with IPT_FLAG_GUI_PLANE, IPT_FLAG_PREVIEW, IPT_FLAG_COUNTERS,
   sharding, preloaded planes, sums / pixel_max NULL or not, chunked launches
   and queued mixes with unmasked calls. Validation is ipt_render_device_async's,
   plus: the mask or m2 sharing a byte with an image buffer or with each
   other: IPT_E_INVALID, before anything is launched. */
int ipt_render_masked_device_async(ipt_ctx* ctx, const ipt_params* p, ipt_image* dev_img,
                                   const uint8_t* dev_mask /* [H][W], may be NULL */,
                                   float* dev_m2 /* [H][W], may be NULL */, void* hip_stream);
/* The same, synchronous (as ipt_render_device). */
int ipt_render_masked_device(ipt_ctx* ctx, const ipt_params* p, ipt_image* dev_img, const uint8_t* dev_mask,
                             float* dev_m2, void* hip_stream);

/* ipt_adapt_device: the next mask. Per pixel d, in f32, operation for operation:
     c = counters[d]
     if (c < min_count)  active, class "starved" (counted in active as well)
     else nf = (float)c;  e2 = m2[d] / (nf * (nf - 1.0f));
          thr = rel_tol * fabsf(pixels[d]) + abs_tol;  t2 = thr * thr;
          active = e2 > t2;     a NaN on either side: inactive, class "nan"
     mask[d] = active ? 1 : 0
   e2 is the squared standard error of the mean. Pixels without a nominal
   source -- under the Grid map with H >= 2, row H-1 -- get mask 0 and are
   counted in no class (a loop that ends on "no active pixel" would otherwise
   never end); with IPT_FLAG_GUI_PLANE in `flags` there is no such row.
   dev_stats (4 uint32, may be NULL) = {active, starved, nan, 0}: integer sums,
   deterministic; the call zeroes them itself, in stream order.
   Stream and wait rules are ipt_display_device's: queued on `hip_stream` (NULL
   = the context's stream), no value crosses to the host, a call on another
   stream waits on the previous display / adapt call's event, ipt_render_wait,
   ipt_upload_scene and ipt_destroy wait for it. No scratch.
   Errors, all raised before a buffer is written: a NULL that is not optional,
   a non-positive size, min_count < 2, a negative or NaN tolerance, an output
   overlapping an input or the other output: IPT_E_INVALID; flags other than
   IPT_FLAG_GUI_PLANE or more than 2^31 pixels: IPT_E_UNSUPPORTED. */
typedef struct ipt_adapt_params {
    int32_t width, height;
    uint32_t min_count; /* >= 2: pixels with fewer samples stay active */
    float rel_tol, abs_tol;
    uint32_t flags;     /* 0 or IPT_FLAG_GUI_PLANE: the plane's row map */
} ipt_adapt_params;
int ipt_adapt_device(ipt_ctx* ctx, const ipt_adapt_params* ap, const float* dev_pixels,
                     const uint32_t* dev_counters, const float* dev_m2, uint8_t* dev_mask,
                     uint32_t* dev_stats /* 4, may be NULL */, void* hip_stream);

/* The loop on host buffers, synchronous, whole frame: renders up to p->spp
   passes (from p->spp_offset) in rounds of round_spp, round 0 unmasked, each
   round followed by ipt_adapt_device; reads the 16 B of stats after each round
   and stops when active == 0 or the passes are used up. host_img is continued
   as ipt_render continues it (zero-initialise before the first call); host_m2
   (may be NULL: zeros in, not returned) likewise; host_mask (may be NULL) gets
   the last mask. stats = {active, starved, nan} of the last round and, in
   stats[3], the passes used. ap's size and IPT_FLAG_GUI_PLANE must be p's:
   IPT_E_INVALID otherwise, as for a NULL ap / host_img / stats or round_spp
   < 1. p->n_shards > 1: IPT_E_UNSUPPORTED -- multi-GPU adaptive rendering
   (a mask per shard, agreed between devices) is out of scope here; a sharded
   caller drives ipt_render_masked_device_async and ipt_adapt_device itself. */
int ipt_render_adaptive(ipt_ctx* ctx, const ipt_params* p, const ipt_adapt_params* ap, int32_t round_spp,
                        ipt_image* host_img, float* host_m2, uint8_t* host_mask, uint32_t* stats);

/* Waits for every queued render; ipt_last_kernel_ms then holds the times of
   the launches since the previous wait (a synchronous render call waits). */
int ipt_render_wait(ipt_ctx* ctx);

/* Per-sample radiance, for bit-exact verification: values[s][iy][ix] is the
   clamped root ray_power of pass p->spp_offset+s at source pixel (ix,iy)
   (main.cpp:211-214) and codes[s][iy][ix] the GridRenderPlane drift code
   (bits 0-1: dx+1, bits 2-3: dy+1 relative to the nominal destination
   (ix, max(H-2-iy,0)), or (ix, H-1-iy) with IPT_FLAG_GUI_PLANE; 0x05 =
   nominal). Host buffers of spp*width*height. */
int ipt_render_values(ipt_ctx* ctx, const ipt_params* p, float* values, uint8_t* codes);

/* The preview estimator's samples with their first hits (ABI 7 addition): the
   verification surface of IPT_FLAG_PREVIEW and an AOV output (hit class,
   position, normal). The preview is implied whether or not the flag is set.
   Host buffers of spp*width*height samples; values and codes as
   ipt_render_values returns them with the flag. kinds and hits may be NULL.
   kinds[s][iy][ix]: bits 0-1 the outcome (0 miss, 1 surface, 2 light), bit 2
   set if si exists, bit 3 set if li exists; 0xff for a sample that was not
   traced (code 0xfe / 0xff).
   hits[s][iy][ix][6]: outcome 1: si.position, si.normal; outcome 2:
   li.position and a zero normal; miss or untraced: zeros. */
int ipt_preview_values(ipt_ctx* ctx, const ipt_params* p, float* values, uint8_t* codes,
                       uint8_t* kinds, float* hits);

/* Host-only (no device needed): the tile plan of a sharded render.
   owned_rows[H] = 1 for destination rows this shard accumulates;
   cand_rows[*n_cand] = source rows whose samples it traces (the nominal
   sources of its rows +-1 for drift, under GridRenderPlane's row map or, with
   IPT_FLAG_GUI_PLANE, the Gui's). Arrays sized H. */
int ipt_shard_plan(const ipt_params* p, uint8_t* owned_rows, int32_t* cand_rows, int32_t* n_cand);

int ipt_get_counters(ipt_ctx* ctx, ipt_counters* out);
int ipt_reset_counters(ipt_ctx* ctx);
/* Phase profile of the path kernel: out[2q] = wave executions of phase q,
 * out[2q+1] = active lanes summed over them (words 0..23, -DIPT_PROF=1
 * builds); out[24+s] = wave-cycles in step segment s (words 24..35,
 * -DIPT_STAMP=1 builds; scripts/prof_phases.sh). Zeros in product builds.
 * Cleared by ipt_reset_counters. */
int ipt_get_profile(ipt_ctx* ctx, uint64_t* out, int n);

/* Timing of the kernels of the render calls completed by the most recent wait
   (a synchronous render, or ipt_render_wait after asynchronous ones): ms from
   HIP events, summed over their launches: [0] = the path's per-sample work,
   raygen_kernel + path_kernel (raygen ~0.2 % of it), each launch counted from
   its start or from its predecessor's end, whichever is later (overlapped
   launches sum to their span); [1] = accumulate kernels. */
int ipt_last_kernel_ms(ipt_ctx* ctx, float* path_ms, float* accumulate_ms);

/* ABI 7 addition: work units of the full-estimator launches completed by the
   most recent wait (ipt_last_kernel_ms's scope; preview and replay launches
   have no pool and are not counted), summed over the launches:
   out[0] = the launches' dense units (passes x candidate rows x width);
   out[1] = the units their pools handed out: total_units - start, where a
            compacting launch's pool starts at the compact range's begin
            rounded down to 256 and any other launch's at 0;
   out[2] = the units that were traced (n_active) for a compacting launch,
            the dense units for any other.
   Without IPT_FLAG_COMPACT the three are equal. A wait that completed no
   such launch leaves the previous values. */
int ipt_last_units(ipt_ctx* ctx, uint64_t out[3]);

/* ABI 7 addition, a test probe: which path_kernel instance the context's most
   recent path-kernel launch took, as the kernel's template arguments:
   out = {MAXSUSP, COUNT, LMODE, GEOM, BOXIN, FIXED} (MAXSUSP 4 or 8 suspended
   levels; COUNT 1 with IPT_FLAG_COUNTERS; LMODE 1 one light, 2 lights in LDS,
   3 light BVH, 4 any light type, 5/6 one axis-aligned light A10/A01, 7/8
   lattice A10/A01 with records in global memory, 9/10 with records in LDS;
   GEOM an IPT_GEOM_* value; BOXIN 1 for the box planes' in-range form; FIXED
   0, -1 for n_rays a power of two, 4 for the fixed four-level tree). Recorded
   at the launch, so valid as soon as a render call has returned.
   IPT_E_INVALID if the context has launched no path kernel (a new context, or
   one that made preview and replay calls only). */
int ipt_last_instance(ipt_ctx* ctx, int32_t out[6]);

/* ABI 7 addition, a test probe: the compaction plan of the call's FIRST
   launch (p as for a render, IPT_FLAG_COMPACT implied; dev_mask [H][W] on the
   device as for ipt_render_masked_device, or NULL). Runs the launch's
   classification, scan, scatter and pool preset, no path kernel, and touches
   no image; synchronous. *n_active and *start as above; host_src[0 ..
   n_active) = the dense units of the compact range, in its order (ascending).
   IPT_E_INVALID if cap < n_active (the two counts are still returned);
   IPT_E_UNSUPPORTED with IPT_FLAG_PREVIEW. Needs an uploaded scene. */
int ipt_compact_plan(ipt_ctx* ctx, const ipt_params* p, const uint8_t* dev_mask, uint32_t* host_src, uint64_t cap,
                     uint64_t* n_active, uint64_t* start);

/* ---- image post-process on the GPU, bit-exact --------
   ipt_smooth: GridRenderPlane::smooth(side) (in_place = 1: pixels are
   replaced, as the reference's in-place filter leaves them) or
   computeSmoothedMax(side) (in_place = 0: pixels untouched); *max_value gets
   the reference's max_value (GridRenderPlane.cpp:10-59). Host buffers
   (width*height floats, row-major). side 1 is undefined behaviour in the
   reference (its size_t loop runs past row 0): IPT_E_UNSUPPORTED.
   ipt_glare: Gui's glare bloom (gui.cpp:28-52), out = glare(in, cutoff);
   images up to 4096 x 4096. */
int ipt_smooth(ipt_ctx* ctx, float* pixels, int width, int height, int side, int in_place, float* max_value);
int ipt_glare(ipt_ctx* ctx, const float* in, float* out, int width, int height, float cutoff);

/* ---- display pipeline on the GPU (ABI 6), bit-exact -------------------------
   Gui::updateDisplay / Gui::save (gui.cpp:11-16, 54-70) for a plane that stays
   on the device: glare(image, cutoff) -> normalize (max, /max, powf(., 1/2.2),
   cut to [0,1]) -> normalize(0,255) and the 8-bit cast. width*height row-major
   buffers:
     processed  glare(pixels, glare_cutoff) exactly as ipt_glare computes it, or
                a copy of pixels when glare_cutoff == 0
     tone       processed / mx, powf(., (float)(1.0f/2.2f)), cut to [0,1] (NaN
                passes); mx is the reference's sequential max fold from element
                0: NaN if and only if element 0 is NaN, otherwise the first
                occurrence of the maximum of the non-NaN elements. NaN results
                are the x86 host's (a NaN operand quieted; 0/0, inf/inf and
                powf of a negative: 0xffc00000)
     gray8      m, M = the same folds (min, max) over tone; m == M gives 0;
                otherwise (uint8_t)((v - m) / (M - m) * 255.0f + 0.0f), NaN
                gives 0 (the host's cast of NaN is undefined and yields 0 on
                x86; both sides state 0)
   Errors: a NULL pointer that is not optional, a non-positive size or a
   negative / NaN cutoff: IPT_E_INVALID; glare on an image wider or taller
   than 4096 (ipt_glare's limit), more than 2^31 pixels, an infinite cutoff or
   flags != 0: IPT_E_UNSUPPORTED. */
typedef struct ipt_display_params {
    int32_t width, height;
    float glare_cutoff; /* > 0: Gui::updateDisplay's glare(image, cutoff) first;
                           0: no glare (Gui::finalize / Gui::save) */
    uint32_t flags;     /* 0 */
} ipt_display_params;

/* Device buffers (hipMalloc'd or torch CUDA tensors), any alignment a float /
   byte array may have. Stream semantics of ipt_render_device_async: the
   kernels run on `hip_stream` (NULL = the context's own stream) after the work
   already queued there, the call returns once they are queued, the outputs
   are complete when the stream reaches that point, and ipt_render_wait,
   ipt_upload_scene and ipt_destroy wait for them. No value crosses to the
   host inside the call: the bright-pixel count, mx, m and M stay in device
   memory where the next kernel reads them. dev_processed and dev_tone may be
   NULL (the context's scratch is used). The scratch (bright list of 16 B per
   pixel when glare is on, block counts, the scalars, 4 B per pixel for each
   output not passed) belongs to the context, grows to the largest image seen
   and is freed by ipt_destroy: a second call at the same size allocates,
   frees and synchronises nothing. The input and output buffers must stay
   valid until the stream has passed the call; dev_pixels is only read and
   may not overlap an output. */
int ipt_display_device(ipt_ctx* ctx, const ipt_display_params* p, const float* dev_pixels, float* dev_processed,
                       float* dev_tone, uint8_t* dev_gray8, void* hip_stream);
/* Host buffers: the same kernels, synchronous (uploads pixels, downloads the
   outputs asked for; processed and tone may be NULL). */
int ipt_display(ipt_ctx* ctx, const ipt_display_params* p, const float* pixels, float* processed, float* tone,
                uint8_t* gray8);
/* ---- display statistics on the GPU (ABI 7 additions), bit-exact ---------------
   The two parts of Gui::updateDisplay that decide the exposure, beside the
   pipeline above (entry points and one struct added; no layout changes, as
   ABI 4 added entry points to ABI 3). With A = processed (the glare output,
   or the pixels when glare_cutoff == 0):
     stats[0]  mx, the max fold of ipt_display_device
     stats[1]  mx / 100000.0f (IEEE f32, subnormals kept; a NaN mx quieted)
     stats[2]  the white point (below)
     stats[3]  0
     hist[b]   CImg get_histogram(hist_buckets, stats[1], mx) of A (gui.cpp:
               83-88, CImg.h:33484-33495), in double as CImg computes it:
               vmin, vmax = the two bounds, swapped unless stats[1] < mx; an
               element counts iff vmin <= val <= vmax; its bucket is nb-1 when
               val == vmax, otherwise (unsigned)((val - vmin) * nb / (vmax -
               vmin)). So: an all-zero image counts every pixel in the last
               bucket, a NaN mx counts nothing, an infinite mx counts the
               infinities only, a negative mx swaps the bounds. uint32 counts.
     white     white_rank < 0: mx (normalize() as the reference builds it).
               white_rank >= width*height: mx (CImg kth_smallest: max()).
               Otherwise CImg kth_smallest(white_rank) of A (gui.cpp:13), the
               element at that 0-based index of the ascending order. Two points
               CImg leaves to its algorithm are stated: -0 orders before +0,
               and NaNs of either sign order after +inf; a rank that lands
               among them yields 0x7fc00000.
     tone      cut(powf(A / white, (float)(1.0f/2.2f)), 0, 1), the pipeline's
               arithmetic with white in place of mx; gray8 from tone as above.
   With white_rank < 0, processed, tone and gray8 equal ipt_display_device's
   bit for bit. dev_processed, dev_tone, dev_gray8, dev_hist and dev_stats may
   each be NULL, and a stage nobody asked for is not run (a histogram-only call
   evaluates no powf). Errors: ipt_display_device's rules (no output is
   mandatory), and hist_buckets outside 0..4096 or hist_buckets > 0 with a NULL
   dev_hist: IPT_E_INVALID; all refused before a buffer is touched. */
typedef struct ipt_display_stats_params {
    int32_t width, height;
    float glare_cutoff;   /* exactly as ipt_display_params */
    int32_t hist_buckets; /* 0: no histogram; 1..4096; the Gui's is 400 */
    int64_t white_rank;   /* < 0: white = the max fold; k >= 0: white = kth_smallest(k) */
    uint32_t flags;       /* 0 */
} ipt_display_stats_params;

/* Device buffers; stream and scratch rules are ipt_display_device's: the work
   runs on `hip_stream` (NULL = the context's stream) and the call returns once
   it is queued; no value crosses to the host inside the call (mx, the radix
   prefixes, the remaining rank and the white point stay in device memory,
   where the next kernel reads them); the scratch (ipt_display_device's plus
   24 KiB of digit counts) belongs to the context and grows to the largest
   request, so a repeated call at the same size allocates, frees and
   synchronises nothing; a call on another stream waits on the previous call's
   event; ipt_render_wait, ipt_upload_scene and ipt_destroy wait for queued
   calls. dev_hist holds hist_buckets counts, dev_stats 4 floats. */
int ipt_display_stats_device(ipt_ctx* ctx, const ipt_display_stats_params* p, const float* dev_pixels,
                             float* dev_processed, float* dev_tone, uint8_t* dev_gray8, uint32_t* dev_hist,
                             float* dev_stats, void* hip_stream);
/* Host buffers: the same kernels, synchronous. */
int ipt_display_stats(ipt_ctx* ctx, const ipt_display_stats_params* p, const float* pixels, float* processed,
                      float* tone, uint8_t* gray8, uint32_t* hist, float* stats);
/* Probes of the display chain's powf (ipt_math.h powf_, glibc 2.35's
   __powf_fma restated): out[i] = powf(x[i], y), host buffers; y finite, > 0
   and not an integer (IPT_E_UNSUPPORTED otherwise). ipt_powf_host is the
   library's host build of the code the kernels run. */
int ipt_powf_host(const float* x, float y, float* out, int64_t n);
int ipt_powf_device(ipt_ctx* ctx, const float* x, float y, float* out, int64_t n);

/* ---- PGM output on the GPU (ABI 7 additions), bit-exact -------------------------
   The reference's written output (main.cpp:291-309) for a plane that stays on
   the device: GridRenderPlane::smooth(2) -> computeSmoothedMax(5) ->
   n_val(v, max_value, 500, 0.6f) -> result.pgm (entry points and one struct
   added; no layout changes).

   ipt_smooth_device: ipt_smooth on device buffers, in stream order.
     dev_out != NULL  GridRenderPlane::smooth(side): dev_out gets the filtered
                      plane (pixels with x < side-1 or y < side-1 keep their
                      input value). dev_out == dev_in is allowed (the context's
                      scratch holds the copy the filter reads).
     dev_out == NULL  computeSmoothedMax(side): no pixel is written.
     dev_max          1 float, may be NULL: the reference's max_value, the
                      running `accum > max` from 0 over the window means (a
                      NaN never wins, an all-negative plane gives +0).
   side 0 and a side larger than the image are valid: no pixel qualifies, the
   maximum is 0 and the pixels are unchanged (copied when out of place).
   Errors, all raised before a buffer is touched: a NULL ctx or dev_in, a
   non-positive size, a negative side, or buffers that overlap other than
   dev_out == dev_in: IPT_E_INVALID; side 1 (undefined behaviour in the
   reference), a side above 64 (a queued kernel is bounded at 64^2 adds per
   pixel; the reference uses 2 and 5) or more than 2^31 pixels:
   IPT_E_UNSUPPORTED. */
int ipt_smooth_device(ipt_ctx* ctx, const float* dev_in, float* dev_out /* NULL: computeSmoothedMax */, int width,
                      int height, int side, float* dev_max /* 1 float, may be NULL */, void* hip_stream);

/* ipt_pgm_device: the whole chain. width*height row-major buffers.
     smoothed  the pixels n_val reads: smooth(smooth_side) of dev_pixels, or a
               copy of them when smooth_side == 0
     max_value the one n_val divides by; the reference's sequence decides (the
               last stage that sets it wins), the first matching rule applies:
                 1. max_side >= 2: computeSmoothedMax(max_side) of `smoothed`
                 2. smooth_side >= 2: smooth's value
                 3. dev_pixel_max != NULL: its fold from 0 with `>`
                    (GridRenderPlane::max_value of an ipt_image's pixel_max)
                 4. otherwise p->max_value as given, any float
     gray8     ipt::n_val / main.cpp:225-235 per pixel, in f32:
                 adj = v * contrast / max_value   (two operations, IEEE
                       division, subnormals kept)
                 adj = contrast < adj ? contrast : adj;  adj = adj < 1 ? 1 : adj
                       (std::min / std::max exactly: a NaN adj stays)
                 fn = logf(adj) / logf(contrast);  fn = powf(fn, gamma)
                 n = (int)(256.0f * fn) clamped to 0..255; a NaN gives 0 (the
                       x86 conversion yields INT_MIN, then max(0, .))
               with glibc 2.35's logf and powf restated (ipt_math.h). E.g. with
               contrast 500, gamma 0.6: max_value 0 gives 255 for every v > 0
               and 0 for v <= 0 or NaN; an infinite or NaN max_value gives 0.
     stats     {max_value used, logf(contrast), 0, 0}
   dev_pixel_max, dev_smoothed, dev_gray8 and dev_stats may each be NULL, and a
   stage nobody asked for is not run. dev_pixels (and dev_pixel_max) are only
   read and may not overlap an output; outputs may not overlap each other.
   Errors, all raised before a buffer is touched: a NULL that is not optional,
   a non-positive size, a negative side or an overlap: IPT_E_INVALID; side 1, a
   side above 64, flags != 0, more than 2^31 pixels, contrast not finite or not
   > 1, gamma outside powf's domain here (finite, > 0, no integer):
   IPT_E_UNSUPPORTED. */
typedef struct ipt_pgm_params {
    int32_t width, height;
    int32_t smooth_side; /* 0: none; >= 2: GridRenderPlane::smooth(side) first (main.cpp: 2) */
    int32_t max_side;    /* 0: none; >= 2: computeSmoothedMax(side) of the (smoothed) pixels (main.cpp: 5) */
    float contrast;      /* main.cpp: 500 */
    float gamma;         /* main.cpp: 0.6f */
    float max_value;     /* used only by rule 4 */
    uint32_t flags;      /* 0 */
} ipt_pgm_params;

/* Device buffers, any alignment a float / byte array may have. Stream and
   scratch rules are ipt_display_device's (for both calls above): the work
   runs on `hip_stream` (NULL = the context's stream) and the call returns once
   it is queued; no value crosses to the host inside the call (the maxima,
   max_value and logf(contrast) stay in device memory, where the next kernel
   reads them); the scratch (32 B of scalars, 4 B per pixel when smooth runs
   without dev_smoothed or in place) belongs to the context and grows to the
   largest request, so a repeated call at the same size allocates, frees and
   synchronises nothing; a call on another stream waits on the previous call's
   event; ipt_render_wait, ipt_upload_scene and ipt_destroy wait for queued
   calls. */
int ipt_pgm_device(ipt_ctx* ctx, const ipt_pgm_params* p, const float* dev_pixels,
                   const float* dev_pixel_max /* may be NULL */, float* dev_smoothed /* may be NULL */,
                   uint8_t* dev_gray8 /* may be NULL */, float* dev_stats /* 4 floats, may be NULL */,
                   void* hip_stream);
/* Host buffers: the same kernels (and limits), synchronous. */
int ipt_pgm(ipt_ctx* ctx, const ipt_pgm_params* p, const float* pixels, const float* pixel_max, float* smoothed,
            uint8_t* gray8, float* stats);
/* Probes of the PGM chain's logf (ipt_math.h logf_, glibc 2.35's __logf_fma
   restated): out[i] = logf(x[i]) for x in [1, FLT_MAX], host buffers. Outside
   that domain (x < 1, negative, +inf, NaN) both return the quiet NaN
   0x7fc00000 by definition, so that host and device agree there too.
   ipt_logf_host is the library's host build of the code the kernels run. */
int ipt_logf_host(const float* x, float* out, int64_t n);
int ipt_logf_device(ipt_ctx* ctx, const float* x, float* out, int64_t n);

/* ---- denoising on the GPU (ABI 7 additions) --------------------------------------
   A variance-guided, geometry-aware a-trous filter between "render" and
   "display", for a plane that stays on the device: ipt_guides_device writes
   each pixel's first hit, ipt_denoise_device filters the plane with them and
   with the m2 plane ipt_render_masked_device keeps (entry points and two
   structs added; no layout change). The filter is not the reference's (its
   only spatial filter is smooth(side)); its definition is the one below, and
   the kernels compute it bit for bit.

   ipt_guides_device: dev_guides[yd][xd] = the first hit of ONE preview sample,
   pass p->spp_offset of ipt_preview_values (same Philox stream, jitter, kinds
   and hits), of the pixel's NOMINAL source, written at the nominal destination
   whatever the sample's drift code:
     Grid map:  yd <= H-2 takes source row H-2-yd; row H-1 has no nominal
                source (as in ipt_adapt_device): kind 0xff, zeros. H == 1: row
                0 takes source row 0.
     IPT_FLAG_GUI_PLANE: yd takes source row H-1-yd.
   kind is ipt_preview_values' kinds byte (0xff: the sample was not traced),
   pos = hits[0..2], normal = hits[3..5] (a light outcome: the light position
   and a zero normal; a miss: zeros), zero = 0.
   p->spp must be 1 (IPT_E_INVALID otherwise, as for a NULL dev_guides);
   n_rays and depth_max are not read; n_shards > 1 or a flag other than
   IPT_FLAG_GUI_PLANE and IPT_FLAG_PREVIEW: IPT_E_UNSUPPORTED. No plane is
   accumulated into. Stream and wait rules are ipt_display_device's: the record
   plane is complete when `hip_stream` (NULL = the context's stream) reaches
   the point after the call; ipt_render_wait, ipt_upload_scene and ipt_destroy
   wait for it. */
typedef struct ipt_guide { /* 32 B, one per destination pixel */
    float pos[3];
    uint32_t kind; /* ipt_preview_values' kinds byte, 0xff = no source */
    float normal[3];
    uint32_t zero;
} ipt_guide;
int ipt_guides_device(ipt_ctx* ctx, const ipt_params* p, ipt_guide* dev_guides /* [H][W] */, void* hip_stream);
/* Host buffer: the same kernels, synchronous. */
int ipt_guides(ipt_ctx* ctx, const ipt_params* p, ipt_guide* guides /* [H][W] */);

/* ipt_denoise_device. All f32, no contraction, IEEE division and square root,
   no exp / pow / log. max(a, 0) below is `a > 0 ? a : 0` (a NaN gives 0).
   Participation: pixel d takes part iff
     (guides[d].kind & 3) == 1   (a surface)
     c = counters[d] >= 2
     pixels[d] is finite
     var0 = m2[d] / (nf * (nf - 1.0f)) is finite,  nf = (float)c
   Every other pixel (light, miss, no source, starved, non-finite) is copied
   unchanged to dev_out, gets var_out = var0 if c >= 2, else 0, and is never
   read as a tap.
   Iteration k = 0 .. iterations-1, s = 1 << k, reads (col, var) of iteration
   k-1 (iteration 0: pixels and var0) and writes new ones for every
   participating centre p at (x, y):
     gs = gw = 0; for dy = -1..1, dx = -1..1 (dy outer), q = (x+dx, y+dy)
       inside the frame and participating:
         g = {1/4 centre, 1/8 edge, 1/16 corner};  gs += g * var_q;  gw += g
     gv = gs / gw                   (distance 1 whatever s)
     den = sigma_l * sqrtf(gv) + 0x1p-20f
     sw = sc = sv = 0; for dy = -2..2, dx = -2..2 (dy outer), q = (x + s*dx,
       y + s*dy) inside the frame and participating (the centre included):
         h  = hk[|dx|] * hk[|dy|],  hk = {3/8, 1/4, 1/16}
         wn = max((nx*nx' + ny*ny') + nz*nz', 0), then wn = wn * wn,
              normal_pow times          (n the centre's normal, n' the tap's)
         D  = P_q - P_p;  e = fabsf((nx*Dx + ny*Dy) + nz*Dz)
         t  = max(1.0f - e / sigma_z, 0);                    wz = t * t
         u  = max(1.0f - fabsf(col_q - col_p) / den, 0);     wl = u * u
         w  = h * ((wn * wz) * wl)
         sw += w;  sc += w * col_q;  sv += (w * w) * var_q
     sw == 0: col' = col_p, var' = var_p; otherwise col' = sc / sw,
     var' = sv / (sw * sw)
   dev_out gets the last iteration's col, dev_var_out (may be NULL) its var.
   Errors, all raised before a buffer is written: a NULL that is not optional,
   a non-positive size, iterations outside 1..6, normal_pow outside 0..7, a
   sigma that is not > 0 (NaN included): IPT_E_INVALID; an output sharing a
   byte with an input or with the other output: IPT_E_INVALID; more than 2^31
   pixels: IPT_E_UNSUPPORTED. The scratch (two planes of 32 B records) belongs
   to the context, is allocated on first use and grows to the largest frame
   seen. Stream and wait rules are ipt_display_device's: queued on `hip_stream`
   (NULL = the context's stream), no value crosses to the host, a call on
   another stream waits on the previous post-process call's event. */
typedef struct ipt_denoise_params {
    int32_t width, height;
    int32_t iterations; /* 1..6; iteration k uses tap step 1 << k */
    float sigma_l;      /* colour, in standard errors, > 0 */
    int32_t normal_pow; /* 0..7 squarings of max(dot, 0) */
    float sigma_z;      /* plane distance, world units, > 0 */
} ipt_denoise_params;
int ipt_denoise_device(ipt_ctx* ctx, const ipt_denoise_params* dp, const float* dev_pixels,
                       const uint32_t* dev_counters, const float* dev_m2, const ipt_guide* dev_guides,
                       float* dev_out, float* dev_var_out /* may be NULL */, void* hip_stream);
/* Host buffers: the same kernels, synchronous. */
int ipt_denoise(ipt_ctx* ctx, const ipt_denoise_params* dp, const float* pixels, const uint32_t* counters,
                const float* m2, const ipt_guide* guides, float* out, float* var_out /* may be NULL */);

/* A measuring probe: the kernel times, in ms from HIP events, of the passes of
   the context's last ipt_denoise_device call made with IPT_DENOISE_PROFILE=1
   in the environment (without it the call records nothing and this returns
   IPT_E_INVALID): ms[0] = the prepare pass, ms[1 + k] = iteration k, the rest
   0. Waits for that call. IPT_DENOISE_FORM=direct / tiled in the environment
   makes every iteration of a call run that tap-loop form (DESIGN.md
   "Denoising"; the results are the same bits). */
int ipt_denoise_pass_ms(ipt_ctx* ctx, float ms[7]);

/* ---- temporal reprojection on the GPU (ABI 7 additions) ---------------------------
   Carries an accumulated frame across a camera move: from the previous
   camera's planes and guide plane and the new camera's guide plane to the new
   frame's starting planes, which ipt_render_masked_device continues as any
   preloaded plane (entry points and one struct added; no layout change). Every
   surface of the reference is Lambertian: what ray_power_recursive returns at
   a surface hit does not depend on the incoming direction, so the history of a
   point that is still visible is valid data for the new frame and only has to
   be resampled to the new pixel grid. The definition is the one below, and the
   kernel computes it bit for bit.

   All f32 adds, multiplies and IEEE divisions, no contraction, no exp / pow /
   sqrt; every dot product is (x*x' + y*y') + z*z'; every comparison is written
   so that a NaN falls on the rejecting side. W = width, H = height. For each
   destination pixel d = (xd, yd) of the new frame, g = cur_guides[d], P =
   g.pos, n = g.normal:
   1. (g.kind & 3) != 1 or a component of P not finite: the outputs are
      (0, 0, 0), class "not_surface".
   2. Projection into prev_camera (SimpleCamera::sampleRay inverted; its
      direction need not have length 1):
        v = P - position
        a = v.right;  b = v.up;  c = v.direction;  dd = direction.direction
        t = c / dd                      !(t > 0): empty (0, 0, 0), "disoccluded"
        sx = (a / t + 0.5f) * (float)W;  fx = sx - 0.5f
        sy = (b / t + 0.5f) * (float)H;  fy = sy - 0.5f
        !(fx >= -1.0f && fx < (float)W) or the same of fy and H: empty,
        "disoccluded"  (a NaN or an infinity ends here, before any conversion)
        x0 = floorf(fx);  tx = fx - x0;  y0 = floorf(fy);  ty = fy - y0
   3. Four taps (j, i) in {0, 1}^2, j outer: source pixel (x0 + i, y0 + j),
      bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty). The tap's plane index q
      is the destination pixel whose nominal source that source pixel is
      (ipt_guides_device's map): source row r goes to row H-2-r for r <= H-2
      under the Grid map (row H-1 is no pixel's nominal source and is no tap;
      H == 1: row 0), to H-1-r with IPT_FLAG_GUI_PLANE; the column stays. A tap
      is used iff
        the source pixel is inside the frame and has such a q
        (prev_guides[q].kind & 3) == 1
        c_q = prev_counters[q] >= 2
        prev_pixels[q] is finite
        var_q = prev_m2[q] / (nf * (nf - 1.0f)) is finite,  nf = (float)c_q
        n.n_q >= normal_min                       (n_q = prev_guides[q].normal)
        fabsf(n.(P_q - P)) <= sigma_z             (P_q = prev_guides[q].pos)
      (binary: the resampling stays a plain interpolation), and then
        cc = min(c_q, max_count);  r = (float)c_q / (float)cc;  ve = var_q * r
        sw += bw;  sm += bw * prev_pixels[q];  sv += (bw * bw) * ve
        sc += bw * (float)cc
      (the history cap: a capped pixel's variance of the mean is that of cc
      samples, so that new samples outweigh a long history after a move).
   4. sw == 0: empty, "disoccluded". Otherwise
        mean = sm / sw;  var = sv / (sw * sw);  cf = sc / sw
        c' = (uint32)cf clamped to [2, max_count];  nf' = (float)c'
        out_pixels = mean;  out_counters = c';  out_m2 = var * (nf' * (nf' - 1.0f))
      class "reused". mean and out_m2 are produced as computed, with no
      test of their own: finite inputs that pass step 3 with an m2 near
      FLT_MAX can give out_m2 = +inf (var * (nf' * (nf' - 1.0f)) overflows
      where a tap with a small counter is blended with one that lifts c').
      The next ipt_adapt_device and ipt_reproject_device treat such a pixel
      as any pixel whose variance is not finite.
   5. dev_stats (4 uint32, may be NULL) = {reused, disoccluded, not_surface, 0}:
      integer sums, deterministic; the call zeroes them itself, in stream order.
   The three classes sum to W * H. Under the Grid map row H-1 of the new frame
   (no nominal source: its guide has kind 0xff) is "not_surface". `sums` and
   `pixel_max` are not produced: a caller that keeps them restarts them.
   The call always takes a whole frame (a sharded caller assembles its planes
   first, as for the denoiser). No scratch. Stream and wait rules are
   ipt_display_device's: queued on `hip_stream` (NULL = the context's stream),
   no value crosses to the host, a call on another stream waits on the
   previous post-process call's event.
   Errors, all raised before a byte is written: a NULL that is not optional, a
   non-positive size, sigma_z not > 0 (NaN included), a NaN normal_min,
   max_count outside 2 .. 1 << 24, an output sharing a byte with an input or
   with another output: IPT_E_INVALID; a flag other than IPT_FLAG_GUI_PLANE or
   more than 2^31 pixels: IPT_E_UNSUPPORTED. */
typedef struct ipt_reproject_params {
    int32_t width, height;
    uint32_t flags;         /* 0 or IPT_FLAG_GUI_PLANE: the row map of BOTH frames */
    ipt_camera prev_camera; /* the camera the previous planes and guides were taken with */
    float sigma_z;          /* plane distance, world units, > 0 (the denoiser's meaning) */
    float normal_min;       /* a tap's n.n' must be >= this; any value but NaN */
    uint32_t max_count;     /* history cap, 2 .. 1 << 24 */
} ipt_reproject_params;
int ipt_reproject_device(ipt_ctx* ctx, const ipt_reproject_params* rp, const float* dev_prev_pixels,
                         const uint32_t* dev_prev_counters, const float* dev_prev_m2,
                         const ipt_guide* dev_prev_guides, const ipt_guide* dev_cur_guides, float* dev_out_pixels,
                         uint32_t* dev_out_counters, float* dev_out_m2, uint32_t* dev_stats /* 4, may be NULL */,
                         void* hip_stream);
/* Host buffers: the same kernel, synchronous. */
int ipt_reproject(ipt_ctx* ctx, const ipt_reproject_params* rp, const float* prev_pixels,
                  const uint32_t* prev_counters, const float* prev_m2, const ipt_guide* prev_guides,
                  const ipt_guide* cur_guides, float* out_pixels, uint32_t* out_counters, float* out_m2,
                  uint32_t* stats /* 4, may be NULL */);

/* ---- the path's DDF samplers, exactly as the kernels evaluate them -----------
   For sampler validation (the reference's chi^2 harness, check_ddf.cpp:114-203)
   and bit-exact checks. Uses the uploaded scene. kind:
     IPT_DDF_COSINE  RotateDdf(CosineDdf, to): params = to[3]
     IPT_DDF_LIGHT   DdfFromLight (lighting.cpp:38-73) of scene light params[3]
                     at origin params[0..2]
     IPT_DDF_MIXTURE UnionDdf(lights..., RotateDdf(CosineDdf, normal)) with
                     the scene's unite() weights: origin params[0..2], normal
                     params[3..5]
     IPT_DDF_COSINE_TABLE  IPT_DDF_COSINE as the path kernel samples it, from
                     the exact CosineDdf tables indexed by the draws' 24 bits
                     (u1, u2 must lie on the RNG's 2^-24 grid)
   ipt_ddf_sample: u = n x {pick, u1, u2} uniforms in [0,1) -> n directions
   (vec3() where the reference's sampler returns it); ipt_ddf_value: n
   directions -> n DDF values. Host buffers. */
#define IPT_DDF_COSINE 0
#define IPT_DDF_LIGHT 1
#define IPT_DDF_MIXTURE 2
#define IPT_DDF_COSINE_TABLE 3
int ipt_ddf_sample(ipt_ctx* ctx, int kind, const float* params, const float* u, int64_t n, float* dirs);
int ipt_ddf_value(ipt_ctx* ctx, int kind, const float* params, const float* dirs, int64_t n, float* values);

/* ---- portable-math probes (same code as the kernels), for tests ---------
   fn: 0 acosf, 1 sinf, 2 cosf, 3 (float)acos((double)x), 4 sincosf->sin,
       5 sincosf->cos, 6 sqrtf, 7 CosineDdf z/M_PI, 8 (float)(2*M_PI*u),
       9 a/b over the division pairs of the fast-division proof (x's bit
         pattern -> an in-range numerator and hashed denominator),
      10 the range-free division (box planes) over the same pairs,
      11 the squares-first length comparison over near-tie pairs (0/1),
      12 the 32-bit work-unit division over hashed (n, d) pairs (bit pattern),
      13 the range-free sqrtf on [2^-96, 2^126) (sqrtf elsewhere),
      14 / 15 sin / cos of the RotateDdf angle (float)acos((double)z) for
         z = x; the self-check compares the path kernel's frame table
      16 (ipt_math_selfcheck only) the sphere-in-box frame without glm's
         zero terms against the exact build, over directions hashed from
         the bit pattern (incl. zero / tiny x and y)
      17 / 18 (ipt_math_selfcheck only) the reciprocal by the hardware rcp
         and one / two Newton corrections against the round-4 range-free
         1.0f / x sequence (three corrections)
      19 / 20 (ipt_math_selfcheck only) the range-free division against
         IEEE a/b over the division pairs of 10 / pairs whose divisors have
         all-ones-like significands
      21 (ipt_math_selfcheck only) the range-free division against IEEE a/b
         over every pair of significands (a, b in [1, 2)): pattern indices
         up to 2^46, i = (a's significand << 23) | b's; first_bad reports
         the a significand (i >> 23)
      22 (ipt_math_selfcheck only) the range-free reciprocal's exact scaling:
         rcp(b) == sign(b) 2^-e rcp(m) for |b| = m 2^e in [2^-40, 2^41) */
int ipt_math_host(int fn, const float* in, float* out, int64_t n);
/* Philox4x32-10 blocks exactly as the kernels generate the per-path stream
   that replaces randf() (include/randf.h:6-11; draw k of path (pass s, pixel
   p) is word k%4 of philox({k/4, s, p, 0}, {seed lo, seed hi})), for
   known-answer tests: out[4i..4i+3] = philox(ctr[4i..4i+3], {key0, key1}).
   ctx NULL: the host build of the same code; otherwise on ctx's device. */
int ipt_philox(ipt_ctx* ctx, uint32_t key0, uint32_t key1, const uint32_t* ctr, uint32_t* out, int64_t n);
int ipt_math_device(ipt_ctx* ctx, int fn, const float* in, float* out, int64_t n);
/* Device self-check of the fast math paths: for every float bit pattern b in
 * [lo_bits, hi_bits) (hi_bits <= 2^32; 2^46 for fn 21) compares function fn as the kernels
 * compute it with its exact restatement, on the device. Returns the number of
 * differing results (NaN == NaN) and the lowest differing pattern (0xffffffff
 * if none). Used to prove a fast path exhaustively (all 2^32 inputs). */
int ipt_math_selfcheck(ipt_ctx* ctx, int fn, uint64_t lo_bits, uint64_t hi_bits, uint64_t* mismatches,
                       uint32_t* first_bad);

/* ---- the render plane's replay on chosen samples (ABI 7 addition), for tests --
   The probe of accumulate_kernel: what a render does after its path kernel,
   with the caller's samples in place of traced ones (one entry point added; no
   layout change). values and codes are host buffers [spp][H][W], whole frames,
   exactly as ipt_render_values returns them (codes relative to the nominal
   destination of the call's plane); dev_img is a device image as
   ipt_render_device takes it (sums and pixel_max may be NULL, the plane may be
   preloaded). Synchronous: the image is complete on return. `hip_stream` as
   ipt_render_device's (NULL = the context's own stream).
   Read from p: width, height, spp, tile_rows, n_shards, shard_id and
   IPT_FLAG_GUI_PLANE; no scene is needed. The call runs the render's own code
   behind the path kernel -- the shard plan (ipt_shard_plan), the candidate-row
   layout, the per-launch drift flags, the chunking into launches, the one
   accumulate_kernel launch per chunk -- with a small marking kernel in the
   place of raygen and path kernel: it moves each sample into the candidate
   layout, flags the nominal and the destination pixel of every code other
   than 0x05, and stores value 0 and code 0xfe where the destination row
   belongs to another shard, as a render does.
   Refused on the host, before any device buffer is touched or anything is
   launched: a NULL pointer, a non-positive size, a negative spp, a shard_id
   outside the plan, a code >= 0x10 or with a field of 3 (0xfe and 0xff, the
   library's own markers, among them), a code whose destination (ix + dx,
   nominal row + dy) lies outside [0, W) x [0, H) under the call's row map:
   IPT_E_INVALID; any flag other than IPT_FLAG_GUI_PLANE, or more than
   IPT_REPLAY_MAX_SAMPLES = 2^24 samples (spp * width * height; the call
   stages them on the device, 5 B each): IPT_E_UNSUPPORTED. spp == 0 is a
   no-op. */
#define IPT_REPLAY_MAX_SAMPLES (1 << 24)
int ipt_replay_samples(ipt_ctx* ctx, const ipt_params* p, const float* values, const uint8_t* codes,
                       ipt_image* dev_img, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* IPT_CAPI_H */
