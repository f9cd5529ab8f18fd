// ipt_host.h — the C++ host side above the C-ABI (include/ipt_capi.h).
//
// It mirrors the reference's host surface for the hot path, with the same
// names, argument meanings and defaults, so that scene setup and output code
// written against the reference reads the same here:
//   Scene / Geometry / Lighting / Camera / RenderPlane  (tracer_interfaces.h:26-54)
//   GeometrySphereInBox                                 (geometry/GeometrySphereInBox.h)
//   CollectionLighting::addSquareLight/addTriangleLight (CollectionLighting.h:11-20)
//   AreaLight                                           (lighting/lighting.h:15-29)
//   SimpleCamera(position, direction, up_hint=(0,0,1))  (SimpleCamera.h:9-17)
//   GridRenderPlane{pixels, pixel_counters, width, height, max_value}
//                                                       (GridRenderPlane.h:8-18)
//   GuiRenderPlane{width, height, pixels, value_counter} (gui.h:16-20, the
//     image and counters of the Gui, the plane main.cpp renders into)
//   make_scene_box()                                    (sample_scenes.cpp:20-41)
// plus the synthetic BASELINE scenes (C3 sphere list, C5 light grid).
//
// Objects here are scene DESCRIPTIONS: nothing in this layer traces a ray on
// the CPU. Rendering is GpuRenderer / render_samples_gpu, i.e. ipt_render on
// a gfx950 GPU, and it throws IptError(IPT_E_DEVICE) when there is none.
// Every sample_scenes entry and light type of the reference is supported;
// geometry or light classes outside them throw IptError(IPT_E_UNSUPPORTED)
// when flattened.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ipt_capi.h"

namespace ipt {

// glm::vec3 stand-in: plain float data; arithmetic goes through ipt_math.h so
// that constructor arithmetic matches the reference's glm order bit for bit.
struct vec3f {
    float x = 0.0f, y = 0.0f, z = 0.0f;
};

struct IptError : std::runtime_error {
    int code;
    IptError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// ------------------------------------------------------------- geometry
struct Geometry {
    virtual ~Geometry() = default;
};
// Box walls {+x,+y,+z,-x,-z} and the r=0.5 sphere at the origin.
struct GeometrySphereInBox : Geometry {};
// The same box walls plus a list of spheres with FractalSpheres::traceRay's
// acceptance rule (FractalSpheres.cpp:75-84): BASELINE configs[2].
struct SpheresInBox : Geometry {
    struct Sphere {
        vec3f center;
        float radius;
    };
    std::vector<Sphere> spheres;
};

// The z = -1 face (GeometryFloor.cpp:10-23), unrotated CosineDdf.
struct GeometryFloor : Geometry {};
// The x = -1, y = -1, z = -1 faces (GeometryCorner.cpp:10-42).
struct GeometryCorner : Geometry {};
// FractalSpheres (FractalSpheres.cpp:46-97): the generated sphere chain
// between two r=0.5 spheres at (-2,0,0) and (2,0,0), no walls.
// GeometrySmallPt (GeometrySmallPt.cpp:11-58): smallpt's room of 7 spheres,
// intersected in double precision.
struct GeometrySmallPt : Geometry {
    struct Sphere {
        double rad;
        vec3f p;
    };
    std::vector<Sphere> spheres;
    GeometrySmallPt();
};
struct FractalSpheres : Geometry {
    std::vector<float> rs;
    std::vector<vec3f> cs;
    FractalSpheres();
};

// ------------------------------------------------------------- lighting
struct Light {
    float power = 1.0f;
    virtual ~Light() = default;
};
// Light(corner, x_axis, y_axis, power, type) (lighting.cpp:79-90).
struct AreaLight : Light {
    enum type_t { TYPE_DIAMOND = 0, TYPE_TRIANLE = 1 };  // the reference's spelling (lighting.h:17)
    vec3f position, x_axis, y_axis;
    type_t type = TYPE_DIAMOND;
    AreaLight(vec3f corner, vec3f x_axis, vec3f y_axis, float power, type_t type = TYPE_DIAMOND);
};

// SphereLight(origin, radius, power=1) (lighting.h:44-54)
struct SphereLight : Light {
    vec3f position;
    float radius;
    SphereLight(vec3f origin, float radius, float power = 1.0f);
};
// PointLight(origin, virtual_radius, power=1) (lighting.h:31-42)
struct PointLight : Light {
    vec3f position;
    float virtual_radius;
    PointLight(vec3f origin, float virtual_radius, float power = 1.0f);
};
// InvertedSphereLight(origin, radius, power) (lighting.h:57-72)
struct InvertedSphereLight : SphereLight {
    InvertedSphereLight(vec3f origin, float radius, float power);
};

struct Lighting {
    virtual ~Lighting() = default;
};
struct CollectionLighting : Lighting {
    std::vector<std::shared_ptr<const Light>> lights;
    // y_side = cross(normal, x_side) (CollectionLighting.cpp:42-46)
    void addSquareLight(vec3f corner, vec3f normal, vec3f x_side, float power = 1.0f);
    void addTriangleLight(vec3f corner, vec3f x_side, vec3f y_side, float power = 1.0f);
    void addPointLight(vec3f position, float virtual_radius, float power = 1.0f);
    void addSphereLight(vec3f position, float radius, float power = 1.0f);
    void addOuterLight(float radius, float power = 1.0f);  // InvertedSphereLight at the origin
};

// --------------------------------------------------------------- camera
struct Camera {
    virtual ~Camera() = default;
};
struct SimpleCamera : Camera {
    vec3f position, direction, right, up;
    // right = normalize(cross(direction, up_hint)); up = normalize(cross(right, direction))
    SimpleCamera(vec3f position, vec3f direction, vec3f up_hint = vec3f{0.0f, 0.0f, 1.0f});
};

struct Scene {
    std::shared_ptr<const Geometry> geometry;
    std::shared_ptr<const Lighting> lighting;
    std::shared_ptr<const Camera> camera;
};

// ---------------------------------------------------------------- plane
struct RenderPlane {
    virtual ~RenderPlane() = default;
};
// Running mean per pixel as GridRenderPlane::addRay keeps it (including its
// row mapping, GridRenderPlane.cpp:61-75); filled by the GPU accumulate kernel.
struct GridRenderPlane : RenderPlane {
    std::vector<float> pixels;
    std::vector<size_t> pixel_counters;
    size_t width, height;
    float max_value = 0;
    GridRenderPlane(size_t width, size_t height);
};

// The Gui's image and value_counter (gui.h:16-20) without its window: the
// plane the reference program renders into, displays and saves (main.cpp:
// 250-289). Gui::addRay (gui.cpp:165-182) maps a sample to
//   ix = min(size_t(x*W), W-1)   iy = min(size_t(H - y*H), H-1)
// (the reference's 640 and 639 generalised), a plain vertical flip, where
// GridRenderPlane's size_t(H - y*H - 1) folds source rows H-2 and H-1 into row
// 0. Filled by the GPU accumulate kernel (IPT_FLAG_GUI_PLANE); addRay here is
// the CPU restatement, for tests.
struct GuiRenderPlane : RenderPlane {
    size_t width, height;
    std::vector<float> pixels;          // image(ix, iy), row-major
    std::vector<size_t> value_counter;  // value_counter[iy][ix]
    GuiRenderPlane(size_t width, size_t height);
    void resetImage();                  // gui.cpp:154-162
    void addRay(float x, float y, float value);  // gui.cpp:168-178
};

// --------------------------------------------------------- sample scenes
Scene make_scene_box();                                   // sample_scenes[0]
Scene make_scene_box_lights(int k);                       // [0]'s light as k*k squares (C5: k=16)
Scene make_scene_spheres(int n, uint64_t seed = 1);       // box + n spheres (C3: n=10000)
Scene make_scene_random_lights(int n, uint64_t seed = 7);  // overlapping random emitters (tests)
Scene make_scene_square_lit_by_square();                  // sample_scenes.cpp:73-85
Scene make_scene_lit_corner();                            // sample_scenes.cpp:88-108
Scene make_scene_fractal();                               // sample_scenes.cpp:43-55
Scene make_scene_smallpt();                               // sample_scenes.cpp:57-71
// "box", "box_lights:K", "spheres:N[:SEED]", "random_lights:N[:SEED]", "fractal", ...
Scene make_scene_by_name(const std::string& name);

// --------------------------------------------------------------- render
struct RenderParams {
    int spp = 1;          // sample passes (render_sample calls) in this call
    int spp_offset = 0;   // index of the first pass (RNG stream), for progressive rendering
    int n_rays = 16;      // main.cpp:53 ray_power(..., n_rays)
    int depth_max = 8;    // main.cpp:94
    uint64_t seed = 20241223;
    bool counters = false;
    // ray_power_preview (main.cpp:55-92) instead of ray_power_recursive: the
    // frame shown while the camera moves (IPT_FLAG_PREVIEW; n_rays and
    // depth_max are then not read). Every render call below takes it.
    bool preview = false;
    // unit compaction (IPT_FLAG_COMPACT): the path kernel's pool holds the
    // traced samples alone (masked samples of render_adaptive's rounds and
    // shards' halo rows leave it) -- the same image bit for bit; DESIGN.md
    // 4.16 has what it costs. Every render call below takes it; no effect
    // with preview.
    bool compact = false;
    // the guided a-trous filter of GpuRenderer::denoise (ipt_denoise): its
    // iterations (1..6, iteration k taps at step 1 << k; 0: no filter is
    // asked for) and sigmas: colour in standard errors, squarings of the
    // normals' clamped dot product, distance from the centre's plane in world
    // units. No render call reads them.
    int denoise_iterations = 0;
    float denoise_sigma_l = 4.0f;
    int denoise_normal_pow = 5;
    float denoise_sigma_z = 0.1f;
    // destination-row tile shard of this call (ipt_params.tile_rows / n_shards /
    // shard_id): n_shards <= 1 renders the whole frame
    int tile_rows = 16;
    int n_shards = 1;
    int shard_id = 0;
};

// Scene -> POD (ipt_scene). Owns the arrays the POD points into.
struct FlatScene {
    ipt_scene scene{};
    std::vector<ipt_area_light> lights;
    std::vector<ipt_sphere> spheres;
};
FlatScene flatten(const Scene& s);  // throws IptError(IPT_E_UNSUPPORTED)

// What GpuRenderer::display_stats returns: the 8-bit picture, the histogram
// counts and {max, max / 100000.0f, white point} of the processed image.
struct DisplayStats {
    std::vector<uint8_t> gray8;
    std::vector<uint32_t> hist;
    float max = 0.0f, hist_min = 0.0f, white = 0.0f;
};

// Adaptive sampling (ipt_render_adaptive): the loop's rule and round size, and
// what it returns. A pixel stays active while it has fewer than min_count
// samples or the squared standard error of its mean, m2 / (n (n - 1)), exceeds
// (rel_tol |mean| + abs_tol)^2; inactive pixels are not traced.
struct AdaptParams {
    float rel_tol = 0.05f;
    float abs_tol = 1e-3f;
    int min_count = 8;  // >= 2
    int round_spp = 4;  // passes per round; round 0 traces every pixel
};
struct AdaptResult {
    uint32_t active = 0, starved = 0, nan = 0;  // of the last round (ipt_adapt_device's stats)
    int passes = 0;                             // passes used, <= RenderParams::spp
    std::vector<uint8_t> mask;                  // the last mask, by nominal destination pixel
    std::vector<float> m2;                      // the second-moment plane
};

// Temporal reprojection (ipt_reproject): which history a tap may carry over --
// within sigma_z world units of the new hit's plane, its normal within
// normal_min of the new one (a dot product), at most max_count samples'
// weight -- and what the call returns besides the plane.
struct ReprojectParams {
    float sigma_z = 0.1f;
    float normal_min = 0.9f;
    uint32_t max_count = 64;  // 2 .. 1 << 24
};
struct ReprojectResult {
    uint32_t reused = 0, disoccluded = 0, not_surface = 0;  // ipt_reproject's stats
    std::vector<float> m2;                                  // the new frame's second-moment plane
};

class GpuRenderer {
   public:
    explicit GpuRenderer(int device = 0);
    ~GpuRenderer();
    GpuRenderer(const GpuRenderer&) = delete;
    GpuRenderer& operator=(const GpuRenderer&) = delete;
    void upload(const Scene& s);
    // spp passes of render_sample accumulated into plane (bit-exact GridRenderPlane semantics)
    void render(GridRenderPlane& plane, const RenderParams& p);
    // the same into the Gui's plane (Gui::addRay's row map, IPT_FLAG_GUI_PLANE)
    void render(GuiRenderPlane& plane, const RenderParams& p);
    // up to p.spp passes in rounds of a.round_spp, each followed by the next
    // mask on the device, until no pixel is active (ipt_render_adaptive; one
    // device, whole frame: p.n_shards > 1 throws IPT_E_UNSUPPORTED). The plane
    // is continued as render() continues it; the second moments start at zero.
    // m2_in (width*height, e.g. ReprojectResult::m2): the second moments the
    // plane comes with, continued like the plane.
    AdaptResult render_adaptive(GridRenderPlane& plane, const RenderParams& p, const AdaptParams& a,
                                const std::vector<float>* m2_in = nullptr);
    AdaptResult render_adaptive(GuiRenderPlane& plane, const RenderParams& p, const AdaptParams& a,
                                const std::vector<float>* m2_in = nullptr);
    // p.spp unmasked passes through the masked entry point, which keeps the
    // second moments the filter below needs (one round of ipt_render_adaptive:
    // round 0 traces every pixel; this layer holds host buffers only and
    // links no HIP runtime, and that call is the C-ABI's host-buffer way to the
    // masked entry point. It also runs one ipt_adapt_device pass whose mask
    // is dropped). Returns m2; the plane is continued as render() continues
    // it, bit for bit.
    std::vector<float> render_m2(GridRenderPlane& plane, const RenderParams& p,
                                 const std::vector<float>* m2_in = nullptr);
    std::vector<float> render_m2(GuiRenderPlane& plane, const RenderParams& p,
                                 const std::vector<float>* m2_in = nullptr);
    // The plane carried across a camera move (ipt_reproject): on entry the
    // plane, m2 and prev_guides are the previous camera's, cur_guides the new
    // camera's (guides() after upload() of the new scene); on return the plane
    // holds the new frame's starting mean and counters (zeros where nothing
    // could be reused) and the result its m2, for render_m2 / render_adaptive
    // to continue. A GridRenderPlane's max_value restarts at 0.
    ReprojectResult reproject(GridRenderPlane& plane, const std::vector<float>& m2,
                              const std::vector<ipt_guide>& prev_guides, const std::vector<ipt_guide>& cur_guides,
                              const SimpleCamera& prev_camera, const ReprojectParams& rp = ReprojectParams());
    ReprojectResult reproject(GuiRenderPlane& plane, const std::vector<float>& m2,
                              const std::vector<ipt_guide>& prev_guides, const std::vector<ipt_guide>& cur_guides,
                              const SimpleCamera& prev_camera, const ReprojectParams& rp = ReprojectParams());
    // the guide plane (ipt_guides): the first hit of pass p.spp_offset's preview
    // sample per destination pixel, [height][width], under the Grid row map or,
    // with gui_plane, the Gui's
    std::vector<ipt_guide> guides(size_t width, size_t height, const RenderParams& p, bool gui_plane = false);
    // the plane's pixels filtered (ipt_denoise) with p.denoise_iterations and
    // its sigmas, m2 (render_m2's, or AdaptResult::m2) and the guide plane;
    // var_out, when given, gets the filtered variance of the mean. The plane
    // itself is not changed.
    std::vector<float> denoise(const GridRenderPlane& plane, const std::vector<float>& m2,
                               const std::vector<ipt_guide>& guides, const RenderParams& p,
                               std::vector<float>* var_out = nullptr);
    std::vector<float> denoise(const GuiRenderPlane& plane, const std::vector<float>& m2,
                               const std::vector<ipt_guide>& guides, const RenderParams& p,
                               std::vector<float>* var_out = nullptr);
    // the same into a C-ABI image (32-bit counters); with p.n_shards > 1 only
    // the shard's rows of it are read and written (ipt_render). flags: further
    // IPT_FLAG_* bits of the call (IPT_FLAG_GUI_PLANE for a Gui plane's image,
    // IPT_FLAG_PREVIEW as p.preview sets it)
    void render_image(ipt_image& img, size_t width, size_t height, const RenderParams& p, uint32_t flags = 0);
    // host <-> device bytes of the last render (ipt_transfer_bytes): the
    // context keeps its rows of the plane on its device between calls
    void transfer_bytes(uint64_t* host_to_device, uint64_t* device_to_host) const;
    ipt_counters counters() const;
    void last_kernel_ms(float* path_ms, float* accumulate_ms) const;
    // GridRenderPlane::smooth / computeSmoothedMax (GridRenderPlane.cpp:10-59) on the GPU
    void smooth(GridRenderPlane& plane, size_t side);
    void computeSmoothedMax(GridRenderPlane& plane, size_t side);
    // Gui's glare bloom (gui.cpp:28-52) of the plane's pixels
    std::vector<float> glare(const GridRenderPlane& plane, float cutoff);
    // Gui::updateDisplay / Gui::save on the GPU (ipt_display): glare with
    // glare_cutoff when it is > 0, tone map, normalize(0, 255), 8-bit cast.
    // With glare_cutoff 0 the bytes equal to_gray8(plane).
    std::vector<uint8_t> display(const GridRenderPlane& plane, float glare_cutoff = 0.0f);
    // The same with Gui::updateDisplay's statistics (ipt_display_stats): the
    // histogram window's counts (gui.cpp:83-88; buckets 0: none) and the white
    // point of normalize()'s kth_smallest remedy (gui.cpp:13; white_rank < 0:
    // the maximum, and gray8 then equals display()'s).
    DisplayStats display_stats(const GridRenderPlane& plane, float glare_cutoff = 0.0f, int buckets = 400,
                               int64_t white_rank = -1);
    DisplayStats display_stats(const GuiRenderPlane& plane, float glare_cutoff = 0.0f, int buckets = 400,
                               int64_t white_rank = -1);
    // main.cpp's written output on the GPU (ipt_pgm): the bytes of result.pgm
    // for the plane as it stands, n_val(pixel, max_value, contrast, gamma) per
    // pixel, after GridRenderPlane::smooth(smooth_side) and
    // computeSmoothedMax(max_side) of a copy when a side is >= 2 (main.cpp: 2
    // and 5). With both sides 0 the plane's max_value divides, and the bytes
    // equal what write_pgm(path, plane, contrast, gamma) prints.
    std::vector<uint8_t> pgm(const GridRenderPlane& plane, size_t smooth_side = 0, size_t max_side = 0,
                             float contrast = 500.0f, float gamma = 0.6f);
    ipt_ctx* handle() const { return ctx_; }

   private:
    ipt_ctx* ctx_ = nullptr;
};

// One-shot convenience (the INTEGRATION.md adapter's shape).
void render_samples_gpu(const Scene& scene, GridRenderPlane& plane, const RenderParams& p, int device = 0);
void render_samples_gpu(const Scene& scene, GuiRenderPlane& plane, const RenderParams& p, int device = 0);

// N contexts (one per entry of `devices`; a device may repeat), i.e. the
// node's GPUs in one process. The reference renders with several worker
// threads into one plane (main.cpp:256-285); here the destination rows are cut
// into tile_rows-row tiles dealt round-robin to the contexts (ipt_shard_plan),
// each context is driven by its own host thread and renders into the caller's
// plane directly: its device keeps the context's own rows between calls, a call
// moves only those rows (16 B per owned pixel, ipt_render) and no other row is
// touched (one owner per pixel, so nothing is summed or merged). Each shard traces
// only the samples that can land in its rows, with the same (seed, pass, pixel)
// streams: the plane is bit-identical to GpuRenderer::render's.
class MultiGpuRenderer {
   public:
    explicit MultiGpuRenderer(const std::vector<int>& devices, int tile_rows = 16);
    void upload(const Scene& s);
    void render(GridRenderPlane& plane, const RenderParams& p);
    void render(GuiRenderPlane& plane, const RenderParams& p);
    // host <-> device bytes of the last render, summed over the contexts
    void transfer_bytes(uint64_t* host_to_device, uint64_t* device_to_host) const;
    size_t size() const { return r_.size(); }
    GpuRenderer& context(size_t k) { return *r_[k]; }
    // the slowest context's kernel time of the last render (path, accumulate ms)
    void last_kernel_ms(float* path_ms, float* accumulate_ms) const;

   private:
    void render_shards(ipt_image img, size_t width, size_t height, const RenderParams& p, uint32_t flags);
    std::vector<std::unique_ptr<GpuRenderer>> r_;
    int tile_rows_;
};

// --------------------------------------------------------------- output
// Gui's display normalisation (gui.cpp:11-16): (v / max)^(1/2.2), cut to [0, 1].
std::vector<float> tone_map(const GridRenderPlane& plane);
// ... with a chosen white point in place of the maximum (the remedy noted at gui.cpp:13)
std::vector<float> tone_map(const GridRenderPlane& plane, float white);
// Gui::updateDisplay's histogram window (gui.cpp:83-88): CImg
// get_histogram(buckets, max / 100000.0f, max) of the plane (CImg.h:33484-33495).
std::vector<uint32_t> histogram(const GridRenderPlane& plane, int buckets = 400);
// CImg kth_smallest(k) (CImg.h:29441-29473): the element at 0-based index k of
// the ascending order, the maximum for k >= size; -0 before +0, NaNs after
// +inf (a rank among them gives the quiet NaN 0x7fc00000), as ipt_capi.h states.
float kth_smallest(const GridRenderPlane& plane, uint64_t k);
// The reference's rank expression, arg.width()*arg.height()*0.95 (gui.cpp:13),
// for any fraction: (uint64_t)((int)(width*height) * fraction), in double.
uint64_t white_rank_for(size_t width, size_t height, double fraction);
// Gui::save (gui.cpp:133-135): tone map, CImg normalize(0, 255) (CImg.h
// normalize(a,b): (v - min)/(max - min)*255), then the 8-bit PNG writer's
// (unsigned char) cast. Written as a grayscale 8-bit PNG.
std::vector<uint8_t> to_gray8(const GridRenderPlane& plane);
void write_png_gray8(const std::string& path, size_t width, size_t height, const std::vector<uint8_t>& v);
// Raw outputs: PFM (float pixels, bottom-to-top rows per the format) and a
// little binary dump of counters.
void write_pfm(const std::string& path, const GridRenderPlane& plane);
// main.cpp's PGM writer (main.cpp:225-235 n_val, 297-309): ASCII P2, each pixel
// mapped by log(clamp(v*contrast/max, 1, contrast))/log(contrast), ^gamma, *256.
int n_val(float val, float max, float contrast, float gamma);
void write_pgm(const std::string& path, const GridRenderPlane& plane, float contrast = 500.0f, float gamma = 0.6f);
// The same ASCII P2 layout from bytes already mapped (GpuRenderer::pgm).
void write_pgm_bytes(const std::string& path, size_t width, size_t height, const std::vector<uint8_t>& bytes);

}  // namespace ipt
