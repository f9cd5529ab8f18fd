// ipt_render — headless C++ front end of the GPU path (the reference's main.cpp
// render loop, main.cpp:237-312, without the X11 Gui): builds a sample scene,
// renders `passes` batches of `spp` render_sample passes into a
// GridRenderPlane on one MI355X through GpuRenderer (C-ABI), and writes the
// Gui-normalised 8-bit PNG (Gui::save, gui.cpp:133-135) plus optional raw
// float pixels (PFM) and counters.
//
//   ipt_render [--scene box|box_lights:K|spheres:N[:SEED]|random_lights:N[:SEED]]
//              [--width 640] [--height 640] [--spp 16] [--passes 1]
//              [--n-rays 16] [--depth 8] [--seed 20241223] [--device 0]
//              [--devices 0,1,...,7 [--tile-rows 16]]
//              [--out result.png] [--pfm pixels.pfm] [--counts counts.u32]
//              [--pgm result.pgm] [--smooth SIDE] [--smoothed-max SIDE]
//              [--glare CUTOFF --glare-out glare.pfm]
//              [--gpu-display] [--gui-plane] [--preview] [--white-percentile F]
//              [--compact]
//              [--histogram hist.txt [--hist-buckets 400]]
//              [--adaptive REL [--adaptive-abs A] [--min-spp N] [--round-spp R]]
//              [--denoise K [--denoise-sigma L,N,Z]]
//              [--reproject-from DX,DY,DZ[:SPP] [--reproject-sigma Z,NMIN,CAP]]
//
// --reproject-from DX,DY,DZ[:SPP] carries a frame across a camera move
// (GpuRenderer::reproject, ipt_capi.h "temporal reprojection"): SPP passes
// (default --spp) are rendered, with their second moments, from the scene's
// camera displaced by (DX, DY, DZ), and that camera's guide plane is taken;
// then the scene's own camera is uploaded, its guide plane taken, the planes
// reprojected to it, and the render continues with --spp passes from pass SPP
// on. --reproject-sigma Z,NMIN,CAP sets the plane distance in world units
// (0.1), the least dot product of the two normals (0.9) and the history cap in
// samples (64). It composes with --gui-plane, --adaptive, --denoise,
// --gpu-display, --pgm and every output option; one device, one batch
// (--passes 1), not with --preview. The JSON line then carries
// "reproject_reused", "reproject_disoccluded" and "reproject_not_surface".
// --denoise K filters the rendered plane with K iterations (1..6) of the guided
// a-trous filter (GpuRenderer::denoise, ipt_capi.h "denoising"; iteration k
// taps at step 1 << k) before every output stage: --smooth, --glare, --pgm,
// --gpu-display, the PNG and --pfm see the filtered pixels. --denoise-sigma
// L,N,Z sets the colour sigma in standard errors (4), the squarings of the
// normals' dot product (5) and the plane distance in world units (0.1). The
// filter needs the plane's second moments: with --adaptive it takes that
// loop's; otherwise the render runs through the masked entry point with no
// mask (the same plane, bit for bit). One device and one batch (--passes 1).
// --adaptive REL renders adaptively (GpuRenderer::render_adaptive): rounds of
// --round-spp passes (4), each followed on the device by the next sample mask,
// until no pixel is active or --spp, here the cap, is used up. A pixel stays
// active while it has fewer than --min-spp samples (8) or the standard error
// of its mean exceeds REL * |mean| + A (--adaptive-abs, 1e-3). One device and
// one batch (--passes 1); composes with --gui-plane, --preview and every
// output option. The JSON line then carries "adaptive_passes" (passes used)
// and "adaptive_active" (pixels still active at the end).
// --compact renders with unit compaction (IPT_FLAG_COMPACT): the path kernel's
// work pool holds only the samples that are traced (the masked samples of an
// --adaptive render's rounds leave it); every output is the same bytes. It
// composes with every other option (no effect with --preview).
// --gui-plane renders into the Gui's plane (GuiRenderPlane, Gui::addRay's row
// map, gui.cpp:165-182) instead of a GridRenderPlane: the plane the reference
// program displays and saves, so that with --gpu-display the chain render ->
// Gui plane -> glare -> tone map -> 8-bit is the reference's main loop on the
// device. It composes with --gpu-display, --glare, --passes, --devices, --pfm
// and --counts; --smooth, --smoothed-max and --pgm are GridRenderPlane's
// filters and main.cpp's PGM writer for it and are refused.
// --preview renders with the reference's preview estimator (ray_power_preview,
// main.cpp:55-92: one geometry trace and one light trace per camera ray, the
// frame a viewer shows while the camera moves; IPT_FLAG_PREVIEW). --n-rays and
// --depth are then not read. It composes with --gui-plane, --gpu-display,
// --devices and every output option.
// --gpu-display takes the PNG's bytes from GpuRenderer::display (the display
// pipeline on the GPU, with the --glare cutoff's bloom when one is given, as
// Gui::updateDisplay shows it) instead of the host's to_gray8; without
// --glare the file is the same bytes.
// --white-percentile F (with --gpu-display) divides by the value at rank
// (int)(W*H)*F of the displayed image instead of its maximum, the remedy the
// reference notes beside normalize() (gui.cpp:13; F = 0.95 is its constant):
// the PNG's bytes come from GpuRenderer::display_stats.
// --histogram writes the counts of Gui::updateDisplay's histogram window
// (gui.cpp:83-88, --hist-buckets of them, 400 as the Gui's) of the displayed
// image, one per line, computed on the GPU by the same call.
// --smooth applies GridRenderPlane::smooth(SIDE) on the GPU before output;
// --glare writes Gui's glare bloom of the plane (gui.cpp:28-52, GPU) as PFM;
// --pgm writes main.cpp's contrast/gamma PGM (main.cpp:297-309), after
// GridRenderPlane::computeSmoothedMax(SIDE) with --smoothed-max (main.cpp:293;
// the reference's sequence is --smooth 2 --smoothed-max 5). With --gpu-display
// the PGM's numbers come from GpuRenderer::pgm (the smoothed maximum, logf,
// powf and the 8-bit mapping on the GPU) instead of the host's n_val loop; the
// file is the same bytes.
// --devices renders with one context per listed device (MultiGpuRenderer: the
// rows cut into --tile-rows tiles dealt round-robin, owned rows assembled at
// the end of each batch; a device may repeat); the image is the same bits.
//
// Prints one JSON line: scene, size, passes, Mpaths/s (whole call and kernel).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ipt_host.h"

namespace {
[[noreturn]] void usage(const char* msg) {
    std::fprintf(stderr, "ipt_render: %s\n", msg);
    std::fprintf(stderr,
                 "usage: ipt_render [--scene NAME] [--width W] [--height H] [--spp S] [--passes P]\n"
                 "                  [--n-rays N] [--depth D] [--seed X] [--device I]\n"
                 "                  [--devices I,J,... [--tile-rows 16]]\n"
                 "                  [--out result.png] [--pfm pixels.pfm] [--counts counts.u32]\n"
                 "                  [--pgm result.pgm] [--smooth SIDE] [--smoothed-max SIDE]\n"
                 "                  [--glare CUTOFF --glare-out F.pfm]\n"
                 "                  [--gpu-display] [--gui-plane] [--preview] [--white-percentile F]\n"
                 "                  [--compact]\n"
                 "                  [--histogram hist.txt [--hist-buckets 400]]\n"
                 "                  [--adaptive REL [--adaptive-abs A] [--min-spp N] [--round-spp R]]\n"
                 "                  [--denoise K [--denoise-sigma L,N,Z]]\n"
                 "                  [--reproject-from DX,DY,DZ[:SPP] [--reproject-sigma Z,NMIN,CAP]]\n");
    std::exit(2);
}
}  // namespace

int main(int argc, char** argv) {
    std::string scene_name = "box", out = "result.png", pfm, counts, pgm, glare_out, hist_out;
    double white_percentile = -1.0;
    long hist_buckets = 400;
    long smooth = 0, smoothed_max = 0;
    bool gpu_display = false, gui_plane = false, preview = false, compact = false;
    double glare = -1.0, adaptive_rel = -1.0, adaptive_abs = 1e-3;
    long min_spp = 8, round_spp = 4, denoise = 0, denoise_pow = 5;
    double denoise_l = 4.0, denoise_z = 0.1;
    bool reproject = false;
    double from[3] = {0.0, 0.0, 0.0}, reproject_z = 0.1, reproject_nmin = 0.9;
    long reproject_spp = 0, reproject_cap = 64;
    long width = 640, height = 640, spp = 16, passes = 1, n_rays = 16, depth = 8, device = 0, tile_rows = 16;
    std::vector<int> devices;
    unsigned long long seed = 20241223ull;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) usage(("missing value for " + a).c_str());
            return argv[++i];
        };
        if (a == "--scene") scene_name = val();
        else if (a == "--width") width = std::atol(val());
        else if (a == "--height") height = std::atol(val());
        else if (a == "--spp") spp = std::atol(val());
        else if (a == "--passes") passes = std::atol(val());
        else if (a == "--n-rays") n_rays = std::atol(val());
        else if (a == "--depth") depth = std::atol(val());
        else if (a == "--seed") seed = std::strtoull(val(), nullptr, 0);
        else if (a == "--device") device = std::atol(val());
        else if (a == "--devices") {
            devices.clear();
            for (const char* c = val(); *c;) {
                devices.push_back(std::atoi(c));
                while (*c && *c != ',') ++c;
                if (*c == ',') ++c;
            }
        } else if (a == "--tile-rows") tile_rows = std::atol(val());
        else if (a == "--out") out = val();
        else if (a == "--pfm") pfm = val();
        else if (a == "--counts") counts = val();
        else if (a == "--pgm") pgm = val();
        else if (a == "--smooth") smooth = std::atol(val());
        else if (a == "--smoothed-max") smoothed_max = std::atol(val());
        else if (a == "--glare") glare = std::atof(val());
        else if (a == "--glare-out") glare_out = val();
        else if (a == "--gpu-display") gpu_display = true;
        else if (a == "--gui-plane") gui_plane = true;
        else if (a == "--preview") preview = true;
        else if (a == "--compact") compact = true;
        else if (a == "--white-percentile") white_percentile = std::atof(val());
        else if (a == "--histogram") hist_out = val();
        else if (a == "--hist-buckets") hist_buckets = std::atol(val());
        else if (a == "--adaptive") adaptive_rel = std::atof(val());
        else if (a == "--adaptive-abs") adaptive_abs = std::atof(val());
        else if (a == "--min-spp") min_spp = std::atol(val());
        else if (a == "--round-spp") round_spp = std::atol(val());
        else if (a == "--denoise") denoise = std::atol(val());
        else if (a == "--denoise-sigma") {
            if (std::sscanf(val(), "%lf,%ld,%lf", &denoise_l, &denoise_pow, &denoise_z) != 3)
                usage("--denoise-sigma takes L,N,Z");
        }
        else if (a == "--reproject-from") {
            const int got = std::sscanf(val(), "%lf,%lf,%lf:%ld", &from[0], &from[1], &from[2], &reproject_spp);
            if (got < 3 || (got == 4 && reproject_spp <= 0)) usage("--reproject-from takes DX,DY,DZ[:SPP], SPP >= 1");
            reproject = true;
        } else if (a == "--reproject-sigma") {
            if (std::sscanf(val(), "%lf,%lf,%ld", &reproject_z, &reproject_nmin, &reproject_cap) != 3)
                usage("--reproject-sigma takes Z,NMIN,CAP");
        }
        else usage(("unknown option " + a).c_str());
    }
    if (width <= 0 || height <= 0 || spp <= 0 || passes <= 0 || n_rays < 0 || depth < 0) usage("bad sizes");
    if (gui_plane && smooth > 0) usage("--smooth is GridRenderPlane::smooth; the Gui plane (--gui-plane) has none");
    if (gui_plane && smoothed_max > 0) usage("--smoothed-max is GridRenderPlane::computeSmoothedMax; not with --gui-plane");
    if (smoothed_max < 0 || (smoothed_max > 0 && pgm.empty())) usage("--smoothed-max takes a side and needs --pgm");
    if (gui_plane && !pgm.empty()) usage("--pgm is main.cpp's writer for a GridRenderPlane; not with --gui-plane");
    if (white_percentile >= 0.0 && !gpu_display) usage("--white-percentile needs --gpu-display");
    if (!(white_percentile < 0.0) && !(white_percentile <= 1.0)) usage("--white-percentile takes a fraction in [0, 1]");
    if (hist_buckets < 1 || hist_buckets > 4096) usage("--hist-buckets takes 1..4096");
    const bool adaptive = adaptive_rel >= 0.0;
    if (adaptive && (passes != 1 || devices.size() > 1)) usage("--adaptive renders one batch on one device");
    if (adaptive && (!(adaptive_abs >= 0.0) || min_spp < 2 || round_spp < 1))
        usage("--adaptive-abs >= 0, --min-spp >= 2, --round-spp >= 1");
    if (denoise < 0 || denoise > 6) usage("--denoise takes 1..6 iterations");
    if (denoise > 0 && (passes != 1 || devices.size() > 1)) usage("--denoise filters one batch on one device");
    if (denoise > 0 && (!(denoise_l > 0.0) || !(denoise_z > 0.0) || denoise_pow < 0 || denoise_pow > 7))
        usage("--denoise-sigma: L > 0, N in 0..7, Z > 0");
    if (reproject && (passes != 1 || devices.size() > 1)) usage("--reproject-from carries one batch on one device");
    if (reproject && preview) usage("--reproject-from continues the full estimator's plane; not with --preview");
    if (reproject && (!(reproject_z > 0.0) || reproject_nmin != reproject_nmin || reproject_cap < 2 ||
                      reproject_cap > (1l << 24)))
        usage("--reproject-sigma: Z > 0, NMIN a number, CAP in 2..16777216");
    if (reproject && reproject_spp == 0) reproject_spp = spp;
    try {
        const ipt::Scene scene = ipt::make_scene_by_name(scene_name);
        if (devices.empty()) devices.push_back((int)device);
        if (tile_rows <= 0) usage("bad --tile-rows");
        ipt::MultiGpuRenderer gpus(devices, (int)tile_rows);
        ipt::GpuRenderer& gpu = gpus.context(0);  // post-process runs on the first context
        gpus.upload(scene);
        // the output stages below read a GridRenderPlane's size, pixels and
        // counters; a Gui plane's are moved into `plane` once it is rendered
        ipt::GridRenderPlane plane((size_t)width, (size_t)height);
        ipt::GuiRenderPlane gui(gui_plane ? (size_t)width : 0, gui_plane ? (size_t)height : 0);
        ipt::RenderParams p;
        p.spp = (int)spp;
        p.n_rays = (int)n_rays;
        p.depth_max = (int)depth;
        p.seed = seed;
        p.preview = preview;
        p.compact = compact;
        p.denoise_iterations = (int)denoise;
        p.denoise_sigma_l = (float)denoise_l;
        p.denoise_normal_pow = (int)denoise_pow;
        p.denoise_sigma_z = (float)denoise_z;
        std::vector<float> m2;
        double kernel_ms = 0.0;
        ipt::AdaptResult ar;
        ipt::ReprojectResult rr;
        const auto t0 = std::chrono::steady_clock::now();
        if (reproject) {
            // the history: reproject_spp passes from the displaced camera, and its guides
            const auto cam = std::dynamic_pointer_cast<const ipt::SimpleCamera>(scene.camera);
            if (!cam) throw ipt::IptError(IPT_E_UNSUPPORTED, "--reproject-from needs a SimpleCamera");
            const auto moved = std::make_shared<ipt::SimpleCamera>(*cam);
            moved->position = ipt::vec3f{cam->position.x + (float)from[0], cam->position.y + (float)from[1],
                                         cam->position.z + (float)from[2]};
            ipt::Scene prev_scene = scene;
            prev_scene.camera = moved;
            gpus.upload(prev_scene);
            ipt::RenderParams hp = p;
            hp.spp = (int)reproject_spp;
            m2 = gui_plane ? gpu.render_m2(gui, hp) : gpu.render_m2(plane, hp);
            const std::vector<ipt_guide> prev_guides = gpu.guides((size_t)width, (size_t)height, hp, gui_plane);
            // the new camera: its guides, the planes resampled to it, and the render goes on from pass reproject_spp
            gpus.upload(scene);
            const std::vector<ipt_guide> cur_guides = gpu.guides((size_t)width, (size_t)height, hp, gui_plane);
            ipt::ReprojectParams rp;
            rp.sigma_z = (float)reproject_z;
            rp.normal_min = (float)reproject_nmin;
            rp.max_count = (uint32_t)reproject_cap;
            rr = gui_plane ? gpu.reproject(gui, m2, prev_guides, cur_guides, *moved, rp)
                           : gpu.reproject(plane, m2, prev_guides, cur_guides, *moved, rp);
            m2 = rr.m2;
            p.spp_offset = (int)reproject_spp;
        }
        const std::vector<float>* m2_in = reproject ? &m2 : nullptr;
        if (adaptive) {
            ipt::AdaptParams ad;
            ad.rel_tol = (float)adaptive_rel;
            ad.abs_tol = (float)adaptive_abs;
            ad.min_count = (int)min_spp;
            ad.round_spp = (int)round_spp;
            ar = gui_plane ? gpu.render_adaptive(gui, p, ad, m2_in) : gpu.render_adaptive(plane, p, ad, m2_in);
            m2 = ar.m2;
        } else if (denoise > 0 || reproject) {
            m2 = gui_plane ? gpu.render_m2(gui, p, m2_in) : gpu.render_m2(plane, p, m2_in);
        }
        for (long pass = 0; pass < passes && !adaptive && denoise == 0 && !reproject; ++pass) {  // progressive: each batch continues the RNG stream
            p.spp_offset = (int)(pass * spp);
            if (gui_plane) gpus.render(gui, p);
            else gpus.render(plane, p);
            float pm = 0.0f, am = 0.0f;
            gpus.last_kernel_ms(&pm, &am);
            kernel_ms += pm + am;
        }
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        uint64_t h2d = 0, d2h = 0;  // the last batch's plane transfers (all contexts)
        gpus.transfer_bytes(&h2d, &d2h);
        if (gui_plane) {
            plane.pixels = std::move(gui.pixels);
            plane.pixel_counters = std::move(gui.value_counter);
            // (the Gui keeps no max_value; the JSON line reports the plane's largest pixel)
            for (float v : plane.pixels) plane.max_value = v > plane.max_value ? v : plane.max_value;
        }
        if (denoise > 0)  // (the plane holds either map's pixels by now; the guides follow the map)
            plane.pixels = gpu.denoise(plane, m2, gpu.guides(plane.width, plane.height, p, gui_plane), p);
        if (smooth > 0) gpu.smooth(plane, (size_t)smooth);
        if (glare >= 0.0 && !glare_out.empty()) {
            ipt::GridRenderPlane g(plane.width, plane.height);
            g.pixels = gpu.glare(plane, (float)glare);
            ipt::write_pfm(glare_out, g);
        }
        if (!pgm.empty() && gpu_display) {
            ipt::write_pgm_bytes(pgm, plane.width, plane.height, gpu.pgm(plane, 0, (size_t)smoothed_max));
        } else if (!pgm.empty()) {
            if (smoothed_max > 0) gpu.computeSmoothedMax(plane, (size_t)smoothed_max);
            ipt::write_pgm(pgm, plane);
        }
        if (white_percentile >= 0.0 || !hist_out.empty()) {
            // one call gives the picture, the histogram and the white point
            const int64_t rank =
                white_percentile >= 0.0 ? (int64_t)ipt::white_rank_for(plane.width, plane.height, white_percentile) : -1;
            const ipt::DisplayStats ds = gpu.display_stats(plane, gpu_display && glare > 0.0 ? (float)glare : 0.0f,
                                                           hist_out.empty() ? 0 : (int)hist_buckets, rank);
            if (!hist_out.empty()) {
                std::ofstream f(hist_out);
                for (uint32_t c : ds.hist) f << c << "\n";
            }
            if (!out.empty())
                ipt::write_png_gray8(out, plane.width, plane.height, gpu_display ? ds.gray8 : ipt::to_gray8(plane));
        } else if (!out.empty())
            ipt::write_png_gray8(out, plane.width, plane.height,
                                 gpu_display ? gpu.display(plane, glare > 0.0 ? (float)glare : 0.0f)
                                             : ipt::to_gray8(plane));
        if (!pfm.empty()) ipt::write_pfm(pfm, plane);
        if (!counts.empty()) {
            std::ofstream f(counts, std::ios::binary);
            for (size_t c : plane.pixel_counters) {
                const uint32_t v = (uint32_t)c;
                f.write(reinterpret_cast<const char*>(&v), 4);
            }
        }
        const double paths = (double)width * height * spp * passes;
        std::printf(
            "{\"scene\": \"%s\", \"width\": %ld, \"height\": %ld, \"spp\": %ld, \"passes\": %ld, "
            "\"n_rays\": %ld, \"depth_max\": %ld, \"devices\": %zu, \"max_value\": %.9g, \"seconds\": %.4f, "
            "\"Mpaths_per_s\": %.3f, \"kernel_Mpaths_per_s\": %.3f, \"last_batch_h2d_bytes\": %llu, "
            "\"last_batch_d2h_bytes\": %llu, \"plane\": \"%s\"",
            scene_name.c_str(), width, height, spp, passes, n_rays, depth, gpus.size(), (double)plane.max_value, secs,
            paths / secs / 1e6, kernel_ms > 0 ? paths / (kernel_ms * 1e-3) / 1e6 : 0.0, (unsigned long long)h2d,
            (unsigned long long)d2h, gui_plane ? "gui" : "grid");
        if (adaptive) std::printf(", \"adaptive_passes\": %d, \"adaptive_active\": %u", ar.passes, ar.active);
        if (reproject)
            std::printf(", \"reproject_reused\": %u, \"reproject_disoccluded\": %u, \"reproject_not_surface\": %u",
                        rr.reused, rr.disoccluded, rr.not_surface);
        std::printf("}\n");
    } catch (const ipt::IptError& e) {
        std::fprintf(stderr, "ipt_render: error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
