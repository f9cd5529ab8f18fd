// ipt_internal.h — what the library's translation units share about a context
// (defined in ipt_kernels.hip); not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "../../include/ipt_capi.h"

namespace ipt_internal {
int ctx_fail(ipt_ctx* ctx, int code, const std::string& msg);  // records ipt_last_error, returns code
hipStream_t ctx_stream(ipt_ctx* ctx);
int ctx_device(ipt_ctx* ctx);
int ctx_cus(ipt_ctx* ctx);

// One buffer of the post-processing scratch: `cap` elements of `elem` bytes.
// What the elements are is ipt_post.hip's business (its record types and the
// casts stay there); a failed growth leaves {nullptr, 0}.
struct ScratchBuf {
    void* p = nullptr;
    size_t cap = 0, elem = 0;
};

// The post-processing scratch (ipt_post.hip), owned by the context and shared
// by every queued entry point of that file (display, display statistics,
// smooth / PGM, adapt, denoise): each buffer grows to the largest frame seen
// and is freed by ipt_destroy. `done` is recorded on the caller's stream after
// each queued call; the next call on another stream waits for it on the
// device, and the context's drain waits for it on the host (ipt_render_wait,
// ipt_upload_scene, ipt_destroy).
struct PostScratch {
    // (in the order the buffers grow; the first three hold one record)
    enum Buf {
        kScalars,    // bright count, image max key, tone min / max
        kStats,      // ipt_display_stats_device: mx, white point, radix prefix, digit counts
        kPgm,        // ipt_smooth_device / ipt_pgm_device: the maxima, max_value, logf(contrast)
        kBright,     // bright-pixel records, one per pixel at most
        kBlocks,     // per-block bright counts, then their exclusive scan
        kProcessed,  // glare output (smooth output, in-place copy) when the caller passes none
        kTone,       // tone-mapped image when the caller passes none
        kDenoise,    // ipt_denoise_device: per pixel, one record of each of the two planes
        kBufs
    };
    ScratchBuf buf[kBufs];
    // ipt_denoise_pass_ms (IPT_DENOISE_PROFILE=1): events around the last call's passes
    hipEvent_t denoise_ev[8] = {};
    int denoise_timed = 0;  // iterations of the last profiled call, 0: none
    hipEvent_t done = nullptr;
    hipStream_t last_stream = nullptr;
    bool used = false;
};
PostScratch& ctx_post(ipt_ctx* ctx);
int post_wait(ipt_ctx* ctx);     // waits for the queued display work (0 or IPT_E_DEVICE)
void post_release(ipt_ctx* ctx);  // frees the scratch (after post_wait)
// ipt_guides_device's scatter (ipt_post.hip): one pass of the FULL preview
// kernel's kinds and hits, [H][W] in source order, into the guide plane
hipError_t launch_guide_scatter(hipStream_t st, const uint8_t* kinds, const float* hits, ipt_guide* dev_guides, int W,
                                int H, bool gui);

// Owning device allocation: a call's temporaries are freed on every return
// path, early error returns included; release() hands the pointer over, a
// move hands it to another DevBuf (which frees what it held).
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);  // (o frees the old allocation when it goes)
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    T* release() {
        T* q = p;
        p = nullptr;
        return q;
    }
};
}  // namespace ipt_internal
