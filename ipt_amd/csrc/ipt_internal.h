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

// The display pipeline's scratch (ipt_post.hip), owned by the context: grows to
// the largest image seen, freed by ipt_destroy. `done` is recorded on the
// caller's stream after each ipt_display_device; the context's drain waits
// for it (ipt_render_wait, ipt_upload_scene, ipt_destroy).
struct PostScratch {
    void* bright = nullptr;        // bright-pixel records, one per pixel at most
    unsigned int* blocks = nullptr;  // per-block bright counts, then their exclusive scan
    void* scalars = nullptr;       // bright count, image max key, tone min / max
    void* stats = nullptr;         // ipt_display_stats_device: mx, white point, radix prefix, digit counts
    void* pgm = nullptr;           // ipt_smooth_device / ipt_pgm_device: the maxima, max_value, logf(contrast)
    float* processed = nullptr;    // glare output (smooth output, in-place copy) when the caller passes none
    float* tone = nullptr;         // tone-mapped image when the caller passes none
    void* denoise = nullptr;       // ipt_denoise_device: two planes of 32 B records (denoise_cap pixels each)
    size_t bright_cap = 0, blocks_cap = 0, processed_cap = 0, tone_cap = 0, denoise_cap = 0;
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
