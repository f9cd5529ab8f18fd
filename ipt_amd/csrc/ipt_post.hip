// ipt_post.hip — the reference's image post-process on the GPU (SURVEY.md
// §8(f) row 2), bit-exact:
//   GridRenderPlane::smooth(side) / computeSmoothedMax(side)
//                                  (src/GridRenderPlane.cpp:10-59)
//   Gui's glare bloom               (src/gui.cpp:28-52: draw_halo + glare)
//   main.cpp's PGM output           (src/main.cpp:225-235, 291-309: n_val after
//                                    smooth and computeSmoothedMax; "PGM path" below)
//
// smooth: the reference filters in place, walking y and x downwards from the
// bottom-right corner and reading pixels (y-yy, x-xx), yy, xx < side. Every
// pixel it reads is at or above-left of the one it writes and is written later
// (or is the same pixel, read before the write), so the in-place filter equals
// an out-of-place one: one thread per pixel, the side*side sum in the
// reference's order (yy outer, xx inner, float adds), accum /= side*side.
// The running max starts at 0 and takes `accum > max` (NaN never wins).
//
// glare: out = img; for every pixel with !(val <= cutoff), in raster order,
// coef = (float)(0.1*val/cutoff) (f64), C = cutoff*coef, and every output
// pixel gets += C/(0.25+r)/(0.25+r) (float) with r = (float)hypot(dx, dy);
// then out.cut(0, cutoff). Per output pixel the halos are added in the
// bright pixels' raster order, so one thread per output pixel walking the
// bright list (staged through LDS) reproduces the sequence. (float)hypot of
// two ints equals sqrtf((float)(dx^2+dy^2)) while the sum < 2^24 and
// (float)sqrt((double)sum) above (checked against glibc for all |dx|,|dy| <
// 4096, tests/test_post.py); images are limited to 4096 x 4096 accordingly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ipt_capi.h"
#include "ipt_internal.h"
#include "ipt_math.h"

namespace {

using namespace ipt;

constexpr int kPostBlock = 256;

// KEEP: a pixel the filter leaves alone (x < side-1 or y < side-1) is copied
// from `in`, so that `out` is the whole filtered plane (ipt_smooth_device out
// of place; ipt_smooth copies the plane first instead)
template <bool KEEP>
__global__ __launch_bounds__(kPostBlock) void smooth_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int W, int H, int side, unsigned int* max_bits) {
    const int x = blockIdx.x * kPostBlock + threadIdx.x, y = blockIdx.y;
    float cand = 0.0f;
    if (KEEP && x < W && (x < side - 1 || y < side - 1)) out[(size_t)y * W + x] = in[(size_t)y * W + x];
    if (x < W && x >= side - 1 && y >= side - 1) {
        float accum = 0.0f;
        for (int yy = 0; yy < side; ++yy) {
            const float* row = in + (size_t)(y - yy) * W + x;
            for (int xx = 0; xx < side; ++xx) accum += row[-xx];
        }
        accum = accum / (float)((unsigned)side * (unsigned)side);  // size_t -> float, exact below 2^24
        if (out) out[(size_t)y * W + x] = accum;
        cand = accum > 0.0f ? accum : 0.0f;  // `if (accum > max_value)` with max_value >= 0
    }
    // block max of non-negative floats: their bit patterns order as integers
    __shared__ unsigned int red[kPostBlock / 64];
    unsigned int m = __float_as_uint(cand);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int b = red[0];
        for (int i = 1; i < kPostBlock / 64; ++i) b = max(b, red[i]);
        if (b) atomicMax(max_bits, b);
    }
}

struct Bright {
    int x, y;
    float c;  // C = cutoff * coef
    int pad;
};

constexpr int kGlareChunk = 512;

// nb_dev non-NULL: the bright count is read there (ipt_display_device: it
// never leaves the device, and the grid does not depend on it)
__global__ __launch_bounds__(kPostBlock) void glare_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           int W, int H, const Bright* __restrict__ bright, int nb,
                                                           float cutoff, const unsigned int* __restrict__ nb_dev) {
    __shared__ Bright tile[kGlareChunk];
    if (nb_dev) nb = (int)*nb_dev;
    const int x = blockIdx.x * kPostBlock + threadIdx.x, y = blockIdx.y;
    const bool live = x < W;
    float v = live ? in[(size_t)y * W + x] : 0.0f;
    const float r0 = 0.25f;
    for (int base = 0; base < nb; base += kGlareChunk) {
        const int n = min(kGlareChunk, nb - base);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kPostBlock) tile[i] = bright[base + i];
        __syncthreads();
        if (live)
            for (int i = 0; i < n; ++i) {
                const int dx = x - tile[i].x, dy = y - tile[i].y;  // |dx|, |dy| < 4096
                const unsigned int s = (unsigned int)(dx * dx + dy * dy);
                const float r = s < (1u << 24) ? __builtin_sqrtf((float)s) : (float)__builtin_sqrt((double)s);
                const float val = (tile[i].c / (r0 + r)) / (r0 + r);
                v = v + val;
            }
    }
    if (live) out[(size_t)y * W + x] = v < 0.0f ? 0.0f : (v > cutoff ? cutoff : v);  // cimg::cut
}

// ---------------------------------------------------------------- display
// ipt_display_device: glare -> tone map -> 8-bit without a value crossing to
// the host. Kernels in stream order; the launch boundary is the only
// synchronisation between workgroups, and every cross-workgroup combination
// is an integer max, so the result does not depend on dispatch order.
//
// Bright-pixel compaction (raster order, as the glare sums need): a block owns
// kCompactSpan consecutive pixels. bright_count_kernel writes each block's
// count, bright_scan_kernel (one workgroup) turns the counts into exclusive
// offsets and leaves the total in DisplayScalars::nb, bright_scatter_kernel
// recomputes the flags and places each record at offset + the pixels before it
// in the block (wave ballot + the earlier waves' counts through LDS).
//
// Folds: the reference's `mx = max(mx, v)` from element 0 keeps the FIRST
// maximum and skips NaN unless element 0 is one. The image max is therefore
// an atomicMax over 64-bit keys {value key, ~index}: the value key orders all
// floats (negative ones reversed, -0 == +0), the index part prefers the
// earliest element among equals (only +-0 differ in bits), NaN gives key 0;
// "element 0 is NaN" is read from element 0 itself. tone is >= +0 or NaN, so
// its min and max are integer folds of the bit patterns (min as max of ~bits,
// so one memset to 0 initialises every scalar).
constexpr int kCompactRounds = 4;
constexpr int kCompactSpan = kPostBlock * kCompactRounds;
constexpr int kPostWaves = kPostBlock / 64;

struct DisplayScalars {
    unsigned long long max_key;
    unsigned int nb;
    unsigned int tone_max;      // bits of max(tone)
    unsigned int tone_min_inv;  // ~bits of min(tone)
    unsigned int pad;
};

__device__ __forceinline__ bool is_nan_(float v) { return (f2u(v) & 0x7fffffffu) > 0x7f800000u; }

__global__ __launch_bounds__(kPostBlock) void bright_count_kernel(const float* __restrict__ in, long long n,
                                                                  float cutoff, unsigned int* __restrict__ counts) {
    __shared__ unsigned int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kCompactSpan;
    unsigned int c = 0;
    for (int r = 0; r < kCompactRounds; ++r) {
        const long long i = base + r * kPostBlock + threadIdx.x;
        const bool b = i < n && !(in[i] <= cutoff);
        c += (unsigned int)__popcll(__ballot(b));
    }
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup: counts[0..nblk) -> exclusive offsets in place, total -> sc->nb
__global__ __launch_bounds__(kPostBlock) void bright_scan_kernel(unsigned int* __restrict__ counts, int nblk,
                                                                 DisplayScalars* __restrict__ sc) {
    __shared__ unsigned int part[kPostBlock];
    const int per = (nblk + kPostBlock - 1) / kPostBlock;
    const int lo = min((int)threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    unsigned int s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int acc = 0;
        for (int t = 0; t < kPostBlock; ++t) {
            const unsigned int v = part[t];
            part[t] = acc;
            acc += v;
        }
        sc->nb = acc;
    }
    __syncthreads();
    unsigned int off = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        const unsigned int v = counts[i];
        counts[i] = off;
        off += v;
    }
}

__global__ __launch_bounds__(kPostBlock) void bright_scatter_kernel(const float* __restrict__ in, int W, long long n,
                                                                    float cutoff,
                                                                    const unsigned int* __restrict__ offsets,
                                                                    Bright* __restrict__ bright) {
    __shared__ unsigned int wave_cnt[kPostWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kCompactSpan;
    unsigned int run = offsets[blockIdx.x];
    for (int r = 0; r < kCompactRounds; ++r) {
        const long long i = base + r * kPostBlock + threadIdx.x;
        const float val = i < n ? in[i] : 0.0f;
        const bool b = i < n && !(val <= cutoff);  // gui.cpp:40-47; NaN is bright
        const unsigned long long mask = __ballot(b);
        if (lane == 0) wave_cnt[wave] = (unsigned int)__popcll(mask);
        __syncthreads();
        unsigned int before = 0, all = 0;
        for (int w = 0; w < kPostWaves; ++w) {
            const unsigned int c = wave_cnt[w];
            before += w < wave ? c : 0u;
            all += c;
        }
        if (b) {
            const unsigned int dst = run + before + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
            const float coef = (float)(0.1 * (double)val / (double)cutoff);
            if ((long long)dst < n) bright[dst] = Bright{(int)(i % W), (int)(i / W), cutoff * coef, 0};
        }
        run += all;
        __syncthreads();  // wave_cnt is rewritten next round
    }
}

// value key of a non-NaN float: unsigned order == float order, -0 == +0
__device__ __forceinline__ unsigned long long max_key_(float v, unsigned int idx) {
    unsigned int u = f2u(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0ull;
    if (u == 0x80000000u) u = 0u;
    const unsigned int k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)k << 32) | (unsigned long long)(0xffffffffu - idx);
}

// v[0..3] = p[i..i+3] (0 past n): one 16-byte load where the array's alignment allows
__device__ __forceinline__ void load4_(const float* __restrict__ p, long long i, long long n, bool vec, float* v) {
    if (vec && i + 3 < n) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.0f;
    }
}

// max over the workgroup, valid in thread 0
template <class T>
__device__ __forceinline__ T block_max_(T m, T* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const T other = __shfl_xor(m, o);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    T b = red[0];
    for (int w = 1; w < kPostWaves; ++w) b = red[w] > b ? red[w] : b;
    __syncthreads();
    return b;
}

__global__ __launch_bounds__(kPostBlock) void image_max_kernel(const float* __restrict__ in, long long n,
                                                               DisplayScalars* __restrict__ sc) {
    __shared__ unsigned long long red[kPostWaves];
    const long long i = ((long long)blockIdx.x * kPostBlock + threadIdx.x) * 4;
    float v[4];
    load4_(in, i, n, ((uintptr_t)in & 15u) == 0, v);
    unsigned long long m = 0ull;
    for (int j = 0; j < 4; ++j)
        if (i + j < n) {
            const unsigned long long k = max_key_(v[j], (unsigned int)(i + j));
            m = k > m ? k : m;
        }
    m = block_max_(m, red);
    if (threadIdx.x == 0 && m) atomicMax(&sc->max_key, m);
}

// tone_map (ipt_host.cpp): v / mx, powf(., p), cut to [0,1] (NaN passes)
__global__ __launch_bounds__(kPostBlock) void tone_kernel(const float* __restrict__ in, float* __restrict__ tone,
                                                          long long n, float p, DisplayScalars* __restrict__ sc) {
    __shared__ unsigned int red[kPostWaves];
    const unsigned long long key = sc->max_key;
    const float first = in[0];
    const float mx = (is_nan_(first) || !key) ? first : in[0xffffffffu - (unsigned int)key];
    const long long i = ((long long)blockIdx.x * kPostBlock + threadIdx.x) * 4;
    float v[4];
    load4_(in, i, n, ((uintptr_t)in & 15u) == 0, v);
    unsigned int hi = 0u, lo_inv = 0u;
    for (int j = 0; j < 4; ++j) {
        const float w = powf_(div_x86nan_(v[j], mx), p);
        v[j] = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
        if (i + j < n && !is_nan_(v[j])) {
            hi = max(hi, f2u(v[j]));
            lo_inv = max(lo_inv, ~f2u(v[j]));
        }
    }
    if (((uintptr_t)tone & 15u) == 0 && i + 3 < n) {
        *reinterpret_cast<float4*>(tone + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (i + j < n) tone[i + j] = v[j];
    }
    hi = block_max_(hi, red);
    lo_inv = block_max_(lo_inv, red);
    if (threadIdx.x == 0) {
        if (hi) atomicMax(&sc->tone_max, hi);
        if (lo_inv) atomicMax(&sc->tone_min_inv, lo_inv);
    }
}

// to_gray8 (ipt_host.cpp): CImg normalize(0, 255) and the unsigned char cast
__global__ __launch_bounds__(kPostBlock) void gray8_kernel(const float* __restrict__ tone, uint8_t* __restrict__ out,
                                                           long long n, const DisplayScalars* __restrict__ sc) {
    const float t0 = tone[0];
    const bool nan0 = is_nan_(t0);  // the folds start at element 0: NaN there stays
    const float m = nan0 ? t0 : u2f(~sc->tone_min_inv), M = nan0 ? t0 : u2f(sc->tone_max);
    const long long i = ((long long)blockIdx.x * kPostBlock + threadIdx.x) * 4;
    float v[4];
    load4_(tone, i, n, ((uintptr_t)tone & 15u) == 0, v);
    uint8_t b[4];
    for (int j = 0; j < 4; ++j) {
        float t = v[j];
        if (m != M && (m != 0.0f || M != 255.0f))
            t = (t - m) / (M - m) * 255.0f + 0.0f;
        else if (m == M)
            t = 0.0f;
        b[j] = is_nan_(t) ? (uint8_t)0 : (uint8_t)t;
    }
    if (((uintptr_t)out & 3u) == 0 && i + 3 < n) {
        *reinterpret_cast<uchar4*>(out + i) = make_uchar4(b[0], b[1], b[2], b[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (i + j < n) out[i + j] = b[j];
    }
}

__global__ __launch_bounds__(kPostBlock) void powf_kernel(const float* __restrict__ x, float y, float* __restrict__ out,
                                                          long long n) {
    const long long i = (long long)blockIdx.x * kPostBlock + threadIdx.x;
    if (i < n) out[i] = powf_(x[i], y);
}

// ---------------------------------------------------------- display statistics
// ipt_display_stats_device (ABI 7 additions): Gui::updateDisplay's histogram
// window (gui.cpp:83-88, CImg get_histogram) and a white point chosen by rank
// (normalize()'s kth_smallest remedy, gui.cpp:13) beside the max fold. Every
// count is an integer, so no result depends on the order of the atomics, and
// the control values (mx, mx/100000, the radix prefix, the remaining rank and
// the white point) stay in StatsScalars between the kernels.
//
// Both histograms are privatised: a workgroup counts into LDS and flushes its
// non-empty bins with one global atomic each; the grid is a multiple of the
// CU count, not of n. The LDS atomics are issued per lane: a constant image,
// where all 64 lanes of a wave hit one address, costs 10-15 % more than a
// render, and combining equal bins within the wave first (ballot on the first
// live lane's bin) changed neither by more than the run-to-run spread
// (DESIGN.md 4.8), so there is none.
//
// Rank selection: radix select on the order-preserving key (-0 before +0, NaN
// of either sign above +inf), most significant digit first, kSelPasses digits
// of kSelBits[] bits. Per pass: select_hist_kernel counts the digit of the
// elements that match the prefix so far, select_scan_kernel (one workgroup)
// finds the digit that holds the remaining rank and extends the prefix.
constexpr int kSelPasses = 3;  // (four 8-bit passes measured 8-12 % slower: two more launches)
constexpr int kSelBits[kSelPasses] = {11, 11, 10};
constexpr int kSelDigits = 2048;      // counts per pass (the widest digit)
constexpr int kHistMaxBuckets = 4096;  // 16 KiB of LDS
constexpr int kStatsBlocksPerCu = 8;

struct StatsScalars {
    float mx, lo, white;
    unsigned int prefix;     // the selected key's digits so far, in place
    unsigned int remaining;  // rank among the elements that match the prefix
    unsigned int pad[3];
    unsigned int digits[kSelPasses][kSelDigits];
};

// order-preserving key of the selection (ipt_capi.h): unsigned order == the
// stated order of floats
__device__ __forceinline__ unsigned int sel_key_(float v) {
    const unsigned int u = f2u(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey_(unsigned int k) {
    if (k == 0xffffffffu) return u2f(0x7fc00000u);
    return u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ void lds_count_(unsigned int* lh, int b) {
    if (b >= 0) atomicAdd(&lh[b], 1u);
}

// mx from the max fold's key (as tone_kernel reads it), mx / 100000.0f, and the
// selection's start: rank k, or white = mx when no rank is selected
__global__ void stats_init_kernel(const float* __restrict__ in, const DisplayScalars* __restrict__ sc,
                                  StatsScalars* __restrict__ ss, unsigned int k, int have_max) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float mx = 0.0f;
    if (have_max) {
        const unsigned long long key = sc->max_key;
        const float first = in[0];
        mx = (is_nan_(first) || !key) ? first : in[0xffffffffu - (unsigned int)key];
    }
    ss->mx = mx;
    ss->lo = div_x86nan_(mx, 100000.0f);
    ss->white = mx;
    ss->prefix = 0u;
    ss->remaining = k;
}

// CImg get_histogram(nb, lo, mx) (CImg.h:33484-33495) in double
__global__ __launch_bounds__(kPostBlock) void bucket_hist_kernel(const float* __restrict__ in, long long n, int nb,
                                                                 const StatsScalars* __restrict__ ss,
                                                                 unsigned int* __restrict__ hist) {
    __shared__ unsigned int lh[kHistMaxBuckets];
    for (int b = threadIdx.x; b < nb; b += kPostBlock) lh[b] = 0u;
    __syncthreads();
    const float lo = ss->lo, mx = ss->mx;
    const bool lt = lo < mx;
    const double vmin = (double)(lt ? lo : mx), vmax = (double)(lt ? mx : lo);
    const double levels = (double)(unsigned int)nb, span = vmax - vmin;
    const bool vec = ((uintptr_t)in & 15u) == 0;
    const long long stride = (long long)gridDim.x * kPostBlock * 4;
    for (long long base = (long long)blockIdx.x * kPostBlock * 4; base < n; base += stride) {
        const long long i = base + (long long)threadIdx.x * 4;
        float v[4];
        load4_(in, i, n, vec, v);
        for (int j = 0; j < 4; ++j) {
            const double val = (double)v[j];
            int b = -1;
            if (i + j < n && val >= vmin && val <= vmax) {
                const unsigned int q = val == vmax ? (unsigned int)nb - 1u : (unsigned int)((val - vmin) * levels / span);
                b = q < (unsigned int)nb ? (int)q : -1;  // (q < nb always: val < vmax by an f32 ulp)
            }
            lds_count_(lh, b);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += kPostBlock) {
        const unsigned int c = lh[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

// one digit of the keys that match the prefix: bits [shift, shift + bits)
__global__ __launch_bounds__(kPostBlock) void select_hist_kernel(const float* __restrict__ in, long long n, int shift,
                                                                 int bits, const StatsScalars* __restrict__ ss,
                                                                 unsigned int* __restrict__ counts) {
    __shared__ unsigned int lh[kSelDigits];
    const int nd = 1 << bits;
    for (int d = threadIdx.x; d < nd; d += kPostBlock) lh[d] = 0u;
    __syncthreads();
    const unsigned int prefix = ss->prefix;
    const unsigned int above = shift + bits >= 32 ? 0u : ~0u << (shift + bits);
    const bool vec = ((uintptr_t)in & 15u) == 0;
    const long long stride = (long long)gridDim.x * kPostBlock * 4;
    for (long long base = (long long)blockIdx.x * kPostBlock * 4; base < n; base += stride) {
        const long long i = base + (long long)threadIdx.x * 4;
        float v[4];
        load4_(in, i, n, vec, v);
        for (int j = 0; j < 4; ++j) {
            const unsigned int key = sel_key_(v[j]);
            const bool hit = i + j < n && (key & above) == prefix;
            lds_count_(lh, hit ? (int)((key >> shift) & (unsigned int)(nd - 1)) : -1);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < nd; d += kPostBlock) {
        const unsigned int c = lh[d];
        if (c) atomicAdd(&counts[d], c);
    }
}

// one workgroup: the digit whose counts hold the remaining rank; last pass:
// the key is complete and the white point is its float
__global__ __launch_bounds__(kPostBlock) void select_scan_kernel(const unsigned int* __restrict__ counts, int shift,
                                                                 int bits, int last, StatsScalars* __restrict__ ss) {
    __shared__ unsigned int part[kPostBlock];
    const int nd = 1 << bits, per = (nd + kPostBlock - 1) / kPostBlock;
    const int lo = min((int)threadIdx.x * per, nd), hi = min(lo + per, nd);
    const unsigned int rank = ss->remaining, prefix = ss->prefix;
    unsigned int s = 0;
    for (int d = lo; d < hi; ++d) s += counts[d];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int acc = 0;
        for (int t = 0; t < kPostBlock; ++t) {
            const unsigned int v = part[t];
            part[t] = acc;
            acc += v;
        }
    }
    __syncthreads();
    unsigned int off = part[threadIdx.x];
    if (rank >= off && rank - off < s)  // exactly one thread: rank < the sum of all counts
        for (int d = lo; d < hi; ++d) {
            const unsigned int c = counts[d];
            if (rank - off < c) {
                const unsigned int key = prefix | ((unsigned int)d << shift);
                ss->prefix = key;
                ss->remaining = rank - off;
                if (last) ss->white = sel_unkey_(key);
                break;
            }
            off += c;
        }
}

// tone_kernel with the white point of StatsScalars in place of the max fold
__global__ __launch_bounds__(kPostBlock) void tone_white_kernel(const float* __restrict__ in, float* __restrict__ tone,
                                                                long long n, float p,
                                                                const StatsScalars* __restrict__ ss,
                                                                DisplayScalars* __restrict__ sc) {
    __shared__ unsigned int red[kPostWaves];
    const float white = ss->white;
    const long long i = ((long long)blockIdx.x * kPostBlock + threadIdx.x) * 4;
    float v[4];
    load4_(in, i, n, ((uintptr_t)in & 15u) == 0, v);
    unsigned int hi = 0u, lo_inv = 0u;
    for (int j = 0; j < 4; ++j) {
        const float w = powf_(div_x86nan_(v[j], white), p);
        v[j] = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
        if (i + j < n && !is_nan_(v[j])) {
            hi = max(hi, f2u(v[j]));
            lo_inv = max(lo_inv, ~f2u(v[j]));
        }
    }
    if (((uintptr_t)tone & 15u) == 0 && i + 3 < n) {
        *reinterpret_cast<float4*>(tone + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (i + j < n) tone[i + j] = v[j];
    }
    hi = block_max_(hi, red);
    lo_inv = block_max_(lo_inv, red);
    if (threadIdx.x == 0) {
        if (hi) atomicMax(&sc->tone_max, hi);
        if (lo_inv) atomicMax(&sc->tone_min_inv, lo_inv);
    }
}

__global__ void stats_out_kernel(const StatsScalars* __restrict__ ss, float* __restrict__ stats) {
    const unsigned int t = threadIdx.x;
    if (t < 4 && blockIdx.x == 0) stats[t] = t == 0 ? ss->mx : (t == 1 ? ss->lo : (t == 2 ? ss->white : 0.0f));
}

// ------------------------------------------------------------------ PGM path
// ipt_smooth_device / ipt_pgm_device (ABI 7 additions): main.cpp:291-309 on a
// plane that stays on the device, smooth(side) -> computeSmoothedMax(side) ->
// n_val -> bytes. Every maximum is a fold from 0 with `>`, i.e. the largest
// positive element (NaN never wins), so it is an integer max of bit patterns
// and does not depend on dispatch order. The maxima, the max_value n_val
// divides by and logf_(contrast) stay in PgmScalars between the kernels.
struct PgmScalars {
    unsigned int smooth_max;  // bits of smooth()'s max_value
    unsigned int window_max;  // bits of computeSmoothedMax()'s
    unsigned int fold_max;    // bits of the pixel_max plane's fold
    unsigned int pad;
    float max_value;     // the one n_val divides by (ipt_capi.h: the last stage that sets it)
    float log_contrast;  // logf_(contrast)
    float zero[2];
};
enum { kPgmMaxGiven = 0, kPgmMaxSmooth, kPgmMaxWindow, kPgmMaxFold };

// GridRenderPlane::max_value as PlaneIo::finish folds pixel_max: from 0, `v > max`
__global__ __launch_bounds__(kPostBlock) void fold_max_kernel(const float* __restrict__ in, long long n,
                                                              unsigned int* __restrict__ max_bits) {
    __shared__ unsigned int red[kPostWaves];
    const long long i = ((long long)blockIdx.x * kPostBlock + threadIdx.x) * 4;
    float v[4];
    load4_(in, i, n, ((uintptr_t)in & 15u) == 0, v);  // (0 past n: the fold's start)
    unsigned int m = 0u;
    for (int j = 0; j < 4; ++j) m = max(m, v[j] > 0.0f ? f2u(v[j]) : 0u);
    m = block_max_(m, red);
    if (threadIdx.x == 0 && m) atomicMax(max_bits, m);
}

__global__ void pgm_setup_kernel(PgmScalars* __restrict__ ps, int which, float given, float contrast,
                                 float* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float mx = which == kPgmMaxWindow   ? u2f(ps->window_max)
                     : which == kPgmMaxSmooth ? u2f(ps->smooth_max)
                     : which == kPgmMaxFold   ? u2f(ps->fold_max)
                                              : given;
    const float lc = logf_(contrast);
    ps->max_value = mx;
    ps->log_contrast = lc;
    if (stats) stats[0] = mx, stats[1] = lc, stats[2] = 0.0f, stats[3] = 0.0f;
}

// ipt::n_val (main.cpp:225-235). adj is in [1, contrast] or NaN after the two
// clamps (std::min / std::max: a NaN first argument stays); a NaN ends as
// byte 0 on the host (cvttss2si gives INT_MIN, then max(0, .)), stated here.
__device__ __forceinline__ uint8_t n_val_(float val, float mx, float contrast, float log_contrast, float gamma) {
    float adj = val * contrast / mx;
    adj = contrast < adj ? contrast : adj;
    adj = adj < 1.0f ? 1.0f : adj;
    if (is_nan_(adj)) return 0;
    float fn = logf_(adj) / log_contrast;
    fn = powf_(fn, gamma);
    const float t = 256.0f * fn;  // in [0, 256]: 0 <= fn <= 1
    const int n = (int)t;
    return (uint8_t)(n < 0 ? 0 : (n > 255 ? 255 : n));
}

__global__ __launch_bounds__(kPostBlock) void n_val_kernel(const float* __restrict__ in, uint8_t* __restrict__ out,
                                                           long long n, float contrast, float gamma,
                                                           const PgmScalars* __restrict__ ps) {
    const float mx = ps->max_value, lc = ps->log_contrast;
    const long long i = ((long long)blockIdx.x * kPostBlock + threadIdx.x) * 4;
    if (i >= n) return;
    float v[4];
    load4_(in, i, n, ((uintptr_t)in & 15u) == 0, v);
    uint8_t b[4];
    for (int j = 0; j < 4; ++j) b[j] = n_val_(v[j], mx, contrast, lc, gamma);
    if (((uintptr_t)out & 3u) == 0 && i + 3 < n) {
        *reinterpret_cast<uchar4*>(out + i) = make_uchar4(b[0], b[1], b[2], b[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (i + j < n) out[i + j] = b[j];
    }
}

__global__ __launch_bounds__(kPostBlock) void logf_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                          long long n) {
    const long long i = (long long)blockIdx.x * kPostBlock + threadIdx.x;
    if (i < n) out[i] = logf_(x[i]);
}

// ipt_adapt_device: the next sample mask from the plane's mean, counter and
// second moment, one thread per pixel, in f32 and with no contraction. Pixels
// from no_source on (the Grid map's row H-1, which no sample has as its
// nominal destination) get mask 0 and are counted nowhere. stats = {active,
// starved, nan, 0}: integer adds, one per wave and class, so the sums do not
// depend on the order of the waves.
__global__ __launch_bounds__(kPostBlock) void adapt_kernel(const float* __restrict__ pixels,
                                                           const uint32_t* __restrict__ counters,
                                                           const float* __restrict__ m2, uint8_t* __restrict__ mask,
                                                           long long n, long long no_source, uint32_t min_count,
                                                           float rel_tol, float abs_tol, uint32_t* stats) {
    const long long i = (long long)blockIdx.x * kPostBlock + threadIdx.x;
    bool active = false, starved = false, nan = false;
    if (i < n) {
        if (i < no_source) {
            const uint32_t c = counters[i];
            if (c < min_count) {
                active = starved = true;
            } else {
                const float nf = (float)c;
                const float e2 = div_(m2[i], nf * (nf - 1.0f));
                const float thr = rel_tol * fabsf(pixels[i]) + abs_tol;
                const float t2 = thr * thr;
                active = e2 > t2;
                nan = e2 != e2 || t2 != t2;
            }
        }
        mask[i] = active ? 1 : 0;
    }
    if (stats) {
        const bool cls[3] = {active, starved, nan};
        for (int k = 0; k < 3; ++k) {
            const unsigned int c = (unsigned int)__popcll(__ballot(cls[k]));
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&stats[k], c);
        }
    }
}

// ipt_reproject_device: the previous camera's planes resampled to the new
// frame's pixels (ipt_capi.h "temporal reprojection"), one thread per
// destination pixel, in f32 and with no contraction. A thread reads its own
// guide, projects its hit into the previous camera and gathers up to four
// taps of a guide and three plane values each; every tap's loads are issued
// before the first acceptance test (a tap outside the frame reads the
// thread's own pixel and is dropped), so that the four gathers are in flight
// together. One dword per load and store: the caller's planes may have any
// alignment a float has. stats = {reused, disoccluded, not_surface, 0}, added
// per wave by ballot as adapt_kernel's.
struct RpArgs {
    const float* pixels;
    const uint32_t* counters;
    const float* m2;
    const uint32_t* prev_guides;
    const uint32_t* cur_guides;
    float* out_pixels;
    uint32_t* out_counters;
    float* out_m2;
    uint32_t* stats;
    float pos[3], dir[3], right[3], up[3];  // the previous camera
    int W, H, gui;
    float sigma_z, normal_min;
    uint32_t max_count;
    long long n;
};

__device__ __forceinline__ float rp_dot_(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(kPostBlock) void reproject_kernel(const RpArgs r) {
    const long long i = (long long)blockIdx.x * kPostBlock + threadIdx.x;
    bool reused = false, disoccluded = false, not_surface = false;
    if (i < r.n) {
        const uint32_t* g = r.cur_guides + 8 * i;
        const float Px = u2f(g[0]), Py = u2f(g[1]), Pz = u2f(g[2]);
        const uint32_t kind = g[3];
        const float nx = u2f(g[4]), ny = u2f(g[5]), nz = u2f(g[6]);
        float mean = 0.0f, m2o = 0.0f;
        uint32_t co = 0;
        if ((kind & 3u) != 1u || !isfinite_(Px) || !isfinite_(Py) || !isfinite_(Pz)) {
            not_surface = true;
        } else {
            disoccluded = true;
            const int W = r.W, H = r.H;
            const float vx = Px - r.pos[0], vy = Py - r.pos[1], vz = Pz - r.pos[2];
            const float a = rp_dot_(vx, vy, vz, r.right[0], r.right[1], r.right[2]);
            const float b = rp_dot_(vx, vy, vz, r.up[0], r.up[1], r.up[2]);
            const float c = rp_dot_(vx, vy, vz, r.dir[0], r.dir[1], r.dir[2]);
            const float dd = rp_dot_(r.dir[0], r.dir[1], r.dir[2], r.dir[0], r.dir[1], r.dir[2]);
            const float t = div_(c, dd);
            const float fx = (div_(a, t) + 0.5f) * (float)W - 0.5f;
            const float fy = (div_(b, t) + 0.5f) * (float)H - 0.5f;
            if (t > 0.0f && fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const float tx = fx - x0f, ty = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                // the loads of all four taps, then the tests and the sums in tap order
                bool in[4];
                uint32_t kq[4], cq[4];
                float pq[4], mq[4], qp[4][3], qn[4][3];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int xs = x0 + (k & 1), rs = y0 + (k >> 1);
                    // the destination row whose nominal source row rs is (-1: none)
                    const int yq = (rs < 0 || rs >= H) ? -1
                                   : (r.gui ? H - 1 - rs : (H == 1 ? 0 : (rs <= H - 2 ? H - 2 - rs : -1)));
                    in[k] = yq >= 0 && xs >= 0 && xs < W;
                    const long long q = in[k] ? (long long)yq * W + xs : i;
                    const uint32_t* gq = r.prev_guides + 8 * q;
                    qp[k][0] = u2f(gq[0]); qp[k][1] = u2f(gq[1]); qp[k][2] = u2f(gq[2]);
                    kq[k] = gq[3];
                    qn[k][0] = u2f(gq[4]); qn[k][1] = u2f(gq[5]); qn[k][2] = u2f(gq[6]);
                    cq[k] = r.counters[q];
                    pq[k] = r.pixels[q];
                    mq[k] = r.m2[q];
                }
                float sw = 0.0f, sm = 0.0f, sv = 0.0f, sc = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float bw = ((k & 1) ? tx : 1.0f - tx) * ((k >> 1) ? ty : 1.0f - ty);
                    const float nf = (float)cq[k];
                    const float var = div_(mq[k], nf * (nf - 1.0f));
                    const float dn = rp_dot_(nx, ny, nz, qn[k][0], qn[k][1], qn[k][2]);
                    const float e = fabs_(rp_dot_(nx, ny, nz, qp[k][0] - Px, qp[k][1] - Py, qp[k][2] - Pz));
                    const bool ok = in[k] && (kq[k] & 3u) == 1u && cq[k] >= 2u && isfinite_(pq[k]) &&
                                    isfinite_(var) && dn >= r.normal_min && e <= r.sigma_z;
                    if (ok) {
                        const uint32_t cc = cq[k] < r.max_count ? cq[k] : r.max_count;
                        const float ccf = (float)cc;
                        const float ve = var * div_(nf, ccf);
                        sw += bw;
                        sm += bw * pq[k];
                        sv += (bw * bw) * ve;
                        sc += bw * ccf;
                    }
                }
                if (sw != 0.0f) {
                    mean = div_(sm, sw);
                    const float var = div_(sv, sw * sw);
                    const uint32_t cu = (uint32_t)div_(sc, sw);
                    co = cu < 2u ? 2u : (cu > r.max_count ? r.max_count : cu);
                    const float nf = (float)co;
                    m2o = var * (nf * (nf - 1.0f));
                    reused = true;
                    disoccluded = false;
                }
            }
        }
        r.out_pixels[i] = mean;
        r.out_counters[i] = co;
        r.out_m2[i] = m2o;
    }
    if (r.stats) {
        const bool cls[3] = {reused, disoccluded, not_surface};
        for (int k = 0; k < 3; ++k) {
            const unsigned int c = (unsigned int)__popcll(__ballot(cls[k]));
            if ((threadIdx.x & 63) == 0 && c) atomicAdd(&r.stats[k], c);
        }
    }
}

// ------------------------------------------------------------------ denoising
// ipt_guides_device's second half: the FULL preview kernel's per-sample kinds
// and hits of one pass, [H][W] in source order, into the guide plane in
// destination order under the plane's nominal row map. One thread per
// destination pixel; a row without a nominal source gets kind 0xff and zeros.
// (one dword per store: the caller's plane may have any alignment a float has)
__global__ __launch_bounds__(kPostBlock) void guide_scatter_kernel(const uint8_t* __restrict__ kinds,
                                                                   const float* __restrict__ hits,
                                                                   uint32_t* __restrict__ out, int W, int H, int gui,
                                                                   long long n) {
    const long long i = (long long)blockIdx.x * kPostBlock + threadIdx.x;
    if (i >= n) return;
    const int yd = (int)(i / W), xd = (int)(i - (long long)yd * W);
    const int ys = gui ? H - 1 - yd : (H == 1 ? 0 : (yd <= H - 2 ? H - 2 - yd : -1));
    uint32_t r[8] = {0, 0, 0, 0xffu, 0, 0, 0, 0};
    if (ys >= 0) {
        const long long u = (long long)ys * W + xd;
        const float* h = hits + 6 * u;
        r[0] = f2u(h[0]); r[1] = f2u(h[1]); r[2] = f2u(h[2]);
        r[3] = kinds[u];
        r[4] = f2u(h[3]); r[5] = f2u(h[4]); r[6] = f2u(h[5]);
    }
    uint32_t* o = out + 8 * i;
    for (int j = 0; j < 8; ++j) o[j] = r[j];
}

// The filter's per-pixel record, two float4 per pixel: {P, col}, {n, var}. A
// tap is two 16-byte loads. A pixel that does not take part carries zeros and
// the var bits kDnSkip, and a tap that finds them is skipped. No arithmetic
// produces these bits in a participating record: its col and var0 are finite,
// the NaNs of its P and n are made canonical here, so every NaN in flight is
// a canonical or quieted one, and a NaN var is stored canonical.
constexpr uint32_t kDnSkip = 0xffffffffu;
__device__ __forceinline__ float dn_canon_(float x) { return x != x ? u2f(0x7fc00000u) : x; }
__device__ __forceinline__ float dn_pos_(float x) { return x > 0.0f ? x : 0.0f; }  // max(x, 0), NaN gives 0

// var0 = m2 / (nf * (nf - 1)) where c >= 2, else 0 (ipt_adapt_device's e2)
__device__ __forceinline__ float dn_var0_(uint32_t c, float m2) {
    if (c < 2) return 0.0f;
    const float nf = (float)c;
    return div_(m2, nf * (nf - 1.0f));
}

__global__ __launch_bounds__(kPostBlock) void denoise_prepare_kernel(const float* __restrict__ pixels,
                                                                     const uint32_t* __restrict__ counters,
                                                                     const float* __restrict__ m2,
                                                                     const uint32_t* __restrict__ guides,
                                                                     float4* __restrict__ rec, long long n) {
    const long long i = (long long)blockIdx.x * kPostBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = counters[i];
    const float px = pixels[i];
    const float var0 = dn_var0_(c, m2[i]);
    const uint32_t* g = guides + 8 * i;
    const bool part = (g[3] & 3u) == 1u && c >= 2 && isfinite_(px) && isfinite_(var0);
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, u2f(kDnSkip));
    if (part) {
        a = make_float4(dn_canon_(u2f(g[0])), dn_canon_(u2f(g[1])), dn_canon_(u2f(g[2])), px);
        b = make_float4(dn_canon_(u2f(g[4])), dn_canon_(u2f(g[5])), dn_canon_(u2f(g[6])), var0);
    }
    rec[2 * i] = a;
    rec[2 * i + 1] = b;
}

// What one iteration hands over: the record planes, the frame, the step and,
// for the last iteration (LAST), the caller's planes.
struct DnArgs {
    const float4* in;
    float4* out_rec;
    int W, H, s, npow;
    float sigma_l, sigma_z;
    const uint32_t* pixels;  // LAST: bit copies of the pixels that take no part
    const uint32_t* counters;
    const float* m2;
    float* out;
    float* var_out;
};

constexpr int kDnTileW = 32, kDnTileH = 8;  // one workgroup's pixels (256 threads)

// one tap of the 5 x 5 kernel, in the contract's operation order
__device__ __forceinline__ void dn_tap_(const float4 a, const float4 b, const float4 qa, const float4 qb, float h,
                                        float den, float sigma_z, int npow, float& sw, float& sc, float& sv) {
    float wn = dn_pos_((b.x * qb.x + b.y * qb.y) + b.z * qb.z);
    for (int j = 0; j < npow; ++j) wn = wn * wn;
    const float dx = qa.x - a.x, dy = qa.y - a.y, dz = qa.z - a.z;
    const float e = fabs_((b.x * dx + b.y * dy) + b.z * dz);
    const float t = dn_pos_(1.0f - div_(e, sigma_z));
    const float wz = t * t;
    const float u = dn_pos_(1.0f - div_(fabs_(qa.w - a.w), den));
    const float wl = u * u;
    const float w = h * ((wn * wz) * wl);
    sw += w;
    sc += w * qa.w;
    sv += (w * w) * qb.w;
}

__device__ __forceinline__ float dn_hk_(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1 ? 0.25f : 0.0625f); }

// the centre's finish: the quotients, or the centre itself when no weight is left
__device__ __forceinline__ void dn_finish_(const float4 a, const float4 b, float sw, float sc, float sv, float& col,
                                           float& var) {
    col = a.w;
    var = b.w;
    if (!(sw == 0.0f)) {
        col = div_(sc, sw);
        var = dn_canon_(div_(sv, sw * sw));
    }
}

// the pixel's outputs: the next record, or with LAST the caller's planes
template <bool LAST>
__device__ __forceinline__ void dn_store_(const DnArgs& d, size_t i, const float4 a, const float4 b, bool part,
                                          float col, float var) {
    if (!LAST) {
        d.out_rec[2 * i] = make_float4(a.x, a.y, a.z, col);
        d.out_rec[2 * i + 1] = make_float4(b.x, b.y, b.z, var);
        return;
    }
    if (part) {
        d.out[i] = col;
        if (d.var_out) d.var_out[i] = var;
    } else {
        reinterpret_cast<uint32_t*>(d.out)[i] = d.pixels[i];
        if (d.var_out) d.var_out[i] = dn_var0_(d.counters[i], d.m2[i]);
    }
}

// Direct form: one thread per pixel, every tap gathered from the record plane
// (25 x 2 16-byte loads at stride s, 9 4-byte loads for the variance prefilter).
// (a one-dimensional grid of tiles_x * tiles_y workgroups: a frame may be 2^31 pixels tall)
template <bool LAST>
__global__ __launch_bounds__(kPostBlock) void denoise_direct_kernel(const DnArgs d, unsigned tiles_x) {
    const unsigned by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x = (int)(bx * kDnTileW + (threadIdx.x & (kDnTileW - 1)));
    const int y = (int)(by * kDnTileH + (threadIdx.x / kDnTileW));
    if (x >= d.W || y >= d.H) return;
    const size_t i = (size_t)y * d.W + x;
    const float4 a = d.in[2 * i], b = d.in[2 * i + 1];
    if (f2u(b.w) == kDnSkip) {
        dn_store_<LAST>(d, i, a, b, false, 0.0f, u2f(kDnSkip));
        return;
    }
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= d.H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= d.W) continue;
            const float vq = d.in[2 * ((size_t)yy * d.W + xx) + 1].w;
            if (f2u(vq) == kDnSkip) continue;
            const float g = (dx == 0 && dy == 0) ? 0.25f : ((dx == 0 || dy == 0) ? 0.125f : 0.0625f);
            gs += g * vq;
            gw += g;
        }
    }
    const float den = d.sigma_l * sqrt_(div_(gs, gw)) + 0x1p-20f;
    float sw = 0.0f, sc = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const long long yy = (long long)y + (long long)d.s * dy;
        if (yy < 0 || yy >= d.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const long long xx = (long long)x + (long long)d.s * dx;
            if (xx < 0 || xx >= d.W) continue;
            const size_t q = (size_t)yy * d.W + (size_t)xx;
            const float4 qb = d.in[2 * q + 1];
            if (f2u(qb.w) == kDnSkip) continue;
            const float4 qa = d.in[2 * q];
            dn_tap_(a, b, qa, qb, dn_hk_(dx) * dn_hk_(dy), den, d.sigma_z, d.npow, sw, sc, sv);
        }
    }
    float col, var;
    dn_finish_(a, b, sw, sc, sv, col, var);
    dn_store_<LAST>(d, i, a, b, true, col, var);
}

// Lattice-tiled form: a workgroup owns a 32 x 8 tile of the pixels congruent
// to (rx, ry) mod s, whose taps are the dense neighbours in that sub-lattice.
// It stages the tile and a halo of 2 in LDS (36 x 12 records, 13.5 KiB; a
// record outside the frame is staged as one that takes no part) and reads the
// 25 taps from there, in the same order. A one-dimensional grid: column index
// rx * tiles_x + tile column over min(s, W) residues, row index likewise over
// min(s, H). The variance prefilter's neighbours are at
// distance 1, outside the sub-lattice for s >= 2: read from global memory.
constexpr int kDnHalo = 2, kDnLdsW = kDnTileW + 2 * kDnHalo, kDnLdsH = kDnTileH + 2 * kDnHalo;
template <bool LAST>
__global__ __launch_bounds__(kPostBlock) void denoise_tiled_kernel(const DnArgs d, unsigned tiles_x, unsigned tiles_y,
                                                                   unsigned cols) {
    __shared__ float4 la[kDnLdsH * kDnLdsW], lb[kDnLdsH * kDnLdsW];
    const unsigned gy = blockIdx.x / cols, gx = blockIdx.x - gy * cols;
    const int rx = (int)(gx / tiles_x), ry = (int)(gy / tiles_y);
    // (64-bit: tile origin plus halo may pass 2^31 on a frame that long)
    const long long u0 = (long long)(gx - rx * tiles_x) * kDnTileW, v0 = (long long)(gy - ry * tiles_y) * kDnTileH;
    // (uniform: the whole workgroup leaves before the barrier)
    if ((long long)rx + (long long)d.s * u0 >= d.W || (long long)ry + (long long)d.s * v0 >= d.H) return;
    for (int k = threadIdx.x; k < kDnLdsH * kDnLdsW; k += kPostBlock) {
        const int lv = k / kDnLdsW, lu = k - lv * kDnLdsW;
        const long long xx = (long long)rx + (long long)d.s * (u0 + lu - kDnHalo);
        const long long yy = (long long)ry + (long long)d.s * (v0 + lv - kDnHalo);
        float4 qa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qb = make_float4(0.0f, 0.0f, 0.0f, u2f(kDnSkip));
        if (xx >= 0 && xx < d.W && yy >= 0 && yy < d.H) {
            const size_t q = (size_t)yy * d.W + (size_t)xx;
            qa = d.in[2 * q];
            qb = d.in[2 * q + 1];
        }
        la[k] = qa;
        lb[k] = qb;
    }
    __syncthreads();
    const int tu = threadIdx.x & (kDnTileW - 1), tv = threadIdx.x / kDnTileW;
    const long long xl = (long long)rx + (long long)d.s * (u0 + tu), yl = (long long)ry + (long long)d.s * (v0 + tv);
    if (xl >= d.W || yl >= d.H) return;
    const int x = (int)xl, y = (int)yl;
    const size_t i = (size_t)y * d.W + x;
    const int lc = (tv + kDnHalo) * kDnLdsW + tu + kDnHalo;
    const float4 a = la[lc], b = lb[lc];
    if (f2u(b.w) == kDnSkip) {
        dn_store_<LAST>(d, i, a, b, false, 0.0f, u2f(kDnSkip));
        return;
    }
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= d.H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= d.W) continue;
            const float vq = d.in[2 * ((size_t)yy * d.W + xx) + 1].w;
            if (f2u(vq) == kDnSkip) continue;
            const float g = (dx == 0 && dy == 0) ? 0.25f : ((dx == 0 || dy == 0) ? 0.125f : 0.0625f);
            gs += g * vq;
            gw += g;
        }
    }
    const float den = d.sigma_l * sqrt_(div_(gs, gw)) + 0x1p-20f;
    float sw = 0.0f, sc = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int lq = lc + dy * kDnLdsW + dx;
            const float4 qb = lb[lq];
            if (f2u(qb.w) == kDnSkip) continue;
            dn_tap_(a, b, la[lq], qb, dn_hk_(dx) * dn_hk_(dy), den, d.sigma_z, d.npow, sw, sc, sv);
        }
    }
    float col, var;
    dn_finish_(a, b, sw, sc, sv, col, var);
    dn_store_<LAST>(d, i, a, b, true, col, var);
}

// powf_'s stated domain for y (ipt_math.h)
bool powf_y_ok(float y) { return isfinite_(y) && y > 0.0f && y != std::trunc(y); }

using ipt_internal::PostScratch;
using ipt_internal::ScratchBuf;

#define POSTCHECK(ctx, expr)                                                                            \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return ipt_internal::ctx_fail(ctx, IPT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// grids: one thread per element, four elements per thread
unsigned int blocks_for(long long n) { return (unsigned int)((n + kPostBlock - 1) / kPostBlock); }
unsigned int quads_for(long long n) { return (unsigned int)((n + 4ll * kPostBlock - 1) / (4ll * kPostBlock)); }

// the frame rules the two display entry points share, under `name`'s prefix
// (the caller has tested ctx and the pointers)
int frame_check(ipt_ctx* ctx, const char* name, int W, int H, float glare_cutoff, uint32_t flags) {
    const std::string pre = std::string(name) + ": ";
    if (W <= 0 || H <= 0 || !(glare_cutoff >= 0.0f))
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, pre + "bad arguments");
    if (glare_cutoff > 0.0f && (W > 4096 || H > 4096))  // ipt_glare's limit (the hypot equivalence)
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED, pre + "glare on images up to 4096 x 4096");
    if ((long long)W * H > (1ll << 31) || flags != 0 || !isfinite_(glare_cutoff))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED, pre + "at most 2^31 pixels, finite cutoff, flags 0");
    return IPT_OK;
}

// the argument rules of ipt_display / ipt_display_device (ipt_capi.h)
int display_check(ipt_ctx* ctx, const ipt_display_params* p, const float* pixels, const uint8_t* gray8) {
    if (!ctx) return IPT_E_INVALID;
    if (!p || !pixels || !gray8) return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_display: bad arguments");
    return frame_check(ctx, "ipt_display", p->width, p->height, p->glare_cutoff, p->flags);
}

// the argument rules of ipt_display_stats / ipt_display_stats_device:
// display_check's (no output is mandatory here) and the histogram's
int stats_check(ipt_ctx* ctx, const ipt_display_stats_params* p, const float* pixels, const uint32_t* hist) {
    if (!ctx) return IPT_E_INVALID;
    if (!p || !pixels || p->hist_buckets < 0 || p->hist_buckets > kHistMaxBuckets || (p->hist_buckets > 0 && !hist))
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_display_stats: bad arguments");
    return frame_check(ctx, "ipt_display_stats", p->width, p->height, p->glare_cutoff, p->flags);
}

// [a, a + na) and [b, b + nb) share a byte (a NULL range shares none)
bool overlap_(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}

// some pair of the n buffers overlaps, the pairs among the inputs (those before
// first_output) apart
bool any_overlap(const void* const* bufs, const size_t* lens, int n, int first_output) {
    for (int a = 0; a < n; ++a)
        for (int b = std::max(a + 1, first_output); b < n; ++b)
            if (overlap_(bufs[a], lens[a], bufs[b], lens[b])) return true;
    return false;
}

constexpr int kSmoothMaxSide = 64;  // 64^2 adds per pixel bound a queued kernel

// the side rules of ipt_smooth_device / ipt_pgm_device, after the INVALID ones
bool side_unsupported_(int side) { return side == 1 || side > kSmoothMaxSide; }

// the argument rules of ipt_smooth_device (ipt_capi.h)
int smooth_check(ipt_ctx* ctx, const float* in, const float* out, int width, int height, int side, const float* mx) {
    if (!ctx) return IPT_E_INVALID;
    if (!in || width <= 0 || height <= 0 || side < 0)
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_smooth_device: bad arguments");
    const size_t bytes = (size_t)width * (size_t)height * sizeof(float);
    if ((out != in && overlap_(in, bytes, out, bytes)) || overlap_(in, bytes, mx, sizeof(float)) ||
        overlap_(out, bytes, mx, sizeof(float)))
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_smooth_device: the buffers overlap");
    if (side_unsupported_(side) || (long long)width * height > (1ll << 31))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED,
                                      "ipt_smooth_device: side 0 or 2..64 (1 is undefined behaviour in the "
                                      "reference), at most 2^31 pixels");
    return IPT_OK;
}

// the argument rules of ipt_pgm / ipt_pgm_device (ipt_capi.h)
int pgm_check(ipt_ctx* ctx, const ipt_pgm_params* p, const float* pixels, const float* pixel_max,
              const float* smoothed, const uint8_t* gray8, const float* stats) {
    if (!ctx) return IPT_E_INVALID;
    if (!p || !pixels || p->width <= 0 || p->height <= 0 || p->smooth_side < 0 || p->max_side < 0)
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_pgm: bad arguments");
    const size_t n = (size_t)p->width * (size_t)p->height;
    const void* buf[5] = {pixels, pixel_max, smoothed, gray8, stats};
    const size_t len[5] = {n * sizeof(float), n * sizeof(float), n * sizeof(float), n, 4 * sizeof(float)};
    if (any_overlap(buf, len, 5, 2))  // every pair but the two inputs
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_pgm: the buffers overlap");
    if (side_unsupported_(p->smooth_side) || side_unsupported_(p->max_side) || p->flags != 0 ||
        (long long)p->width * p->height > (1ll << 31))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED,
                                      "ipt_pgm: sides 0 or 2..64, flags 0, at most 2^31 pixels");
    if (!isfinite_(p->contrast) || !(p->contrast > 1.0f) || !powf_y_ok(p->gamma))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED,
                                      "ipt_pgm: contrast finite and > 1, gamma finite, > 0 and no integer");
    return IPT_OK;
}

// the argument rules of ipt_denoise / ipt_denoise_device (ipt_capi.h)
int denoise_check(ipt_ctx* ctx, const ipt_denoise_params* p, const float* pixels, const uint32_t* counters,
                  const float* m2, const ipt_guide* guides, const float* out, const float* var_out) {
    if (!ctx) return IPT_E_INVALID;
    if (!p || !pixels || !counters || !m2 || !guides || !out || p->width <= 0 || p->height <= 0 ||
        p->iterations < 1 || p->iterations > 6 || p->normal_pow < 0 || p->normal_pow > 7 || !(p->sigma_l > 0.0f) ||
        !(p->sigma_z > 0.0f))
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID,
                                      "ipt_denoise: bad arguments (iterations 1..6, normal_pow 0..7, sigmas > 0)");
    if ((long long)p->width * p->height > (1ll << 31))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED, "ipt_denoise: at most 2^31 pixels");
    const size_t n = (size_t)p->width * (size_t)p->height;
    const void* buf[6] = {pixels, counters, m2, guides, out, var_out};
    const size_t len[6] = {n * 4, n * 4, n * 4, n * sizeof(ipt_guide), n * 4, n * 4};
    if (any_overlap(buf, len, 6, 4))  // every pair with an output in it
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_denoise: an output overlaps another buffer");
    return IPT_OK;
}

// the argument rules of ipt_reproject / ipt_reproject_device (ipt_capi.h)
int reproject_check(ipt_ctx* ctx, const ipt_reproject_params* p, const float* pixels, const uint32_t* counters,
                    const float* m2, const ipt_guide* prev_guides, const ipt_guide* cur_guides, const float* out_pixels,
                    const uint32_t* out_counters, const float* out_m2, const uint32_t* stats) {
    if (!ctx) return IPT_E_INVALID;
    if (!p || !pixels || !counters || !m2 || !prev_guides || !cur_guides || !out_pixels || !out_counters || !out_m2 ||
        p->width <= 0 || p->height <= 0 || !(p->sigma_z > 0.0f) || p->normal_min != p->normal_min ||
        p->max_count < 2u || p->max_count > (1u << 24))
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID,
                                      "ipt_reproject: bad arguments (sigma_z > 0, normal_min no NaN, max_count 2..1<<24)");
    if ((p->flags & ~(uint32_t)IPT_FLAG_GUI_PLANE) != 0 || (long long)p->width * p->height > (1ll << 31))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED,
                                      "ipt_reproject: IPT_FLAG_GUI_PLANE alone, at most 2^31 pixels");
    const size_t n = (size_t)p->width * (size_t)p->height;
    const void* buf[9] = {pixels, counters, m2, prev_guides, cur_guides, out_pixels, out_counters, out_m2, stats};
    const size_t len[9] = {n * 4, n * 4, n * 4, n * sizeof(ipt_guide), n * sizeof(ipt_guide), n * 4, n * 4, n * 4, 16};
    if (any_overlap(buf, len, 9, 5))  // every pair with an output in it
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_reproject: an output overlaps another buffer");
    return IPT_OK;
}

// Which tap-loop form an iteration runs. IPT_DENOISE_FORM=direct / tiled
// (diagnostics, the A/B of scripts/denoise_bench.py) forces one for every
// step; otherwise the measured choice (DESIGN.md "Denoising").
constexpr int kDnAuto = 0, kDnDirect = 1, kDnTiled = 2;
constexpr int kDnTiledMaxStep = 8;  // auto: steps up to here run the tiled form, larger ones the direct form
int denoise_form() {
    const char* e = std::getenv("IPT_DENOISE_FORM");
    if (!e) return kDnAuto;
    return std::strcmp(e, "direct") == 0 ? kDnDirect : (std::strcmp(e, "tiled") == 0 ? kDnTiled : kDnAuto);
}
struct DnRecord {
    float4 a, b;
};

// ---- the queued-call protocol ------------------------------------------------
// Every queued entry point is: check the arguments (before any HIP call), say
// what it needs of the context's scratch, post_begin, its memsets and launches
// on the stream post_begin chose, post_queued.

// what a call needs of each scratch buffer, in elements (0: not used)
struct PostNeeds {
    size_t n[PostScratch::kBufs] = {};
};

// the buffers' element sizes; kDenoise holds both planes' records of a pixel
constexpr size_t kPostElem[PostScratch::kBufs] = {sizeof(DisplayScalars), sizeof(StatsScalars), sizeof(PgmScalars),
                                                  sizeof(Bright),         sizeof(unsigned int), sizeof(float),
                                                  sizeof(float),          2 * sizeof(DnRecord)};

template <class T>
T* scratch(PostScratch& S, PostScratch::Buf b) {
    return static_cast<T*>(S.buf[b].p);
}

// (Re)allocates a scratch buffer: the old one is dropped first, and a failure
// leaves a null pointer with capacity 0, so that the next call tries again.
int post_grow(ipt_ctx* ctx, ScratchBuf& b, size_t count, size_t elem_bytes) {
    if (b.p) (void)hipFree(b.p);
    b = ScratchBuf{};
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, count * elem_bytes);
    if (e != hipSuccess)
        return ipt_internal::ctx_fail(ctx, e == hipErrorOutOfMemory ? IPT_E_OOM : IPT_E_DEVICE,
                                      std::string("display scratch: ") + hipGetErrorString(e));
    b = ScratchBuf{q, count, elem_bytes};
    return IPT_OK;
}

// Picks the stream (*st: the caller's, or the context's), makes the scratch
// hold what the call needs and orders the call behind the previous one. Only
// the first call or a larger frame allocates or waits on the host.
int post_begin(ipt_ctx* ctx, void* hip_stream, const PostNeeds& needs, hipStream_t* st) {
    (void)hipSetDevice(ipt_internal::ctx_device(ctx));
    *st = hip_stream ? (hipStream_t)hip_stream : ipt_internal::ctx_stream(ctx);
    PostScratch& S = ipt_internal::ctx_post(ctx);
    bool grow = !S.done;
    for (int b = 0; b < PostScratch::kBufs; ++b) grow |= needs.n[b] > S.buf[b].cap;
    if (grow) {
        if (const int rc = ipt_internal::post_wait(ctx)) return rc;
        if (!S.done) POSTCHECK(ctx, hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
        for (int b = 0; b < PostScratch::kBufs; ++b)  // (in the enum's order)
            if (needs.n[b] > S.buf[b].cap)
                if (const int rc = post_grow(ctx, S.buf[b], needs.n[b], kPostElem[b])) return rc;
    }
    // the scratch is shared: a call on another stream runs after the previous one
    if (S.used && S.last_stream != *st) POSTCHECK(ctx, hipStreamWaitEvent(*st, S.done, 0));
    return IPT_OK;
}

// after the call's last launch: the event the next call and the context's drain wait for
int post_queued(ipt_ctx* ctx, hipStream_t st) {
    PostScratch& S = ipt_internal::ctx_post(ctx);
    POSTCHECK(ctx, hipGetLastError());
    POSTCHECK(ctx, hipEventRecord(S.done, st));
    S.used = true;
    S.last_stream = st;
    return IPT_OK;
}

// smooth(side) moves some pixel (side 0, or larger than the image: none qualifies)
bool smooth_filters(int W, int H, int side) { return side >= 2 && side <= W && side <= H; }

// smooth(side) of `in` into `out` (the whole plane; NULL: the maximum alone),
// max_value's bits into *max_bits (zeroed by the caller). in != out.
// Where no pixel qualifies the plane is copied and the maximum stays 0.
hipError_t launch_smooth(hipStream_t st, const float* in, float* out, int W, int H, int side,
                         unsigned int* max_bits) {
    if (!smooth_filters(W, H, side))
        return out ? hipMemcpyAsync(out, in, (size_t)W * H * sizeof(float), hipMemcpyDeviceToDevice, st) : hipSuccess;
    dim3 grid(blocks_for(W), H);
    if (out)
        hipLaunchKernelGGL(smooth_kernel<true>, grid, dim3(kPostBlock), 0, st, in, out, W, H, side, max_bits);
    else
        hipLaunchKernelGGL(smooth_kernel<false>, grid, dim3(kPostBlock), 0, st, in, out, W, H, side, max_bits);
    return hipSuccess;
}

// what a glare stage on n pixels needs of the scratch
void glare_needs(PostNeeds& need, long long n, bool own_plane) {
    need.n[PostScratch::kBright] = (size_t)n;
    need.n[PostScratch::kBlocks] = (size_t)((n + kCompactSpan - 1) / kCompactSpan);
    need.n[PostScratch::kProcessed] = own_plane ? (size_t)n : 0;
}

// The glare stage of the two display entry points (`run`: bright count, scan,
// scatter, glare, into dev_processed or the context's plane), or the copy a
// caller's dev_processed gets without one. *plane: what the later stages read.
hipError_t queue_glare(hipStream_t st, PostScratch& S, DisplayScalars* sc, const float* dev_pixels,
                       float* dev_processed, int W, int H, float cutoff, bool run, const float** plane) {
    const long long n = (long long)W * H;
    *plane = dev_pixels;
    if (!run && !dev_processed) return hipSuccess;
    if (!run) return hipMemcpyAsync(dev_processed, dev_pixels, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st);
    Bright* bright = scratch<Bright>(S, PostScratch::kBright);
    unsigned int* blocks = scratch<unsigned int>(S, PostScratch::kBlocks);
    float* out = dev_processed ? dev_processed : scratch<float>(S, PostScratch::kProcessed);
    const unsigned int nblk = (unsigned int)((n + kCompactSpan - 1) / kCompactSpan);
    hipLaunchKernelGGL(bright_count_kernel, dim3(nblk), dim3(kPostBlock), 0, st, dev_pixels, n, cutoff, blocks);
    hipLaunchKernelGGL(bright_scan_kernel, dim3(1), dim3(kPostBlock), 0, st, blocks, (int)nblk, sc);
    hipLaunchKernelGGL(bright_scatter_kernel, dim3(nblk), dim3(kPostBlock), 0, st, dev_pixels, W, n, cutoff,
                       (const unsigned int*)blocks, bright);
    hipLaunchKernelGGL(glare_kernel, dim3(blocks_for(W), H), dim3(kPostBlock), 0, st, dev_pixels, out, W, H,
                       (const Bright*)bright, 0, cutoff, (const unsigned int*)&sc->nb);
    *plane = out;
    return hipSuccess;
}

// tone_map's exponent (gui.cpp:11-16)
float tone_gamma() {
    const float inv_gamma = 2.2f;
    return (float)(double)(1.0f / inv_gamma);
}

// ---- host round trips ----------------------------------------------------------
// A host wrapper's device temporaries on the context's stream: in() allocates
// and uploads, out() allocates and remembers the download (at_least: elements
// to allocate where count may be 0), finish() queues the downloads in out()'s
// order and waits. A NULL host pointer gives NULL and no work. The first
// failure sticks (rc, with the context's message) and makes the later calls
// no-ops: a wrapper tests rc before it launches. The temporaries go with the
// stage, on every return path.
struct HostStage {
    struct Out {
        void* host;
        const void* dev;
        size_t bytes;
    };
    ipt_ctx* ctx;
    hipStream_t st;
    int rc = IPT_OK;
    std::vector<ipt_internal::DevBuf<void>> bufs;
    std::vector<Out> outs;

    explicit HostStage(ipt_ctx* c) : ctx(c), st(ipt_internal::ctx_stream(c)) {
        (void)hipSetDevice(ipt_internal::ctx_device(c));
    }
    void check(hipError_t e, const char* what) {
        if (e != hipSuccess && rc == IPT_OK)
            rc = ipt_internal::ctx_fail(ctx, IPT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    }
    void* scratch(size_t bytes) {
        bufs.emplace_back();
        if (rc == IPT_OK) check(hipMalloc(&bufs.back().p, bytes), "hipMalloc");
        return bufs.back().p;
    }
    template <class T>
    T* in(const T* host, size_t count, size_t at_least = 0) {
        T* p = host ? static_cast<T*>(scratch(std::max(count, at_least) * sizeof(T))) : nullptr;
        if (p) check(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, st), "hipMemcpyAsync (upload)");
        return p;
    }
    template <class T>
    T* out(T* host, size_t count, size_t at_least = 0) {
        T* p = host ? static_cast<T*>(scratch(std::max(count, at_least) * sizeof(T))) : nullptr;
        if (p) outs.push_back({host, p, count * sizeof(T)});
        return p;
    }
    int finish() {
        for (const Out& o : outs)
            if (rc == IPT_OK) check(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (download)");
        if (rc == IPT_OK) check(hipStreamSynchronize(st), "hipStreamSynchronize");
        return rc;
    }
};

// fn(lo, hi) over [0, n) on up to 16 threads, a contiguous range each
template <class Fn>
void parallel_for(int64_t n, Fn fn) {
    const int nt = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([=]() { fn(n * t / nt, n * (t + 1) / nt); });
    for (auto& t : th) t.join();
}

}  // namespace

extern "C" {

int ipt_smooth(ipt_ctx* ctx, float* pixels, int width, int height, int side, int in_place, float* max_value) {
    if (!ctx) return IPT_E_INVALID;
    if (!pixels || !max_value || width <= 0 || height <= 0 || side < 0 || side > 4096)
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_smooth: bad arguments");
    if (side == 1)  // GridRenderPlane.cpp:14: `y >= side-1` with size_t never fails, the loop runs past row 0
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED,
                                      "ipt_smooth: side 1 is undefined behaviour in the reference");
    HostStage hs(ctx);
    hipStream_t st = hs.st;
    const size_t n = (size_t)width * height;
    unsigned int mb = 0;
    const float* din = hs.in(pixels, n);
    unsigned int* dmax = hs.out(&mb, 1);
    float* dout = hs.out(in_place ? pixels : nullptr, n);
    if (hs.rc) return hs.rc;
    if (in_place) POSTCHECK(ctx, hipMemcpyAsync(dout, din, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    POSTCHECK(ctx, hipMemsetAsync(dmax, 0, sizeof(unsigned int), st));
    if (smooth_filters(width, height, side)) {  // (its own launch: side up to 4096 here, 64 in ipt_smooth_device)
        hipLaunchKernelGGL(smooth_kernel<false>, dim3(blocks_for(width), height), dim3(kPostBlock), 0, st, din, dout,
                           width, height, side, dmax);
        POSTCHECK(ctx, hipGetLastError());
    }
    if (const int rc = hs.finish()) return rc;
    *max_value = __builtin_bit_cast(float, mb);
    return IPT_OK;
}

int ipt_glare(ipt_ctx* ctx, const float* in, float* out, int width, int height, float cutoff) {
    if (!ctx) return IPT_E_INVALID;
    if (!in || !out || width <= 0 || height <= 0)
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_glare: bad arguments");
    if (width > 4096 || height > 4096)  // the hypot equivalence is proven for |dx|, |dy| < 4096
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED, "ipt_glare: images up to 4096 x 4096");
    // bright pixels in raster order (gui.cpp:40-47); `val <= cutoff` false for NaN too
    std::vector<Bright> b;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const float val = in[(size_t)y * width + x];
            if (val <= cutoff) continue;
            const float coef = (float)(0.1 * (double)val / (double)cutoff);
            b.push_back(Bright{x, y, cutoff * coef, 0});
        }
    const size_t n = (size_t)width * height;
    HostStage hs(ctx);
    const float* din = hs.in(in, n);
    float* dout = hs.out(out, n);
    const Bright* db = b.empty() ? static_cast<const Bright*>(hs.scratch(sizeof(Bright))) : hs.in(b.data(), b.size());
    if (hs.rc) return hs.rc;
    hipLaunchKernelGGL(glare_kernel, dim3(blocks_for(width), height), dim3(kPostBlock), 0, hs.st, din, dout, width,
                       height, db, (int)b.size(), cutoff, (const unsigned int*)nullptr);
    POSTCHECK(ctx, hipGetLastError());
    return hs.finish();
}

int ipt_display_device(ipt_ctx* ctx, const ipt_display_params* p, const float* dev_pixels, float* dev_processed,
                       float* dev_tone, uint8_t* dev_gray8, void* hip_stream) {
    if (const int rc = display_check(ctx, p, dev_pixels, dev_gray8)) return rc;
    const bool glare = p->glare_cutoff > 0.0f;
    const long long n = (long long)p->width * p->height;
    PostNeeds need;
    need.n[PostScratch::kScalars] = 1;
    if (glare) glare_needs(need, n, !dev_processed);
    need.n[PostScratch::kTone] = dev_tone ? 0 : (size_t)n;
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, need, &st)) return rc;
    PostScratch& S = ipt_internal::ctx_post(ctx);
    DisplayScalars* sc = scratch<DisplayScalars>(S, PostScratch::kScalars);
    POSTCHECK(ctx, hipMemsetAsync(sc, 0, sizeof(DisplayScalars), st));
    const float* processed;
    POSTCHECK(ctx, queue_glare(st, S, sc, dev_pixels, dev_processed, p->width, p->height, p->glare_cutoff, glare,
                               &processed));
    float* tone = dev_tone ? dev_tone : scratch<float>(S, PostScratch::kTone);
    const unsigned int quads = quads_for(n);
    hipLaunchKernelGGL(image_max_kernel, dim3(quads), dim3(kPostBlock), 0, st, processed, n, sc);
    hipLaunchKernelGGL(tone_kernel, dim3(quads), dim3(kPostBlock), 0, st, processed, tone, n, tone_gamma(), sc);
    hipLaunchKernelGGL(gray8_kernel, dim3(quads), dim3(kPostBlock), 0, st, (const float*)tone, dev_gray8, n,
                       (const DisplayScalars*)sc);
    return post_queued(ctx, st);
}

int ipt_display(ipt_ctx* ctx, const ipt_display_params* p, const float* pixels, float* processed, float* tone,
                uint8_t* gray8) {
    if (const int rc = display_check(ctx, p, pixels, gray8)) return rc;
    const size_t n = (size_t)p->width * p->height;
    HostStage hs(ctx);
    const float* din = hs.in(pixels, n);
    float* dproc = hs.out(processed, n);
    float* dtone = hs.out(tone, n);
    uint8_t* dgray = hs.out(gray8, n);
    if (hs.rc) return hs.rc;
    if (const int rc = ipt_display_device(ctx, p, din, dproc, dtone, dgray, hs.st)) return rc;
    return hs.finish();
}

int ipt_display_stats_device(ipt_ctx* ctx, const ipt_display_stats_params* p, const float* dev_pixels,
                             float* dev_processed, float* dev_tone, uint8_t* dev_gray8, uint32_t* dev_hist,
                             float* dev_stats, void* hip_stream) {
    if (const int rc = stats_check(ctx, p, dev_pixels, dev_hist)) return rc;
    const bool glare = p->glare_cutoff > 0.0f;
    const long long n = (long long)p->width * p->height;
    const int nb = p->hist_buckets;
    // what was asked for decides what runs
    const bool want_tone = dev_tone || dev_gray8;
    const bool select = p->white_rank >= 0 && p->white_rank < n && (want_tone || dev_stats);
    const bool want_max = nb > 0 || dev_stats || (want_tone && !select);
    const bool want_image = want_max || select || want_tone;  // the glare output is read at all
    const bool run_glare = glare && (want_image || dev_processed);
    PostNeeds need;
    need.n[PostScratch::kScalars] = need.n[PostScratch::kStats] = 1;
    if (run_glare) glare_needs(need, n, !dev_processed);
    need.n[PostScratch::kTone] = dev_gray8 && !dev_tone ? (size_t)n : 0;
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, need, &st)) return rc;
    PostScratch& S = ipt_internal::ctx_post(ctx);
    DisplayScalars* sc = scratch<DisplayScalars>(S, PostScratch::kScalars);
    StatsScalars* ss = scratch<StatsScalars>(S, PostScratch::kStats);
    POSTCHECK(ctx, hipMemsetAsync(sc, 0, sizeof(DisplayScalars), st));
    if (select) POSTCHECK(ctx, hipMemsetAsync(ss->digits, 0, sizeof(ss->digits[0]) * kSelPasses, st));
    if (nb > 0) POSTCHECK(ctx, hipMemsetAsync(dev_hist, 0, (size_t)nb * sizeof(uint32_t), st));
    const float* processed;
    POSTCHECK(ctx, queue_glare(st, S, sc, dev_pixels, dev_processed, p->width, p->height, p->glare_cutoff, run_glare,
                               &processed));
    const unsigned int quads = quads_for(n);
    // the histograms' grid follows the device, not the image
    const unsigned int hgrid = std::min<unsigned int>(quads, (unsigned)(std::max(ipt_internal::ctx_cus(ctx), 1) * kStatsBlocksPerCu));
    if (want_max) hipLaunchKernelGGL(image_max_kernel, dim3(quads), dim3(kPostBlock), 0, st, processed, n, sc);
    if (want_image)
        hipLaunchKernelGGL(stats_init_kernel, dim3(1), dim3(64), 0, st, processed, (const DisplayScalars*)sc, ss,
                           select ? (unsigned int)p->white_rank : 0u, want_max ? 1 : 0);
    if (nb > 0)
        hipLaunchKernelGGL(bucket_hist_kernel, dim3(hgrid), dim3(kPostBlock), 0, st, processed, n, nb,
                           (const StatsScalars*)ss, dev_hist);
    if (select)
        for (int pass = 0, shift = 32; pass < kSelPasses; ++pass) {
            shift -= kSelBits[pass];
            hipLaunchKernelGGL(select_hist_kernel, dim3(hgrid), dim3(kPostBlock), 0, st, processed, n, shift,
                               kSelBits[pass], (const StatsScalars*)ss, ss->digits[pass]);
            hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kPostBlock), 0, st,
                               (const unsigned int*)ss->digits[pass], shift, kSelBits[pass],
                               pass == kSelPasses - 1 ? 1 : 0, ss);
        }
    if (want_tone) {
        float* tone = dev_tone ? dev_tone : scratch<float>(S, PostScratch::kTone);
        hipLaunchKernelGGL(tone_white_kernel, dim3(quads), dim3(kPostBlock), 0, st, processed, tone, n, tone_gamma(),
                           (const StatsScalars*)ss, sc);
        if (dev_gray8)
            hipLaunchKernelGGL(gray8_kernel, dim3(quads), dim3(kPostBlock), 0, st, (const float*)tone, dev_gray8, n,
                               (const DisplayScalars*)sc);
    }
    if (dev_stats) hipLaunchKernelGGL(stats_out_kernel, dim3(1), dim3(64), 0, st, (const StatsScalars*)ss, dev_stats);
    return post_queued(ctx, st);
}

int ipt_display_stats(ipt_ctx* ctx, const ipt_display_stats_params* p, const float* pixels, float* processed,
                      float* tone, uint8_t* gray8, uint32_t* hist, float* stats) {
    if (const int rc = stats_check(ctx, p, pixels, hist)) return rc;
    const size_t n = (size_t)p->width * p->height, nb = (size_t)p->hist_buckets;
    HostStage hs(ctx);
    const float* din = hs.in(pixels, n);
    float* dproc = hs.out(processed, n);
    float* dtone = hs.out(tone, n);
    uint8_t* dgray = hs.out(gray8, n);
    uint32_t* dhist = hs.out(nb ? hist : nullptr, nb);  // (a buffer passed with hist_buckets 0 is not written)
    float* dstats = hs.out(stats, 4);
    if (hs.rc) return hs.rc;
    if (const int rc = ipt_display_stats_device(ctx, p, din, dproc, dtone, dgray, dhist, dstats, hs.st)) return rc;
    return hs.finish();
}

int ipt_smooth_device(ipt_ctx* ctx, const float* dev_in, float* dev_out, int width, int height, int side,
                      float* dev_max, void* hip_stream) {
    if (const int rc = smooth_check(ctx, dev_in, dev_out, width, height, side, dev_max)) return rc;
    const size_t n = (size_t)width * (size_t)height;
    const bool filters = smooth_filters(width, height, side);
    const bool in_place = dev_out == dev_in;
    PostNeeds need;
    need.n[PostScratch::kPgm] = 1;
    need.n[PostScratch::kProcessed] = in_place && filters ? n : 0;
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, need, &st)) return rc;
    PostScratch& S = ipt_internal::ctx_post(ctx);
    PgmScalars* ps = scratch<PgmScalars>(S, PostScratch::kPgm);
    POSTCHECK(ctx, hipMemsetAsync(ps, 0, sizeof(PgmScalars), st));
    if (in_place) {  // the filter reads the context's copy (nothing changes when no pixel qualifies)
        if (filters) {
            float* copy = scratch<float>(S, PostScratch::kProcessed);
            POSTCHECK(ctx, hipMemcpyAsync(copy, dev_in, n * sizeof(float), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(smooth_kernel<false>, dim3(blocks_for(width), height), dim3(kPostBlock), 0, st,
                               (const float*)copy, dev_out, width, height, side, &ps->smooth_max);
        }
    } else {
        POSTCHECK(ctx, launch_smooth(st, dev_in, dev_out, width, height, side, &ps->smooth_max));
    }
    if (dev_max) POSTCHECK(ctx, hipMemcpyAsync(dev_max, &ps->smooth_max, sizeof(float), hipMemcpyDeviceToDevice, st));
    return post_queued(ctx, st);
}

int ipt_pgm_device(ipt_ctx* ctx, const ipt_pgm_params* p, const float* dev_pixels, const float* dev_pixel_max,
                   float* dev_smoothed, uint8_t* dev_gray8, float* dev_stats, void* hip_stream) {
    if (const int rc = pgm_check(ctx, p, dev_pixels, dev_pixel_max, dev_smoothed, dev_gray8, dev_stats)) return rc;
    const int W = p->width, H = p->height;
    const long long n = (long long)W * H;
    const bool smooth = p->smooth_side >= 2, window = p->max_side >= 2;
    const int which = window ? kPgmMaxWindow : smooth ? kPgmMaxSmooth : dev_pixel_max ? kPgmMaxFold : kPgmMaxGiven;
    // a stage nobody reads is not run: smooth's pixels feed the bytes, the
    // window maximum and dev_smoothed, its maximum only rule 2
    const bool run_smooth = smooth && (dev_smoothed || dev_gray8 || window || dev_stats);
    PostNeeds need;
    need.n[PostScratch::kPgm] = 1;
    need.n[PostScratch::kProcessed] = run_smooth && !dev_smoothed ? (size_t)n : 0;
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, need, &st)) return rc;
    PostScratch& S = ipt_internal::ctx_post(ctx);
    PgmScalars* ps = scratch<PgmScalars>(S, PostScratch::kPgm);
    POSTCHECK(ctx, hipMemsetAsync(ps, 0, sizeof(PgmScalars), st));
    const float* plane = dev_pixels;  // the pixels n_val reads
    if (run_smooth) {
        float* out = dev_smoothed ? dev_smoothed : scratch<float>(S, PostScratch::kProcessed);
        POSTCHECK(ctx, launch_smooth(st, dev_pixels, out, W, H, p->smooth_side, &ps->smooth_max));
        plane = out;
    } else if (dev_smoothed) {
        POSTCHECK(ctx, hipMemcpyAsync(dev_smoothed, dev_pixels, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    const unsigned int quads = quads_for(n);
    if (dev_gray8 || dev_stats) {
        if (window) POSTCHECK(ctx, launch_smooth(st, plane, nullptr, W, H, p->max_side, &ps->window_max));
        if (which == kPgmMaxFold)
            hipLaunchKernelGGL(fold_max_kernel, dim3(quads), dim3(kPostBlock), 0, st, dev_pixel_max, n, &ps->fold_max);
        hipLaunchKernelGGL(pgm_setup_kernel, dim3(1), dim3(64), 0, st, ps, which, p->max_value, p->contrast, dev_stats);
    }
    if (dev_gray8)
        hipLaunchKernelGGL(n_val_kernel, dim3(quads), dim3(kPostBlock), 0, st, plane, dev_gray8, n, p->contrast,
                           p->gamma, (const PgmScalars*)ps);
    return post_queued(ctx, st);
}

int ipt_adapt_device(ipt_ctx* ctx, const ipt_adapt_params* p, const float* dev_pixels, const uint32_t* dev_counters,
                     const float* dev_m2, uint8_t* dev_mask, uint32_t* dev_stats, void* hip_stream) {
    if (!ctx) return IPT_E_INVALID;
    if (!p || !dev_pixels || !dev_counters || !dev_m2 || !dev_mask || p->width <= 0 || p->height <= 0 ||
        p->min_count < 2 || !(p->rel_tol >= 0.0f) || !(p->abs_tol >= 0.0f))
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID,
                                      "ipt_adapt_device: bad arguments (min_count >= 2, tolerances >= 0)");
    if ((p->flags & ~(uint32_t)IPT_FLAG_GUI_PLANE) != 0 || (long long)p->width * p->height > (1ll << 31))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED,
                                      "ipt_adapt_device: IPT_FLAG_GUI_PLANE alone, at most 2^31 pixels");
    const long long n = (long long)p->width * p->height;
    {
        const size_t len[5] = {(size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n, 16};
        const void* with_mask[4] = {dev_pixels, dev_counters, dev_m2, dev_mask};
        const void* with_stats[5] = {dev_pixels, dev_counters, dev_m2, nullptr, dev_stats};
        if (any_overlap(with_mask, len, 4, 3) || any_overlap(with_stats, len, 5, 3))
            return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_adapt_device: an output overlaps an input");
        if (overlap_(dev_mask, (size_t)n, dev_stats, 16))
            return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_adapt_device: the outputs overlap");
    }
    // (no scratch of its own: the event alone, so that the context's waits cover the call)
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, PostNeeds{}, &st)) return rc;
    // the Grid map's row H-1 (H >= 2) is no sample's nominal destination
    const bool gui = (p->flags & IPT_FLAG_GUI_PLANE) != 0;
    const long long no_source = (!gui && p->height >= 2) ? (long long)(p->height - 1) * p->width : n;
    if (dev_stats) POSTCHECK(ctx, hipMemsetAsync(dev_stats, 0, 4 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(adapt_kernel, dim3(blocks_for(n)), dim3(kPostBlock), 0, st, dev_pixels, dev_counters, dev_m2,
                       dev_mask, n, no_source, p->min_count, p->rel_tol, p->abs_tol, dev_stats);
    return post_queued(ctx, st);
}

int ipt_reproject_device(ipt_ctx* ctx, const ipt_reproject_params* p, const float* dev_prev_pixels,
                         const uint32_t* dev_prev_counters, const float* dev_prev_m2, const ipt_guide* dev_prev_guides,
                         const ipt_guide* dev_cur_guides, float* dev_out_pixels, uint32_t* dev_out_counters,
                         float* dev_out_m2, uint32_t* dev_stats, void* hip_stream) {
    if (const int rc = reproject_check(ctx, p, dev_prev_pixels, dev_prev_counters, dev_prev_m2, dev_prev_guides,
                                       dev_cur_guides, dev_out_pixels, dev_out_counters, dev_out_m2, dev_stats))
        return rc;
    // (no scratch of its own: the event alone, so that the context's waits cover the call)
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, PostNeeds{}, &st)) return rc;
    RpArgs a{};
    a.pixels = dev_prev_pixels;
    a.counters = dev_prev_counters;
    a.m2 = dev_prev_m2;
    a.prev_guides = reinterpret_cast<const uint32_t*>(dev_prev_guides);
    a.cur_guides = reinterpret_cast<const uint32_t*>(dev_cur_guides);
    a.out_pixels = dev_out_pixels;
    a.out_counters = dev_out_counters;
    a.out_m2 = dev_out_m2;
    a.stats = dev_stats;
    for (int k = 0; k < 3; ++k) {
        a.pos[k] = p->prev_camera.position[k];
        a.dir[k] = p->prev_camera.direction[k];
        a.right[k] = p->prev_camera.right[k];
        a.up[k] = p->prev_camera.up[k];
    }
    a.W = p->width;
    a.H = p->height;
    a.gui = (p->flags & IPT_FLAG_GUI_PLANE) != 0 ? 1 : 0;
    a.sigma_z = p->sigma_z;
    a.normal_min = p->normal_min;
    a.max_count = p->max_count;
    a.n = (long long)p->width * p->height;
    if (dev_stats) POSTCHECK(ctx, hipMemsetAsync(dev_stats, 0, 4 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(reproject_kernel, dim3(blocks_for(a.n)), dim3(kPostBlock), 0, st, a);
    return post_queued(ctx, st);
}

int ipt_reproject(ipt_ctx* ctx, const ipt_reproject_params* p, const float* prev_pixels, const uint32_t* prev_counters,
                  const float* prev_m2, const ipt_guide* prev_guides, const ipt_guide* cur_guides, float* out_pixels,
                  uint32_t* out_counters, float* out_m2, uint32_t* stats) {
    if (const int rc = reproject_check(ctx, p, prev_pixels, prev_counters, prev_m2, prev_guides, cur_guides, out_pixels,
                                       out_counters, out_m2, stats))
        return rc;
    const size_t n = (size_t)p->width * p->height;
    HostStage hs(ctx);
    const float* dpx = hs.in(prev_pixels, n);
    const uint32_t* dcnt = hs.in(prev_counters, n);
    const float* dm2 = hs.in(prev_m2, n);
    const ipt_guide* dpg = hs.in(prev_guides, n);
    const ipt_guide* dcg = hs.in(cur_guides, n);
    float* dopx = hs.out(out_pixels, n);
    uint32_t* docnt = hs.out(out_counters, n);
    float* dom2 = hs.out(out_m2, n);
    uint32_t* dst = hs.out(stats, 4);
    if (hs.rc) return hs.rc;
    if (const int rc = ipt_reproject_device(ctx, p, dpx, dcnt, dm2, dpg, dcg, dopx, docnt, dom2, dst, hs.st)) return rc;
    return hs.finish();
}

int ipt_denoise_device(ipt_ctx* ctx, const ipt_denoise_params* p, const float* dev_pixels, const uint32_t* dev_counters,
                       const float* dev_m2, const ipt_guide* dev_guides, float* dev_out, float* dev_var_out,
                       void* hip_stream) {
    if (const int rc = denoise_check(ctx, p, dev_pixels, dev_counters, dev_m2, dev_guides, dev_out, dev_var_out))
        return rc;
    const int W = p->width, H = p->height;
    const size_t n = (size_t)W * (size_t)H;
    PostNeeds need;
    need.n[PostScratch::kDenoise] = n;
    hipStream_t st;
    if (const int rc = post_begin(ctx, hip_stream, need, &st)) return rc;
    PostScratch& S = ipt_internal::ctx_post(ctx);
    // the two record planes, one after the other
    float4* rec[2] = {scratch<float4>(S, PostScratch::kDenoise),
                      scratch<float4>(S, PostScratch::kDenoise) + 2 * S.buf[PostScratch::kDenoise].cap};
    // (diagnostics: an event after every pass, read by ipt_denoise_pass_ms)
    const char* prof = std::getenv("IPT_DENOISE_PROFILE");
    const bool timed = prof && std::atoi(prof) != 0;
    S.denoise_timed = 0;
    if (timed) {
        for (hipEvent_t& e : S.denoise_ev)
            if (!e) POSTCHECK(ctx, hipEventCreate(&e));
        POSTCHECK(ctx, hipEventRecord(S.denoise_ev[0], st));
    }
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3(blocks_for((long long)n)), dim3(kPostBlock), 0, st, dev_pixels,
                       dev_counters, dev_m2, reinterpret_cast<const uint32_t*>(dev_guides), rec[0], (long long)n);
    if (timed) POSTCHECK(ctx, hipEventRecord(S.denoise_ev[1], st));
    const int form = denoise_form();
    for (int k = 0; k < p->iterations; ++k) {
        const bool last = k == p->iterations - 1;
        DnArgs d{};
        d.in = rec[k & 1];
        d.out_rec = rec[(k & 1) ^ 1];
        d.W = W;
        d.H = H;
        d.s = 1 << k;
        d.npow = p->normal_pow;
        d.sigma_l = p->sigma_l;
        d.sigma_z = p->sigma_z;
        d.pixels = reinterpret_cast<const uint32_t*>(dev_pixels);
        d.counters = dev_counters;
        d.m2 = dev_m2;
        d.out = dev_out;
        d.var_out = dev_var_out;
        if (form == kDnTiled || (form == kDnAuto && d.s <= kDnTiledMaxStep)) {
            // the sub-lattice of a residue has ceil(W / s) x ceil(H / s) pixels at most
            // (64-bit: W or H may be within a tile of 2^31)
            const unsigned tx = (unsigned)((((long long)W + d.s - 1) / d.s + kDnTileW - 1) / kDnTileW);
            const unsigned ty = (unsigned)((((long long)H + d.s - 1) / d.s + kDnTileH - 1) / kDnTileH);
            const unsigned cols = tx * (unsigned)std::min(d.s, W), rows = ty * (unsigned)std::min(d.s, H);
            if (last)
                hipLaunchKernelGGL(denoise_tiled_kernel<true>, dim3(cols * rows), dim3(kPostBlock), 0, st, d, tx, ty, cols);
            else
                hipLaunchKernelGGL(denoise_tiled_kernel<false>, dim3(cols * rows), dim3(kPostBlock), 0, st, d, tx, ty, cols);
        } else {
            const unsigned tx = (unsigned)(((long long)W + kDnTileW - 1) / kDnTileW);
            const unsigned ty = (unsigned)(((long long)H + kDnTileH - 1) / kDnTileH);
            if (last)
                hipLaunchKernelGGL(denoise_direct_kernel<true>, dim3(tx * ty), dim3(kPostBlock), 0, st, d, tx);
            else
                hipLaunchKernelGGL(denoise_direct_kernel<false>, dim3(tx * ty), dim3(kPostBlock), 0, st, d, tx);
        }
        if (timed) POSTCHECK(ctx, hipEventRecord(S.denoise_ev[2 + k], st));
    }
    if (timed) S.denoise_timed = p->iterations;
    return post_queued(ctx, st);
}

int ipt_denoise_pass_ms(ipt_ctx* ctx, float* ms) {
    if (!ctx) return IPT_E_INVALID;
    ipt_internal::PostScratch& S = ipt_internal::ctx_post(ctx);
    if (!ms || S.denoise_timed <= 0)
        return ipt_internal::ctx_fail(ctx, IPT_E_INVALID,
                                      "ipt_denoise_pass_ms: no ipt_denoise_device call under IPT_DENOISE_PROFILE=1");
    (void)hipSetDevice(ipt_internal::ctx_device(ctx));
    POSTCHECK(ctx, hipEventSynchronize(S.denoise_ev[1 + S.denoise_timed]));
    for (int k = 0; k < 7; ++k) ms[k] = 0.0f;
    for (int k = 0; k <= S.denoise_timed; ++k)
        POSTCHECK(ctx, hipEventElapsedTime(&ms[k], S.denoise_ev[k], S.denoise_ev[k + 1]));
    return IPT_OK;
}

int ipt_denoise(ipt_ctx* ctx, const ipt_denoise_params* p, const float* pixels, const uint32_t* counters,
                const float* m2, const ipt_guide* guides, float* out, float* var_out) {
    if (const int rc = denoise_check(ctx, p, pixels, counters, m2, guides, out, var_out)) return rc;
    const size_t n = (size_t)p->width * p->height;
    HostStage hs(ctx);
    const float* dpx = hs.in(pixels, n);
    const uint32_t* dcnt = hs.in(counters, n);
    const float* dm2 = hs.in(m2, n);
    const ipt_guide* dg = hs.in(guides, n);
    float* dout = hs.out(out, n);
    float* dvar = hs.out(var_out, n);
    if (hs.rc) return hs.rc;
    if (const int rc = ipt_denoise_device(ctx, p, dpx, dcnt, dm2, dg, dout, dvar, hs.st)) return rc;
    return hs.finish();
}

int ipt_pgm(ipt_ctx* ctx, const ipt_pgm_params* p, const float* pixels, const float* pixel_max, float* smoothed,
            uint8_t* gray8, float* stats) {
    if (const int rc = pgm_check(ctx, p, pixels, pixel_max, smoothed, gray8, stats)) return rc;
    const size_t n = (size_t)p->width * p->height;
    const bool need_fold = pixel_max && p->smooth_side < 2 && p->max_side < 2;  // the only rule that reads it
    HostStage hs(ctx);
    const float* din = hs.in(pixels, n);
    const float* dpmax = hs.in(need_fold ? pixel_max : nullptr, n);
    float* dsm = hs.out(smoothed, n);
    uint8_t* dgray = hs.out(gray8, n);
    float* dstats = hs.out(stats, 4);
    if (hs.rc) return hs.rc;
    if (const int rc = ipt_pgm_device(ctx, p, din, dpmax, dsm, dgray, dstats, hs.st)) return rc;
    return hs.finish();
}

int ipt_logf_host(const float* x, float* out, int64_t n) {
    if (!x || !out || n < 0) return IPT_E_INVALID;
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) out[i] = logf_(x[i]);
    });
    return IPT_OK;
}

int ipt_logf_device(ipt_ctx* ctx, const float* x, float* out, int64_t n) {
    if (!ctx) return IPT_E_INVALID;
    if (!x || !out || n < 0) return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_logf_device: bad arguments");
    HostStage hs(ctx);
    const float* din = hs.in(x, (size_t)n, 1);  // (at least one element: n may be 0)
    float* dout = hs.out(out, (size_t)n, 1);
    if (hs.rc) return hs.rc;
    if (n > 0)
        hipLaunchKernelGGL(logf_kernel, dim3(blocks_for(n)), dim3(kPostBlock), 0, hs.st, din, dout, (long long)n);
    POSTCHECK(ctx, hipGetLastError());
    return hs.finish();
}

int ipt_powf_host(const float* x, float y, float* out, int64_t n) {
    if (!x || !out || n < 0) return IPT_E_INVALID;
    if (!powf_y_ok(y)) return IPT_E_UNSUPPORTED;
    parallel_for(n, [=](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) out[i] = powf_(x[i], y);
    });
    return IPT_OK;
}

int ipt_powf_device(ipt_ctx* ctx, const float* x, float y, float* out, int64_t n) {
    if (!ctx) return IPT_E_INVALID;
    if (!x || !out || n < 0) return ipt_internal::ctx_fail(ctx, IPT_E_INVALID, "ipt_powf_device: bad arguments");
    if (!powf_y_ok(y))
        return ipt_internal::ctx_fail(ctx, IPT_E_UNSUPPORTED, "ipt_powf_device: y must be finite, > 0 and no integer");
    HostStage hs(ctx);
    const float* din = hs.in(x, (size_t)n, 1);  // (at least one element: n may be 0)
    float* dout = hs.out(out, (size_t)n, 1);
    if (hs.rc) return hs.rc;
    if (n > 0)
        hipLaunchKernelGGL(powf_kernel, dim3(blocks_for(n)), dim3(kPostBlock), 0, hs.st, din, y, dout,
                           (long long)n);
    POSTCHECK(ctx, hipGetLastError());
    return hs.finish();
}

}  // extern "C"

namespace ipt_internal {
int post_wait(ipt_ctx* ctx) {
    PostScratch& S = ctx_post(ctx);
    if (!S.used) return IPT_OK;
    S.used = false;
    const hipError_t e = hipEventSynchronize(S.done);
    if (e != hipSuccess) return ctx_fail(ctx, IPT_E_DEVICE, std::string("display work failed: ") + hipGetErrorString(e));
    return IPT_OK;
}

void post_release(ipt_ctx* ctx) {
    PostScratch& S = ctx_post(ctx);
    for (const ScratchBuf& b : S.buf)
        if (b.p) (void)hipFree(b.p);
    if (S.done) (void)hipEventDestroy(S.done);
    for (hipEvent_t e : S.denoise_ev)
        if (e) (void)hipEventDestroy(e);
    S = PostScratch{};
}

hipError_t launch_guide_scatter(hipStream_t st, const uint8_t* kinds, const float* hits, ipt_guide* dev_guides, int W,
                                int H, bool gui) {
    const long long n = (long long)W * H;
    hipLaunchKernelGGL(guide_scatter_kernel, dim3(blocks_for(n)), dim3(kPostBlock), 0, st, kinds, hits,
                       reinterpret_cast<uint32_t*>(dev_guides), W, H, gui ? 1 : 0, n);
    return hipGetLastError();
}
}  // namespace ipt_internal
