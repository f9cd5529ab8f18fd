// ipt_math.h — portable, bit-reproducible arithmetic for the ipt path tracer.
//
// Compiled by hipcc for BOTH the gfx950 device code and the host side of the
// product library (same source, same operation order, -ffp-contract=off), so
// a value computed on the GPU is bit-identical to the value the host side of
// the library computes for the exhaustive math tests.
//
// What it reproduces:
//  * glm 0.9.9.7 vec3/mat3 arithmetic in glm's operation order
//    (reference include/glm/detail/func_geometric.inl:8-90,
//     detail/type_mat3x3.inl:468-474, detail/func_matrix.inl:268-291,
//     ext/matrix_transform.inl:18-47).
//  * the libm functions the reference calls on its hot path, as shipped in the
//    image's glibc 2.35 (x86_64, FMA/AVX2 ifunc variants that the reference
//    binary binds to on any FMA-capable host):
//      acosf  -> fdlibm __ieee754_acosf   (float ops, no FMA)
//      sinf/cosf/sincosf -> ARM optimized-routines sinf/cosf (__sinf_fma,
//                 __cosf_fma: double-precision polynomial, FMA-contracted
//                 exactly where GCC contracted glibc's source)
//      (float)acos((double)x) -> fdlibm __ieee754_acos restated in double;
//                 only its rounding to float is used by the reference
//                 (libddf/ddf_detail.h:82) and that rounding is verified equal
//                 to glibc's for every float input in tests/.
//      powf  -> ARM optimized-routines powf (__powf_fma), for the display
//                 chain's gamma only (powf_ below; tests/test_display_cpu.py)
//      logf  -> ARM optimized-routines logf (__logf_fma), for the PGM chain's
//                 n_val only (logf_ below, x in [1, FLT_MAX]; tests/test_pgm_cpu.py)
//    Constants were read from the image's libm.so.6 .rodata and the operation
//    graphs from its disassembly; tests/test_math_exhaustive.py checks every
//    float input of each function's reachable domain against the host libm.
#pragma once

#include <stdint.h>

#ifndef IPT_HD
#define IPT_HD __host__ __device__ inline
#endif

namespace ipt {

// ---------------------------------------------------------------- bit casts
IPT_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
IPT_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
IPT_HD uint64_t d2u(double d) { return __builtin_bit_cast(uint64_t, d); }
IPT_HD double u2d(uint64_t u) { return __builtin_bit_cast(double, u); }

IPT_HD float fabs_(float x) { return u2f(f2u(x) & 0x7fffffffu); }
IPT_HD bool isfinite_(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
IPT_HD float inf_() { return u2f(0x7f800000u); }
IPT_HD double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
IPT_HD double sqrtd_(double x) { return __builtin_sqrt(x); }

// IEEE f32 sqrt and division: the device compiler's own sequences. (Wave-
// guarded variants that drop their range handling measured neutral (sqrt) and
// -12 % (division: the guard and its branch cost more than v_div_scale /
// v_div_fixup); the range-free cores below are used only where a host or
// algebraic proof bounds the operands.)
IPT_HD float sqrt_(float x) { return __builtin_sqrtf(x); }
IPT_HD float div_(float a, float b) { return a / b; }

// a/b without the range handling of the compiler's sequence (no v_div_scale /
// v_div_fmas / v_div_fixup): the reciprocal, one Newton step and ONE quotient
// residual step (round 5; two before). Bit-identical to a/b when |a| in
// [2^-40, 2^41) or a = +-0 (then a signed zero, whose sign the callers never
// observe) and |b| in [2^-40, 2^41). Why one residual step suffices: the
// Newton step makes y = RN(1/b) (exhaustively, fn 17 below), and with y the
// correctly rounded reciprocal and q0 = RN(a*y) within an ulp of a/b, q0 +
// y*RN(a - b*q0) (the residual exact by fma) is the correctly rounded quotient
// in the absence of over/underflow (Markstein's theorem for fma division).
// Device checks: ipt_math_selfcheck fn 10 (2^32 hashed pairs over the range)
// and fn 20 (2^32 pairs with divisors of all-ones-like significands, the
// theorem's hard case), 0 mismatches. Callers must guarantee the range.
IPT_HD float div_inrange_(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float y = __builtin_amdgcn_rcpf(b);
    y = __builtin_fmaf(__builtin_fmaf(-b, y, 1.0f), y, y);
    const float q0 = a * y;
    return __builtin_fmaf(__builtin_fmaf(-b, q0, a), y, q0);
#else
    return a / b;
#endif
}

// 1/b by the hardware reciprocal and Newton corrections: STEPS = 1 (y1) or 2
// (y2) of the corrections that the round-4 div_inrange_(1.0f, b) applied (y1,
// then q1 == y2, then q2). ipt_math_selfcheck fn 17 / 18 compare them with
// that three-correction sequence over all 2^32 floats: both are identical to
// it bit for bit everywhere (round 5, `profiles/round5_rcp_check.txt`), so
// rcp_inrange_ below takes one correction instead of three.
template <int STEPS>
IPT_HD float rcp_newton_(float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float y = __builtin_amdgcn_rcpf(b);
    y = __builtin_fmaf(__builtin_fmaf(-b, y, 1.0f), y, y);
    if (STEPS >= 2) y = __builtin_fmaf(__builtin_fmaf(-b, y, 1.0f), y, y);
    return y;
#else
    return 1.0f / b;
#endif
}
// == the three-correction 1.0f / b for every float b (exhaustive device check above)
IPT_HD float rcp_inrange_(float b) { return rcp_newton_<1>(b); }

// Correctly rounded sqrtf for x = +0 or in [2^-96, 2^126): the hardware root (within
// one ulp, no denormal scaling needed in this range) corrected by the signs of
// the residuals of its two neighbours (the sequence of the IEEE expansion
// without its range handling). Equal to sqrtf on every float of the range
// (exhaustive GPU check, math probe 13).
IPT_HD float sqrt_inrange_(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sd = u2f(f2u(s) - 1u), su = u2f(f2u(s) + 1u);
    const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
    const float s1 = rd <= 0.0f ? sd : s;
    return ru > 0.0f ? su : s1;
#else
    return __builtin_sqrtf(x);
#endif
}

// ------------------------------------------------------------------ vec3
// glm::vec3 with glm's component-wise operators; no FMA anywhere.
struct vec3 {
    float x, y, z;
};
IPT_HD vec3 v3(float x, float y, float z) { vec3 r; r.x = x; r.y = y; r.z = z; return r; }
IPT_HD vec3 operator+(vec3 a, vec3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
IPT_HD vec3 operator-(vec3 a, vec3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
IPT_HD vec3 operator-(vec3 a) { return v3(-a.x, -a.y, -a.z); }
IPT_HD vec3 operator*(vec3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
IPT_HD vec3 operator*(float s, vec3 a) { return v3(s * a.x, s * a.y, s * a.z); }
IPT_HD bool is_zero(vec3 a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }
// glm compute_dot<vec3>: tmp = a*b; tmp.x + tmp.y + tmp.z   (func_geometric.inl:48-55)
IPT_HD float dot(vec3 a, vec3 b) {
    float tx = a.x * b.x, ty = a.y * b.y, tz = a.z * b.z;
    return (tx + ty) + tz;
}
// glm compute_cross (func_geometric.inl:68-79)
IPT_HD vec3 cross(vec3 x, vec3 y) {
    return v3(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}
// glm length = sqrt(dot(v,v)) (func_geometric.inl:8-14)
IPT_HD float length(vec3 v) { return sqrt_(dot(v, v)); }
// glm normalize = v * inversesqrt(dot(v,v)), inversesqrt = 1/sqrt (func_exponential.inl:136-139)
IPT_HD vec3 normalize(vec3 v) {
    float s = div_(1.0f, sqrt_(dot(v, v)));
    return v * s;
}

// normalize for dot(v, v) in [2^-80, 2^80] (root in [2^-40, 2^40]): the same
// roundings as normalize() through the range-free root and quotient
IPT_HD vec3 normalize_inrange_(vec3 v) {
    const float s = rcp_inrange_(sqrt_inrange_(dot(v, v)));
    return v * s;
}

// column-major mat3, m[c][r] as glm
struct mat3 {
    vec3 c[3];
};
// glm mat3 * vec3 (type_mat3x3.inl:468-474): row i = (m0i*vx + m1i*vy) + m2i*vz
IPT_HD vec3 mul(const mat3& m, vec3 v) {
    return v3(m.c[0].x * v.x + m.c[1].x * v.y + m.c[2].x * v.z,
              m.c[0].y * v.x + m.c[1].y * v.y + m.c[2].y * v.z,
              m.c[0].z * v.x + m.c[1].z * v.y + m.c[2].z * v.z);
}
IPT_HD float el(const mat3& m, int c, int r) {
    const vec3& v = m.c[c];
    return r == 0 ? v.x : (r == 1 ? v.y : v.z);
}
// glm compute_inverse<3,3> (func_matrix.inl:268-291), cofactor / determinant
template <bool INRANGE = false>
IPT_HD mat3 inverse(const mat3& M) {
    const float m00 = M.c[0].x, m01 = M.c[0].y, m02 = M.c[0].z;
    const float m10 = M.c[1].x, m11 = M.c[1].y, m12 = M.c[1].z;
    const float m20 = M.c[2].x, m21 = M.c[2].y, m22 = M.c[2].z;
    float det = m00 * (m11 * m22 - m21 * m12);
    det = det - m10 * (m01 * m22 - m21 * m02);
    det = det + m20 * (m01 * m12 - m11 * m02);
    // glm writes "+ m00*(..) - m10*(..) + m20*(..)"; unary + is exact
    const float o = INRANGE ? rcp_inrange_(det) : div_(1.0f, det);  // INRANGE: det in [2^-40, 2^41)
    mat3 I;
    I.c[0].x = (m11 * m22 - m21 * m12) * o;
    I.c[1].x = -(m10 * m22 - m20 * m12) * o;
    I.c[2].x = (m10 * m21 - m20 * m11) * o;
    I.c[0].y = -(m01 * m22 - m21 * m02) * o;
    I.c[1].y = (m00 * m22 - m20 * m02) * o;
    I.c[2].y = -(m00 * m21 - m20 * m01) * o;
    I.c[0].z = (m01 * m12 - m11 * m02) * o;
    I.c[1].z = -(m00 * m12 - m10 * m02) * o;
    I.c[2].z = (m00 * m11 - m10 * m01) * o;
    return I;
}

// ------------------------------------------------------------------ acosf
// glibc 2.35 sysdeps/ieee754/flt-32/e_acosf.c (fdlibm), constants verified
// against libm.so.6 .rodata (0x9c958..0x9c98c).
// Branch-free over fdlibm's three argument ranges: every lane evaluates the
// exact operation sequence of its own branch (selects only pick results), so
// the value is the glibc one while a wave pays one division/sqrt chain, not
// three (the |x|<0.5 and x>0.5 ranges both occur within every wave).
IPT_HD float acosf_(float x) {
    const float one = 1.0f;
    const float pi = u2f(0x40490fdau);
    const float pio2_hi = u2f(0x3fc90fdau);
    const float pio2_lo = u2f(0x33a22168u);
    const float two_pio2_lo = u2f(0x34222168u);  // (float)2.0*pio2_lo, folded by GCC
    const float pS0 = u2f(0x3e2aaaabu), pS1 = -u2f(0x3ea6b090u), pS2 = u2f(0x3e4e0aa8u),
                pS3 = -u2f(0x3d241146u), pS4 = u2f(0x3a4f7f04u), pS5 = u2f(0x3811ef08u);
    const float qS1 = -u2f(0x4019d139u), qS2 = u2f(0x4001572du), qS3 = -u2f(0x3f303361u),
                qS4 = u2f(0x3d9dc62eu);
    const uint32_t hx = f2u(x);
    const uint32_t ix = hx & 0x7fffffffu;
    const bool small = ix < 0x3f000000u;  // |x| < 0.5
    const bool neg = (int32_t)hx < 0;     // x < -0.5 when !small
    const float z = small ? x * x : (neg ? (one + x) * 0.5f : (one - x) * 0.5f);
    const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const float r = div_(p, q);
    const float sq = sqrt_(z);
    const float r_small = pio2_hi - (x - (pio2_lo - x * r));
    const float r_neg = pi - 2.0f * (sq + (r * sq - pio2_lo));
    const float df = u2f(f2u(sq) & 0xfffff000u);
    const float c = div_(z - df * df, sq + df);
    const float r_pos = 2.0f * (df + (r * sq + c));
    float res = small ? r_small : (neg ? r_neg : r_pos);
    if (small && ix <= 0x32800000u) res = pio2_hi + pio2_lo;
    if (ix == 0x3f800000u) res = (int32_t)hx > 0 ? 0.0f : pi + two_pio2_lo;
    if (ix > 0x3f800000u) res = (x - x) * inf_();  // |x|>1 or NaN: NaN
    return res;
}

// ------------------------------------------------------------ sinf / cosf
// ARM optimized-routines single-precision sin/cos as built into glibc 2.35
// (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, sincosf.h) in its FMA ifunc
// variant. Table __sincosf_table read from libm .rodata 0xb30c0.
struct sincos_tab {
    double c0, c1, s1, c2, s2, c3, s3, c4;
};
IPT_HD sincos_tab sincos_table(int which) {
    sincos_tab t;
    const double sg = which ? -1.0 : 1.0;
    t.c0 = sg * 1.0;
    t.c1 = sg * u2d(0xbfdffffffd0c621cull);
    t.s1 = u2d(0xbfc555545995a603ull);
    t.c2 = sg * u2d(0x3fa55553e1068f19ull);
    t.s2 = u2d(0x3f81107605230bc4ull);
    t.c3 = sg * u2d(0xbf56c087e89a359dull);
    t.s3 = u2d(0xbf2994eb3774cf24ull);
    t.c4 = sg * u2d(0x3ef99343027bf8c3ull);
    return t;
}
IPT_HD double sincos_sign(int q) { return (q == 1 || q == 2) ? -1.0 : 1.0; }
IPT_HD uint32_t abstop12(float x) { return (f2u(x) >> 20) & 0x7ffu; }

// sin polynomial on reduced x (n even) — __sinf_fma @7b359 / @7b2e0
IPT_HD float sin_poly_(double x, double x2, const sincos_tab& p) {
    double s1 = fma_(x2, p.s3, p.s2);
    double x3 = x2 * x;
    double x7 = x2 * x3;
    double s = fma_(x3, p.s1, x);
    return (float)fma_(s1, x7, s);
}
// cos polynomial on reduced x (n odd for sin) — __sinf_fma @7b388
IPT_HD float cos_poly_(double x2, const sincos_tab& p) {
    double x4 = x2 * x2;
    double c1 = fma_(x2, p.c1, p.c0);
    double c2 = fma_(x2, p.c4, p.c3);
    double x6 = x2 * x4;
    double c = fma_(x4, p.c2, c1);
    return (float)fma_(c2, x6, c);
}

// reduce_large (sincosf.h) with __inv_pio4 (libm .rodata 0xb3060)
IPT_HD double reduce_large_(uint32_t xi, int* np) {
    const uint32_t inv_pio4[24] = {
        0xa2u,       0xa2f9u,     0xa2f983u,   0xa2f9836eu, 0xf9836e4eu, 0x836e4e44u,
        0x6e4e4415u, 0x4e441529u, 0x441529fcu, 0x1529fc27u, 0x29fc2757u, 0xfc2757d1u,
        0x2757d1f5u, 0x57d1f534u, 0xd1f534ddu, 0xf534ddc0u, 0x34ddc0dbu, 0xddc0db62u,
        0xc0db6295u, 0xdb629599u, 0x6295993cu, 0x95993c43u, 0x993c4390u, 0x3c439041u};
    const uint32_t* arr = &inv_pio4[(xi >> 26) & 15];
    int shift = (xi >> 23) & 7;
    uint64_t n, res0, res1, res2;
    xi = (xi & 0xffffffu) | 0x800000u;
    xi <<= shift;
    res0 = (uint64_t)(uint32_t)(xi * arr[0]);
    res1 = (uint64_t)xi * arr[4];
    res2 = (uint64_t)xi * arr[8];
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    n = (res0 + (1ull << 61)) >> 62;
    res0 -= n << 62;
    double x = (double)(int64_t)res0;
    *np = (int)n;
    return x * u2d(0x3c1921fb54442d18ull);  // pi * 2^-62
}

// fast reduction: n = round(x*2/pi) via (int)(x*hpi_inv*2^24) + 2^23 >> 24; x - n*hpi (one FMA)
IPT_HD double reduce_fast_(double x, int* np) {
    const double hpi_inv = u2d(0x41645f306dc9c883ull);  // 0x1.45f306dc9c883p+23
    double r = x * hpi_inv;
    int n = ((int32_t)r + 0x800000) >> 24;
    *np = n;
    return fma_(-(double)n, u2d(0x3ff921fb54442d18ull), x);
}

IPT_HD void sincosf_small_(float y, float* sp, float* cp);
IPT_HD float sinf_(float y) {
    double x = y;
    if (abstop12(y) < abstop12(120.0f)) {
        float sv, cv;
        sincosf_small_(y, &sv, &cv);
        return sv;
    } else if (abstop12(y) < abstop12(u2f(0x7f800000u))) {
        uint32_t xi = f2u(y);
        int sign = xi >> 31;
        int n;
        x = reduce_large_(xi, &n);
        double s = sincos_sign((n + sign) & 3);
        sincos_tab p = sincos_table(((n + sign) & 2) ? 1 : 0);
        double x2 = x * x;
        if ((n & 1) == 0) return sin_poly_(x * s, x2, p);
        return cos_poly_(x2, p);
    }
    return (y - y) / (y - y);
}

IPT_HD float cosf_(float y) {
    double x = y;
    if (abstop12(y) < abstop12(120.0f)) {
        float sv, cv;
        sincosf_small_(y, &sv, &cv);
        return cv;
    } else if (abstop12(y) < abstop12(u2f(0x7f800000u))) {
        uint32_t xi = f2u(y);
        int sign = xi >> 31;
        int n;
        x = reduce_large_(xi, &n);
        double s = sincos_sign((n + sign) & 3);
        sincos_tab p = sincos_table(((n + sign) & 2) ? 1 : 0);
        double x2 = x * x;
        if (n & 1) return sin_poly_(x * s, x2, p);
        return cos_poly_(x2, p);
    }
    return (y - y) / (y - y);
}

// sin and cos of the same argument sharing one reduction, for |y| < 120
// (every argument the path tracer produces: rotation angles in [0,pi],
// CosineDdf angles in [0,pi/2] and [0,2pi)). Equal bit-for-bit to
// sinf_/cosf_ there (glibc's __sincosf_fma SLP-vectorises the same FMA graph;
// tests/test_math_exhaustive.py checks the equality against host sincosf).
// Branch-free: for |y| < pi/4 glibc skips the reduction, but reduce_fast_
// then yields n = 0 and x - 0*hpi == x exactly (fma with a -0 product), i.e.
// the same polynomial inputs; only |y| < 2^-12 needs a select.
//
// The quadrant's signs are applied last: glibc selects sign-flipped cosine
// coefficients (sg * c_i, sincos_table) and multiplies x by s = +-1; every
// FMA of the cosine polynomial has all-sign-flipped operands and the sine
// polynomial is odd in x, and round-to-nearest is symmetric, so the results
// are exactly sg * cos_poly(c_i) and s * sin_poly(x): two sign flips of the
// float results instead of selected f64 constants (same bits for every input).
IPT_HD void sincosf_small_(float y, float* sp, float* cp) {
    int n;
    const double x = reduce_fast_((double)y, &n);
    const sincos_tab p = sincos_table(0);
    const double x2 = x * x;
    const uint32_t s_neg = ((n & 3) == 1 || (n & 3) == 2) ? 0x80000000u : 0u;  // sincos_sign(n & 3)
    const uint32_t g_neg = (n & 2) ? 0x80000000u : 0u;                         // sincos_table's sg
    const float a = u2f(f2u(sin_poly_(x, x2, p)) ^ s_neg);
    const float b = u2f(f2u(cos_poly_(x2, p)) ^ g_neg);
    const bool tiny = abstop12(y) < abstop12(0x1p-12f);
    *sp = tiny ? y : ((n & 1) ? b : a);
    *cp = tiny ? 1.0f : ((n & 1) ? a : b);
}
IPT_HD void sincosf_(float y, float* sp, float* cp) {
    if (abstop12(y) < abstop12(120.0f)) {
        sincosf_small_(y, sp, cp);
        return;
    }
    *sp = sinf_(y);
    *cp = cosf_(y);
}
// sinf for |y| < 120 (same arithmetic as sinf_ there)
IPT_HD float sinf_small_(float y) {
    float sv, cv;
    sincosf_small_(y, &sv, &cv);
    return sv;
}

// ------------------------------------------------- (float)acos((double)x)
// fdlibm e_acos.c (double). Used only through its rounding to float; the
// equality of that rounding with glibc's acos for all float inputs in [-1,1]
// is checked exhaustively in tests/test_math_exhaustive.py.
IPT_HD double acos_d_(double x) {
    const double pi = u2d(0x400921fb54442d18ull);
    const double pio2_hi = u2d(0x3ff921fb54442d18ull);
    const double pio2_lo = u2d(0x3c91a62633145c07ull);
    const double pS0 = u2d(0x3fc5555555555555ull), pS1 = u2d(0xbfd4d61203eb6f7dull),
                 pS2 = u2d(0x3fc9c1550e884455ull), pS3 = u2d(0xbfa48228b5688f3bull),
                 pS4 = u2d(0x3f49efe07501b288ull), pS5 = u2d(0x3f023de10dfdf709ull);
    const double qS1 = u2d(0xc0033a271c8a2d4bull), qS2 = u2d(0x40002ae59c598ac8ull),
                 qS3 = u2d(0xbfe6066c1b8d0159ull), qS4 = u2d(0x3fb3b8c5b12e9282ull);
    const uint64_t hx64 = d2u(x);
    const uint32_t hx = (uint32_t)(hx64 >> 32);
    const uint32_t ix = hx & 0x7fffffffu;
    // branch-free over fdlibm's three ranges (see acosf_)
    const bool small = ix < 0x3fe00000u;
    const bool neg = (int32_t)hx < 0;
    const double z = small ? x * x : (neg ? (1.0 + x) * 0.5 : (1.0 - x) * 0.5);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    const double sq = sqrtd_(z);
    const double r_small = pio2_hi - (x - (pio2_lo - x * r));
    const double r_neg = pi - 2.0 * (sq + (r * sq - pio2_lo));
    const double df = u2d(d2u(sq) & 0xffffffff00000000ull);
    const double c = (z - df * df) / (sq + df);
    const double r_pos = 2.0 * (df + (r * sq + c));
    double res = small ? r_small : (neg ? r_neg : r_pos);
    if (small && ix <= 0x3c600000u) res = pio2_hi + pio2_lo;
    if (ix >= 0x3ff00000u) {
        if (((ix - 0x3ff00000u) | (uint32_t)hx64) == 0)
            res = (int32_t)hx > 0 ? 0.0 : pi + 2.0 * pio2_lo;
        else
            res = (x - x) * (double)inf_();
    }
    return res;
}
IPT_HD float acos_f64_to_f32_exact(float x) { return (float)acos_d_((double)x); }

// RotateDdf's angle (float)acos((double)x) (ddf_detail.h:82), fast device path.
// acos_d_ costs two IEEE f64 divisions and an IEEE f64 sqrt, each a long
// correction sequence on gfx950. Here fdlibm's formulas are evaluated with the
// hardware f64 reciprocal / reciprocal-sqrt refined by Newton steps (relative
// error of A a few 1e-16), and the float rounding of A is accepted when A(1-d)
// and A(1+d), d = 2^-44, round to the same float: rounding is monotonic, so
// the exact value and fdlibm's (both within d of A) round there too (Ziv's
// test). Otherwise, and for |x| >= 1, the exact restatement decides. Equal to
// acos_f64_to_f32_exact on every float (device self-check over all 2^32
// inputs, tests/test_gpu_parity.py::test_fast_acos_exhaustive).
IPT_HD float acos_f64_to_f32(float xf) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double x = (double)xf;
    const double ax = __builtin_fabs(x);
    const double pi = u2d(0x400921fb54442d18ull);
    const double pio2_hi = u2d(0x3ff921fb54442d18ull);
    const double pio2_lo = u2d(0x3c91a62633145c07ull);
    const double pS0 = u2d(0x3fc5555555555555ull), pS1 = u2d(0xbfd4d61203eb6f7dull),
                 pS2 = u2d(0x3fc9c1550e884455ull), pS3 = u2d(0xbfa48228b5688f3bull),
                 pS4 = u2d(0x3f49efe07501b288ull), pS5 = u2d(0x3f023de10dfdf709ull);
    const double qS1 = u2d(0xc0033a271c8a2d4bull), qS2 = u2d(0x40002ae59c598ac8ull),
                 qS3 = u2d(0xbfe6066c1b8d0159ull), qS4 = u2d(0x3fb3b8c5b12e9282ull);
    const bool small = ax < 0.5;
    const double z = small ? x * x : (1.0 - ax) * 0.5;
    const double p = z * __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z,
                         __builtin_fma(z, pS5, pS4), pS3), pS2), pS1), pS0);
    const double q = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, qS4, qS3), qS2), qS1), 1.0);
    double y = __builtin_amdgcn_rcp(q);
    y = __builtin_fma(y, __builtin_fma(-q, y, 1.0), y);
    y = __builtin_fma(y, __builtin_fma(-q, y, 1.0), y);
    const double r = p * y;
    // sqrt(z) by Goldschmidt from rsq (z in (0, 0.25] off the small branch)
    const double zs = small ? 0.25 : z;
    const double g0 = __builtin_amdgcn_rsq(zs);
    double sg = zs * g0, h = 0.5 * g0;
    double t = __builtin_fma(-sg, h, 0.5);
    sg = __builtin_fma(sg, t, sg);
    h = __builtin_fma(h, t, h);
    t = __builtin_fma(-sg, sg, zs);
    sg = __builtin_fma(t, h, sg);
    double A;
    if (small)
        A = pio2_hi - (x - (pio2_lo - x * r));
    else if (x < 0.0)
        A = pi - 2.0 * (sg + (r * sg - pio2_lo));
    else
        A = 2.0 * (sg + r * sg);
    const double d = u2d(0x3d30000000000000ull);  // 2^-44
    const float lo = (float)(A * (1.0 - d)), hi = (float)(A * (1.0 + d));
    if (lo == hi && ax < 1.0) return lo;
    return (float)acos_d_(x);
#else
    return acos_f64_to_f32_exact(xf);
#endif
}

// ------------------------------------------------------------------ powf
// ARM optimized-routines powf as built into glibc 2.35
// (sysdeps/ieee754/flt-32/e_powf.c, powf_log2_data.c, exp2f_data.c) in its FMA
// ifunc variant __powf_fma: log2(x) by a 16-entry table and a degree-5
// polynomial, y*log2(x) in double, 2^that by a 32-entry table and a cubic.
// Tables read from libm .rodata (__powf_log2_data 0xb2f20: {invc, logc}[16]
// then poly[5]; __exp2f_data 0xb2b80: tab[32], shift 0x1.8p+47, poly[3]); the
// disassembly (0x7aef0) contracts EVERY multiply-add of the source into an
// FMA, r = z*invc - 1 included.
//
// Scope (the display chain's gamma, x/max in [0,1] with y = 1/2.2 or 0.6):
// y must be finite, > 0 and not an integer; ipt_powf_* reject other y. For
// such y the result equals libm's bit for bit on every x >= 0, +-0, +-inf and
// NaN (x*x there: 0, +inf, the quieted NaN). The rare path is simplified:
// glibc's (x-x)/(x-x) for finite x < 0 is stated as the x86 default NaN
// 0xffc00000 (the device's 0/0 has the other sign), and the over/underflow
// exits return +inf / +0 without raising exceptions.
IPT_HD float powf_(float x, float y) {
    const uint64_t log2_tab[16][2] = {
        {0x3ff661ec79f8f3beull, 0xbfdefec65b963019ull}, {0x3ff571ed4aaf883dull, 0xbfdb0b6832d4fca4ull},
        {0x3ff49539f0f010b0ull, 0xbfd7418b0a1fb77bull}, {0x3ff3c995b0b80385ull, 0xbfd39de91a6dcf7bull},
        {0x3ff30d190c8864a5ull, 0xbfd01d9bf3f2b631ull}, {0x3ff25e227b0b8ea0ull, 0xbfc97c1d1b3b7af0ull},
        {0x3ff1bb4a4a1a343full, 0xbfc2f9e393af3c9full}, {0x3ff12358f08ae5baull, 0xbfb960cbbf788d5cull},
        {0x3ff0953f419900a7ull, 0xbfaa6f9db6475fceull}, {0x3ff0000000000000ull, 0x0000000000000000ull},
        {0x3fee608cfd9a47acull, 0x3fb338ca9f24f53dull}, {0x3feca4b31f026aa0ull, 0x3fc476a9543891baull},
        {0x3feb2036576afce6ull, 0x3fce840b4ac4e4d2ull}, {0x3fe9c2d163a1aa2dull, 0x3fd40645f0c6651cull},
        {0x3fe886e6037841edull, 0x3fd88e9c2c1b9ff8ull}, {0x3fe767dcf5534862ull, 0x3fdce0a44eb17bccull}};
    const uint64_t exp2_tab[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
        0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
        0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
        0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
        0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
        0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
    const double A0 = u2d(0x3fd27616c9496e0bull), A1 = u2d(0xbfd71969a075c67aull), A2 = u2d(0x3fdec70a6ca7baddull),
                 A3 = u2d(0xbfe7154748bef6c8ull), A4 = u2d(0x3ff71547652ab82bull);
    const double C0 = u2d(0x3fac6af84b912394ull), C1 = u2d(0x3fcebfce50fac4f3ull), C2 = u2d(0x3fe62e42ff0c52d6ull);
    const double shift = u2d(0x42e8000000000000ull);  // 0x1.8p+47 = 0x1.8p52 / 32
    uint32_t ix = f2u(x);
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {  // x < 2^-126, inf or NaN
        const uint32_t ax = ix & 0x7fffffffu;
        if (ax == 0) return 0.0f;                          // x*x
        if (ax == 0x7f800000u) return inf_();              // x*x
        if (ax > 0x7f800000u) return u2f(ix | 0x00400000u);  // x*x of a NaN: quieted, sign and payload kept
        if (ix & 0x80000000u) return u2f(0xffc00000u);     // __math_invalidf
        ix = f2u(x * 8388608.0f) & 0x7fffffffu;            // subnormal: scale by 2^23
        ix -= 23u << 23;
    }
    // log2_inline
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) & 15u);
    const uint32_t top = tmp & 0xff800000u;
    const uint32_t iz = ix - top;
    const int k = (int32_t)top >> 23;
    const double invc = u2d(log2_tab[i][0]), logc = u2d(log2_tab[i][1]);
    const double z = (double)u2f(iz);
    const double r = fma_(z, invc, -1.0);
    const double y0 = logc + (double)k;
    const double r2 = r * r;
    const double py = fma_(A0, r, A1);
    const double pp = fma_(A2, r, A3);
    const double r4 = r2 * r2;
    double q = fma_(A4, r, y0);
    q = fma_(pp, r2, q);
    const double logx = fma_(py, r4, q);
    const double ylogx = (double)y * logx;
    if (((d2u(ylogx) >> 47) & 0xffffu) >= 0x80bfu) {  // |y log2 x| >= 126
        if (ylogx > u2d(0x405fffffffd1d571ull)) return inf_();  // __math_oflowf
        if (ylogx <= -150.0) return 0.0f;                       // __math_uflowf
    }
    // exp2_inline
    double kd = ylogx + shift;
    const uint64_t ki = d2u(kd);
    kd = kd - shift;
    const double rr = ylogx - kd;
    const uint64_t t = exp2_tab[ki & 31u] + (ki << 47);
    const double s = u2d(t);
    const double zz = fma_(C0, rr, C1);
    const double rr2 = rr * rr;
    double e = fma_(C2, rr, 1.0);
    e = fma_(zz, rr2, e);
    return (float)(e * s);
}

// ------------------------------------------------------------------ logf
// ARM optimized-routines logf as built into glibc 2.35
// (sysdeps/ieee754/flt-32/e_logf.c, logf_data.c): a 16-entry {invc, logc}
// table and a cubic, in double. Table read from libm .rodata (__logf_data
// 0xb2ce0: {invc, logc}[16], then ln2 and poly[3] at 0xb2de0). The plain
// (uncontracted) form below and the form with every multiply-add fused both
// equal the image's logf (__logf_fma) on all 1 065 353 216 floats of
// [1, FLT_MAX], so this is built with -ffp-contract=off as everything else.
//
// Scope (the PGM chain: n_val's adj is clamped to [1, contrast]): x in
// [1, FLT_MAX]. Outside it (x < 1, negative, +inf, NaN) the result is the quiet
// NaN 0x7fc00000 by definition, the same on the host and on the device.
IPT_HD float logf_(float x) {
    const uint64_t tab[16][2] = {
        {0x3ff661ec79f8f3beull, 0xbfd57bf7808caadeull}, {0x3ff571ed4aaf883dull, 0xbfd2bef0a7c06ddbull},
        {0x3ff49539f0f010b0ull, 0xbfd01eae7f513a67ull}, {0x3ff3c995b0b80385ull, 0xbfcb31d8a68224e9ull},
        {0x3ff30d190c8864a5ull, 0xbfc6574f0ac07758ull}, {0x3ff25e227b0b8ea0ull, 0xbfc1aa2bc79c8100ull},
        {0x3ff1bb4a4a1a343full, 0xbfba4e76ce8c0e5eull}, {0x3ff12358f08ae5baull, 0xbfb1973c5a611cccull},
        {0x3ff0953f419900a7ull, 0xbfa252f438e10c1eull}, {0x3ff0000000000000ull, 0x0000000000000000ull},
        {0x3fee608cfd9a47acull, 0x3faaa5aa5df25984ull}, {0x3feca4b31f026aa0ull, 0x3fbc5e53aa362eb4ull},
        {0x3feb2036576afce6ull, 0x3fc526e57720db08ull}, {0x3fe9c2d163a1aa2dull, 0x3fcbc2860d224770ull},
        {0x3fe886e6037841edull, 0x3fd1058bc8a07ee1ull}, {0x3fe767dcf5534862ull, 0x3fd4043057b6ee09ull}};
    const double ln2 = u2d(0x3fe62e42fefa39efull);
    const double A0 = u2d(0xbfd00ea348b88334ull), A1 = u2d(0x3fd5575b0be00b6aull), A2 = u2d(0xbfdffffef20a4123ull);
    const uint32_t ix = f2u(x);
    if (ix - 0x3f800000u > 0x7f7fffffu - 0x3f800000u) return u2f(0x7fc00000u);  // outside [1, FLT_MAX]
    if (ix == 0x3f800000u) return 0.0f;
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> 19) & 15u);
    const int k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & 0xff800000u);
    const double invc = u2d(tab[i][0]), logc = u2d(tab[i][1]);
    const double z = (double)u2f(iz);
    const double r = z * invc - 1.0;
    const double y0 = logc + (double)k * ln2;
    const double r2 = r * r;
    double y = A1 * r + A2;
    y = A0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

// a / b with the NaN results of the x86 host the reference runs on stated
// explicitly (the device's division picks another operand's payload and the
// other sign for an invalid quotient): a NaN operand comes back quieted, the
// dividend's first (divss returns its first source); 0/0 and inf/inf give the
// default NaN 0xffc00000. Every other quotient is the IEEE one.
IPT_HD float div_x86nan_(float a, float b) {
    const uint32_t ua = f2u(a) & 0x7fffffffu, ub = f2u(b) & 0x7fffffffu;
    if (ua > 0x7f800000u) return u2f(f2u(a) | 0x00400000u);
    if (ub > 0x7f800000u) return u2f(f2u(b) | 0x00400000u);
    if ((ua == 0 && ub == 0) || (ua == 0x7f800000u && ub == 0x7f800000u)) return u2f(0xffc00000u);
    return a / b;
}

// --------------------------------------------------- mixed-precision helpers
// The reference compares floats against the double literal 1e-6
// (geometric_utils.cpp:14,23,45-48; lighting.cpp:116,120). For a float f,
// (double)f < 1e-6 <=> f < 0x358637be (the smallest float above 1e-6 is
// 0x358637be; float(1e-6) = 0x358637bd < 1e-6).
IPT_HD bool lt_1em6(float f) { return f < u2f(0x358637beu); }

// CosineDdf::value (ddf.cpp:232-238): (float)((double)z / M_PI).
// For every float z in [0, 2], (float)(z * (double)(1/M_PI)) rounds to the
// same float as the f64 quotient (checked exhaustively against host libm in
// tests/test_math_exhaustive.py::test_mixed_precision_helpers), so the f64
// division is a multiply. The reference only reaches z in [0, 1+2^-22]
// (z = (inverse*d).z with |d| = 1 and an orthonormal inverse).
IPT_HD float div_pi_to_f32(float z) { return (float)((double)z * u2d(0x3fd45f306dc9c883ull)); }

// CosineDdf::sample phi (ddf.cpp:228): (float)(2*M_PI*(double)u2)
IPT_HD float two_pi_times(float u) { return (float)(u2d(0x401921fb54442d18ull) * (double)u); }
// two_pi_times(u01(g << 8)) for a 24-bit g: u = g 2^-24 exactly, so the double
// product 2pi * u is RN(2pi * g * 2^-24) = RN((2pi 2^-24) * g) -- the same
// real product, the constant scaled by a power of two -- from g directly
IPT_HD float two_pi_times_u24(uint32_t g) { return (float)(u2d(0x3e9921fb54442d18ull) * (double)g); }

// ------------------------------------------------------------ RNG (Philox)
// Philox4x32-10 (Salmon et al., SC'11; Random123 constants).
struct u32x4 {
    uint32_t v[4];
};
IPT_HD void mulhilo32(uint32_t a, uint32_t b, uint32_t* hi, uint32_t* lo) {
    uint64_t p = (uint64_t)a * (uint64_t)b;
    *hi = (uint32_t)(p >> 32);
    *lo = (uint32_t)p;
}
// a ^ b ^ c: one v_bitop3_b32 (truth table 0x96) on gfx950
IPT_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
IPT_HD u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                           uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#if defined(__HIP_DEVICE_COMPILE__)
    // the round keys are two scalar adds each: keep them in the loop, where
    // they cost SALU slots, instead of hoisted and spilled to VGPR lanes
    // (every reload a v_readlane + hazard nops on the VALU)
    asm volatile("" : "+s"(k0), "+s"(k1));
#endif
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        mulhilo32(M0, c0, &hi0, &lo0);
        mulhilo32(M1, c2, &hi1, &lo1);
        uint32_t n0 = xor3(hi1, c1, k0);
        uint32_t n2 = xor3(hi0, c3, k1);
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    u32x4 out;
    out.v[0] = c0;
    out.v[1] = c1;
    out.v[2] = c2;
    out.v[3] = c3;
    return out;
}
// uniform float in [0,1): top 24 bits * 2^-24 (never 1.0, so randf.h's retry
// loop at include/randf.h:8-9 never fires)
IPT_HD float u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }

}  // namespace ipt
