// Host check of trace_box_planes_nearest (ipt_path.h): the
// nearest-candidate form against trace_box_planes_only, bit for bit on t and
// prim, and its hit point against o + d*t wherever prim >= 0, for both INRANGE
// forms. argv[1] = number of random rays per form (default 20 M). Rays:
//   origins on the walls (exactly and one ulp inside), on the r = 0.5 sphere,
//   in the interior, at a camera outside the open (-y) side, and beyond +-1 on
//   one or two axes; half of the directions aimed at faces, edges and corners;
//   axis-parallel directions; directions with a NaN, +-inf or +-0 component;
//   origins up to 2^38 (INRANGE = false only); the diagonal (1,1,1)/sqrt(3)
//   from (1/4,1/4,1/4), a three-way tie.
// The random rays (finite directions) also compare box_sphere_t, the box
// trace's sphere test that hands out its hit point, with sphere_t<true, INR>.
// Prints, per form, "rays N mismatches M none A hit B mono C full D
// sphere_hits S" (the outcome classes of the new form). Exit status 0 = no
// mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../ipt_amd/csrc/ipt_path.h"

using namespace ipt;

namespace {

struct Tally {
    long rays = 0, mism = 0, cls[4] = {0, 0, 0, 0}, sphere_hits = 0;
};

template <bool INR>
void check(vec3 o, vec3 d, Tally& T) {
    int p0 = -7, p1 = -7, c = -1;
    vec3 hit = v3(0, 0, 0);
    const float t0 = trace_box_planes_only<INR>(o, d, &p0);
    const float t1 = trace_box_planes_nearest<INR>(o, d, &p1, &hit, &c);
    bool bad = f2u(t0) != f2u(t1) || p0 != p1 || c < 0 || c > 3;
    if (!bad && p1 >= 0) {
        const vec3 q = v3(o.x + d.x * t1, o.y + d.y * t1, o.z + d.z * t1);
        bad = f2u(q.x) != f2u(hit.x) || f2u(q.y) != f2u(hit.y) || f2u(q.z) != f2u(hit.z);
    }
    ++T.rays;
    if (c >= 0 && c <= 3) ++T.cls[c];
    if (bad) {
        if (T.mism < 10)
            std::printf("MISMATCH inr %d o %a %a %a d %a %a %a: only t %a prim %d, nearest t %a prim %d class %d\n",
                        (int)INR, o.x, o.y, o.z, d.x, d.y, d.z, t0, p0, t1, p1, c);
        ++T.mism;
    }
}

// box_sphere_t (the box trace's sphere test with its hit point handed out)
// against sphere_t<true, INR>, for finite directions
template <bool INR>
void check_sphere(vec3 o, vec3 d, Tally& T) {
    vec3 hit = v3(0, 0, 0);
    const float t0 = sphere_t<true, INR>(0.5f, o, d);
    const float t1 = box_sphere_t<INR>(0.5f, o, d, &hit);
    bool bad = f2u(t0) != f2u(t1);
    if (!bad && t1 != inf_()) {
        const vec3 q = o + d * t1;
        bad = f2u(q.x) != f2u(hit.x) || f2u(q.y) != f2u(hit.y) || f2u(q.z) != f2u(hit.z);
    }
    if (t1 != inf_()) ++T.sphere_hits;
    if (bad) {
        if (T.mism < 10)
            std::printf("MISMATCH sphere inr %d o %a %a %a d %a %a %a: sphere_t %a, box_sphere_t %a\n", (int)INR, o.x, o.y,
                        o.z, d.x, d.y, d.z, t0, t1);
        ++T.mism;
    }
}

template <bool INR>
Tally run(long n) {
    Tally T;
    std::mt19937_64 rng(INR ? 11 : 12);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    auto pm1 = [&]() { return (rng() & 1) ? 1.0f : -1.0f; };
    auto unit = [&]() {
        for (;;) {
            const vec3 v = v3(U(rng), U(rng), U(rng));
            const float l = dot(v, v);
            if (l > 1e-4f && l <= 1.0f) return normalize(v);
        }
    };
    // a point of the box's surface: a face, an edge (two coordinates +-1) or a corner
    auto target = [&]() {
        vec3 t = v3(U(rng), U(rng), U(rng));
        const int kind = (int)(rng() % 3), a = (int)(rng() % 3);
        float* c[3] = {&t.x, &t.y, &t.z};
        *c[a] = pm1();
        if (kind >= 1) *c[(a + 1) % 3] = pm1();
        if (kind == 2) *c[(a + 2) % 3] = pm1();
        return t;
    };
    auto origin = [&](int kind) {
        vec3 o = v3(U(rng), U(rng), U(rng));
        float* c[3] = {&o.x, &o.y, &o.z};
        const int a = (int)(rng() % 3);
        switch (kind) {
            case 0:  // on a wall
                *c[a] = pm1();
                break;
            case 1:  // one ulp inside a wall
                *c[a] = std::nextafter(pm1(), 0.0f);
                break;
            case 2:  // on the r = 0.5 sphere
                o = unit() * 0.5f;
                break;
            case 3:  // interior
                break;
            case 4:  // the camera outside the open side
                o = v3(U(rng) * 0.5f, -2.0f - (U(rng) + 1.0f) * 2.0f, U(rng) * 0.5f);
                break;
            case 5:  // beyond +-1 on one axis
                *c[a] = pm1() * (1.0f + (U(rng) + 1.0f) * 2.0f);
                break;
            case 6:  // beyond +-1 on two axes
                *c[a] = pm1() * (1.0f + (U(rng) + 1.0f) * 2.0f);
                *c[(a + 1) % 3] = pm1() * (1.0f + (U(rng) + 1.0f) * 2.0f);
                break;
            default:  // far away (INRANGE = false): up to 2^38
                o = v3(std::ldexp(U(rng), (int)(rng() % 39)), std::ldexp(U(rng), (int)(rng() % 39)),
                       std::ldexp(U(rng), (int)(rng() % 39)));
                break;
        }
        return o;
    };
    const int kinds = INR ? 7 : 8;
    for (long r = 0; r < n; ++r) {
        const vec3 o = origin((int)(r % kinds));
        vec3 d;
        if ((r / kinds) & 1) {
            const vec3 w = target() - o;
            d = dot(w, w) > 0.0f ? normalize(w) : unit();
        } else {
            d = unit();
        }
        check<INR>(o, d, T);
        check_sphere<INR>(o, d, T);
    }
    // axis-parallel directions and special components, from every origin class
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float special[] = {nan, inf, -inf, 0.0f, -0.0f, 1.0f, -1.0f, 1e-7f, -1e-7f, 1e-6f, 0x1p-140f, -0x1p-140f};
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    for (int rep = 0; rep < 200; ++rep)
        for (int k = 0; k < kinds; ++k) {
            const vec3 o = origin(k);
            for (int a = 0; a < 3; ++a)
                for (int s = 0; s < ns; ++s) {
                    // one special component, the others random
                    vec3 d = unit();
                    (a == 0 ? d.x : (a == 1 ? d.y : d.z)) = special[s];
                    check<INR>(o, d, T);
                    // two special components (axis-parallel when both are zeros)
                    for (int s2 = 0; s2 < ns; ++s2) {
                        vec3 e = d;
                        (a == 0 ? e.y : (a == 1 ? e.z : e.x)) = special[s2];
                        check<INR>(o, e, T);
                        vec3 f = v3(special[s2], special[s2], special[s2]);
                        (a == 0 ? f.x : (a == 1 ? f.y : f.z)) = special[s];
                        check<INR>(o, f, T);
                    }
                }
        }
    // the three-way tie, and its mirror images
    const float q = 1.0f / std::sqrt(3.0f);
    for (int m = 0; m < 8; ++m) {
        const vec3 sg = v3(m & 1 ? -1.0f : 1.0f, m & 2 ? -1.0f : 1.0f, m & 4 ? -1.0f : 1.0f);
        check<INR>(v3(0.25f * sg.x, 0.25f * sg.y, 0.25f * sg.z), v3(q * sg.x, q * sg.y, q * sg.z), T);
        check<INR>(v3(0.25f * sg.x, 0.25f * sg.y, 0.25f * sg.z), normalize(sg), T);
    }
    std::printf("inrange %d rays %ld mismatches %ld none %ld hit %ld mono %ld full %ld sphere_hits %ld\n", (int)INR, T.rays,
                T.mism, T.cls[0], T.cls[1], T.cls[2], T.cls[3], T.sphere_hits);
    return T;
}

}  // namespace

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 20000000;
    const Tally a = run<false>(n);
    const Tally b = run<true>(n);
    return (a.mism == 0 && b.mism == 0) ? 0 : 1;
}
