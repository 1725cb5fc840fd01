// shading.hpp — everything the megakernel does once a ray's hit is accepted (or it missed):
// the HitRecord rebuilt from (primitive, t) and the instance back-transforms, Texture::value_at,
// the HDRI texel, and Material::emitted / scatter in their two forms (the staged shade<> and the
// split scatter()).  Included by render.hip; tests/hip/kat_device.hip includes it too, so the
// known-answer tests run these very functions.  The block is written in namespace gsd's names
// (d3, mk, Ray, ...): an includer says `using namespace gsd;` before it includes this file, as
// both do -- the header itself opens no namespace for those who include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../../include/grayshift_gpu.h"
#include "kernel_abi.hpp"
#include "devmath.hpp"
#include "geometry.hpp"
#include "perlin.hpp"

// (everything inlined: GS_MIN_WAVES, kernel_abi.hpp)
#ifndef GS_NOINLINE
#define GS_NOINLINE __forceinline__
#endif

struct HitRec {
    d3 p, n;
    double u, v;
    uint32_t mat;
    bool front;
};

__device__ __forceinline__ void sphere_uv(d3 p, double& u, double& v) {  // sphere.rs:55-60
    const double PI = 3.14159265358979323846;
    double theta = acos(-p.y);
    double phi = atan2(-p.z, p.x) + PI;
    u = phi / (2.0 * PI);
    v = theta / PI;
}

// Recompute the HitRecord of the accepted primitive at t (the values the reference
// built when it accepted it), then apply the instance back-transforms innermost-first.
// hit_inst: the chain the hit came through (GS_REF_NONE: none); outer: for a hit through a
// chain inside a BVH that is itself under a chain (round 6), that BVH's chain (applied first
// going in, last coming out), else GS_REF_NONE.
// The n-th instance of the concatenated chain (outer's, then hit_inst's).
__device__ __forceinline__ uint32_t chain_at(const DevScene& sc, uint32_t outer, uint32_t inner, int n) {
    uint32_t cur = outer != GS_REF_NONE ? outer : inner;
    bool in_outer = outer != GS_REF_NONE;
#pragma unroll 1
    for (int k = 0; k < 2 * GS_MAX_CHAIN; k++) {
        if ((cur >> GS_REF_SHIFT) != GS_REF_INSTANCE) {  // the outer chain ended: the inner one
            if (!in_outer) break;
            in_outer = false;
            cur = inner;
            k--;
            continue;
        }
        if (n-- == 0) return cur & GS_REF_MASK;
        cur = sc.inst[cur & GS_REF_MASK].child;
    }
    return 0u;
}
template <bool DEEP>  // GS_FEAT_GENERAL kernels: chains longer than 4, two chains
__device__ GS_NOINLINE HitRec reconstruct(const DevScene& sc, Ray r, double t, uint32_t hit_ref,
                                           uint32_t hit_inst, uint32_t outer = GS_REF_NONE) {
    HitRec h;
    uint32_t ch0 = 0, ch1 = 0, ch2 = 0, ch3 = 0;
    int nch = 0;
    bool deep = DEEP && outer != GS_REF_NONE;  // two chains, or one longer than 4: the re-walking path
    if (hit_inst != GS_REF_NONE && !deep) {
        uint32_t cur = hit_inst;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if ((cur >> GS_REF_SHIFT) != GS_REF_INSTANCE) break;
            uint32_t i = cur & GS_REF_MASK;
            if (k == 0) ch0 = i; else if (k == 1) ch1 = i; else if (k == 2) ch2 = i; else ch3 = i;
            nch = k + 1;
            const gs_instance& in = sc.inst[i];
            inst_forward(in, r);
            cur = in.child;
        }
        if (DEEP && (cur >> GS_REF_SHIFT) == GS_REF_INSTANCE) {  // deeper than 4: on through the rest
            deep = true;
#pragma unroll 1
            for (int k = 4; k < GS_MAX_CHAIN && (cur >> GS_REF_SHIFT) == GS_REF_INSTANCE; k++) {
                const gs_instance& in = sc.inst[cur & GS_REF_MASK];
                inst_forward(in, r);
                cur = in.child;
                nch = k + 1;
            }
        }
    } else if (DEEP && deep) {  // the outer chain, then the inner one
        uint32_t cur = outer;
        bool in_outer = true;
#pragma unroll 1
        for (int k = 0; k < 2 * GS_MAX_CHAIN; k++) {
            if ((cur >> GS_REF_SHIFT) != GS_REF_INSTANCE) {
                if (!in_outer || hit_inst == GS_REF_NONE) break;
                in_outer = false;
                cur = hit_inst;
                continue;
            }
            const gs_instance& in = sc.inst[cur & GS_REF_MASK];
            inst_forward(in, r);
            cur = in.child;
            nch++;
        }
    }
    const uint32_t kind = hit_ref >> GS_REF_SHIFT, idx = hit_ref & GS_REF_MASK;
    d3 p, outward;
    double u = 0.0, v = 0.0;
    if (kind == GS_REF_SPHERE || kind == GS_REF_MSPHERE) {
        d3 c;
        double rad;
        if (kind == GS_REF_SPHERE) {
            DSphere s = sc.spheres[idx];
            c = mk(s.cx, s.cy, s.cz);
            rad = s.r;
            h.mat = sc.sphere_mat[idx];
        } else {
            const gs_msphere& s = sc.mspheres[idx];
            c = add(ld3(s.center_start), muls(ld3(s.center_path), r.time));
            rad = s.radius;
            h.mat = s.material;
        }
        p = add(r.o, muls(r.d, t));
        outward = divs(sub(p, c), rad);
        if (sc.mats[h.mat].needs_uv) sphere_uv(outward, u, v);
    } else if (kind == GS_REF_QUAD) {
        const gs_quad& q = sc.quads[idx];
        p = add(r.o, muls(r.d, t));
        d3 planar = sub(p, ld3(q.q));
        u = dot(ld3(q.w), cross(planar, ld3(q.v)));
        v = dot(ld3(q.w), cross(ld3(q.u), planar));
        outward = ld3(q.normal);
        h.mat = q.material;
    } else if (kind == GS_REF_MEDIUM) {  // volume.rs:54-62: ray.at(t), normal (1, 0, 0), u = v = 0
        p = add(r.o, muls(r.d, t));
        outward = mk(1.0, 0.0, 0.0);
        h.mat = sc.media[idx].material;
    } else {  // triangle
        const gs_triangle& tr = sc.tris[idx];
        double tt;
        tri_hit(tr, r, tt, u, v);
        p = add(r.o, muls(r.d, t));
        outward = ld3(tr.normal);
        h.mat = tr.material;
    }
    // HitRecord::new (hittable.rs:26-43)
    h.front = dot(r.d, outward) < 0.0;
    d3 n = h.front ? outward : neg(outward);
    // Innermost instance first (RotateY inside Translate: rotate back, then translate).
    if (!DEEP || !deep) {
        if (nch > 3) inst_backward(sc.inst[ch3], p, n);
        if (nch > 2) inst_backward(sc.inst[ch2], p, n);
        if (nch > 1) inst_backward(sc.inst[ch1], p, n);
        if (nch > 0) inst_backward(sc.inst[ch0], p, n);
    } else {
#pragma unroll 1
        for (int k = nch - 1; k >= 0; k--) inst_backward(sc.inst[chain_at(sc, outer, hit_inst, k)], p, n);
    }
    h.p = p;
    h.n = n;
    h.u = u;
    h.v = v;
    return h;
}

// The same for a hit that can only be a stationary sphere outside any instance (sphere-only
// trees, GS_FEAT_SPHLEAF): reconstruct's sphere branch and HitRecord::new, nothing else; UV
// false when no material needs uv (GS_FEAT_PLAIN).
template <bool UV>
__device__ __forceinline__ HitRec reconstruct_sphere(const DevScene& sc, const Ray& r, double t, uint32_t hit_ref) {
    HitRec h;
    const uint32_t idx = hit_ref & GS_REF_MASK;
    const DSphere s = sc.spheres[idx];
    const d3 c = mk(s.cx, s.cy, s.cz);
    h.mat = sc.sphere_mat[idx];
    const d3 p = add(r.o, muls(r.d, t));
    const d3 outward = divs(sub(p, c), s.r);
    h.u = 0.0;
    h.v = 0.0;
    if (UV && sc.mats[h.mat].needs_uv) sphere_uv(outward, h.u, h.v);
    h.front = dot(r.d, outward) < 0.0;  // hittable.rs:26-43
    h.n = h.front ? outward : neg(outward);
    h.p = p;
    return h;
}

// Texture::value_at (texture.rs:27-95); checkered nesting resolved iteratively.
__device__ GS_NOINLINE d3 texture_value(const DevScene& sc, uint32_t tex, double u, double v, d3 p,
                                         unsigned long long* cnt) {
#pragma unroll 1
    for (int depth = 0; depth < 16; depth++) {
        const gs_texture& t = sc.texs[tex];
        if (t.kind == GS_TEX_SOLID) return ld3(t.color);
        if (t.kind == GS_TEX_CHECKERED) {
            int32_t xi = sat_i32(floor(t.scale_inv * p.x));
            int32_t yi = sat_i32(floor(t.scale_inv * p.y));
            int32_t zi = sat_i32(floor(t.scale_inv * p.z));
            int32_t s = (int32_t)((uint32_t)xi + (uint32_t)yi + (uint32_t)zi);
            tex = (s % 2 == 0) ? t.even : t.odd;
            continue;
        }
        if (t.kind == GS_TEX_NOISE) {  // texture.rs:127-130
            atomicAdd(&cnt[C_NOISE], 1ull);
            const double n = noise_value(sc.noise_perm, t.color[0], p.x, p.y, p.z);
            return mk(n, n, n);
        }
        // GS_TEX_IMAGE
        const gs_image im = sc.images[t.image];
        double uc = u, vc = v;
        if (uc < 0.0) uc = 0.0;
        if (uc > 1.0) uc = 1.0;
        if (vc < 0.0) vc = 0.0;
        if (vc > 1.0) vc = 1.0;
        vc = 1.0 - vc;
        uint64_t i = sat_u64(uc * (double)im.width, 4294967295.0, 4294967295ull);
        uint64_t j = sat_u64(vc * (double)im.height, 4294967295.0, 4294967295ull);
        if (i > im.width - 1) i = im.width - 1;  // reference panics here (u == 1); documented clamp
        if (j > im.height - 1) j = im.height - 1;
        const uint8_t* px = sc.texels + im.offset + (j * (uint64_t)im.width + i) * 3;
        atomicAdd(&cnt[C_IMG], 1ull);
        return muls(mk((double)px[0], (double)px[1], (double)px[2]), 1.0 / 255.0);
    }
    return mk(0.0, 0.0, 0.0);
}

// HDRI::sample's texel (camera.rs:257-270) for an already normalised, rotated direction.
__device__ __forceinline__ d3 hdri_texel(const DevScene& sc, d3 rot, unsigned long long* cnt) {
    const gs_background& bg = sc.bg;
    uint32_t x, y;
    // f32 angles where they certify the texel, else the reference's f64 atan2 / asin
    // (sky_index_f32 / sky_index_f64, geometry.hpp)
    if (!sky_index_f32(rot, bg.width, bg.height, x, y)) sky_index_f64(rot, bg.width, bg.height, x, y);
    const uint64_t k = y * (uint64_t)bg.width + x;
    atomicAdd(&cnt[C_HDRI], 1ull);
    if (sc.hdri_rgbe) {
        // RGBE8 texel (4 B): m * 2^(e-136) is exactly the f32 radiant produced, so the
        // f64 value equals the reference's `color.r as f64` (verified per texel at upload).
        const uint32_t t = sc.hdri_rgbe[k];
        const uint32_t e = t >> 24;
        const double sc2 = e ? ldexp(1.0, (int)e - 136) : 0.0;
        return mk((double)(t & 0xffu) * sc2, (double)((t >> 8) & 0xffu) * sc2, (double)((t >> 16) & 0xffu) * sc2);
    }
    const float* px = sc.hdri + k * 3;
    return mk((double)px[0], (double)px[1], (double)px[2]);
}

__device__ __forceinline__ d3 checker(const DMaterial& m, d3 p) {  // texture.rs:58-70
    int32_t xi = sat_i32(floor(m.param * p.x));
    int32_t yi = sat_i32(floor(m.param * p.y));
    int32_t zi = sat_i32(floor(m.param * p.z));
    int32_t s = (int32_t)((uint32_t)xi + (uint32_t)yi + (uint32_t)zi);
    return (s % 2 == 0) ? ld3(m.a) : ld3(m.b);
}

// One shading lane: a miss (Camera::sample_background, camera.rs:201,228-233) or a hit
// (the HitRecord, then Material::emitted / scatter, material.rs).  cont = 1: the path
// continues from p along dir with attenuation col; cont = 0: it ends with radiance col
// (sky or emitted colour; 0 for an absorbed ray).
struct ShadeOut {
    d3 col, dir;
    uint32_t cont;
};

// Written as stages every shading lane passes through together, whatever its case, so
// a wave holding several cases pays once for the work they share instead of once per
// divergent branch: one unit() for the first normalisation (the rotated sky direction,
// the Lambertian ONB's w, the metal reflection, the dielectric's unit direction), one
// sqrt and division for the second (the ONB's v axis, random_unit_vector, and the
// dielectric's sin θ), one sqrt for the third (the cosine direction's unit, refract's
// parallel part), and one RNG draw for the Lambertian's r1 and the dielectric's Schlick
// draw.  Every lane evaluates exactly the reference's expressions on the same operands
// in the same order; only which lanes issue an instruction together changes.
// A hit lane's ray.o becomes the hit point p (the next ray's origin) as soon as p is
// known: nothing after the HitRecord reads the old origin, and p need not stay live.
template <bool PLAIN, bool SPH, bool GEN>
__device__ __forceinline__ ShadeOut shade(const DevScene& sc, Ray& ray, double t, uint32_t hit_ref,
                                          uint32_t hit_inst, uint64_t& rng, unsigned long long* cnt,
                                          uint32_t hit_outer = GS_REF_NONE) {
    const double PI = 3.14159265358979323846;
    ShadeOut o;
    o.cont = 0;
    o.col = mk(0.0, 0.0, 0.0);
    o.dir = mk(0.0, 0.0, 0.0);
    const bool miss = hit_ref == GS_REF_NONE;
    HitRec h;
    h.p = h.n = mk(0.0, 0.0, 0.0);
    h.u = h.v = 0.0;
    h.front = false;
    uint32_t kind = 0;  // 0: a miss
    const DMaterial* m = sc.mats;
    if (!miss) {
        atomicAdd(&cnt[C_HITS], 1ull);
        h = PLAIN ? reconstruct_sphere<false>(sc, ray, t, hit_ref)
            : SPH ? reconstruct_sphere<true>(sc, ray, t, hit_ref) : reconstruct<GEN>(sc, ray, t, hit_ref, hit_inst, hit_outer);
        m = &sc.mats[h.mat];
        kind = m->kind;
        ray.o = h.p;
    }
    const bool lamb = kind >= DM_LAMB_SOLID && kind <= DM_LAMB_TEX;  // material.rs:45-68
    const bool metal = kind == DM_METAL;                              // :87-102
    const bool diel = kind == DM_DIELECTRIC;                          // :123-148
    const bool iso = !PLAIN && (kind == DM_ISO_SOLID || kind == DM_ISO_TEX);  // :185-196
    const bool sky = miss && sc.bg.kind != GS_BG_SOLID;

    // albedo / emitted colour (texture.rs:27-95): one texture_value call site for every kind
    if (!PLAIN && (kind == DM_LAMB_TEX || kind == DM_LIGHT_TEX || kind == DM_ISO_TEX)) {
        o.col = texture_value(sc, m->texture, h.u, h.v, h.p, cnt);
    } else if (kind == DM_LAMB_CHECKER) {
        o.col = checker(*m, h.p);
    } else if (kind == DM_DIELECTRIC) {
        o.col = mk(1.0, 1.0, 1.0);
    } else if (!miss) {
        o.col = ld3(m->a);
    } else if (!sky) {
        o.col = ld3(sc.bg.color);
    }

    // stage 1: the first normalisation
    d3 v1 = mk(1.0, 0.0, 0.0);
    if (sky) {
        const double* R = sc.bg.rot;
        const d3 dir = ray.d;
        v1 = mk(dir.x * R[0] + dir.y * R[1] + dir.z * R[2], dir.x * R[3] + dir.y * R[4] + dir.z * R[5],
                dir.x * R[6] + dir.y * R[7] + dir.z * R[8]);
    } else if (lamb) {
        v1 = h.n;  // OrthonormalBasis::new (ONB.rs:10-23): w = unit(n)
    } else if (metal) {
        v1 = reflect(ray.d, h.n);
    } else if (diel) {
        v1 = ray.d;
    }
    const d3 u1 = unit(v1);

    // stage 2: the sky texel; the second vector to normalise (or sin θ's argument)
    d3 v2 = mk(1.0, 0.0, 0.0);
    double q2 = 1.0, ri = 0.0, cos_theta = 0.0;
    if (sky) {
        o.col = hdri_texel(sc, u1, cnt);
    } else if (lamb) {
        const d3 a = fabs(u1.x) > 0.9 ? mk(0.0, 1.0, 0.0) : mk(1.0, 0.0, 0.0);
        v2 = cross(u1, a);
        q2 = len2(v2);
    } else if (metal || iso) {  // random_unit_vector (util.rs:18-29)
#pragma unroll 1
        for (;;) {
            double x = wy_f64(rng) * 2.0 + -1.0;
            double y = wy_f64(rng) * 2.0 + -1.0;
            double z = wy_f64(rng) * 2.0 + -1.0;
            v2 = mk(x, y, z);
            q2 = len2(v2);
            if (q2 < 1.0) break;
        }
    } else if (diel) {
        ri = h.front ? 1.0 / m->param : m->param;
        cos_theta = fmin(dot(neg(u1), h.n), 1.0);
        q2 = 1.0 - cos_theta * cos_theta;
    }
    const double r2v = sqrt(q2);  // |v2|, or the dielectric's sin θ
    d3 u2 = v2;
    if (lamb || metal || iso) u2 = divs(v2, r2v);

    // stage 3: the scattered direction
    double rd = 0.0;  // the first draw: the Lambertian's r1, the dielectric's Schlick draw
    if (lamb || diel) rd = wy_f64(rng);
    d3 w3 = mk(0.0, 0.0, 0.0), n3 = h.n;
    double q3 = 1.0;
    bool third = false;  // the lane finishes with the stage-3 sqrt
    if (lamb) {
        // random_cosine_direction (util.rs:48-60), r2^(1/4) quirk kept; ONB transform
        const d3 vv = u2;
        const d3 uu = cross(u1, vv);
        double r1 = rd;
        double r2 = wy_f64(rng);
        double phi = 2.0 * PI * r1;
        double r2s = sqrt(r2);
        double sp, cp;
        sincos(phi, &sp, &cp);
        double q = sqrt(r2s);
        d3 cd = mk(cp * q, sp * q, sqrt(1.0 - r2));
        w3 = add(add(muls(uu, cd.x), muls(vv, cd.y)), muls(u1, cd.z));
        q3 = len2(w3);
        third = true;
        o.cont = 1;
    } else if (metal) {
        const d3 reflected = add(u1, muls(u2, m->param));
        if (dot(reflected, h.n) > 0.0) {
            o.dir = reflected;
            o.cont = 1;
        } else {
            o.col = mk(0.0, 0.0, 0.0);  // absorbed
        }
    } else if (iso) {
        o.dir = u2;
        o.cont = 1;
    } else if (diel) {
        const d3 ud = u1;
        double sin_theta = r2v;
        bool cannot_refract = ri * sin_theta > 1.0;
        double r0 = (1.0 - ri) / (1.0 + ri);
        r0 = r0 * r0;
        double x = 1.0 - cos_theta;
        double x2 = x * x;
        double x4 = x2 * x2;
        double refl = r0 + (1.0 - r0) * (x * x4);  // powi(x, 5) as LLVM expands it
        bool fresnel = refl > rd;
        if (cannot_refract || fresnel) {
            o.dir = reflect(ud, h.n);
        } else {  // refract (vec3.rs:57-62)
            double ct = fmin(dot(h.n, neg(ud)), 1.0);
            w3 = muls(add(ud, muls(h.n, ct)), ri);
            q3 = fabs(1.0 - len2(w3));
            third = true;
        }
        o.cont = 1;
    }
    if (third) {
        const double r3 = sqrt(q3);
        if (lamb) o.dir = divs(w3, r3);                    // unit(cosine direction)
        else o.dir = add(w3, muls(n3, -r3));               // r_out_perp + r_out_parallel
    }
    return o;
}

// ---- split shading (scenes with at most two of: sky, Lambertian, metal, dielectric,
// isotropic): one divergent branch per case, no select overhead.
// Camera::sample_background / HDRI::sample (camera.rs:228-233, 257-270).
__device__ GS_NOINLINE d3 background(const DevScene& sc, d3 dir, unsigned long long* cnt) {
    const gs_background& bg = sc.bg;
    if (bg.kind == GS_BG_SOLID) return ld3(bg.color);
    d3 rv = mk(dir.x * bg.rot[0] + dir.y * bg.rot[1] + dir.z * bg.rot[2],
               dir.x * bg.rot[3] + dir.y * bg.rot[4] + dir.z * bg.rot[5],
               dir.x * bg.rot[6] + dir.y * bg.rot[7] + dir.z * bg.rot[8]);
    return hdri_texel(sc, unit(rv), cnt);
}

__device__ __forceinline__ d3 random_unit_vector(uint64_t& rng) {  // util.rs:18-29
    d3 v;
#pragma unroll 1
    for (;;) {
        double x = wy_f64(rng) * 2.0 + -1.0;
        double y = wy_f64(rng) * 2.0 + -1.0;
        double z = wy_f64(rng) * 2.0 + -1.0;
        v = mk(x, y, z);
        if (len2(v) < 1.0) break;
    }
    return unit(v);
}

// Material::emitted + Material::scatter (material.rs).  kind: 0 = path ends with
// `col` (emitted colour; 0 for an absorbed ray), 1 = continues along `dir` with
// attenuation `col`.
struct Scatter {
    d3 col, dir;
    uint64_t rng;
    uint32_t cont;
};

__device__ GS_NOINLINE Scatter scatter(const DevScene& sc, HitRec h, d3 in_dir, uint64_t rng,
                                        unsigned long long* cnt) {
    const DMaterial& m = sc.mats[h.mat];
    Scatter s;
    s.cont = 0;
    s.col = mk(0.0, 0.0, 0.0);
    s.dir = mk(0.0, 0.0, 0.0);
    const uint32_t kind = m.kind;
    if (kind <= DM_LAMB_TEX) {  // Lambertian :45-68
        s.col = kind == DM_LAMB_SOLID ? ld3(m.a)
              : kind == DM_LAMB_CHECKER ? checker(m, h.p)
                                        : texture_value(sc, m.texture, h.u, h.v, h.p, cnt);
        // OrthonormalBasis::new (ONB.rs:10-23)
        d3 w = unit(h.n);
        d3 a = fabs(w.x) > 0.9 ? mk(0.0, 1.0, 0.0) : mk(1.0, 0.0, 0.0);
        d3 vv = unit(cross(w, a));
        d3 uu = cross(w, vv);
        // random_cosine_direction (util.rs:48-60), r2^(1/4) quirk kept
        const double PI = 3.14159265358979323846;
        double r1 = wy_f64(rng);
        double r2 = wy_f64(rng);
        double phi = 2.0 * PI * r1;
        double r2s = sqrt(r2);
        double sp, cp;
        sincos(phi, &sp, &cp);
        double q = sqrt(r2s);
        d3 cd = mk(cp * q, sp * q, sqrt(1.0 - r2));
        s.dir = unit(add(add(muls(uu, cd.x), muls(vv, cd.y)), muls(w, cd.z)));
        s.cont = 1;
    } else if (kind == DM_METAL) {  // :87-102
        d3 reflected = reflect(in_dir, h.n);
        reflected = add(unit(reflected), muls(random_unit_vector(rng), m.param));
        if (dot(reflected, h.n) > 0.0) {
            s.col = ld3(m.a);
            s.dir = reflected;
            s.cont = 1;
        }
    } else if (kind == DM_DIELECTRIC) {  // :123-148
        double ri = h.front ? 1.0 / m.param : m.param;
        d3 ud = unit(in_dir);
        double cos_theta = fmin(dot(neg(ud), h.n), 1.0);
        double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
        bool cannot_refract = ri * sin_theta > 1.0;
        double r0 = (1.0 - ri) / (1.0 + ri);
        r0 = r0 * r0;
        double x = 1.0 - cos_theta;
        double x2 = x * x;
        double x4 = x2 * x2;
        double refl = r0 + (1.0 - r0) * (x * x4);  // powi(x, 5) as LLVM expands it
        bool fresnel = refl > wy_f64(rng);
        s.dir = (cannot_refract || fresnel) ? reflect(ud, h.n) : refract(ud, h.n, ri);
        s.col = mk(1.0, 1.0, 1.0);
        s.cont = 1;
    } else if (kind == DM_ISO_SOLID || kind == DM_ISO_TEX) {  // Isotropic :185-196
        s.col = kind == DM_ISO_SOLID ? ld3(m.a) : texture_value(sc, m.texture, h.u, h.v, h.p, cnt);
        s.dir = random_unit_vector(rng);
        s.cont = 1;
    } else {  // DiffuseLight :165-169 (emits, never scatters)
        s.col = kind == DM_LIGHT_SOLID ? ld3(m.a) : texture_value(sc, m.texture, h.u, h.v, h.p, cnt);
    }
    s.rng = rng;
    return s;
}
