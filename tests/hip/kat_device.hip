// kat_device.hip — TEST INFRASTRUCTURE: runs the megakernel's own device functions
// (grayshift_amd/csrc/device/geometry.hpp, devmath.hpp) over arrays of test cases so
// tests/test_gpu_device_kat.py can compare them bit-for-bit with the CPU oracle on
// adversarial inputs (zero / negative-zero direction components, origins on slab
// planes, tangent rays, closed/open interval ends), the shading stage (shading.hpp) for
// tests/test_gpu_shading_kat.py, the leaf stage (leaf.hpp) for tests/test_gpu_leaf_kat.py and the
// pixel stage's kernels (pixel.hpp) for tests/test_gpu_pixel_kat.py.
// Not part of the product.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../grayshift_amd/csrc/device/devmath.hpp"
#include "../../grayshift_amd/csrc/device/geometry.hpp"
#include "../../grayshift_amd/csrc/device/perlin.hpp"

using namespace gsd;

#include "../../grayshift_amd/csrc/device/leaf.hpp"     // (after the using-directive, as render.hip)
#include "../../grayshift_amd/csrc/device/shading.hpp"  // (after the using-directive: shading.hpp)
#include "../../grayshift_amd/csrc/device/pixel.hpp"    // (the pixel stage's kernels, launched as they are)

__global__ void k_aabb(int n, const double* box, const double* ray, const double* iv, int* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DNode nd{box[6 * i], box[6 * i + 1], box[6 * i + 2], box[6 * i + 3], box[6 * i + 4], box[6 * i + 5], 0, 0, 0, 0};
    d3 o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    d3 d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    d3 inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
    out[i] = box_hit(nd, o, inv, iv[2 * i], iv[2 * i + 1]) ? 1 : 0;
}

// The megakernel's node decision for cert rays: box_cert (f32, certified), and the f64
// box_hit_fast where box_cert is undecided.  out: 0/1 the decision, dec: 0 miss / 1 hit
// certified by f32, 2 undecided; -1 for rays that are not cert rays (not decided here).
__global__ void k_aabb_cert(int n, const double* box, const double* ray, const double* iv, int* out, int* dec) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* b = box + 6 * i;
    DNode nd{b[0], b[1], b[2], b[3], b[4], b[5], 0, 0, 0, 0};
    d3 o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    d3 d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    d3 inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
    bool boxes_ok = true;
    for (int k = 0; k < 6; k++) boxes_ok = boxes_ok && __builtin_fabs(b[k]) <= 1e15;
    // (the product's constants: the refined hardware reciprocal, rcp_cert; the f64 test below
    // keeps the exact 1/d, as the megakernel's inv_of)
    const d3 invc = mk(rcp_cert(d.x), rcp_cert(d.y), rcp_cert(d.z));
    if (!boxes_ok || !cert_ray_ok(o, invc)) {
        out[i] = -1;
        dec[i] = -1;
        return;
    }
    const RayCert rc = make_cert(o, invc);
    bool und;
    bool h = box_cert((float)b[0], (float)b[1], (float)b[2], (float)b[3], (float)b[4], (float)b[5], rc,
                      (float)iv[2 * i], (float)iv[2 * i + 1], und);
    dec[i] = und ? 2 : (h ? 1 : 0);
    if (und) h = box_hit_fast(nd, o, inv, iv[2 * i], iv[2 * i + 1]);
    out[i] = h ? 1 : 0;
}

// rcp_cert (the certified test's 1/d) next to the exact division, per case.
__global__ void k_rcp_cert(int n, const double* d, double* approx, double* exact) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    approx[i] = rcp_cert(d[i]);
    exact[i] = 1.0 / d[i];
}

// div_by (the sphere roots' division through a refined reciprocal) next to the exact quotient.
__global__ void k_div_by(int n, const double* num, const double* den, double* fast, double* exact) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fast[i] = div_by(num[i], den[i], rcp_cert(den[i]));
    exact[i] = num[i] / den[i];
}

__global__ void k_sphere(int n, const double* sph, const double* ray, const double* iv, double* t, int* hit) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    r.d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    r.time = 0.0;
    double tt = 0.0;
    bool h = sphere_accept(mk(sph[4 * i], sph[4 * i + 1], sph[4 * i + 2]), sph[4 * i + 3], r, len2(r.d), iv[2 * i],
                           iv[2 * i + 1], tt);
    hit[i] = h ? 1 : 0;
    t[i] = tt;
}

__global__ void k_tri(int n, const double* tri, const double* ray, double* tuv, int* hit) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gs_triangle g;
    for (int k = 0; k < 3; k++) {
        g.a[k] = tri[9 * i + k];
        g.b[k] = tri[9 * i + 3 + k];
        g.c[k] = tri[9 * i + 6 + k];
    }
    Ray r;
    r.o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    r.d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    r.time = 0.0;
    double t = 0, u = 0, v = 0;
    hit[i] = tri_hit(g, r, t, u, v) ? 1 : 0;
    tuv[3 * i] = t;
    tuv[3 * i + 1] = u;
    tuv[3 * i + 2] = v;
}

__global__ void k_rng(int n, const uint64_t* seed, const uint32_t* pix, const uint32_t* smp, int draws, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t st = stream_seed(seed[i], pix[i], smp[i]);
    for (int k = 0; k < draws; k++) out[(size_t)i * draws + k] = wy_f64(st);
}

// which: 0 sin, 1 cos, 2 acos, 3 asin, 4 atan2(x, y), 5 log (medium_test's free-flight draw),
// 6 ldexp(1.0, (int)x - 136) (hdri_texel's RGBE scale for exponent byte x)
__global__ void k_math(int n, int which, const double* x, const double* y, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r;
    if (which == 0) {
        double s, c;
        sincos(x[i], &s, &c);
        r = s;
    } else if (which == 1) {
        double s, c;
        sincos(x[i], &s, &c);
        r = c;
    } else if (which == 2) {
        r = acos(x[i]);
    } else if (which == 3) {
        r = asin(x[i]);
    } else if (which == 5) {
        r = log(x[i]);
    } else if (which == 6) {
        r = ldexp(1.0, (int)x[i] - 136);
    } else {
        r = atan2(x[i], y[i]);
    }
    out[i] = r;
}

// The sky texel index: f32 certified (-1, -1 when undecided) and the f64 reference path.
__global__ void k_sky(int n, uint32_t W, uint32_t H, const double* dir, int* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const d3 r = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    uint32_t x = 0, y = 0, x64 = 0, y64 = 0;
    const bool ok = sky_index_f32(r, W, H, x, y);
    sky_index_f64(r, W, H, x64, y64);
    out[4 * i] = ok ? (int)x : -1;
    out[4 * i + 1] = ok ? (int)y : -1;
    out[4 * i + 2] = (int)x64;
    out[4 * i + 3] = (int)y64;
}

template <class T>
static T* dcopy(const T* h, size_t n) {
    T* d = nullptr;
    if (hipMalloc(&d, n * sizeof(T) + 8) != hipSuccess) return nullptr;
    if (h) (void)hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
    return d;
}
template <class T>
static void back(T* h, T* d, size_t n) {
    (void)hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    (void)hipFree(d);
}
static dim3 grid(int n) { return dim3((unsigned)((n + 255) / 256)); }

// perlin3 (which 0) or NoiseTexture's channel value at scale s (which 1) per point.
__global__ void k_noise(int n, int which, const uint8_t* perm, double scale, const double* p, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* q = p + 3 * i;
    out[i] = which == 0 ? perlin3(perm, q[0], q[1], q[2]) : noise_value(perm, scale, q[0], q[1], q[2]);
}

// quad_accept over the product's own quad records (the host's normal, D and w derivation).
__global__ void k_quad(int n, const gs_quad* q, const double* ray, const double* iv, double* t, int* hit) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    r.d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    r.time = 0.0;
    double tt = 0.0;
    hit[i] = quad_accept(q[i], r, iv[2 * i], iv[2 * i + 1], tt) ? 1 : 0;
    t[i] = tt;
}

// The sphere tests of the leaf runs.  which: 0 sphere_accept_rr_ra; 1 sphere_disc_rr, then
// sphere_root_take for a real discriminant; 2 the same with sphere_root_take_ra.  As in the
// megakernel, rr = r * r is taken once and ra = rcp_cert(a); the _ra forms are for a in
// [2^-900, 2^900] (the caller's cases).
__global__ void k_sphere_run(int n, int which, const double* sph, const double* ray, const double* iv, double* t,
                             int* hit) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    r.d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    r.time = 0.0;
    const d3 c = mk(sph[4 * i], sph[4 * i + 1], sph[4 * i + 2]);
    const double rr = sph[4 * i + 3] * sph[4 * i + 3];
    const double a = len2(r.d), ra = rcp_cert(a);
    const double tmin = iv[2 * i], tmax = iv[2 * i + 1];
    double tt = 0.0;
    bool h;
    if (which == 0) {
        h = sphere_accept_rr_ra(c, rr, r, a, ra, tmin, tmax, tt);
    } else {
        const SphereDisc q = sphere_disc_rr(c, rr, r, a);
        const bool real = !(q.disc < 0.0);
        h = real && (which == 1 ? sphere_root_take(q.h, q.disc, a, tmin, tmax, tt)
                                : sphere_root_take_ra(q.h, q.disc, a, ra, tmin, tmax, tt));
    }
    hit[i] = h ? 1 : 0;
    t[i] = tt;
}

// which: 0 box_hit, 1 box_hit_v, 2 box_hit_fast (-1 where fast_slab_ray does not hold: the
// megakernel does not call it there)
__global__ void k_box(int n, int which, const double* box, const double* ray, const double* iv, int* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DNode nd{box[6 * i], box[6 * i + 1], box[6 * i + 2], box[6 * i + 3], box[6 * i + 4], box[6 * i + 5], 0, 0, 0, 0};
    d3 o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    d3 d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    d3 inv = mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
    const double tmin = iv[2 * i], tmax = iv[2 * i + 1];
    int r;
    if (which == 0) r = box_hit(nd, o, inv, tmin, tmax) ? 1 : 0;
    else if (which == 1) r = box_hit_v(nd, o, inv, tmin, tmax) ? 1 : 0;
    else r = fast_slab_ray(o, inv) ? (box_hit_fast(nd, o, inv, tmin, tmax) ? 1 : 0) : -1;
    out[i] = r;
}

// A chain of up to three instances per case (kind 0: none): inst_forward on the ray outermost
// first, then inst_backward on (p, n) innermost first, as the megakernel walks a chain.
__global__ void k_inst(int n, const int* kind, const double* par, const double* ray, const double* pn, double* ray_out,
                       double* pn_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gs_instance in[3];
    for (int k = 0; k < 3; k++) {
        in[k].kind = (uint32_t)kind[3 * i + k];
        in[k].child = 0;
        for (int j = 0; j < 3; j++) in[k].p[j] = par[9 * i + 3 * k + j];
    }
    Ray r;
    r.o = mk(ray[6 * i], ray[6 * i + 1], ray[6 * i + 2]);
    r.d = mk(ray[6 * i + 3], ray[6 * i + 4], ray[6 * i + 5]);
    r.time = 0.0;
    for (int k = 0; k < 3; k++)
        if (in[k].kind) inst_forward(in[k], r);
    d3 p = mk(pn[6 * i], pn[6 * i + 1], pn[6 * i + 2]), nn = mk(pn[6 * i + 3], pn[6 * i + 4], pn[6 * i + 5]);
    for (int k = 2; k >= 0; k--)
        if (in[k].kind) inst_backward(in[k], p, nn);
    const double ro[6] = {r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z};
    const double po[6] = {p.x, p.y, p.z, nn.x, nn.y, nn.z};
    for (int j = 0; j < 6; j++) {
        ray_out[6 * i + j] = ro[j];
        pn_out[6 * i + j] = po[j];
    }
}

// which: 0 reflect(v, n), 1 refract(v, n, ratio)
__global__ void k_vec(int n, int which, const double* v, const double* nrm, const double* ratio, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const d3 a = mk(v[3 * i], v[3 * i + 1], v[3 * i + 2]), b = mk(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    const d3 r = which == 0 ? reflect(a, b) : refract(a, b, ratio[i]);
    out[3 * i] = r.x;
    out[3 * i + 1] = r.y;
    out[3 * i + 2] = r.z;
}

__global__ void k_color_byte(int n, const double* c, int* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (int)color_byte(c[i]);
}

// which: 0 sat_i32 (sign-extended), 1 sat_u64 clamped to u64 (HDRI::sample's `as usize`),
// 2 sat_u64 clamped to u32
__global__ void k_sat(int n, int which, const double* f, uint64_t* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = which == 0   ? (uint64_t)(int64_t)sat_i32(f[i])
             : which == 1 ? sat_u64(f[i], 18446744073709551616.0, ~0ull)
                          : sat_u64(f[i], 4294967295.0, 4294967295ull);
}

__global__ void k_udiv(int n, const uint32_t* num, const UDiv* u, uint32_t* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = udiv(num[i], u[i]);
}

// ---- the shading stage (shading.hpp) over the product's own device scene record, passed by
// value as the render kernels' parameter block holds it.  One thread per case; cnt: C_N counters.
__device__ __forceinline__ Ray ray_of(const double* r) {
    Ray y;
    y.o = mk(r[0], r[1], r[2]);
    y.d = mk(r[3], r[4], r[5]);
    y.time = r[6];
    return y;
}
__device__ __forceinline__ void st3(double* o, d3 v) {
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
}

// which: 0 reconstruct<false>, 1 reconstruct<true>, 2 reconstruct_sphere<true>, 3
// reconstruct_sphere<false>.  ray: o, d, time; refs: hit_ref, hit_inst, hit_outer.
// out: p, n, u, v; mf: mat, front.
__global__ void k_reconstruct(int n, int which, DevScene sc, const double* ray, const double* t, const uint32_t* refs,
                              double* out, uint32_t* mf, unsigned long long* cnt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Ray r = ray_of(ray + 7 * i);
    const uint32_t ref = refs[3 * i], inst = refs[3 * i + 1], outer = refs[3 * i + 2];
    HitRec h;
    if (which == 0) h = reconstruct<false>(sc, r, t[i], ref, inst, outer);
    else if (which == 1) h = reconstruct<true>(sc, r, t[i], ref, inst, outer);
    else if (which == 2) h = reconstruct_sphere<true>(sc, r, t[i], ref);
    else h = reconstruct_sphere<false>(sc, r, t[i], ref);
    st3(out + 8 * i, h.p);
    st3(out + 8 * i + 3, h.n);
    out[8 * i + 6] = h.u;
    out[8 * i + 7] = h.v;
    mf[2 * i] = h.mat;
    mf[2 * i + 1] = h.front ? 1u : 0u;
}

// which 0: texture_value(idx, u, v, p); 1: checker(mats[idx], p).  uvp: u, v, p.
__global__ void k_texture(int n, int which, DevScene sc, const uint32_t* idx, const double* uvp, double* out,
                          unsigned long long* cnt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* a = uvp + 5 * i;
    const d3 p = mk(a[2], a[3], a[4]);
    st3(out + 3 * i, which == 0 ? texture_value(sc, idx[i], a[0], a[1], p, cnt) : checker(sc.mats[idx[i]], p));
}

// scatter() on a given HitRec (hr: p, n, u, v; mf: mat, front), in_dir and stream state.
// out: col, dir; cont; the stream state after.
__global__ void k_scatter(int n, DevScene sc, const double* hr, const uint32_t* mf, const double* in_dir,
                          const uint64_t* rng, double* out, uint32_t* cont, uint64_t* rng_out, unsigned long long* cnt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    HitRec h;
    h.p = mk(hr[8 * i], hr[8 * i + 1], hr[8 * i + 2]);
    h.n = mk(hr[8 * i + 3], hr[8 * i + 4], hr[8 * i + 5]);
    h.u = hr[8 * i + 6];
    h.v = hr[8 * i + 7];
    h.mat = mf[2 * i];
    h.front = mf[2 * i + 1] != 0;
    const Scatter s = scatter(sc, h, mk(in_dir[3 * i], in_dir[3 * i + 1], in_dir[3 * i + 2]), rng[i], cnt);
    st3(out + 6 * i, s.col);
    st3(out + 6 * i + 3, s.dir);
    cont[i] = s.cont;
    rng_out[i] = s.rng;
}

// which: 0 shade<0,0,0>, 1 shade<0,0,1>, 2 shade<0,1,0>, 3 shade<1,1,0>.  A miss has hit_ref
// GS_REF_NONE.  out: col, dir, the new ray.o; cont; the stream state after.
__global__ void k_shade(int n, int which, DevScene sc, const double* ray, const double* t, const uint32_t* refs,
                        const uint64_t* rng, double* out, uint32_t* cont, uint64_t* rng_out, unsigned long long* cnt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r = ray_of(ray + 7 * i);
    const uint32_t ref = refs[3 * i], inst = refs[3 * i + 1], outer = refs[3 * i + 2];
    uint64_t st = rng[i];
    ShadeOut o;
    if (which == 0) o = shade<false, false, false>(sc, r, t[i], ref, inst, st, cnt, outer);
    else if (which == 1) o = shade<false, false, true>(sc, r, t[i], ref, inst, st, cnt, outer);
    else if (which == 2) o = shade<false, true, false>(sc, r, t[i], ref, inst, st, cnt, outer);
    else o = shade<true, true, false>(sc, r, t[i], ref, inst, st, cnt, outer);
    st3(out + 9 * i, o.col);
    st3(out + 9 * i + 3, o.dir);
    st3(out + 9 * i + 6, r.o);
    cont[i] = o.cont;
    rng_out[i] = st;
}

__global__ void k_background(int n, DevScene sc, const double* dir, double* out, unsigned long long* cnt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st3(out + 3 * i, background(sc, mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]), cnt));
}

// ---- the leaf stage (leaf.hpp): leaf_other<FEAT, UNI> on the product's device scene, its quad
// traversal records and cube records, one thread per case; a case whose ref is GS_REF_NONE is an
// inactive lane (padding).  The block mirrors the first n_lds quad records and n_lcubes cube
// records in dynamic LDS as gs_render_kernel does (quads first, then cubes, 16 B at a time).
// flags (6 per case): hit, ref, inst, enter, HitRec mat, front.  out (21 per case): t, the ray as
// leaf_other left it (o, d), the HitRec of reconstruct on a hit (p, n, u, v), and for enter != 0
// the f64 box of the entered tree's root node.  cnt: C_N counters per case.  nonuni: set when a
// UNI wave's active lanes did not share one ref.
#define KAT_LEAF_FLAGS 6
#define KAT_LEAF_OUT 21
template <int FEAT, bool UNI>
__device__ __forceinline__ void leaf_case(const DevScene& sc, const QuadSrc& qs, uint32_t ref, const double* ray,
                                          const double* iv, uint64_t rng, uint32_t* flags, double* out,
                                          uint64_t* rng_out, unsigned long long* cnt, uint32_t* nonuni) {
    const Ray r0 = ray_of(ray);
    Ray rl = r0;
    LeafHit lh;
    if (UNI) {  // the wave's ref by readfirstlane, as the leaf pass takes it
        const uint32_t first = __builtin_amdgcn_readfirstlane(ref);
        if (__builtin_amdgcn_ballot_w64(ref != first) != 0) atomicOr(nonuni, 1u);
        lh = leaf_other<FEAT, true>(sc, qs, first, rl, iv[0], iv[1], rng, cnt);
    } else {
        lh = leaf_other<FEAT, false>(sc, qs, ref, rl, iv[0], iv[1], rng, cnt);
    }
    flags[0] = lh.hit ? 1u : 0u;
    flags[1] = lh.ref;
    flags[2] = lh.inst;
    flags[3] = lh.enter;
    flags[4] = 0xFFFFFFFFu;
    flags[5] = 0u;
    out[0] = lh.t;
    st3(out + 1, rl.o);
    st3(out + 4, rl.d);
    for (int k = 7; k < KAT_LEAF_OUT; k++) out[k] = 0.0;
    if (lh.hit) {
        const HitRec h = reconstruct<(FEAT & GS_FEAT_GENERAL) != 0>(sc, r0, lh.t, lh.ref, lh.inst, GS_REF_NONE);
        st3(out + 7, h.p);
        st3(out + 10, h.n);
        out[13] = h.u;
        out[14] = h.v;
        flags[4] = h.mat;
        flags[5] = h.front ? 1u : 0u;
    }
    if ((FEAT & GS_FEAT_NESTED) && lh.enter != 0) {
        const uint32_t link = sc.nroots[lh.enter - 1u];
        if (link < THR_END) {
            const DNode b = box64(sc.tboxes[link >> 5]);
            out[15] = b.mnx; out[16] = b.mny; out[17] = b.mnz;
            out[18] = b.mxx; out[19] = b.mxy; out[20] = b.mxz;
        }
    }
    *rng_out = rng;
}

// which = 2 * f + uni; f: 0 no feature, 1 MEDIA, 2 NESTED, 3 MEDIA | NESTED, 4 MEDIA | NESTED | GENERAL
__global__ void k_leaf(int n, int which, DevScene sc, const TQuad* tquads, uint32_t n_lds, uint32_t n_lcubes,
                       const uint32_t* refs, const double* ray, const double* iv, const uint64_t* rng, uint32_t* flags,
                       double* out, uint64_t* rng_out, unsigned long long* cnt, uint32_t* nonuni) {
    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t* s_quads = smem;
    uint8_t* s_cubes = s_quads + (size_t)n_lds * sizeof(TQuad);
    {
        const uint4* src = reinterpret_cast<const uint4*>(tquads);
        uint4* dst = reinterpret_cast<uint4*>(s_quads);
        for (uint32_t k = threadIdx.x; k < n_lds * 8u; k += blockDim.x) dst[k] = src[k];
        src = reinterpret_cast<const uint4*>(sc.cubes);
        dst = reinterpret_cast<uint4*>(s_cubes);
        for (uint32_t k = threadIdx.x; k < n_lcubes * (GS_CUBE_DOUBLES / 2); k += blockDim.x) dst[k] = src[k];
    }
    const QuadSrc qs{s_quads, tquads, n_lds, s_cubes, n_lcubes};
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ref = refs[i];
    if (ref == GS_REF_NONE) return;
#define KAT_LEAF(F, U) \
    leaf_case<F, U>(sc, qs, ref, ray + 7 * i, iv + 2 * i, rng[i], flags + KAT_LEAF_FLAGS * i, out + KAT_LEAF_OUT * i, \
                    rng_out + i, cnt + (size_t)C_N * i, nonuni)
    switch (which) {
        case 0: KAT_LEAF(0, false); break;
        case 1: KAT_LEAF(0, true); break;
        case 2: KAT_LEAF(GS_FEAT_MEDIA, false); break;
        case 3: KAT_LEAF(GS_FEAT_MEDIA, true); break;
        case 4: KAT_LEAF(GS_FEAT_NESTED, false); break;
        case 5: KAT_LEAF(GS_FEAT_NESTED, true); break;
        case 6: KAT_LEAF(GS_FEAT_MEDIA | GS_FEAT_NESTED, false); break;
        case 7: KAT_LEAF(GS_FEAT_MEDIA | GS_FEAT_NESTED, true); break;
        case 8: KAT_LEAF(GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_GENERAL, false); break;
        case 9: KAT_LEAF(GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_GENERAL, true); break;
        default: break;
    }
#undef KAT_LEAF
}

extern "C" {

int kat_aabb(int n, const double* box, const double* ray, const double* iv, int* out) {
    double *db = dcopy(box, 6 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n), *di = dcopy(iv, 2 * (size_t)n);
    int* dout = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_aabb, grid(n), dim3(256), 0, 0, n, db, dr, di, dout);
    back(out, dout, n);
    (void)hipFree(db); (void)hipFree(dr); (void)hipFree(di);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_aabb_cert(int n, const double* box, const double* ray, const double* iv, int* out, int* dec) {
    double *db = dcopy(box, 6 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n), *di = dcopy(iv, 2 * (size_t)n);
    int* dout = dcopy<int>(nullptr, n);
    int* ddec = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_aabb_cert, grid(n), dim3(256), 0, 0, n, db, dr, di, dout, ddec);
    back(out, dout, n);
    back(dec, ddec, n);
    (void)hipFree(db); (void)hipFree(dr); (void)hipFree(di);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_rcp_cert(int n, const double* d, double* approx, double* exact) {
    double* dd = dcopy(d, n);
    double *da = dcopy<double>(nullptr, n), *de = dcopy<double>(nullptr, n);
    hipLaunchKernelGGL(k_rcp_cert, grid(n), dim3(256), 0, 0, n, dd, da, de);
    back(approx, da, n);
    back(exact, de, n);
    (void)hipFree(dd);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_div_by(int n, const double* num, const double* den, double* fast, double* exact) {
    double *dn = dcopy(num, n), *dd = dcopy(den, n);
    double *df = dcopy<double>(nullptr, n), *de = dcopy<double>(nullptr, n);
    hipLaunchKernelGGL(k_div_by, grid(n), dim3(256), 0, 0, n, dn, dd, df, de);
    back(fast, df, n);
    back(exact, de, n);
    (void)hipFree(dn); (void)hipFree(dd);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_sphere(int n, const double* sph, const double* ray, const double* iv, double* t, int* hit) {
    double *ds = dcopy(sph, 4 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n), *di = dcopy(iv, 2 * (size_t)n);
    double* dt = dcopy<double>(nullptr, n);
    int* dh = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_sphere, grid(n), dim3(256), 0, 0, n, ds, dr, di, dt, dh);
    back(t, dt, n);
    back(hit, dh, n);
    (void)hipFree(ds); (void)hipFree(dr); (void)hipFree(di);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_tri(int n, const double* tri, const double* ray, double* tuv, int* hit) {
    double *dt = dcopy(tri, 9 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n);
    double* dtuv = dcopy<double>(nullptr, 3 * (size_t)n);
    int* dh = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_tri, grid(n), dim3(256), 0, 0, n, dt, dr, dtuv, dh);
    back(tuv, dtuv, 3 * (size_t)n);
    back(hit, dh, n);
    (void)hipFree(dt); (void)hipFree(dr);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_rng(int n, const uint64_t* seed, const uint32_t* pix, const uint32_t* smp, int draws, double* out) {
    uint64_t* ds = dcopy(seed, n);
    uint32_t *dp = dcopy(pix, n), *dm = dcopy(smp, n);
    double* dout = dcopy<double>(nullptr, (size_t)n * draws);
    hipLaunchKernelGGL(k_rng, grid(n), dim3(256), 0, 0, n, ds, dp, dm, draws, dout);
    back(out, dout, (size_t)n * draws);
    (void)hipFree(ds); (void)hipFree(dp); (void)hipFree(dm);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_math(int n, int which, const double* x, const double* y, double* out) {
    double *dx = dcopy(x, n), *dy = dcopy(y ? y : x, n);
    double* dout = dcopy<double>(nullptr, n);
    hipLaunchKernelGGL(k_math, grid(n), dim3(256), 0, 0, n, which, dx, dy, dout);
    back(out, dout, n);
    (void)hipFree(dx); (void)hipFree(dy);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_sky(int n, uint32_t W, uint32_t H, const double* dir, int* out) {
    double* dd = dcopy(dir, 3 * (size_t)n);
    int* dout = dcopy<int>(nullptr, 4 * (size_t)n);
    hipLaunchKernelGGL(k_sky, grid(n), dim3(256), 0, 0, n, W, H, dd, dout);
    back(out, dout, 4 * (size_t)n);
    (void)hipFree(dd);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_noise(int n, int which, const uint8_t* perm256, double scale, const double* p, double* out) {
    uint8_t* dperm = dcopy(perm256, 256);
    double* dp = dcopy(p, 3 * (size_t)n);
    double* dout = dcopy<double>(nullptr, n);
    hipLaunchKernelGGL(k_noise, grid(n), dim3(256), 0, 0, n, which, dperm, scale, dp, dout);
    back(out, dout, n);
    (void)hipFree(dperm); (void)hipFree(dp);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_quad(int n, const void* quads, const double* ray, const double* iv, double* t, int* hit) {
    gs_quad* dq = dcopy((const gs_quad*)quads, (size_t)n);
    double *dr = dcopy(ray, 6 * (size_t)n), *di = dcopy(iv, 2 * (size_t)n);
    double* dt = dcopy<double>(nullptr, n);
    int* dh = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_quad, grid(n), dim3(256), 0, 0, n, dq, dr, di, dt, dh);
    back(t, dt, n);
    back(hit, dh, n);
    (void)hipFree(dq); (void)hipFree(dr); (void)hipFree(di);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_sphere_run(int n, int which, const double* sph, const double* ray, const double* iv, double* t, int* hit) {
    double *ds = dcopy(sph, 4 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n), *di = dcopy(iv, 2 * (size_t)n);
    double* dt = dcopy<double>(nullptr, n);
    int* dh = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_sphere_run, grid(n), dim3(256), 0, 0, n, which, ds, dr, di, dt, dh);
    back(t, dt, n);
    back(hit, dh, n);
    (void)hipFree(ds); (void)hipFree(dr); (void)hipFree(di);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_box(int n, int which, const double* box, const double* ray, const double* iv, int* out) {
    double *db = dcopy(box, 6 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n), *di = dcopy(iv, 2 * (size_t)n);
    int* dout = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_box, grid(n), dim3(256), 0, 0, n, which, db, dr, di, dout);
    back(out, dout, n);
    (void)hipFree(db); (void)hipFree(dr); (void)hipFree(di);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_inst(int n, const int* kind, const double* par, const double* ray, const double* pn, double* ray_out,
             double* pn_out) {
    int* dk = dcopy(kind, 3 * (size_t)n);
    double *dp = dcopy(par, 9 * (size_t)n), *dr = dcopy(ray, 6 * (size_t)n), *dn = dcopy(pn, 6 * (size_t)n);
    double *dro = dcopy<double>(nullptr, 6 * (size_t)n), *dpo = dcopy<double>(nullptr, 6 * (size_t)n);
    hipLaunchKernelGGL(k_inst, grid(n), dim3(256), 0, 0, n, dk, dp, dr, dn, dro, dpo);
    back(ray_out, dro, 6 * (size_t)n);
    back(pn_out, dpo, 6 * (size_t)n);
    (void)hipFree(dk); (void)hipFree(dp); (void)hipFree(dr); (void)hipFree(dn);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_vec(int n, int which, const double* v, const double* nrm, const double* ratio, double* out) {
    double *dv = dcopy(v, 3 * (size_t)n), *dn = dcopy(nrm, 3 * (size_t)n), *dr = dcopy(ratio, n);
    double* dout = dcopy<double>(nullptr, 3 * (size_t)n);
    hipLaunchKernelGGL(k_vec, grid(n), dim3(256), 0, 0, n, which, dv, dn, dr, dout);
    back(out, dout, 3 * (size_t)n);
    (void)hipFree(dv); (void)hipFree(dn); (void)hipFree(dr);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_color_byte(int n, const double* c, int* out) {
    double* dc = dcopy(c, n);
    int* dout = dcopy<int>(nullptr, n);
    hipLaunchKernelGGL(k_color_byte, grid(n), dim3(256), 0, 0, n, dc, dout);
    back(out, dout, n);
    (void)hipFree(dc);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int kat_sat(int n, int which, const double* f, uint64_t* out) {
    double* df = dcopy(f, n);
    uint64_t* dout = dcopy<uint64_t>(nullptr, n);
    hipLaunchKernelGGL(k_sat, grid(n), dim3(256), 0, 0, n, which, df, dout);
    back(out, dout, n);
    (void)hipFree(df);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

// udiv(num, udiv_make(den)): the magic made on the host, as the launches make it
int kat_udiv(int n, const uint32_t* num, const uint32_t* den, uint32_t* out) {
    UDiv* hu = new UDiv[(size_t)n > 0 ? (size_t)n : 1];
    for (int i = 0; i < n; i++) hu[i] = gsd::udiv_make(den[i]);
    uint32_t* dn = dcopy(num, n);
    UDiv* du = dcopy(hu, n);
    delete[] hu;
    uint32_t* dout = dcopy<uint32_t>(nullptr, n);
    hipLaunchKernelGGL(k_udiv, grid(n), dim3(256), 0, 0, n, dn, du, dout);
    back(out, dout, n);
    (void)hipFree(dn); (void)hipFree(du);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

// ---- the shading stage.  scene: the record gs_debug_device_scene_record copied out
// (kat_dev_scene_bytes() bytes); cnt: C_N (kat_counters()) u64, the launch's counters.
int kat_dev_scene_bytes(void) { return (int)sizeof(DevScene); }
int kat_counters(void) { return (int)C_N; }
// The slot of a counter the shading tests read: 0 hits, 1 image texels, 2 HDRI texels, 3 noise evaluations.
int kat_counter_slot(int which) {
    return which == 0 ? (int)C_HITS : which == 1 ? (int)C_IMG : which == 2 ? (int)C_HDRI : which == 3 ? (int)C_NOISE : -1;
}
int kat_dev_scene_rgbe(const void* scene) { return ((const DevScene*)scene)->hdri_rgbe != nullptr ? 1 : 0; }

static unsigned long long* cnt_new() {
    unsigned long long* d = dcopy<unsigned long long>(nullptr, C_N);
    if (d) (void)hipMemset(d, 0, C_N * sizeof(unsigned long long));
    return d;
}
static int finish(unsigned long long* cnt, unsigned long long* dcnt) {
    const hipError_t e = hipDeviceSynchronize();
    back(cnt, dcnt, C_N);
    return e == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1;
}

int kat_reconstruct(int n, int which, const void* scene, const double* ray, const double* t, const uint32_t* refs,
                    double* out, uint32_t* mf, unsigned long long* cnt) {
    const DevScene sc = *(const DevScene*)scene;
    double *dr = dcopy(ray, 7 * (size_t)n), *dt = dcopy(t, n);
    uint32_t* df = dcopy(refs, 3 * (size_t)n);
    double* dout = dcopy<double>(nullptr, 8 * (size_t)n);
    uint32_t* dmf = dcopy<uint32_t>(nullptr, 2 * (size_t)n);
    unsigned long long* dcnt = cnt_new();
    hipLaunchKernelGGL(k_reconstruct, grid(n), dim3(256), 0, 0, n, which, sc, dr, dt, df, dout, dmf, dcnt);
    const int rc = finish(cnt, dcnt);
    back(out, dout, 8 * (size_t)n);
    back(mf, dmf, 2 * (size_t)n);
    (void)hipFree(dr); (void)hipFree(dt); (void)hipFree(df);
    return rc;
}

int kat_texture(int n, int which, const void* scene, const uint32_t* idx, const double* uvp, double* out,
                unsigned long long* cnt) {
    const DevScene sc = *(const DevScene*)scene;
    uint32_t* di = dcopy(idx, n);
    double* du = dcopy(uvp, 5 * (size_t)n);
    double* dout = dcopy<double>(nullptr, 3 * (size_t)n);
    unsigned long long* dcnt = cnt_new();
    hipLaunchKernelGGL(k_texture, grid(n), dim3(256), 0, 0, n, which, sc, di, du, dout, dcnt);
    const int rc = finish(cnt, dcnt);
    back(out, dout, 3 * (size_t)n);
    (void)hipFree(di); (void)hipFree(du);
    return rc;
}

int kat_scatter(int n, const void* scene, const double* hr, const uint32_t* mf, const double* in_dir,
                const uint64_t* rng, double* out, uint32_t* cont, uint64_t* rng_out, unsigned long long* cnt) {
    const DevScene sc = *(const DevScene*)scene;
    double *dh = dcopy(hr, 8 * (size_t)n), *dd = dcopy(in_dir, 3 * (size_t)n);
    uint32_t* dmf = dcopy(mf, 2 * (size_t)n);
    uint64_t* dg = dcopy(rng, n);
    double* dout = dcopy<double>(nullptr, 6 * (size_t)n);
    uint32_t* dc = dcopy<uint32_t>(nullptr, n);
    uint64_t* dgo = dcopy<uint64_t>(nullptr, n);
    unsigned long long* dcnt = cnt_new();
    hipLaunchKernelGGL(k_scatter, grid(n), dim3(256), 0, 0, n, sc, dh, dmf, dd, dg, dout, dc, dgo, dcnt);
    const int rc = finish(cnt, dcnt);
    back(out, dout, 6 * (size_t)n);
    back(cont, dc, n);
    back(rng_out, dgo, n);
    (void)hipFree(dh); (void)hipFree(dd); (void)hipFree(dmf); (void)hipFree(dg);
    return rc;
}

int kat_shade(int n, int which, const void* scene, const double* ray, const double* t, const uint32_t* refs,
              const uint64_t* rng, double* out, uint32_t* cont, uint64_t* rng_out, unsigned long long* cnt) {
    const DevScene sc = *(const DevScene*)scene;
    double *dr = dcopy(ray, 7 * (size_t)n), *dt = dcopy(t, n);
    uint32_t* df = dcopy(refs, 3 * (size_t)n);
    uint64_t* dg = dcopy(rng, n);
    double* dout = dcopy<double>(nullptr, 9 * (size_t)n);
    uint32_t* dc = dcopy<uint32_t>(nullptr, n);
    uint64_t* dgo = dcopy<uint64_t>(nullptr, n);
    unsigned long long* dcnt = cnt_new();
    hipLaunchKernelGGL(k_shade, grid(n), dim3(256), 0, 0, n, which, sc, dr, dt, df, dg, dout, dc, dgo, dcnt);
    const int rc = finish(cnt, dcnt);
    back(out, dout, 9 * (size_t)n);
    back(cont, dc, n);
    back(rng_out, dgo, n);
    (void)hipFree(dr); (void)hipFree(dt); (void)hipFree(df); (void)hipFree(dg);
    return rc;
}

int kat_background(int n, const void* scene, const double* dir, double* out, unsigned long long* cnt) {
    const DevScene sc = *(const DevScene*)scene;
    double* dd = dcopy(dir, 3 * (size_t)n);
    double* dout = dcopy<double>(nullptr, 3 * (size_t)n);
    unsigned long long* dcnt = cnt_new();
    hipLaunchKernelGGL(k_background, grid(n), dim3(256), 0, 0, n, sc, dd, dout, dcnt);
    const int rc = finish(cnt, dcnt);
    back(out, dout, 3 * (size_t)n);
    (void)hipFree(dd);
    return rc;
}

// ---- the leaf stage.  tquads: the device array gs_debug_leaf_stage_record hands out (n_quads
// records); n_cubes: the scene's cube records; n_lds <= n_quads and n_lcubes <= n_cubes: the
// prefixes to mirror in LDS.  Outputs of inactive lanes (ref GS_REF_NONE) stay zero.  Returns 0,
// -1 after a HIP error, -2 for arguments out of range (nothing is launched).
int kat_leaf_flags(void) { return KAT_LEAF_FLAGS; }
int kat_leaf_out(void) { return KAT_LEAF_OUT; }
int kat_tquad_bytes(void) { return (int)sizeof(TQuad); }
// The slot of a test counter, in oracle_hit's order: node visits, sphere, moving sphere, quad,
// triangle, instance, list, medium tests.
int kat_leaf_counter_slot(int which) {
    const int slots[8] = {C_NODES, C_SPH, C_MSPH, C_QUAD, C_TRI, C_INST, C_LIST, C_MED};
    return which >= 0 && which < 8 ? slots[which] : -1;
}

int kat_leaf(int n, int which, const void* scene, const void* tquads, uint32_t n_quads, uint32_t n_cubes,
             uint32_t n_lds, uint32_t n_lcubes, const uint32_t* refs, const double* ray, const double* iv,
             const uint64_t* rng, uint32_t* flags, double* out, uint64_t* rng_out, unsigned long long* cnt,
             uint32_t* nonuni) {
    const size_t lds = (size_t)n_lds * sizeof(TQuad) + (size_t)n_lcubes * (GS_CUBE_DOUBLES * 8);
    if (n <= 0 || which < 0 || which > 9 || n_lds > n_quads || n_lcubes > n_cubes || lds > 48u * 1024u) return -2;
    if ((n_quads != 0 && !tquads) || !scene) return -2;
    const DevScene sc = *(const DevScene*)scene;
    const size_t N = (size_t)n;
    uint32_t* df = dcopy(refs, N);
    double *dr = dcopy(ray, 7 * N), *di = dcopy(iv, 2 * N);
    uint64_t* dg = dcopy(rng, N);
    uint32_t* dflags = dcopy<uint32_t>(nullptr, KAT_LEAF_FLAGS * N);
    double* dout = dcopy<double>(nullptr, KAT_LEAF_OUT * N);
    uint64_t* dgo = dcopy<uint64_t>(nullptr, N);
    unsigned long long* dcnt = dcopy<unsigned long long>(nullptr, C_N * N);
    uint32_t* dnu = dcopy<uint32_t>(nullptr, 1);
    if (!df || !dr || !di || !dg || !dflags || !dout || !dgo || !dcnt || !dnu) {
        (void)hipFree(df); (void)hipFree(dr); (void)hipFree(di); (void)hipFree(dg); (void)hipFree(dflags);
        (void)hipFree(dout); (void)hipFree(dgo); (void)hipFree(dcnt); (void)hipFree(dnu);
        return -1;
    }
    (void)hipMemset(dflags, 0, KAT_LEAF_FLAGS * N * sizeof(uint32_t));
    (void)hipMemset(dout, 0, KAT_LEAF_OUT * N * sizeof(double));
    (void)hipMemset(dgo, 0, N * sizeof(uint64_t));
    (void)hipMemset(dcnt, 0, C_N * N * sizeof(unsigned long long));
    (void)hipMemset(dnu, 0, sizeof(uint32_t));
    hipLaunchKernelGGL(k_leaf, grid(n), dim3(256), lds, 0, n, which, sc, (const TQuad*)tquads, n_lds, n_lcubes, df, dr,
                       di, dg, dflags, dout, dgo, dcnt, dnu);
    const hipError_t e = hipDeviceSynchronize();
    const int rc = e == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1;
    back(flags, dflags, KAT_LEAF_FLAGS * N);
    back(out, dout, KAT_LEAF_OUT * N);
    back(rng_out, dgo, N);
    back(cnt, dcnt, C_N * N);
    back(nonuni, dnu, 1);
    (void)hipFree(df); (void)hipFree(dr); (void)hipFree(di); (void)hipFree(dg);
    return rc;
}

}  // extern "C"

// ---- the pixel stage (pixel.hpp): the product's kernels themselves, launched with 256 threads as
// the launchers launch them, over a KParams filled from plain host arrays.  Every entry checks its
// arguments first -- tile orders, active lists, buffer lengths, segment bounds -- and returns -2
// without a launch when one is off, so a malformed case never reaches the device; -1 after a HIP
// error; 0 otherwise.  Every buffer a kernel can write is an in/out array: the caller's contents
// (its poison pattern) go up before the launch and the buffer comes back after it.
struct KatPixelLayout {
    int32_t W, H, tile_w, tile_h, world, rank;  // the frame (for views: the tall one), the tiles, the partition
    uint32_t slots;   // tile slots of this rank: capacity = slots * tile_w * tile_h
    uint32_t n_pos;   // entries of order (and of vorder)
    uint32_t direct;  // out / out8 are the W x H frame (n_out = W H), else packed (n_out = capacity)
    uint32_t bs, chunk, cpp, fine_px, fine_base;
    uint32_t max_samples;
    uint32_t cap;     // the capacity the caller sized its per-pixel arrays for (accum, pstate, pbatches, the
                      // lists, the maps: their lengths below are multiples of it); must be slots * tile_w * tile_h
    double confidence, tolerance;
    const int32_t* order;  // n_pos entries (-1 or a tile of the frame), or null
    float* out;            // n_out * 3, in/out, or null
    uint8_t* out8;         // n_out * 3, in/out, or null
    uint64_t n_out;
};

namespace {

constexpr uint32_t PX_MAX_CAP = 1u << 22;  // packed pixels a case may have

struct PxCtx {
    KParams kp;
    uint32_t cap, tile_px, n_tiles;
    size_t n_out;
    int32_t* d_order;
    float* d_out;
    uint8_t* d_out8;
    const KatPixelLayout* L;
};

bool px_order_ok(const int32_t* o, uint32_t n, uint32_t n_tiles) {
    for (uint32_t k = 0; k < n; k++)
        if (!(o[k] == -1 || (o[k] >= 0 && (uint32_t)o[k] < n_tiles))) return false;
    return true;
}

// packed_pixel on the host, for the checks: is packed slot k a pixel of the frame?
bool px_real(const KatPixelLayout* L, const int32_t* order, uint32_t k) {
    const uint32_t tile_px = (uint32_t)(L->tile_w * L->tile_h), tiles_x = ((uint32_t)L->W + L->tile_w - 1u) / L->tile_w;
    const uint32_t slot = k / tile_px, w = k % tile_px;
    const uint32_t pos = (uint32_t)L->rank + slot * (uint32_t)L->world;
    const int64_t tile = order ? order[pos] : (int64_t)pos;
    if (tile < 0) return false;
    const uint64_t pi = (uint64_t)(tile % tiles_x) * L->tile_w + w % L->tile_w;
    const uint64_t pj = (uint64_t)(tile / tiles_x) * L->tile_h + w / L->tile_w;
    return pi < (uint64_t)L->W && pj < (uint64_t)L->H;
}

// The layout's checks and the KParams they allow; the order and the outputs go up.
int px_begin(const KatPixelLayout* L, PxCtx& c) {
    std::memset(&c, 0, sizeof(c));
    if (!L) return -2;
    if (L->W < 1 || L->H < 1 || L->W > 32768 || L->H > 32768 || L->tile_w < 1 || L->tile_h < 1 || L->tile_w > 1024 ||
        L->tile_h > 1024 || L->world < 1 || L->world > 1024 || L->rank < 0 || L->rank >= L->world || L->slots < 1 ||
        L->bs < 1 || L->direct > 1u)
        return -2;
    const uint64_t tile_px = (uint64_t)L->tile_w * L->tile_h, cap = tile_px * L->slots;
    if (cap > PX_MAX_CAP || (uint64_t)L->cap != cap) return -2;
    const uint32_t tiles_x = ((uint32_t)L->W + L->tile_w - 1u) / L->tile_w, tiles_y = ((uint32_t)L->H + L->tile_h - 1u) / L->tile_h;
    const uint64_t last_pos = (uint64_t)L->rank + (uint64_t)(L->slots - 1u) * L->world;
    if (last_pos >= (1ull << 31) || (L->order && last_pos >= L->n_pos)) return -2;
    if (L->order && !px_order_ok(L->order, L->n_pos, tiles_x * tiles_y)) return -2;
    if (L->n_out != (L->direct ? (uint64_t)L->W * L->H : cap)) return -2;
    c.L = L;
    c.cap = (uint32_t)cap;
    c.tile_px = (uint32_t)tile_px;
    c.n_tiles = tiles_x * tiles_y;
    c.n_out = (size_t)L->n_out;
    KParams& kp = c.kp;
    kp.cam.image_width = L->W;
    kp.cam.image_height = L->H;
    kp.ss.confidence = L->confidence;
    kp.ss.tolerance = L->tolerance;
    kp.ss.batch_size = L->bs;
    kp.ss.max_samples = L->max_samples;
    kp.rank = L->rank;
    kp.world_size = L->world;
    kp.tile_w = L->tile_w;
    kp.tile_h = L->tile_h;
    kp.tiles_x = (int32_t)tiles_x;
    kp.capacity = c.cap;
    kp.chunk = L->chunk;
    kp.cpp = L->cpp;
    kp.fine_px = L->fine_px;
    kp.fine_base = L->fine_base;
    kp.u_cpp = udiv_make(L->cpp ? L->cpp : 1u);
    kp.u_tpx = udiv_make(c.tile_px);
    kp.u_tw = udiv_make((uint32_t)L->tile_w);
    kp.u_tx = udiv_make(tiles_x);
    kp.u_w = udiv_make((uint32_t)L->W);
    kp.direct = L->direct;
    if (L->order) kp.order = c.d_order = dcopy(L->order, L->n_pos);
    if (L->out) kp.out = c.d_out = dcopy(L->out, c.n_out * 3);
    if (L->out8) kp.out8 = c.d_out8 = dcopy(L->out8, c.n_out * 3);
    if ((L->order && !c.d_order) || (L->out && !c.d_out) || (L->out8 && !c.d_out8)) {
        (void)hipFree(c.d_order); (void)hipFree(c.d_out); (void)hipFree(c.d_out8);
        return -1;
    }
    return 0;
}

// The doubles of `partial` that the chunk sums of a combine over this layout may touch; 0: the
// chunking itself is off (no chunks per pixel, a fine region without a chunk size).
uint64_t px_partial_need(const KatPixelLayout* L, uint32_t cap) {
    if (L->fine_px > cap) return 0;
    uint64_t need = 3;
    if (L->fine_px > 0) {
        if (L->cpp < 1 || L->cpp > 4096) return 0;
        need = (uint64_t)L->fine_px * L->cpp * 3;
    }
    if (L->fine_px < cap) {
        if (L->chunk < 1 || L->bs > 4096) return 0;
        const uint64_t f = ((uint64_t)L->fine_base + (uint64_t)L->bs * (cap - L->fine_px)) * 3;
        need = f > need ? f : need;
    }
    return need;
}

// Syncs, brings the outputs back (or, without `download`, only frees them) and ends the context.
int px_end(PxCtx& c, bool download = true) {
    const hipError_t e = hipDeviceSynchronize();
    const int rc = e == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1;
    if (c.d_out) { if (download && rc == 0) (void)hipMemcpy(c.L->out, c.d_out, c.n_out * 3 * sizeof(float), hipMemcpyDeviceToHost); (void)hipFree(c.d_out); }
    if (c.d_out8) { if (download && rc == 0) (void)hipMemcpy(c.L->out8, c.d_out8, c.n_out * 3, hipMemcpyDeviceToHost); (void)hipFree(c.d_out8); }
    (void)hipFree(c.d_order);
    return rc;
}

// A host array's device copy that comes back when the scope ends well (in/out), or is only freed.
template <class T>
struct PxBuf {
    T* h;
    T* d;
    size_t n;
    bool out;
    PxBuf(T* host, size_t count, bool is_out) : h(host), d(host ? dcopy(host, count) : nullptr), n(count), out(is_out) {}
    PxBuf(const PxBuf&) = delete;
    bool bad() const { return h && !d; }
    void finish(int rc) {
        if (d && out && rc == 0) (void)hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
        (void)hipFree(d);
        d = nullptr;
    }
};

}  // namespace

extern "C" {

int kat_pixel_layout_bytes(void) { return (int)sizeof(KatPixelLayout); }
uint32_t kat_pixel_accum_blocks(uint32_t capacity) { return gs_accum_blocks(capacity); }
uint32_t kat_pixel_stopped_bit(void) { return GS_ADAPT_STOPPED; }

// gs_combine_kernel over grid blocks.  partial: n_partial doubles.
int kat_pixel_combine(const KatPixelLayout* L, uint32_t grid, const double* partial, uint64_t n_partial) {
    PxCtx c;
    if (grid < 1 || grid > 65536u || !partial) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    const uint64_t need = px_partial_need(L, c.cap);
    if (need == 0 || n_partial < need) { (void)px_end(c, false); return -2; }
    PxBuf<double> dp(const_cast<double*>(partial), (size_t)n_partial, false);
    c.kp.partial = dp.d;
    KParams* dP = dcopy(&c.kp, 1);
    if (!dp.bad() && dP) hipLaunchKernelGGL(gs_combine_kernel, dim3(grid), dim3(256), 0, 0, dP);
    rc = px_end(c);
    if (dp.bad() || !dP) rc = -1;
    dp.finish(rc);
    (void)hipFree(dP);
    return rc;
}

// gs_accumulate_kernel, n_pass passes chained on the device: pass p has sample_base p * bs and the
// sums partial[p * n_partial ..]; accum (capacity * 3, in: the sums before pass 0) stays on the
// device between the passes.  After pass p: accum_out[p], out_all / out8_all[p] (n_out * 3 each;
// before each pass the outputs are set to the layout's out / out8 again) and delta_out[p]
// (gs_accum_blocks(capacity) doubles; null: the kernel runs with delta null).
int kat_pixel_accumulate(const KatPixelLayout* L, uint32_t n_pass, const double* partial, uint64_t n_partial,
                         const double* accum, double* accum_out, float* out_all, uint8_t* out8_all, double* delta_out) {
    PxCtx c;
    if (n_pass < 1 || n_pass > 16 || !partial || !accum || !accum_out) return -2;
    if (!L || (L->out && !out_all) || (L->out8 && !out8_all) || (uint64_t)L->bs * n_pass > 0xFFFFFFFFull) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    const uint64_t need = px_partial_need(L, c.cap);
    if (need == 0 || n_partial < need) { (void)px_end(c, false); return -2; }
    const uint32_t blocks = gs_accum_blocks(c.cap);
    const size_t n3 = (size_t)c.cap * 3, o3 = c.n_out * 3;
    PxBuf<double> dp(const_cast<double*>(partial), (size_t)n_partial * n_pass, false);
    PxBuf<double> da(const_cast<double*>(accum), n3, false);
    double* dd = delta_out ? dcopy(delta_out, blocks) : nullptr;
    KParams* dP = dcopy(&c.kp, 1);
    bool ok = !dp.bad() && !da.bad() && dP && (!delta_out || dd);
    for (uint32_t p = 0; ok && p < n_pass; p++) {
        c.kp.partial = dp.d + (size_t)p * n_partial;
        c.kp.accum = da.d;
        c.kp.delta = dd;
        c.kp.sample_base = p * L->bs;
        ok = hipMemcpy(dP, &c.kp, sizeof(KParams), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && dd) ok = hipMemcpy(dd, delta_out + (size_t)p * blocks, blocks * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && c.d_out) ok = hipMemcpy(c.d_out, L->out, o3 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && c.d_out8) ok = hipMemcpy(c.d_out8, L->out8, o3, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) break;
        hipLaunchKernelGGL(gs_accumulate_kernel, dim3(blocks), dim3(256), 0, 0, dP);
        ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
        if (!ok) break;  // (after a HIP error nothing more is launched)
        (void)hipMemcpy(accum_out + (size_t)p * n3, da.d, n3 * sizeof(double), hipMemcpyDeviceToHost);
        if (dd) (void)hipMemcpy(delta_out + (size_t)p * blocks, dd, blocks * sizeof(double), hipMemcpyDeviceToHost);
        if (c.d_out) (void)hipMemcpy(out_all + (size_t)p * o3, c.d_out, o3 * sizeof(float), hipMemcpyDeviceToHost);
        if (c.d_out8) (void)hipMemcpy(out8_all + (size_t)p * o3, c.d_out8, o3, hipMemcpyDeviceToHost);
    }
    rc = px_end(c, false);
    if (!ok) rc = -1;
    dp.finish(rc);
    da.finish(rc);
    (void)hipFree(dd);
    (void)hipFree(dP);
    return rc;
}

// The views of a pass: V views of W x view_h stacked (L->H = V * view_h, tile_h | view_h), vstate
// {before, selected} per view, vorder n_pos entries or null.
static int px_views_ok(const KatPixelLayout* L, const PxCtx& c, const int32_t* vorder, const uint32_t* vstate, uint32_t V,
                       uint32_t view_h) {
    if (!vstate || V < 1 || V > 4096 || view_h < 1 || (uint64_t)V * view_h != (uint64_t)L->H) return -2;
    if (view_h % (uint32_t)L->tile_h != 0) return -2;  // tiles do not straddle views
    for (uint32_t v = 0; v < V; v++)
        if (vstate[2 * v + 1] > 1u || (uint64_t)vstate[2 * v] + L->bs > 0xFFFFFFFFull) return -2;
    if (vorder && !px_order_ok(vorder, L->n_pos, c.n_tiles)) return -2;
    return 0;
}

// gs_views_order_kernel: dst (n_pos entries, in/out) over gs_views_order_blocks(n_pos) blocks, as
// launch_views_order_kernel.
int kat_pixel_views_order(const KatPixelLayout* L, const int32_t* vorder, const uint32_t* vstate, uint32_t V,
                          uint32_t view_h, int32_t* dst) {
    PxCtx c;
    if (!dst || !L || L->n_pos < 1 || L->n_pos > PX_MAX_CAP) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    if (px_views_ok(L, c, vorder, vstate, V, view_h) != 0) { (void)px_end(c, false); return -2; }
    PxBuf<int32_t> dvo(const_cast<int32_t*>(vorder), L->n_pos, false);
    PxBuf<uint32_t> dvs(const_cast<uint32_t*>(vstate), 2 * (size_t)V, false);
    PxBuf<int32_t> dd(dst, L->n_pos, true);
    c.kp.vorder = dvo.d;
    c.kp.vstate = reinterpret_cast<const GsViewState*>(dvs.d);
    KParams* dP = dcopy(&c.kp, 1);
    const bool ok = !dvo.bad() && !dvs.bad() && !dd.bad() && dP;
    if (ok) hipLaunchKernelGGL(gs_views_order_kernel, dim3(gs_views_order_blocks(L->n_pos)), dim3(256), 0, 0, dP, dd.d, L->n_pos, view_h);
    rc = px_end(c, false);
    if (!ok) rc = -1;
    dvo.finish(rc); dvs.finish(rc); dd.finish(rc);
    (void)hipFree(dP);
    return rc;
}

// gs_views_accumulate_kernel, one block per slot.  accum (capacity * 3) and vdelta (slots; null:
// the kernel runs with vdelta null) are in/out.
int kat_pixel_views_accumulate(const KatPixelLayout* L, const int32_t* vorder, const uint32_t* vstate, uint32_t V,
                               uint32_t view_h, const double* partial, uint64_t n_partial, double* accum,
                               double* vdelta) {
    PxCtx c;
    if (!partial || !accum || !L) return -2;
    if (vorder && ((uint64_t)L->rank + (uint64_t)(L->slots - 1u) * L->world >= L->n_pos)) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    const uint64_t need = px_partial_need(L, c.cap);
    if (px_views_ok(L, c, vorder, vstate, V, view_h) != 0 || need == 0 || n_partial < need) { (void)px_end(c, false); return -2; }
    PxBuf<int32_t> dvo(const_cast<int32_t*>(vorder), L->n_pos, false);
    PxBuf<uint32_t> dvs(const_cast<uint32_t*>(vstate), 2 * (size_t)V, false);
    PxBuf<double> dp(const_cast<double*>(partial), (size_t)n_partial, false);
    PxBuf<double> da(accum, (size_t)c.cap * 3, true);
    PxBuf<double> dv(vdelta, L->slots, true);
    c.kp.vorder = dvo.d;
    c.kp.vstate = reinterpret_cast<const GsViewState*>(dvs.d);
    c.kp.u_vpx = udiv_make((uint32_t)L->W * view_h);
    c.kp.partial = dp.d;
    c.kp.accum = da.d;
    c.kp.vdelta = dv.d;
    KParams* dP = dcopy(&c.kp, 1);
    const bool ok = !dvo.bad() && !dvs.bad() && !dp.bad() && !da.bad() && !dv.bad() && dP;
    if (ok) hipLaunchKernelGGL(gs_views_accumulate_kernel, dim3(L->slots), dim3(256), 0, 0, dP);
    rc = px_end(c);
    if (!ok) rc = -1;
    dvo.finish(rc); dvs.finish(rc); dp.finish(rc); da.finish(rc); dv.finish(rc);
    (void)hipFree(dP);
    return rc;
}

// gs_round_init_kernel over grid blocks: active (capacity entries, in/out) and count (1 word,
// in/out: round_counts[0], 0 before the kernel as the launches leave it).
int kat_pixel_round_init(const KatPixelLayout* L, uint32_t grid, uint32_t* active, uint32_t* count) {
    PxCtx c;
    if (grid < 1 || grid > 65536u || !active || !count || *count != 0u) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    PxBuf<uint32_t> dl(active, c.cap, true);
    PxBuf<uint32_t> dc(count, 1, true);
    c.kp.active_buf[0] = dl.d;
    c.kp.round_counts = dc.d;
    KParams* dP = dcopy(&c.kp, 1);
    const bool ok = !dl.bad() && !dc.bad() && dP;
    if (ok) hipLaunchKernelGGL(gs_round_init_kernel, dim3(grid), dim3(256), 0, 0, dP);
    rc = px_end(c);
    if (!ok) rc = -1;
    dl.finish(rc); dc.finish(rc);
    (void)hipFree(dP);
    return rc;
}

// gs_round_params_kernel (one block of 64, as launch_round_params_kernel).  in: round, seg, seg_px,
// chunk_req, whole_mode, bs, lanes, waves, capacity, n_act (round_counts[round]), has_counters,
// poison (the word every field the kernel writes holds before it).  counters: rays, paths (read
// with has_counters).  hint: rpp_hint[2], in/out.  out (24 words): per_sample, chunk, round, cpp,
// u_cpp {d, m, s1, s2}, n_items, fine_base, fine_px, claim, claim_fine, round_base, seg_base, seg_n,
// the list `active` names (0 / 1; 2: neither), the list `next_active` names, the queue word.
#define KAT_PARAMS_IN 12
#define KAT_PARAMS_OUT 24
int kat_pixel_round_params(const uint32_t* in, const unsigned long long* counters, unsigned long long* hint,
                           uint32_t* out) {
    if (!in || !counters || !hint || !out) return -2;
    const uint32_t round = in[0], seg = in[1], seg_px = in[2], bs = in[5], lanes = in[6], waves = in[7], cap = in[8],
                   n_act = in[9], has_counters = in[10], poison = in[11];
    if (round > 4096u || bs < 1 || (uint64_t)seg * seg_px > 0xFFFFFFFFull || (uint64_t)round * bs > 0xFFFFFFFFull ||
        has_counters > 1u)
        return -2;
    KParams kp;
    std::memset(&kp, 0, sizeof(kp));
    kp.ss.batch_size = bs;
    kp.lanes = lanes;
    kp.waves = waves;
    kp.capacity = cap;
    kp.per_sample = kp.chunk = kp.round = kp.cpp = kp.n_items = kp.fine_base = kp.fine_px = kp.claim = kp.claim_fine =
        kp.round_base = kp.seg_base = kp.seg_n = poison;
    kp.u_cpp = UDiv{poison, poison, poison, poison};
    unsigned long long cnt[C_N] = {};
    cnt[C_RAYS] = counters[0];
    cnt[C_PATHS] = counters[1];
    uint32_t* counts = new uint32_t[(size_t)round + 1]();
    counts[round] = n_act;
    PxBuf<uint32_t> dcounts(counts, (size_t)round + 1, false);
    PxBuf<unsigned long long> dcnt(cnt, C_N, false);
    PxBuf<unsigned long long> dh(hint, 2, true);
    uint32_t lists[2] = {0u, 0u}, q = poison;
    PxBuf<uint32_t> dl0(&lists[0], 1, false), dl1(&lists[1], 1, false), dq(&q, 1, true);
    kp.round_counts = dcounts.d;
    kp.counters = has_counters ? dcnt.d : nullptr;
    kp.rpp_hint = dh.d;
    kp.active_buf[0] = dl0.d;
    kp.active_buf[1] = dl1.d;
    kp.queue = dq.d;
    KParams* dP = dcopy(&kp, 1);
    const bool ok = !dcounts.bad() && !dcnt.bad() && !dh.bad() && !dl0.bad() && !dl1.bad() && !dq.bad() && dP;
    if (ok)
        hipLaunchKernelGGL(gs_round_params_kernel, dim3(1), dim3(64), 0, 0, dP, round, seg, seg_px, (int32_t)in[3],
                           (int32_t)in[4]);
    int rc = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess && ok ? 0 : -1;
    KParams r;
    if (rc == 0 && hipMemcpy(&r, dP, sizeof(KParams), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    if (rc == 0) {
        const uint32_t a = r.active == dl0.d ? 0u : r.active == dl1.d ? 1u : 2u;
        const uint32_t nx = r.next_active == dl0.d ? 0u : r.next_active == dl1.d ? 1u : 2u;
        dq.finish(rc);
        const uint32_t w[KAT_PARAMS_OUT] = {r.per_sample, r.chunk, r.round, r.cpp, r.u_cpp.d, r.u_cpp.m, r.u_cpp.s1, r.u_cpp.s2,
                                            r.n_items, r.fine_base, r.fine_px, r.claim, r.claim_fine, r.round_base,
                                            r.seg_base, r.seg_n, a, nx, q, 0u, 0u, 0u, 0u, 0u};
        for (int k = 0; k < KAT_PARAMS_OUT; k++) out[k] = w[k];
    }
    dcounts.finish(rc); dcnt.finish(rc); dh.finish(rc); dl0.finish(rc); dl1.finish(rc); dq.finish(rc);
    (void)hipFree(dP);
    delete[] counts;
    return rc;
}
int kat_pixel_claim_consts(int which) { return which == 0 ? (int)GS_CLAIM_DIV : which == 1 ? (int)GS_CLAIM_FINE : which == 2 ? (int)GS_ROUND_WHOLE_MAX_BATCH : -1; }

// gs_round_combine_kernel (fold 0; fold 2: the same with per_sample 0, a whole-batch round, which the
// kernel must leave alone) or gs_round_fold_kernel (fold 1) of round `round` over grid blocks: the
// segment active[seg_base, seg_base + seg_n) of a list of n_active entries; partial
// seg_n * bs * 3 doubles (sample-major); pstate (capacity * 5), pbatches (capacity; fold only),
// next_active (capacity entries), next_count (round_counts[round + 1]) and pix (counters[C_PIX];
// null: the kernel runs without counters) are in/out.
int kat_pixel_round_step(const KatPixelLayout* L, int fold, uint32_t round, uint32_t grid, const uint32_t* active,
                         uint32_t n_active, uint32_t seg_base, uint32_t seg_n, const double* partial, uint64_t n_partial,
                         double* pstate, uint32_t* pbatches, uint32_t* next_active, uint32_t* next_count,
                         unsigned long long* pix) {
    PxCtx c;
    if (grid < 1 || grid > 65536u || fold < 0 || fold > 2 || round > 4096u || !active || !partial || !pstate ||
        !next_active || !next_count || (fold == 1 && !pbatches) || !L)
        return -2;
    if (GS_ROUND_PIXEL_MAJOR != 0) return -2;  // (the cases are written for the sample-major layout)
    if (n_active < 1 || (uint64_t)seg_base + seg_n > n_active || (uint64_t)(round + 1u) * L->bs > (1ull << 53)) return -2;
    if (n_partial < (uint64_t)seg_n * L->bs * 3 || n_partial < 3) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    bool ok = n_active <= c.cap && (uint64_t)*next_count + seg_n <= c.cap;
    for (uint32_t k = 0; ok && k < n_active; k++)  // (an active pixel is real: `direct` takes its image index)
        ok = active[k] < c.cap && px_real(L, L->order, active[k]);
    if (!ok) { (void)px_end(c, false); return -2; }
    PxBuf<uint32_t> dact(const_cast<uint32_t*>(active), n_active, false);
    PxBuf<double> dp(const_cast<double*>(partial), (size_t)n_partial, false);
    PxBuf<double> ds(pstate, (size_t)c.cap * 5, true);
    PxBuf<uint32_t> db(pbatches, c.cap, true);
    PxBuf<uint32_t> dn(next_active, c.cap, true);
    uint32_t* counts = new uint32_t[(size_t)round + 2]();
    counts[round] = n_active;
    counts[round + 1] = *next_count;
    PxBuf<uint32_t> dcounts(counts, (size_t)round + 2, true);
    unsigned long long cnt[C_N] = {};
    if (pix) cnt[C_PIX] = *pix;
    PxBuf<unsigned long long> dcnt(pix ? cnt : nullptr, C_N, true);
    c.kp.per_sample = fold == 2 ? 0u : 1u;
    c.kp.seg_base = seg_base;
    c.kp.seg_n = seg_n;
    c.kp.round = round;
    c.kp.round_base = round * L->bs;
    c.kp.active = dact.d;
    c.kp.next_active = dn.d;
    c.kp.partial = dp.d;
    c.kp.pstate = ds.d;
    c.kp.pbatches = db.d;
    c.kp.round_counts = dcounts.d;
    c.kp.counters = dcnt.d;
    KParams* dP = dcopy(&c.kp, 1);
    ok = !dact.bad() && !dp.bad() && !ds.bad() && !db.bad() && !dn.bad() && !dcounts.bad() && !dcnt.bad() && dP;
    if (ok) {
        if (fold == 1) hipLaunchKernelGGL(gs_round_fold_kernel, dim3(grid), dim3(256), 0, 0, dP, round);
        else hipLaunchKernelGGL(gs_round_combine_kernel, dim3(grid), dim3(256), 0, 0, dP, round);
    }
    rc = px_end(c);
    if (!ok) rc = -1;
    dact.finish(rc); dp.finish(rc); ds.finish(rc); db.finish(rc); dn.finish(rc); dcounts.finish(rc); dcnt.finish(rc);
    if (rc == 0) {
        *next_count = counts[round + 1];
        if (pix) *pix = cnt[C_PIX];
    }
    (void)hipFree(dP);
    delete[] counts;
    return rc;
}

// gs_round_resolve_kernel over gs_accum_blocks(capacity) blocks.  pstate capacity * 5, pbatches
// capacity; map_samples, map_error (capacity each; null: not asked for) and summary
// (GS_ROUND_SUMMARY_WORDS; null: none) are in/out.
int kat_pixel_round_resolve(const KatPixelLayout* L, const double* pstate, const uint32_t* pbatches,
                            uint32_t* map_samples, float* map_error, unsigned long long* summary) {
    PxCtx c;
    if (!pstate || !pbatches) return -2;
    int rc = px_begin(L, c);
    if (rc) return rc;
    PxBuf<double> ds(const_cast<double*>(pstate), (size_t)c.cap * 5, false);
    PxBuf<uint32_t> db(const_cast<uint32_t*>(pbatches), c.cap, false);
    PxBuf<uint32_t> dm(map_samples, c.cap, true);
    PxBuf<float> de(map_error, c.cap, true);
    PxBuf<unsigned long long> dsum(summary, GS_ROUND_SUMMARY_WORDS, true);
    c.kp.pstate = ds.d;
    c.kp.pbatches = db.d;
    c.kp.map_samples = dm.d;
    c.kp.map_error = de.d;
    c.kp.round_summary = dsum.d;
    KParams* dP = dcopy(&c.kp, 1);
    const bool ok = !ds.bad() && !db.bad() && !dm.bad() && !de.bad() && !dsum.bad() && dP;
    if (ok) hipLaunchKernelGGL(gs_round_resolve_kernel, dim3(gs_accum_blocks(c.cap)), dim3(256), 0, 0, dP);
    rc = px_end(c);
    if (!ok) rc = -1;
    ds.finish(rc); db.finish(rc); dm.finish(rc); de.finish(rc); dsum.finish(rc);
    (void)hipFree(dP);
    return rc;
}

}  // extern "C"
