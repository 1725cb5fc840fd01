// leaf.hpp — the megakernel's leaf stage: what a leaf pass runs for every non-node child but a
// stationary sphere reached directly from a BVH node (leaf_other<FEAT, UNI>): the quad records'
// source (QuadSrc: LDS mirror or global memory), one primitive's test, Translate / RotateY
// chains, HittableLists, Quad::cube lists as straight-line code, ConstantMedium::hit with its
// boundary tests (a BVH's walk and one more medium among them) and its one draw from the lane's
// stream.  With them the small helpers they need: the 16-B / 8-B LDS load types, lo_hi, inv_of
// and the address-space-qualified scene loads (GS_SCENE_AS, sp, ld_*).  Included by render.hip;
// tests/hip/kat_device.hip includes it too, so the known-answer tests run these very functions.
// Written in namespace gsd's names (d3, mk, Ray, ...): an includer says `using namespace gsd;`
// before it includes this file, as both do (as shading.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../../include/grayshift_gpu.h"
#include "kernel_abi.hpp"
#include "devmath.hpp"
#include "geometry.hpp"

// (everything inlined: GS_MIN_WAVES, kernel_abi.hpp)
#ifndef GS_NOINLINE
#define GS_NOINLINE __forceinline__
#endif

// Node and leaf records live in two arrays (32-B TNode, 48-B TLeaf: geometry.hpp); a link
// is a node's byte offset (index << 5: the address arithmetic of a node step is then
// none in LDS and one SGPR-base add in global memory), THR_LEAF | a leaf index, or
// THR_END.  Each block mirrors the most-tested
// prefix of both arrays in LDS.  Address-space-qualified pointers keep the mirror reads
// ds_read instructions: a select between an LDS and a global pointer would compile to
// flat loads, which measured 34% slower on the whole kernel.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) const u32x2 lds_u32x2;
__device__ __forceinline__ double lo_hi(unsigned int lo, unsigned int hi) { return __hiloint2double((int)hi, (int)lo); }

// 1/d for the f64 slab test on the rare paths.  The asm barrier keeps the compiler from
// hoisting these divisions out of the traversal loop (d is loop-invariant) into six
// registers live across the whole loop: recomputed where needed, they cost nothing in
// the common path.
__device__ __forceinline__ d3 inv_of(d3 d) {
    asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z));
    return mk(1.0 / d.x, 1.0 / d.y, 1.0 / d.z);
}

// Quad records for traversal (TQuad): [0, n_lds) from the block's LDS mirror, the rest
// from global memory; 16 B at a time, so a quad whose plane misses reads 32 B, not 128.
struct QuadSrc {
    const uint8_t* lds;
    const TQuad* g;
    uint32_t n_lds;
    // the Quad::cube records mirrored in LDS: [0, n_lcubes) at lcubes (cube_test)
    const uint8_t* lcubes;
    uint32_t n_lcubes;
};

// Scene-record loads of the leaf tests, field by field through a pointer of an explicit
// address space: global (vector loads) or, with UNI — every active lane tests the same
// leaf, a wave-uniform ref — constant, which compiles to scalar loads (the scalar cache:
// no vector-memory instruction, no per-lane address, uniform branches after them).  The
// scene's pointers are generic and load through flat instructions otherwise (which also
// count against lgkmcnt); a whole-struct copy from constant memory is rewritten by the
// optimiser into flat loads again, hence the field-wise copies.
#ifdef __HIP_DEVICE_COMPILE__
#define GS_SCENE_AS(UNI) __attribute__((address_space((UNI) ? 4 : 1)))
#else
#define GS_SCENE_AS(UNI)
#endif
template <bool UNI, class T>
__device__ __forceinline__ const GS_SCENE_AS(UNI) T* sp(const T* p) {
    return (const GS_SCENE_AS(UNI) T*)p;
}
template <bool UNI>
__device__ __forceinline__ uint32_t ld_u32(const uint32_t* p) {
    return *sp<UNI>(p);
}
template <bool UNI>
__device__ __forceinline__ gs_instance ld_inst(const gs_instance* p) {
    const auto q = sp<UNI>(p);
    gs_instance v;
    v.kind = q->kind;
    v.child = q->child;
    v.p[0] = q->p[0];
    v.p[1] = q->p[1];
    v.p[2] = q->p[2];
    return v;
}
template <bool UNI>
__device__ __forceinline__ gs_list ld_list(const gs_list* p) {
    const auto q = sp<UNI>(p);
    gs_list v;
    v.first = q->first;
    v.count = q->count;
    return v;
}
template <bool UNI>
__device__ __forceinline__ gs_medium ld_medium(const gs_medium* p) {
    const auto q = sp<UNI>(p);
    gs_medium v;
    v.boundary = q->boundary;
    v.material = q->material;
    v.density_neg_inv = q->density_neg_inv;
    return v;
}
template <bool UNI>
__device__ __forceinline__ u32x4 quad_part(const QuadSrc& qs, uint32_t i, uint32_t k) {
    if (!UNI && i < qs.n_lds) return *(lds_u32x4*)(qs.lds + i * (uint32_t)sizeof(TQuad) + (k << 4));
    return sp<UNI>(reinterpret_cast<const u32x4*>(qs.g + i))[k];
}
template <int CODE>
__device__ __forceinline__ double d3_c(const d3& v, int which) {  // which: 0 = a, 1 = iu, 2 = iv
    constexpr int A = CODE >> 1, O = CODE & 1;
    const int k = which == 0 ? A : (which == 1 ? (A + 1 + O) % 3 : (A + 2 - O) % 3);
    return k == 0 ? v.x : (k == 1 ? v.y : v.z);
}
template <bool UNI>
__device__ __forceinline__ bool quad_test(const QuadSrc& qs, uint32_t i, const Ray& ray, double tmin, double tmax,
                                          double& t_out) {
    const u32x4 a = quad_part<UNI>(qs, i, 0);
    const u32x4 b = quad_part<UNI>(qs, i, 1);
    return quad_accept_plane(
        mk(lo_hi(a.x, a.y), lo_hi(a.z, a.w), lo_hi(b.x, b.y)), lo_hi(b.z, b.w),
        [&](d3& Q, d3& U, d3& V, d3& W) {
            const u32x4 c = quad_part<UNI>(qs, i, 2), e = quad_part<UNI>(qs, i, 3), f = quad_part<UNI>(qs, i, 4);
            const u32x4 g = quad_part<UNI>(qs, i, 5), h = quad_part<UNI>(qs, i, 6), m = quad_part<UNI>(qs, i, 7);
            Q = mk(lo_hi(c.x, c.y), lo_hi(c.z, c.w), lo_hi(e.x, e.y));
            U = mk(lo_hi(e.z, e.w), lo_hi(f.x, f.y), lo_hi(f.z, f.w));
            V = mk(lo_hi(g.x, g.y), lo_hi(g.z, g.w), lo_hi(h.x, h.y));
            W = mk(lo_hi(h.z, h.w), lo_hi(m.x, m.y), lo_hi(m.z, m.w));
        },
        ray, tmin, tmax, t_out);
}

__device__ __forceinline__ bool cur_next_is_leaf(uint32_t link) { return link > THR_END; }

// Outcome of testing one non-node child against the ray.
struct LeafHit {
    bool hit;
    double t;
    uint32_t ref, inst;
    uint32_t enter;  // GS_FEAT_NESTED: the chain ended in BVH tree `enter - 1` (0: it did not)
};

// One primitive ref against `ray` (already in the primitive's space); accepts into
// `res` ("last accepted wins", as BVH.rs:73-80 and hittable.rs:75-83 compose).
template <bool UNI>
__device__ __forceinline__ void prim_test(const DevScene& sc, const QuadSrc& qs, uint32_t ref, const Ray& ray,
                                          double tmin, double closest, uint32_t inst_ref, LeafHit& res,
                                          unsigned long long* cnt) {
    const uint32_t kind = ref >> GS_REF_SHIFT, idx = ref & GS_REF_MASK;
    double t;
    bool ok = false;
    if (kind == GS_REF_SPHERE) {
        atomicAdd(&cnt[C_SPH], 1ull);
        const auto s = sp<UNI>(sc.spheres + idx);
        ok = sphere_accept(mk(s->cx, s->cy, s->cz), s->r, ray, len2(ray.d), tmin, closest, t);
    } else if (kind == GS_REF_MSPHERE) {
        atomicAdd(&cnt[C_MSPH], 1ull);
        const auto s = sp<UNI>(sc.mspheres + idx);
        const d3 c0 = mk(s->center_start[0], s->center_start[1], s->center_start[2]);
        const d3 cp = mk(s->center_path[0], s->center_path[1], s->center_path[2]);
        d3 c = add(c0, muls(cp, ray.time));
        ok = sphere_accept(c, s->radius, ray, len2(ray.d), tmin, closest, t);
    } else if (kind == GS_REF_QUAD) {
        atomicAdd(&cnt[C_QUAD], 1ull);
        ok = quad_test<UNI>(qs, idx, ray, tmin, closest, t);
    } else if (kind == GS_REF_TRIANGLE) {
        atomicAdd(&cnt[C_TRI], 1ull);
        double u, v;
        const auto q = sp<UNI>(sc.tris + idx);
        gs_triangle tr;
        for (int k = 0; k < 3; k++) {
            tr.a[k] = q->a[k];
            tr.b[k] = q->b[k];
            tr.c[k] = q->c[k];
        }
        ok = tri_hit(tr, ray, t, u, v);
    }
    if (ok) {
        res.hit = true;
        res.t = t;
        res.ref = ref;
        res.inst = inst_ref;
    }
}

// Translate / RotateY chain (hittable.rs:107-113, :179-193): the ray in the innermost
// child's space; returns that child's ref.
template <bool UNI>
__device__ __forceinline__ uint32_t walk_chain(const DevScene& sc, uint32_t cur, Ray& r, unsigned long long* cnt) {
#pragma unroll 1
    for (int k = 0; k < GS_MAX_CHAIN && (cur >> GS_REF_SHIFT) == GS_REF_INSTANCE; k++) {
        const gs_instance in = ld_inst<UNI>(sc.inst + (cur & GS_REF_MASK));
        atomicAdd(&cnt[C_INST], 1ull);
        inst_forward(in, r);
        cur = in.child;
    }
    return cur;
}

// The instance tests of walking a chain again (counted, nothing computed).
template <bool UNI>
__device__ __forceinline__ void chain_count(const DevScene& sc, uint32_t cur, unsigned long long* cnt) {
#pragma unroll 1
    for (int k = 0; k < GS_MAX_CHAIN && (cur >> GS_REF_SHIFT) == GS_REF_INSTANCE; k++) {
        atomicAdd(&cnt[C_INST], 1ull);
        cur = ld_u32<UNI>(&sc.inst[cur & GS_REF_MASK].child);
    }
}

// A Quad::cube list (quad.rs:54-80: six quads in a fixed order, all axis-aligned, added one
// after the other) as straight-line code: face k's plane axis and in-plane axes are
// compile-time constants (cube_code: the aligned form's 2 a + o), so each face is Quad::hit
// in the reduced form aquad_accept states -- the same t, alpha and beta bit for bit -- with
// no selects and no loop, in the list's order with its shrinking closest (hittable.rs:
// 71-86).  Every face value is one of twelve numbers of the box: its corners min = (x0, y0,
// z0) and max = (x1, y1, z1), the edges dx, dy, dz and the three w magnitudes (w_xy of the
// z faces, w_zy of the x faces, w_xz of the y faces), with a sign: the 96-B record
// [x0 y0 z0 x1 y1 z1 dx dy dz w_xy w_zy w_xz] (a negation is exact and free, an f64
// operand modifier).  The host (cube_record) builds a cube only when all six faces' aligned
// records equal what this table derives; the other lists keep the loop.
// (the record is read up front: faces reading their values lazily measured -0.3 to -2.8%)
struct CubeRegs {
    double c[GS_CUBE_DOUBLES];
    template <int J>
    __device__ __forceinline__ double get() const { return c[J]; }
};
template <bool UNI>
__device__ __forceinline__ u32x4 cube_part(const QuadSrc& qs, const double* g, uint32_t cube, uint32_t k, bool lds) {
    if (!UNI && lds) return *(lds_u32x4*)(qs.lcubes + cube * (uint32_t)(GS_CUBE_DOUBLES * 8) + (k << 4));
    return sp<UNI>(reinterpret_cast<const u32x4*>(g + (size_t)cube * GS_CUBE_DOUBLES))[k];
}
template <int K, int F, class Src>
__device__ __forceinline__ double cube_val(const Src& c) {
    constexpr int v = cube_src(K, F);
    if constexpr (v < 0) return -c.template get<-v>();
    else return c.template get<v>();
}
template <int K, class Src>
__device__ __forceinline__ void cube_face(const Src& c, uint32_t q0, const Ray& r, double tmin, uint32_t inst_ref,
                                          LeafHit& res) {
    constexpr int C = cube_code(K);
    const double da = d3_c<C>(r.d, 0);
    if (fabs(da) < 1e-8) return;
    const double t = (cube_val<K, 0>(c) - d3_c<C>(r.o, 0)) / da;
    if (!(tmin <= t && t <= res.t)) return;
    const double pu = (d3_c<C>(r.o, 1) + d3_c<C>(r.d, 1) * t) - cube_val<K, 1>(c);
    const double pv = (d3_c<C>(r.o, 2) + d3_c<C>(r.d, 2) * t) - cube_val<K, 2>(c);
    const double W = cube_val<K, 5>(c);
    const double alpha = W * (pu * cube_val<K, 4>(c));
    const double beta = W * (cube_val<K, 3>(c) * pv);
    if (!(0.0 <= alpha && alpha <= 1.0) || !(0.0 <= beta && beta <= 1.0)) return;
    res.hit = true;
    res.t = t;
    res.ref = GS_MAKE_REF(GS_REF_QUAD, q0 + K);
    res.inst = inst_ref;
}
template <class Src>
__device__ __forceinline__ void cube_faces(const Src& c, uint32_t q0, const Ray& r, double tmin, uint32_t inst_ref,
                                           LeafHit& res) {
    cube_face<0>(c, q0, r, tmin, inst_ref, res);
    cube_face<1>(c, q0, r, tmin, inst_ref, res);
    cube_face<2>(c, q0, r, tmin, inst_ref, res);
    cube_face<3>(c, q0, r, tmin, inst_ref, res);
    cube_face<4>(c, q0, r, tmin, inst_ref, res);
    cube_face<5>(c, q0, r, tmin, inst_ref, res);
}
template <bool UNI>
__device__ __forceinline__ void cube_test(const DevScene& sc, const QuadSrc& qs, uint32_t cube, uint32_t q0,
                                          const Ray& r, double tmin, uint32_t inst_ref, LeafHit& res,
                                          unsigned long long* cnt) {
    atomicAdd(&cnt[C_QUAD], 6ull);
    CubeRegs c;
    // the LDS copy when every lane's cube is mirrored (a wave-uniform choice: a per-lane
    // one ran both kinds of loads under masks, final_scene -2.3%), else global for all
    const bool lds = !UNI && __builtin_amdgcn_ballot_w64(cube >= qs.n_lcubes) == 0;
#pragma unroll
    for (uint32_t k = 0; k < GS_CUBE_DOUBLES / 2; k++) {
        const u32x4 v = cube_part<UNI>(qs, sc.cubes, cube, k, lds);
        c.c[2 * k] = lo_hi(v.x, v.y);
        c.c[2 * k + 1] = lo_hi(v.z, v.w);
    }
    cube_faces(c, q0, r, tmin, inst_ref, res);
}

// A HittableList (hittable.rs:71-86: shrinking closest) or one primitive.
template <bool UNI>
__device__ __forceinline__ void shape_test(const DevScene& sc, const QuadSrc& qs, uint32_t cur, const Ray& r,
                                           double tmin, double closest, uint32_t inst_ref, LeafHit& res,
                                           unsigned long long* cnt) {
    if ((cur >> GS_REF_SHIFT) == GS_REF_LIST) {
        atomicAdd(&cnt[C_LIST], 1ull);
        const gs_list l = ld_list<UNI>(sc.lists + (cur & GS_REF_MASK));
        if (l.count & GS_CUBE_FLAG) {
            cube_test<UNI>(sc, qs, l.first, l.count & ~GS_CUBE_FLAG, r, tmin, inst_ref, res, cnt);
        } else {
#pragma unroll 1
            for (uint32_t k = 0; k < l.count; k++)
                prim_test<UNI>(sc, qs, ld_u32<UNI>(sc.list_refs + l.first + k), r, tmin, res.t, inst_ref, res, cnt);
        }
    } else {
        prim_test<UNI>(sc, qs, cur, r, tmin, closest, inst_ref, res, cnt);
    }
}

// GS_FEAT_GENERAL: the closest hit of `r` over BVH tree `tree` (threaded like the BVHs under
// instances, its last links THR_RET) in [tmin, res.t] -- BVHNode::hit (BVH.rs:69-90) as its
// pre-order walk with the shrinking closest, every node tested with the reference's f64 slab
// test (AABB.rs:58-113) and counted, the leaves' lists and primitives by shape_test.  For a
// BVH as a ConstantMedium boundary: a rare path, read from global memory.
template <bool UNI>
__device__ __forceinline__ void tree_test(const DevScene& sc, const QuadSrc& qs, uint32_t tree, const Ray& r, double tmin,
                                          LeafHit& res, unsigned long long* cnt) {
    uint32_t link = sc.nroots[tree];
    const d3 inv = inv_of(r.d);
#pragma unroll 1
    for (uint32_t guard = 0; link != THR_RET && guard < (1u << 27); guard++) {
        if (link < THR_END) {  // a node record (its byte offset)
            atomicAdd(&cnt[C_NODES], 1ull);
            const TNode& n = sc.tnodes[link >> 5];
            link = box_hit(box64(sc.tboxes[link >> 5]), r.o, inv, tmin, res.t) ? n.hit : n.miss;
        } else {  // a leaf record
            const TLeaf& lf = sc.tleaves[link & ~THR_LEAF];
            shape_test<false>(sc, qs, lf.ref, r, tmin, res.t, GS_REF_NONE, res, cnt);
            link = lf.next;
        }
    }
}

template <bool UNI, int LEVEL>
__device__ __forceinline__ void medium_test(const DevScene& sc, const QuadSrc& qs, uint32_t cur, const Ray& r, double tmin,
                                            double closest, uint32_t inst_ref, uint64_t& rng, LeafHit& res,
                                            unsigned long long* cnt, bool general);
// A medium's boundary in [tmin, DMAX]: a primitive or list; with GS_FEAT_GENERAL also a BVH
// (tree_test) or, one level deep, another medium (its own ConstantMedium::hit, drawing from
// the lane's stream in the reference's order: volume.rs:36-41 calls boundary.hit twice).
template <bool UNI, int LEVEL>
__device__ __forceinline__ void boundary_test(const DevScene& sc, const QuadSrc& qs, uint32_t shape, const Ray& rb,
                                              double tmin, uint64_t& rng, LeafHit& b, unsigned long long* cnt,
                                              bool general) {
    if (general && (shape >> GS_REF_SHIFT) == GS_REF_NODE) {
        tree_test<UNI>(sc, qs, shape & GS_REF_MASK, rb, tmin, b, cnt);
    } else if (LEVEL == 0 && general && (shape >> GS_REF_SHIFT) == GS_REF_MEDIUM) {
        medium_test<false, 1>(sc, qs, shape, rb, tmin, b.t, GS_REF_NONE, rng, b, cnt, true);
    } else {
        shape_test<UNI>(sc, qs, shape, rb, tmin, b.t, GS_REF_NONE, b, cnt);
    }
}

// ConstantMedium::hit (volume.rs:32-63): the boundary hit over Interval::UNIVERSE, again
// from t1 + 0.0001, both clipped to ray_t; then the free-flight distance from the lane's
// RNG stream, drawn here, inside traversal, in the reference's visit order (:48).
// `general` (GS_FEAT_GENERAL kernels): the boundary may be a BVH or a medium (boundary_test).
template <bool UNI, int LEVEL>
__device__ __forceinline__ void medium_test(const DevScene& sc, const QuadSrc& qs, uint32_t cur, const Ray& r, double tmin,
                                            double closest, uint32_t inst_ref, uint64_t& rng, LeafHit& res,
                                            unsigned long long* cnt, bool general) {
    atomicAdd(&cnt[C_MED], 1ull);
    // the boundary now, the density only where it is used (not held through both hits)
    const gs_medium* mp = sc.media + (cur & GS_REF_MASK);
    struct {
        uint32_t boundary;
    } md{ld_u32<UNI>(&mp->boundary)};
    const double DMAX = 1.7976931348623157e308;  // f64::MAX; f64::MIN = -f64::MAX
    // |ray.d| now (the same value volume.rs:55 computes at the end), so the ray itself is
    // not live through the boundary tests: they need only its transform into the
    // boundary's space, which the second boundary.hit call (volume.rs:38-41) would recompute
    // from the same ray bit for bit -- it is reused, and the second walk's instance tests
    // are counted.  (Without it media kernels spill 12-20 B/lane around the cube tests of
    // box boundaries.)
    const double ray_len = sqrt(len2(r.d));
    LeafHit b1;
    b1.hit = false;
    b1.t = DMAX;
    Ray rb = r;
    const uint32_t shape = walk_chain<UNI>(sc, md.boundary, rb, cnt);
    if (general) boundary_test<UNI, LEVEL>(sc, qs, shape, rb, -DMAX, rng, b1, cnt, true);
    else shape_test<UNI>(sc, qs, shape, rb, -DMAX, DMAX, GS_REF_NONE, b1, cnt);
    if (!b1.hit) return;
    chain_count<UNI>(sc, md.boundary, cnt);
    LeafHit b2;
    b2.hit = false;
    b2.t = DMAX;
    if (general) boundary_test<UNI, LEVEL>(sc, qs, shape, rb, b1.t + 0.0001, rng, b2, cnt, true);
    else shape_test<UNI>(sc, qs, shape, rb, b1.t + 0.0001, DMAX, GS_REF_NONE, b2, cnt);
    if (!b2.hit) return;
    double t1 = b1.t, t2 = b2.t;
    if (t1 < tmin) t1 = tmin;
    if (t2 > closest) t2 = closest;
    if (t1 >= t2) return;
    if (t1 < 0.0) t1 = 0.0;
    const double dist_inside_boundary = (t2 - t1) * ray_len;
    const double hit_dist = sp<UNI>(mp)->density_neg_inv * log(wy_f64(rng));
    if (hit_dist > dist_inside_boundary) return;
    res.hit = true;
    res.t = t1 + hit_dist / ray_len;
    res.ref = cur;
    res.inst = inst_ref;
}

// The rarer non-node children (everything but a stationary sphere reached directly
// from a BVH node): moving sphere, quad, triangle, HittableList, ConstantMedium, behind an
// optional Translate/RotateY chain.  `rng`: a medium draws from the lane's stream.  FEAT
// (GS_FEAT_*) is a kernel template argument: scenes without media compile the medium
// test out (it costs the traversal loop 4 VGPRs and spills otherwise).
// A chain that ends in a BVH (GS_FEAT_NESTED: final_scene's box of balls, main.rs:741-755)
// is not walked here: `r` is left in the tree's space and `enter` = tree + 1, and the
// caller walks the tree in the main loop's passes (round 5; see the leaf pass).
template <int FEAT, bool UNI>
__device__ GS_NOINLINE LeafHit leaf_other(const DevScene& sc, const QuadSrc& qs, uint32_t ref, Ray& r, double tmin,
                                           double closest, uint64_t& rng, unsigned long long* cnt) {
    LeafHit res;
    res.hit = false;
    res.t = closest;
    res.ref = GS_REF_NONE;
    res.inst = GS_REF_NONE;
    res.enter = 0;
    const uint32_t inst_ref = (ref >> GS_REF_SHIFT) == GS_REF_INSTANCE ? ref : GS_REF_NONE;
    const uint32_t cur = walk_chain<UNI>(sc, ref, r, cnt);
    if ((FEAT & GS_FEAT_MEDIA) && (cur >> GS_REF_SHIFT) == GS_REF_MEDIUM) {
        medium_test<UNI, 0>(sc, qs, cur, r, tmin, closest, inst_ref, rng, res, cnt, (FEAT & GS_FEAT_GENERAL) != 0);
    } else if ((FEAT & GS_FEAT_NESTED) && (cur >> GS_REF_SHIFT) == GS_REF_NODE) {
        res.enter = (cur & GS_REF_MASK) + 1u;
    } else {
        shape_test<UNI>(sc, qs, cur, r, tmin, closest, inst_ref, res, cnt);
    }
    return res;
}
