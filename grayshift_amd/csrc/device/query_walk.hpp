// query_walk.hpp — the plain walk of the query kernels (query.hip: gs_query_kernel; radiance.hip:
// gs_radiance_kernel): the reference's world.hit (hittable.rs, BVH.rs:69-90) over the threaded
// records the upload makes (DevScene::tnodes / tboxes / tleaves / nroots), one record per step, from
// the tree's first link to THR_END: the f64 slab test on a node's TBox as AABB::hit decides it
// (box_hit_ref), a stationary sphere inline in its leaf record, every other leaf through the leaf
// stage (leaf.hpp: leaf_other<FEAT, false>), and the entry into a BVH under an instance chain with
// its return at THR_RET.  No LDS mirror, no wave-level passes: every record from global memory.
// Written in namespace gsd's names: an includer says `using namespace gsd;` and includes leaf.hpp
// before this file, as for shading.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernel_abi.hpp"
#include "devmath.hpp"
#include "geometry.hpp"

// AABB::hit (AABB.rs:58-113) for a caller's interval, whose ends may be NaN: the updates are the
// reference's own compare-and-assign (`if a > min { min = a }` keeps a NaN end, where geometry.hpp's
// box_hit takes fmax, which is the same only while the ends are numbers -- as a render's always are).
// The reference's early returns do not change the answer: once max <= min holds, later slabs only
// raise min and lower max; with a NaN end no comparison with it ever holds.
__device__ __forceinline__ void slab_ref(double mn, double mx, double o, double inv, double& lo, double& hi) {
    const double t0 = (mn - o) * inv, t1 = (mx - o) * inv;
    const bool s = t0 < t1;
    const double a = s ? t0 : t1, b = s ? t1 : t0;
    lo = a > lo ? a : lo;
    hi = b < hi ? b : hi;
}
__device__ __forceinline__ bool box_hit_ref(const DNode& n, const d3& o, const d3& inv, double tmin, double tmax) {
    double lo = tmin, hi = tmax;
    slab_ref(n.mnx, n.mxx, o.x, inv.x, lo, hi);
    slab_ref(n.mny, n.mxy, o.y, inv.y, lo, hi);
    slab_ref(n.mnz, n.mxz, o.z, inv.z, lo, hi);
    return !(hi <= lo);
}

// A lane's walk of one ray: where it stands and the closest accepted hit so far.
struct QWalk {
    Ray ray;         // the ray in the space of the tree being walked
    d3 inv;          // AABB.rs:62: 1.0 / ray.direction, per axis
    double a;        // sphere.rs:66
    double closest;
    bool hit;
    uint32_t hit_ref, hit_inst, hit_outer;
    uint32_t ninst;  // the instance leaf whose BVH the lane walks (none: the top level)
    uint32_t ret;    // ... and the link after that leaf
    uint32_t cur;    // the record to visit next; THR_END: the walk is done
};

// The walk's start for the ray r0 over (.., tmax).  Node visits and inline sphere tests are counted
// by the caller's registers (c_nodes, c_sph), which outlive a walk.
__device__ __forceinline__ void qwalk_begin(QWalk& w, const Ray& r0, uint32_t root, double tmax) {
    w.ray = r0;
    w.inv = inv_of(r0.d);
    w.a = len2(r0.d);
    w.closest = tmax;
    w.hit = false;
    w.hit_ref = w.hit_inst = w.hit_outer = GS_REF_NONE;
    w.ninst = GS_REF_NONE;
    w.ret = THR_END;
    w.cur = root;
}

// One step: the record at w.cur (which is not THR_END).  ANY: the first accepted hit ends the walk.
// Termination for any ray bits (NaN or zero directions, tmin > tmax, infinities): a link only
// ever points forward in the tree's pre-order -- a node's hit link to the next record, its miss
// link past its subtree, a leaf's link to the next record -- so whatever the tests decide, each
// step moves on and the walk reaches THR_END after at most one visit per record.  A BVH under
// an instance chain is a second finite walk of the same kind, entered from the top level only
// (validate() allows one level), which returns to the saved forward link at THR_RET.  A
// malformed ray is a miss or whatever the reference's arithmetic makes of it, never a fault:
// no index is computed from the ray.
template <int FEAT, bool ANY>
__device__ __forceinline__ void qwalk_step(const DevScene& sc, const QuadSrc& qs, QWalk& w, const Ray& ray0, double tmin,
                                           uint64_t& rng, unsigned long long* cnt, uint32_t& c_nodes, uint32_t& c_sph) {
    constexpr bool kNested = (FEAT & GS_FEAT_NESTED) != 0;
    constexpr bool kGeneral = (FEAT & GS_FEAT_GENERAL) != 0;
    const uint32_t cur = w.cur;
    if (kNested && cur == THR_RET) {  // the nested tree is done: back to the caller's ray
        w.ray = ray0;
        w.inv = inv_of(w.ray.d);
        w.a = len2(w.ray.d);
        w.cur = w.ret;
        w.ninst = GS_REF_NONE;
        return;
    }
    if (cur < THR_END) {  // a node record: its byte offset
        c_nodes++;
        const size_t k = cur >> 5;
        const auto b = sp<false>(sc.tboxes + k);
        DNode nb;
        nb.mnx = b->mnx; nb.mny = b->mny; nb.mnz = b->mnz;
        nb.mxx = b->mxx; nb.mxy = b->mxy; nb.mxz = b->mxz;
        const auto nd = sp<false>(sc.tnodes + k);
        const uint32_t l_hit = nd->hit, l_miss = nd->miss;
        w.cur = box_hit_ref(nb, w.ray.o, w.inv, tmin, w.closest) ? l_hit : l_miss;
        return;
    }
    const auto lf = sp<false>(sc.tleaves + (size_t)(cur & ~THR_LEAF));
    const uint32_t next = lf->next, ref = lf->ref;
    w.cur = next;
    if ((ref >> GS_REF_SHIFT) == GS_REF_SPHERE) {  // a stationary sphere, inline in the record
        c_sph++;
        double t;
        if (sphere_accept_rr(mk(lf->cx, lf->cy, lf->cz), lf->rr, w.ray, w.a, tmin, w.closest, t)) {
            w.hit = true;
            w.closest = t;
            w.hit_ref = ref;
            w.hit_inst = w.ninst;
            w.hit_outer = GS_REF_NONE;
            if (ANY) w.cur = THR_END;
        }
        return;
    }
    Ray rl = w.ray;  // (the ray in the leaf's space after its instance chain)
    const LeafHit lh = leaf_other<FEAT, false>(sc, qs, ref, rl, tmin, w.closest, rng, cnt);
    if (lh.hit) {
        w.hit = true;
        w.closest = lh.t;
        w.hit_ref = lh.ref;
        if (kGeneral && lh.inst != GS_REF_NONE && w.ninst != GS_REF_NONE) {  // a chain inside a tree under a chain
            w.hit_inst = lh.inst;
            w.hit_outer = w.ninst;
        } else {
            w.hit_inst = (!kNested || lh.inst != GS_REF_NONE) ? lh.inst : w.ninst;
            w.hit_outer = GS_REF_NONE;
        }
        if (ANY) {
            w.cur = THR_END;
            return;
        }
    }
    if (kNested && lh.enter != 0 && w.ninst == GS_REF_NONE) {
        // the chain ended in a BVH: walked by the same steps with the ray in the tree's space
        w.ret = next;
        w.ninst = ref;
        w.ray.o = rl.o;
        w.ray.d = rl.d;
        w.inv = inv_of(w.ray.d);
        w.a = len2(w.ray.d);
        w.cur = ld_u32<false>(sc.nroots + (lh.enter - 1u));
    }
}
