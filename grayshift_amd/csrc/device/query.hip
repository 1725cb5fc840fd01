// query.hip — ray queries: the closest hit, or any hit, of caller-supplied rays against a device
// scene (gs_query_rays_async, csrc/host/query.cpp): the reference's world.hit(ray, Interval, rec)
// (hittable.rs, BVH.rs:69-90) for a batch of rays, one ray per lane.
//
// The megakernel's traversal cannot be lifted out of gs_render_kernel, but its two
// ends are headers: the leaf stage (leaf.hpp: leaf_other, LeafHit) and the hit-record stage
// (shading.hpp: reconstruct, HitRec).  gs_query_kernel runs its own plain walk between them, over
// the threaded records the upload already makes (DevScene::tnodes / tboxes / tleaves / nroots): no
// LDS mirror, no wave-level passes, no launch slot, no work queue.  Every node is decided by the
// f64 slab test on its TBox, as AABB::hit decides it (box_hit_ref).  Its own translation unit, linked
// into a library of its own (build.py: libgrayshift_query.so), so nothing of render.hip, kernels.hpp,
// the kernel table or the product's code objects changes with it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/grayshift_gpu.h"
#include "kernel_abi.hpp"
#include "devmath.hpp"
#include "geometry.hpp"

using namespace gsd;

#include "leaf.hpp"
#include "shading.hpp"

namespace {

constexpr int QUERY_THREADS = 256;

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

__device__ __forceinline__ void chain_forward(const DevScene& sc, uint32_t cur, Ray& r) {
#pragma unroll 1
    for (int k = 0; k < GS_MAX_CHAIN && (cur >> GS_REF_SHIFT) == GS_REF_INSTANCE; k++) {
        const gs_instance in = ld_inst<false>(sc.inst + (cur & GS_REF_MASK));
        inst_forward(in, r);
        cur = in.child;
    }
}

}  // namespace

// One ray per lane; 256-lane blocks at one wave per SIMD, so a lane has the whole register file
// and the leaf stage's media and nested paths need no scratch.  FEAT: the MEDIA / NESTED (and, for
// the catch-all set, GENERAL) bits of the scene's feature word; ANY: leave at the first accepted
// hit.  The scene's pointers arrive by value in the kernel arguments and stay wave-uniform.
// The leaf stage counts its tests through a pointer (atomicAdd on cnt[C_*]): each lane's own C_N
// slots in LDS, read once at the end; node visits and inline sphere tests count in registers.
template <int FEAT, bool ANY>
__global__ __launch_bounds__(QUERY_THREADS) void gs_query_kernel(DevScene sc, const TQuad* tquads, uint32_t root,
                                                                const gs_ray* rays, uint32_t n, uint64_t seed,
                                                                gs_ray_hit* hits, uint32_t* counts) {
    constexpr bool kNested = (FEAT & GS_FEAT_NESTED) != 0;
    constexpr bool kGeneral = (FEAT & GS_FEAT_GENERAL) != 0;
    __shared__ unsigned long long s_cnt[QUERY_THREADS * C_N];
    const size_t i = (size_t)blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i >= (size_t)n) return;  // (before anything is read)
    unsigned long long* const cnt = s_cnt + threadIdx.x * C_N;
#pragma unroll
    for (int k = 0; k < C_N; k++) cnt[k] = 0ull;

    const auto rp = sp<false>(reinterpret_cast<const double*>(rays + i));
    Ray ray0;
    ray0.o = mk(rp[0], rp[1], rp[2]);
    ray0.d = mk(rp[3], rp[4], rp[5]);
    ray0.time = rp[6];
    const double tmin = rp[7], tmax = rp[8];
    uint64_t rng = stream_seed(seed, (uint32_t)i, (uint32_t)((uint64_t)i >> 32));
    const QuadSrc qs{nullptr, tquads, 0u, nullptr, 0u};  // no mirror: every record from global memory

    Ray ray = ray0;            // the ray in the space of the tree being walked
    d3 inv = inv_of(ray.d);    // AABB.rs:62: 1.0 / ray.direction, per axis
    double a = len2(ray.d);    // sphere.rs:66
    double closest = tmax;
    bool hit = false;
    uint32_t hit_ref = GS_REF_NONE, hit_inst = GS_REF_NONE, hit_outer = GS_REF_NONE;
    uint32_t ninst = GS_REF_NONE;  // the instance leaf whose BVH the lane walks (none: the top level)
    uint32_t ret = THR_END;        // ... and the link after that leaf
    uint32_t c_nodes = 0, c_sph = 0;
    uint32_t cur = root;
    // Termination for any ray bits (NaN or zero directions, tmin > tmax, infinities): a link only
    // ever points forward in the tree's pre-order -- a node's hit link to the next record, its miss
    // link past its subtree, a leaf's link to the next record -- so whatever the tests decide, each
    // step moves on and the walk reaches THR_END after at most one visit per record.  A BVH under
    // an instance chain is a second finite walk of the same kind, entered from the top level only
    // (validate() allows one level), which returns to the saved forward link at THR_RET.  A
    // malformed ray is a miss or whatever the reference's arithmetic makes of it, never a fault:
    // no index is computed from the ray.
#pragma unroll 1
    while (cur != THR_END) {
        if (kNested && cur == THR_RET) {  // the nested tree is done: back to the caller's ray
            ray = ray0;
            inv = inv_of(ray.d);
            a = len2(ray.d);
            cur = ret;
            ninst = GS_REF_NONE;
            continue;
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
            cur = box_hit_ref(nb, ray.o, inv, tmin, closest) ? l_hit : l_miss;
            continue;
        }
        const auto lf = sp<false>(sc.tleaves + (size_t)(cur & ~THR_LEAF));
        const uint32_t next = lf->next, ref = lf->ref;
        cur = next;
        if ((ref >> GS_REF_SHIFT) == GS_REF_SPHERE) {  // a stationary sphere, inline in the record
            c_sph++;
            double t;
            if (sphere_accept_rr(mk(lf->cx, lf->cy, lf->cz), lf->rr, ray, a, tmin, closest, t)) {
                hit = true;
                closest = t;
                hit_ref = ref;
                hit_inst = ninst;
                hit_outer = GS_REF_NONE;
                if (ANY) break;
            }
            continue;
        }
        Ray rl = ray;  // (the ray in the leaf's space after its instance chain)
        const LeafHit lh = leaf_other<FEAT, false>(sc, qs, ref, rl, tmin, closest, rng, cnt);
        if (lh.hit) {
            hit = true;
            closest = lh.t;
            hit_ref = lh.ref;
            if (kGeneral && lh.inst != GS_REF_NONE && ninst != GS_REF_NONE) {  // a chain inside a tree under a chain
                hit_inst = lh.inst;
                hit_outer = ninst;
            } else {
                hit_inst = (!kNested || lh.inst != GS_REF_NONE) ? lh.inst : ninst;
                hit_outer = GS_REF_NONE;
            }
            if (ANY) break;
        }
        if (kNested && lh.enter != 0 && ninst == GS_REF_NONE) {
            // the chain ended in a BVH: walked in this same loop with the ray in the tree's space
            ret = next;
            ninst = ref;
            ray.o = rl.o;
            ray.d = rl.d;
            inv = inv_of(ray.d);
            a = len2(ray.d);
            cur = ld_u32<false>(sc.nroots + (lh.enter - 1u));
        }
    }

    // The record: HitRecord's fields from reconstruct of (ref, inst, t); one plain store per field.
    double o9[9];
    uint32_t w6[6];
    o9[0] = hit ? closest : tmax;
#pragma unroll
    for (int k = 1; k < 9; k++) o9[k] = 0.0;
    w6[0] = hit ? 1u : 0u;
    w6[1] = 0u;
    w6[2] = w6[3] = w6[4] = GS_REF_NONE;
    w6[5] = 0u;
    if (hit) {
        HitRec h = reconstruct<kGeneral>(sc, ray0, closest, hit_ref, hit_inst, hit_outer);
        const uint32_t kind = hit_ref >> GS_REF_SHIFT;
        if ((kind == GS_REF_SPHERE || kind == GS_REF_MSPHERE) && !sc.mats[h.mat].needs_uv) {
            // reconstruct takes a sphere's u, v only for materials that read them; HitRecord
            // always holds them (sphere.rs:55-60, :83): the same point in the sphere's space
            Ray r = ray0;
            if (hit_outer != GS_REF_NONE) chain_forward(sc, hit_outer, r);
            if (hit_inst != GS_REF_NONE) chain_forward(sc, hit_inst, r);
            d3 c;
            double rad;
            if (kind == GS_REF_SPHERE) {
                const DSphere s = sc.spheres[hit_ref & GS_REF_MASK];
                c = mk(s.cx, s.cy, s.cz);
                rad = s.r;
            } else {
                const gs_msphere& s = sc.mspheres[hit_ref & GS_REF_MASK];
                c = add(ld3(s.center_start), muls(ld3(s.center_path), r.time));
                rad = s.radius;
            }
            sphere_uv(divs(sub(add(r.o, muls(r.d, closest)), c), rad), h.u, h.v);
        }
        o9[1] = h.p.x; o9[2] = h.p.y; o9[3] = h.p.z;
        o9[4] = h.n.x; o9[5] = h.n.y; o9[6] = h.n.z;
        o9[7] = h.u;
        o9[8] = h.v;
        w6[1] = h.front ? 1u : 0u;
        w6[2] = h.mat;
        w6[3] = hit_ref;
        w6[4] = hit_inst;
    }
    {
        const auto hp = (__attribute__((address_space(1))) double*)(reinterpret_cast<double*>(hits + i));
#pragma unroll
        for (int k = 0; k < 9; k++) hp[k] = o9[k];
        const auto wp = (__attribute__((address_space(1))) uint32_t*)(reinterpret_cast<uint32_t*>(hits + i) + 18);
#pragma unroll
        for (int k = 0; k < 6; k++) wp[k] = w6[k];
        *(__attribute__((address_space(1))) uint64_t*)(reinterpret_cast<uint64_t*>(hits + i) + 12) = rng;
    }
    if (counts) {  // oracle.World.HIT_COUNTERS' order
        const auto cp = (__attribute__((address_space(1))) uint32_t*)(counts + i * 8);
        cp[0] = c_nodes + (uint32_t)cnt[C_NODES];  // (+ the GS_FEAT_GENERAL walks of medium-boundary BVHs)
        cp[1] = c_sph + (uint32_t)cnt[C_SPH];
        cp[2] = (uint32_t)cnt[C_MSPH];
        cp[3] = (uint32_t)cnt[C_QUAD];
        cp[4] = (uint32_t)cnt[C_TRI];
        cp[5] = (uint32_t)cnt[C_INST];
        cp[6] = (uint32_t)cnt[C_LIST];
        cp[7] = (uint32_t)cnt[C_MED];
    }
}

namespace {

static_assert(sizeof(gs_ray) == 72 && sizeof(gs_ray_hit) == 104, "the kernel reads and writes these by word");
static_assert(offsetof(gs_ray_hit, hit) == 72 && offsetof(gs_ray_hit, state) == 96, "gs_ray_hit layout");

template <int FEAT>
hipError_t launch_mode(bool any, dim3 grid, hipStream_t st, const DevScene& sc, const TQuad* tquads, uint32_t root,
                       const gs_ray* rays, uint32_t n, uint64_t seed, gs_ray_hit* hits, uint32_t* counts) {
    if (any) hipLaunchKernelGGL((gs_query_kernel<FEAT, true>), grid, dim3(QUERY_THREADS), 0, st, sc, tquads, root, rays, n, seed, hits, counts);
    else hipLaunchKernelGGL((gs_query_kernel<FEAT, false>), grid, dim3(QUERY_THREADS), 0, st, sc, tquads, root, rays, n, seed, hits, counts);
    return hipGetLastError();
}

}  // namespace

// The launch behind gs_query_rays_async (csrc/host/query.cpp, which has checked the arguments):
// the instantiation for the scene's MEDIA / NESTED / GENERAL bits, grid ceil(n / 256).
hipError_t gs_query_launch(int feat, int any, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_ray* rays,
                           uint32_t n, uint64_t seed, gs_ray_hit* hits, uint32_t* counts, hipStream_t st) {
    const dim3 grid((n + QUERY_THREADS - 1u) / QUERY_THREADS);
#define GS_QUERY_CASE(F) \
    return launch_mode<F>(any != 0, grid, st, sc, tquads, root, rays, n, seed, hits, counts)
    if (feat & GS_FEAT_GENERAL) GS_QUERY_CASE(GS_FEAT_GENERAL | GS_FEAT_MEDIA | GS_FEAT_NESTED);
    switch (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED)) {
        case 0: GS_QUERY_CASE(0);
        case GS_FEAT_MEDIA: GS_QUERY_CASE(GS_FEAT_MEDIA);
        case GS_FEAT_NESTED: GS_QUERY_CASE(GS_FEAT_NESTED);
        default: GS_QUERY_CASE(GS_FEAT_MEDIA | GS_FEAT_NESTED);
    }
#undef GS_QUERY_CASE
}
