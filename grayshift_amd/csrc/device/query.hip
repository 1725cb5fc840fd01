// query.hip — ray queries: the closest hit, or any hit, of caller-supplied rays against a device
// scene (gs_query_rays_async, csrc/host/query.cpp): the reference's world.hit(ray, Interval, rec)
// (hittable.rs, BVH.rs:69-90) for a batch of rays, one ray per lane.
//
// The megakernel's traversal cannot be lifted out of gs_render_kernel, but its two
// ends are headers: the leaf stage (leaf.hpp: leaf_other, LeafHit) and the hit-record stage
// (shading.hpp: reconstruct, HitRec).  gs_query_kernel runs a plain walk between them (query_walk.hpp,
// shared with radiance.hip's kernel), over the threaded records the upload already makes
// (DevScene::tnodes / tboxes / tleaves / nroots): no LDS mirror, no wave-level passes, no launch
// slot, no work queue.  Every node is decided by the f64 slab test on its TBox, as AABB::hit
// decides it (box_hit_ref).  Its own translation unit, linked
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
#include "query_walk.hpp"

namespace {

constexpr int QUERY_THREADS = 256;

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

    QWalk w;  // (query_walk.hpp: the walk both query kernels share)
    qwalk_begin(w, ray0, root, tmax);
    uint32_t c_nodes = 0, c_sph = 0;
#pragma unroll 1
    while (w.cur != THR_END) qwalk_step<FEAT, ANY>(sc, qs, w, ray0, tmin, rng, cnt, c_nodes, c_sph);
    const bool hit = w.hit;
    const double closest = w.closest;
    const uint32_t hit_ref = w.hit_ref, hit_inst = w.hit_inst, hit_outer = w.hit_outer;

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
