// radiance.hip — radiance queries: what light comes back along caller-supplied rays
// (gs_query_radiance_async, csrc/host/query.cpp): the reference's Camera::ray_color(ray, depth,
// world) (camera.rs:174-202) for a batch of rays and a number of samples each.
//
// The two ends are headers the ray queries already use: the plain walk (query_walk.hpp) answers
// world.hit over Interval(0.001, f64::MAX), and shade<false, false, GEN> (shading.hpp) answers the
// miss (the sky) or the hit (the HitRecord, Material::emitted / scatter) and moves the ray's origin
// to the hit point.  Between them, the megakernel's path logic (render.hip, "shade"): throughput
// times attenuation, a depth countdown, the terminal radiance T * c.  A translation unit of its own
// in libgrayshift_query.so (build.py), so the product's code objects do not change with it.
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
#include "radiance_loop.hpp"

namespace {

// The fixed-ray case of the lane loop (radiance_loop.hpp): every sample of item i starts along the
// caller's ray i, from stream_seed(seed, i, s) or the caller's state.
struct FixedRay {
    d3 o0, d0;
    const GS_SCENE_AS(false) uint64_t* sp0;
    uint64_t seed;
    uint32_t i;
    __device__ __forceinline__ uint64_t start(uint32_t s) const { return sp0 ? sp0[s] : stream_seed(seed, i, s); }
    __device__ __forceinline__ void ray(uint32_t, uint64_t&, Ray& seg) const {
        seg.o = o0;
        seg.d = d0;
    }
};

}  // namespace

// The lane loop of radiance_loop.hpp over caller rays: item i's samples all start along rays[i]
// (tmin, tmax are not read: every segment is tested over (0.001, f64::MAX)).  The block adds its
// lanes' totals to `counters` once.
template <int FEAT>
__global__ __launch_bounds__(RAD_THREADS) void gs_radiance_kernel(DevScene sc, const TQuad* tquads, uint32_t root,
                                                                  const gs_ray* rays, uint32_t items, uint32_t samples,
                                                                  uint32_t chunk, uint32_t chunks, uint32_t max_depth,
                                                                  uint64_t seed, const uint64_t* states,
                                                                  gs_ray_radiance* dst, unsigned long long* counters,
                                                                  uint32_t shade_batch) {
    __shared__ unsigned long long s_cnt[RAD_THREADS * C_N];
    const uint32_t q = blockIdx.x * RAD_THREADS + threadIdx.x;  // (items < 2^31, checked by the host)
    unsigned long long* const cnt = s_cnt + threadIdx.x * C_N;
#pragma unroll
    for (int k = 0; k < C_N; k++) cnt[k] = 0ull;

    if (q < items) {  // (nothing is read or written for a lane past the last item)
        radiance_lane<FEAT>(sc, tquads, root, q, samples, chunk, chunks, max_depth, dst, shade_batch, cnt,
                            [&](uint32_t i, Ray& seg) {
                                const auto rp = sp<false>(reinterpret_cast<const double*>(rays + i));
                                seg.time = rp[6];
                                return FixedRay{mk(rp[0], rp[1], rp[2]), mk(rp[3], rp[4], rp[5]),
                                                states ? sp<false>(states + (size_t)i * samples) : nullptr, seed, i};
                            });
    }
    if (!counters) return;  // (wave-uniform: a kernel argument)
    __syncthreads();
    radiance_flush_counters(s_cnt, counters);
}

// One lane per ray: rgb = ((0 + C_0) + C_1) + ..., the chunks' world.hit calls summed, the last
// chunk's stream.
__global__ __launch_bounds__(RAD_THREADS) void gs_radiance_combine_kernel(const gs_ray_radiance* part, uint32_t n,
                                                                          uint32_t chunks, gs_ray_radiance* out) {
    const uint32_t i = blockIdx.x * RAD_THREADS + threadIdx.x;
    if (i >= n) return;
    const gs_ray_radiance* const mine = part + (size_t)i * chunks;
    const auto p = (const __attribute__((address_space(1))) double*)(reinterpret_cast<const double*>(mine));
    const auto u = (const __attribute__((address_space(1))) uint64_t*)(reinterpret_cast<const uint64_t*>(mine));
    double r = 0.0, g = 0.0, b = 0.0;
    uint64_t rays = 0, state = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < chunks; k++) {
        r += p[(size_t)k * 5 + 0];
        g += p[(size_t)k * 5 + 1];
        b += p[(size_t)k * 5 + 2];
        rays += u[(size_t)k * 5 + 3];
        state = u[(size_t)k * 5 + 4];
    }
    store_record(out + i, r, g, b, rays, state);
}

// The combine alone, over n items of `chunks` records each: the generated queries' launcher
// (raygen.hip) ends with it too.
hipError_t gs_radiance_combine_launch(const gs_ray_radiance* part, uint32_t n, uint32_t chunks, gs_ray_radiance* out,
                                      hipStream_t st) {
    hipLaunchKernelGGL(gs_radiance_combine_kernel, dim3((n + RAD_THREADS - 1u) / RAD_THREADS), dim3(RAD_THREADS), 0, st,
                       part, n, chunks, out);
    return hipGetLastError();
}

// The launches behind gs_query_radiance_async (csrc/host/query.cpp, which has checked the
// arguments): the instantiation for the scene's MEDIA / NESTED / GENERAL bits over n * chunks
// items, then -- more than one chunk per ray -- the combine over n rays.
hipError_t gs_radiance_launch(int feat, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_ray* rays,
                              uint32_t n, uint32_t samples, uint32_t chunk, uint32_t chunks, uint32_t max_depth,
                              uint64_t seed, const uint64_t* states, gs_ray_radiance* out, gs_ray_radiance* part,
                              unsigned long long* counters, uint32_t shade_batch, hipStream_t st) {
    const uint32_t items = n * chunks;
    const dim3 grid((items + RAD_THREADS - 1u) / RAD_THREADS);
    gs_ray_radiance* const dst = chunks > 1u ? part : out;
#define GS_RAD_CASE(F)                                                                                               \
    hipLaunchKernelGGL((gs_radiance_kernel<F>), grid, dim3(RAD_THREADS), 0, st, sc, tquads, root, rays, items, samples, \
                       chunk, chunks, max_depth, seed, states, dst, counters, shade_batch);                         \
    break
    if (feat & GS_FEAT_GENERAL) {
        do { GS_RAD_CASE(GS_FEAT_GENERAL | GS_FEAT_MEDIA | GS_FEAT_NESTED); } while (0);
    } else {
        switch (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED)) {
            case 0: GS_RAD_CASE(0);
            case GS_FEAT_MEDIA: GS_RAD_CASE(GS_FEAT_MEDIA);
            case GS_FEAT_NESTED: GS_RAD_CASE(GS_FEAT_NESTED);
            default: GS_RAD_CASE(GS_FEAT_MEDIA | GS_FEAT_NESTED);
        }
    }
#undef GS_RAD_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || chunks <= 1u) return e;
    return gs_radiance_combine_launch(part, n, chunks, out, st);
}
