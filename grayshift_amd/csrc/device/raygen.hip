// raygen.hip — radiance queries whose rays are made on the device (gs_query_radiance_gen_async,
// csrc/host/query.cpp): the reference's Camera::sample (camera.rs:138-141) draws the ray of every
// sample from the sample's own stream before it calls ray_color, and so does this kernel.  Item q of
// width * height (row-major) and sample s: the stream starts at stream_seed(seed, q, first_sample +
// s), one of four generators (gs_raygen.kind) draws the ray from it, and the path goes on from the
// stream the generator left -- the lane loop of radiance_loop.hpp, whose two ends are the plain walk
// (query_walk.hpp) and shade<false, false, GEN> (shading.hpp).  The third translation unit of
// libgrayshift_query.so (build.py), so the product's code objects do not change with it.
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

hipError_t gs_radiance_combine_launch(const gs_ray_radiance* part, uint32_t n, uint32_t chunks, gs_ray_radiance* out,
                                      hipStream_t st);

namespace {

static_assert(sizeof(gs_raygen) == 280 && offsetof(gs_raygen, cam) == 16 && offsetof(gs_raygen, origin) == 184 &&
                  offsetof(gs_raygen, axis) == 208,
              "gs_raygen layout (grayshift_gpu.h)");

// A sample's first segment, drawn from its stream.  The gs_raygen is the kernel's own argument, so
// its fields arrive by scalar loads and the kind is wave-uniform: one generator runs per wave, once
// per sample.  Nothing of it is kept in the lane between samples but the item's index.
struct GenFirst {
    const gs_raygen& g;  // (width: the row length for every kind; the launcher copies a camera's)
    const gs_ray* points;
    gs_ray* rays_out;
    uint64_t* states_out;
    uint64_t seed;
    uint32_t i, first_sample, samples;

    __device__ __forceinline__ uint64_t start(uint32_t s) const { return stream_seed(seed, i, first_sample + s); }

    __device__ __forceinline__ void ray(uint32_t s, uint64_t& rng, Ray& seg) const {
        // (o, d and time are set by every branch and go to the segment once, after them: a store to
        // another field at each branch's end would keep the segment in private memory)
        d3 o, d;
        double time;
        if (g.kind == GS_GEN_HEMISPHERE) {
            // Lambertian::scatter's direction (material.rs:52-53) about the caller's point and normal
            const auto pp = sp<false>(reinterpret_cast<const double*>(points + i));
            o = mk(pp[0], pp[1], pp[2]);
            // OrthonormalBasis::new (ONB.rs:10-23)
            d3 w = unit(mk(pp[3], pp[4], pp[5]));
            d3 a = fabs(w.x) > 0.9 ? mk(0.0, 1.0, 0.0) : mk(1.0, 0.0, 0.0);
            d3 vv = unit(cross(w, a));
            d3 uu = cross(w, vv);
            // random_cosine_direction (util.rs:48-60), r2^(1/4) quirk kept
            const double PI = 3.14159265358979323846;
            double r1 = wy_f64(rng);
            double r2 = wy_f64(rng);
            double phi = 2.0 * PI * r1;
            double r2s = sqrt(r2);
            double sp_, cp_;
            sincos(phi, &sp_, &cp_);
            double q = sqrt(r2s);
            d3 cd = mk(cp_ * q, sp_ * q, sqrt(1.0 - r2));
            d = unit(add(add(muls(uu, cd.x), muls(vv, cd.y)), muls(w, cd.z)));
            time = pp[6];
        } else {
            const uint32_t pj = i / (uint32_t)g.width, pi = i - pj * (uint32_t)g.width;
            double offx = wy_f64(rng) - 0.5;
            double offy = wy_f64(rng) - 0.5;
            double si = (double)pi + offx, sj = (double)pj + offy;
            if (g.kind == GS_GEN_CAMERA) {  // Camera::get_ray (camera.rs:204-221)
                const gs_camera& cam = g.cam;
                d3 ps = add(add(ld3(cam.starting_pixel_pos), muls(ld3(cam.pixel_delta_u), si)),
                            muls(ld3(cam.pixel_delta_v), sj));
                d3 org;
                if (cam.defocus_angle <= 0.0) {
                    org = ld3(cam.center);
                } else {  // defocus_disk_sample (camera.rs:223-226, util.rs:36-46)
                    double dx, dy;
#pragma unroll 1
                    for (;;) {
                        dx = wy_f64(rng) * 2.0 + -1.0;
                        dy = wy_f64(rng) * 2.0 + -1.0;
                        if (dx * dx + dy * dy + 0.0 * 0.0 < 1.0) break;
                    }
                    org = add(add(ld3(cam.center), muls(ld3(cam.defocus_disk_u), dx)), muls(ld3(cam.defocus_disk_v), dy));
                }
                o = org;
                d = sub(ps, org);
            } else if (g.kind == GS_GEN_PANORAMA) {  // query.panorama_rays' convention, in the axes' frame
                const double PI = 3.14159265358979323846;
                double theta = ((si + 0.5) / (double)g.width - 0.5) * (2.0 * PI);
                double phi = (0.5 - (sj + 0.5) / (double)g.height) * PI;
                double st, ct, sp_, cp_;
                sincos(theta, &st, &ct);
                sincos(phi, &sp_, &cp_);
                d3 dl = unit(mk(cp_ * ct, cp_ * st, sp_));
                o = ld3(g.origin);
                d = add(add(muls(ld3(g.axis[0]), dl.x), muls(ld3(g.axis[1]), dl.y)), muls(ld3(g.axis[2]), dl.z));
            } else {  // GS_GEN_ORTHO: query.ortho_rays' rectangle
                o = add(add(ld3(g.origin), muls(ld3(g.axis[0]), (si + 0.5) / (double)g.width)),
                            muls(ld3(g.axis[1]), (sj + 0.5) / (double)g.height));
                d = ld3(g.axis[2]);
            }
            time = wy_f64(rng);
        }
        seg.o = o;
        seg.d = d;
        seg.time = time;
        // the pair gs_query_radiance takes back: the ray, and the stream right after its generation
        const size_t k = (size_t)i * samples + s;
        if (rays_out) {  // (wave-uniform: a kernel argument)
            const auto rp = (__attribute__((address_space(1))) double*)(reinterpret_cast<double*>(rays_out + k));
            rp[0] = o.x;
            rp[1] = o.y;
            rp[2] = o.z;
            rp[3] = d.x;
            rp[4] = d.y;
            rp[5] = d.z;
            rp[6] = time;
            rp[7] = 0.001;
            rp[8] = 1.7976931348623157e308;
        }
        if (states_out) ((__attribute__((address_space(1))) uint64_t*)states_out)[k] = rng;
    }
};

}  // namespace

// The lane loop of radiance_loop.hpp with a generated first segment; the launch shape, the records
// and the counters are gs_radiance_kernel's.  rays_out / states_out (nullable): [items / chunks *
// samples] each, written by the lane that traces the sample.
template <int FEAT>
__global__ __launch_bounds__(RAD_THREADS) void gs_raygen_kernel(DevScene sc, const TQuad* tquads, uint32_t root,
                                                                gs_raygen gen, const gs_ray* points, uint32_t items,
                                                                uint32_t samples, uint32_t first_sample, uint32_t chunk,
                                                                uint32_t chunks, uint32_t max_depth, uint64_t seed,
                                                                gs_ray_radiance* dst, unsigned long long* counters,
                                                                gs_ray* rays_out, uint64_t* states_out,
                                                                uint32_t shade_batch) {
    __shared__ unsigned long long s_cnt[RAD_THREADS * C_N];
    const uint32_t q = blockIdx.x * RAD_THREADS + threadIdx.x;  // (items < 2^31, checked by the host)
    unsigned long long* const cnt = s_cnt + threadIdx.x * C_N;
#pragma unroll
    for (int k = 0; k < C_N; k++) cnt[k] = 0ull;

    if (q < items) {  // (nothing is read or written for a lane past the last item)
        radiance_lane<FEAT>(sc, tquads, root, q, samples, chunk, chunks, max_depth, dst, shade_batch, cnt,
                            [&](uint32_t i, Ray&) {
                                return GenFirst{gen, points, rays_out, states_out, seed, i, first_sample, samples};
                            });
    }
    if (!counters) return;  // (wave-uniform: a kernel argument)
    __syncthreads();
    radiance_flush_counters(s_cnt, counters);
}

// The launches behind gs_query_radiance_gen_async (csrc/host/query.cpp, which has checked the
// arguments): the instantiation for the scene's MEDIA / NESTED / GENERAL bits over n * chunks
// items, then -- more than one chunk per item -- radiance.hip's combine over n items.
hipError_t gs_raygen_launch(int feat, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_raygen& gen,
                            const gs_ray* points, uint32_t n, uint32_t samples, uint32_t first_sample, uint32_t chunk,
                            uint32_t chunks, uint32_t max_depth, uint64_t seed, gs_ray_radiance* out, gs_ray_radiance* part,
                            unsigned long long* counters, gs_ray* rays_out, uint64_t* states_out, uint32_t shade_batch,
                            hipStream_t st) {
    const uint32_t items = n * chunks;
    const dim3 grid((items + RAD_THREADS - 1u) / RAD_THREADS);
    gs_ray_radiance* const dst = chunks > 1u ? part : out;
#define GS_GEN_CASE(F)                                                                                                \
    hipLaunchKernelGGL((gs_raygen_kernel<F>), grid, dim3(RAD_THREADS), 0, st, sc, tquads, root, gen, points, items, samples, \
                       first_sample, chunk, chunks, max_depth, seed, dst, counters, rays_out, states_out, shade_batch); \
    break
    if (feat & GS_FEAT_GENERAL) {
        do { GS_GEN_CASE(GS_FEAT_GENERAL | GS_FEAT_MEDIA | GS_FEAT_NESTED); } while (0);
    } else {
        switch (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED)) {
            case 0: GS_GEN_CASE(0);
            case GS_FEAT_MEDIA: GS_GEN_CASE(GS_FEAT_MEDIA);
            case GS_FEAT_NESTED: GS_GEN_CASE(GS_FEAT_NESTED);
            default: GS_GEN_CASE(GS_FEAT_MEDIA | GS_FEAT_NESTED);
        }
    }
#undef GS_GEN_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || chunks <= 1u) return e;
    return gs_radiance_combine_launch(part, n, chunks, out, st);
}
