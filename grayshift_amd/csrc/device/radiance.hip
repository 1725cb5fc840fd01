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

namespace {

constexpr int RAD_THREADS = 256;

static_assert(sizeof(gs_ray) == 72 && sizeof(gs_ray_radiance) == 40, "the kernels read and write these by word");
static_assert(offsetof(gs_ray_radiance, rays) == 24 && offsetof(gs_ray_radiance, state) == 32, "gs_ray_radiance layout");

__device__ __forceinline__ void store_record(gs_ray_radiance* dst, double r, double g, double b, uint64_t rays,
                                             uint64_t state) {
    const auto dp = (__attribute__((address_space(1))) double*)(reinterpret_cast<double*>(dst));
    dp[0] = r;
    dp[1] = g;
    dp[2] = b;
    const auto wp = (__attribute__((address_space(1))) uint64_t*)(reinterpret_cast<uint64_t*>(dst));
    wp[3] = rays;
    wp[4] = state;
}

}  // namespace

// Work item q = (ray q / chunks, samples [(q % chunks) * chunk, + chunk) of it) per lane; 256-lane
// blocks at one wave per SIMD, as gs_query_kernel.  The lane's loop is flat: an iteration is one
// walk step, or -- at THR_END -- one shade, or the start of the lane's next sample, so a lane whose
// path has ended goes on with its next sample while its neighbours still walk (nested loops over
// samples, segments and records would make a wave wait at every path's end for its longest path).
// shade_batch (1 .. 64): lanes at THR_END a wave collects before it runs the shade for them.
// The item's record -- sum of its samples' colours in sample order from +0.0, world.hit calls, the
// stream after its last sample -- goes to dst[q]: the caller's output when a ray is one chunk, else
// the scratch gs_radiance_combine_kernel folds.  The leaf stage and the shading count through the
// lane's own C_N slots in LDS; the block adds its totals to `counters` once.
template <int FEAT>
__global__ __launch_bounds__(RAD_THREADS) void gs_radiance_kernel(DevScene sc, const TQuad* tquads, uint32_t root,
                                                                  const gs_ray* rays, uint32_t items, uint32_t samples,
                                                                  uint32_t chunk, uint32_t chunks, uint32_t max_depth,
                                                                  uint64_t seed, const uint64_t* states,
                                                                  gs_ray_radiance* dst, unsigned long long* counters,
                                                                  uint32_t shade_batch) {
    constexpr bool kGeneral = (FEAT & GS_FEAT_GENERAL) != 0;
    __shared__ unsigned long long s_cnt[RAD_THREADS * C_N];
    const uint32_t q = blockIdx.x * RAD_THREADS + threadIdx.x;  // (items < 2^31, checked by the host)
    unsigned long long* const cnt = s_cnt + threadIdx.x * C_N;
#pragma unroll
    for (int k = 0; k < C_N; k++) cnt[k] = 0ull;

    if (q < items) {  // (nothing is read or written for a lane past the last item)
        const uint32_t i = q / chunks, ck = q - i * chunks;
        const auto rp = sp<false>(reinterpret_cast<const double*>(rays + i));
        Ray seg;  // the path's current segment, in the world's space
        const d3 o0 = mk(rp[0], rp[1], rp[2]), d0 = mk(rp[3], rp[4], rp[5]);
        seg.time = rp[6];  // (tmin, tmax are not read: every segment is tested over (0.001, f64::MAX))
        const double tmin = 0.001, tmax = 1.7976931348623157e308;  // camera.rs:177
        const QuadSrc qs{nullptr, tquads, 0u, nullptr, 0u};  // no mirror: every record from global memory
        const auto sp0 = states ? sp<false>(states + (size_t)i * samples) : nullptr;

        uint32_t s = ck * chunk;
        const uint32_t s_end = (samples - s < chunk) ? samples : s + chunk;
        double sr = 0.0, sg = 0.0, sb = 0.0;  // the chunk's sum: ((0 + c) + c) + ...
        double Tr = 1.0, Tg = 1.0, Tb = 1.0;
        uint64_t rng = 0, n_rays = 0, n_paths = 0;
        uint32_t depth = 0, c_nodes = 0, c_sph = 0;
        bool need = true;  // the lane's next step starts a sample
        QWalk w;
        w.cur = THR_END;
        // A segment's start: the lane's 32-bit node and sphere counts go to its 64-bit slots first (a
        // walk visits each record at most once and there are fewer than 2^27, so the counts cannot
        // wrap inside a segment, however long max_depth makes the path), then the walk begins.
        auto begin_segment = [&]() {
            cnt[C_NODES] += c_nodes;
            cnt[C_SPH] += c_sph;
            c_nodes = c_sph = 0;
            qwalk_begin(w, seg, root, tmax);
            n_rays++;
        };
#pragma unroll 1
        for (;;) {
            if (need) {  // the lane's next sample, or the end of its item
                if (s == s_end) break;
                rng = sp0 ? sp0[s] : stream_seed(seed, i, s);
                s++;
                n_paths++;
                if (max_depth == 0) {  // ray_color(ray, 0) = 0 (camera.rs:175): no ray is traced
                    sr += 0.0;
                    sg += 0.0;
                    sb += 0.0;
                    continue;
                }
                seg.o = o0;
                seg.d = d0;
                Tr = Tg = Tb = 1.0;
                depth = max_depth;
                begin_segment();
                need = false;
            }
            const bool walking = w.cur != THR_END;
            // Lanes whose walk is done wait for company before they shade: the shade is many times a
            // walk step, and a wave pays for it whenever one lane takes it.  They go when shade_batch
            // lanes wait, or when no lane of the wave walks any more (so no lane waits for ever: a
            // walking lane steps in every iteration, and every walk ends).  Which lanes run together
            // moves no bit: each lane computes its own path in its own order.  Nor does anything rest
            // on the ballots seeing the whole wave: were the loop's lanes not reconverged here, a
            // ballot over part of them would only make batches smaller -- m_walk != 0 always means
            // that a lane counted in it steps in this very iteration.
            const uint64_t m_walk = __builtin_amdgcn_ballot_w64(walking);
            const uint64_t m_wait = __builtin_amdgcn_ballot_w64(!walking);
            if (walking) {
                qwalk_step<FEAT, false>(sc, qs, w, seg, tmin, rng, cnt, c_nodes, c_sph);
                continue;
            }
            if (m_walk != 0ull && (uint32_t)__popcll(m_wait) < shade_batch) continue;
            // the segment's walk is done: the sky, or the hit's emitted colour and scatter
            const ShadeOut so = shade<false, false, kGeneral>(sc, seg, w.closest, w.hit_ref, w.hit_inst, rng, cnt, w.hit_outer);
            double Lr = 0.0, Lg = 0.0, Lb = 0.0;
            if (so.cont) {
                Tr = Tr * so.col.x;
                Tg = Tg * so.col.y;
                Tb = Tb * so.col.z;
                depth--;
                if (depth > 0) {
                    seg.d = so.dir;  // (seg.o = p: set by shade)
                    begin_segment();
                    continue;
                }  // else ray_color(.., 0) = 0 (camera.rs:175): black
            } else {
                // sky (camera.rs:201), emitter (DiffuseLight never scatters) or absorbed (col = 0)
                Lr = Tr * so.col.x;
                Lg = Tg * so.col.y;
                Lb = Tb * so.col.z;
            }
            sr += Lr;
            sg += Lg;
            sb += Lb;
            need = true;
        }
        store_record(dst + q, sr, sg, sb, n_rays, rng);
        cnt[C_NODES] += c_nodes;
        cnt[C_SPH] += c_sph;
        cnt[C_RAYS] += n_rays;
        cnt[C_PATHS] += n_paths;
    }
    if (!counters) return;  // (wave-uniform: a kernel argument)
    __syncthreads();
    if (threadIdx.x < C_N && threadIdx.x != C_PIX) {  // (pixels: left alone)
        unsigned long long t = 0ull;
#pragma unroll 1
        for (int l = 0; l < RAD_THREADS; l++) t += s_cnt[l * C_N + threadIdx.x];
        if (t) atomicAdd(&counters[threadIdx.x], t);
    }
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
    hipLaunchKernelGGL(gs_radiance_combine_kernel, dim3((n + RAD_THREADS - 1u) / RAD_THREADS), dim3(RAD_THREADS), 0, st,
                       part, n, chunks, out);
    return hipGetLastError();
}
