// radiance_loop.hpp — the lane loop of the radiance kernels (radiance.hip: gs_radiance_kernel, the
// caller's one ray for every sample of an item; raygen.hip: gs_raygen_kernel, a ray drawn on the
// device from each sample's own stream).  Between the plain walk (query_walk.hpp) and shade<false,
// false, GEN> (shading.hpp): the megakernel's path logic -- throughput times attenuation, a depth
// countdown, the terminal radiance T * c -- parameterised by how a sample's first segment is made.
// Written in namespace gsd's names: an includer says `using namespace gsd;` and includes leaf.hpp,
// shading.hpp and query_walk.hpp before this file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../../include/grayshift_gpu.h"

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

// Work item q = (item q / chunks, samples [(q % chunks) * chunk, + chunk) of it) per lane; 256-lane
// blocks at one wave per SIMD, as gs_query_kernel.  The lane's loop is flat: an iteration is one
// walk step, or -- at THR_END -- one shade, or the start of the lane's next sample, so a lane whose
// path has ended goes on with its next sample while its neighbours still walk (nested loops over
// samples, segments and records would make a wave wait at every path's end for its longest path).
// shade_batch (1 .. 64): lanes at THR_END a wave collects before it runs the shade for them.
// The item's record -- sum of its samples' colours in sample order from +0.0, world.hit calls, the
// stream after its last sample -- goes to dst[q]: the caller's output when an item is one chunk,
// else the scratch gs_radiance_combine_kernel folds.  The leaf stage and the shading count through
// the lane's own C_N slots in LDS (cnt).
//
// first(i): a FIRST for item i, made once before the loop, with
//   uint64_t start(uint32_t s)            the stream sample s begins with
//   void ray(uint32_t s, uint64_t& rng, Ray& seg)
//                                         the sample's first segment (o, d, time), drawing from rng
// ray() is not called at max_depth 0: such a sample draws nothing and traces nothing.  At the call
// the path state is dead (T, the segment and the walk are all set anew after it), so what ray()
// needs lives in registers only while it runs.
template <int FEAT, class MakeFirst>
__device__ __forceinline__ void radiance_lane(const DevScene& sc, const TQuad* tquads, uint32_t root, uint32_t q,
                                              uint32_t samples, uint32_t chunk, uint32_t chunks, uint32_t max_depth,
                                              gs_ray_radiance* dst, uint32_t shade_batch, unsigned long long* const cnt,
                                              MakeFirst make_first) {
    constexpr bool kGeneral = (FEAT & GS_FEAT_GENERAL) != 0;
    const uint32_t i = q / chunks, ck = q - i * chunks;
    Ray seg;  // the path's current segment, in the world's space
    auto first = make_first(i, seg);
    const double tmin = 0.001, tmax = 1.7976931348623157e308;  // camera.rs:177
    const QuadSrc qs{nullptr, tquads, 0u, nullptr, 0u};  // no mirror: every record from global memory

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
            rng = first.start(s);
            if (max_depth == 0) {  // ray_color(ray, 0) = 0 (camera.rs:175): no ray is made or traced
                s++;
                n_paths++;
                sr += 0.0;
                sg += 0.0;
                sb += 0.0;
                continue;
            }
            first.ray(s, rng, seg);
            s++;
            n_paths++;
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

// The block adds its lanes' totals to `counters` once (after a __syncthreads; pixels: left alone).
__device__ __forceinline__ void radiance_flush_counters(const unsigned long long* s_cnt, unsigned long long* counters) {
    if (threadIdx.x < C_N && threadIdx.x != C_PIX) {
        unsigned long long t = 0ull;
#pragma unroll 1
        for (int l = 0; l < RAD_THREADS; l++) t += s_cnt[l * C_N + threadIdx.x];
        if (t) atomicAdd(&counters[threadIdx.x], t);
    }
}
