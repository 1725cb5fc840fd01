// query.cpp — the host side of the ray queries (gs_query_rays_async, gs_query_rays) and the radiance
// queries (gs_query_radiance_async, gs_query_radiance, and gs_query_radiance_gen_async,
// gs_query_radiance_gen with their rays made on the device): the argument checks, the scratch sizing,
// the scene's mutex around the launches, and the synchronous forms' copies.  The kernels and their
// instantiation tables are csrc/device/query.hip's, radiance.hip's and raygen.hip's.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>

#include "render_host.hpp"

hipError_t gs_query_launch(int feat, int any, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_ray* rays,
                           uint32_t n, uint64_t seed, gs_ray_hit* hits, uint32_t* counts, hipStream_t st);

hipError_t gs_radiance_launch(int feat, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_ray* rays,
                              uint32_t n, uint32_t samples, uint32_t chunk, uint32_t chunks, uint32_t max_depth,
                              uint64_t seed, const uint64_t* states, gs_ray_radiance* out, gs_ray_radiance* part,
                              unsigned long long* counters, uint32_t shade_batch, hipStream_t st);

hipError_t gs_raygen_launch(int feat, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_raygen& gen,
                            const gs_ray* points, uint32_t n, uint32_t samples, uint32_t first_sample, uint32_t chunk,
                            uint32_t chunks, uint32_t max_depth, uint64_t seed, gs_ray_radiance* out, gs_ray_radiance* part,
                            unsigned long long* counters, gs_ray* rays_out, uint64_t* states_out, uint32_t shade_batch,
                            hipStream_t st);

static_assert(sizeof(gs_ray) == 72 && sizeof(gs_ray_hit) == 104, "gs_ray / gs_ray_hit layout (grayshift_gpu.h)");
static_assert(sizeof(gs_ray_radiance) == 40, "gs_ray_radiance layout (grayshift_gpu.h)");
static_assert(sizeof(gs_camera) == 168 && sizeof(gs_raygen) == 280 && offsetof(gs_raygen, cam) == 16 &&
                  offsetof(gs_raygen, origin) == 184 && offsetof(gs_raygen, axis) == 208,
              "gs_raygen layout (grayshift_gpu.h)");

// Lanes of a wave that wait at their walk's end before the wave shades them (gs_debug_set_radiance_batch;
// MI355X, C4's world: DESIGN.md §3.7).  Scheduling only: every choice returns the same bits.
#define GS_RADIANCE_SHADE_BATCH 24
static std::atomic<int32_t> g_radiance_batch{GS_RADIANCE_SHADE_BATCH};

// A radiance query's chunking: `chunk` samples per work item (0: 16), chunks per ray; false when
// the arguments are bad (n < 0, no samples, 2^31 items or more).
static bool radiance_items(int64_t n, uint32_t samples, uint32_t chunk, uint32_t& chunk_out, uint32_t& chunks) {
    if (n < 0 || samples == 0) return false;
    chunk_out = chunk ? chunk : 16u;
    chunks = (samples - 1u) / chunk_out + 1u;
    return n < ((int64_t)1 << 31) && n * (int64_t)chunks < ((int64_t)1 << 31);
}

// The checks both forms share, on the arguments alone (nothing of the scene is read).
static gs_status check_args(const char* who, const gs_device_scene* ds, const void* rays, int64_t n, int32_t mode,
                            const void* hits) {
    if (!ds || !rays || !hits) return fail(GS_ERR_ARG, std::string(who) + ": null argument");
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(GS_ERR_ARG, std::string(who) + ": n must be in [0, 2^31)");
    if (mode != GS_QUERY_CLOSEST && mode != GS_QUERY_ANY)
        return fail(GS_ERR_ARG, std::string(who) + ": mode must be GS_QUERY_CLOSEST or GS_QUERY_ANY");
    return GS_OK;
}

extern "C" {

gs_status gs_query_rays_async(const gs_device_scene* ds, const gs_ray* d_rays, int64_t n, int32_t mode, uint64_t seed,
                              gs_ray_hit* d_hits, uint32_t* d_counts, void* stream) {
    gs_status e = check_args("gs_query_rays_async", ds, d_rays, n, mode, d_hits);
    if (e != GS_OK) return e;
    if (n == 0) return GS_OK;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev != ds->device) return fail(GS_ERR_ARG, "scene lives on another device");
    const hipStream_t st = (hipStream_t)stream;
    gs_device_scene* mds = const_cast<gs_device_scene*>(ds);
    // Under the scene's mutex, as a render's launch: the placement pilot's end rewrites the threaded
    // records and the root in place under it, after waiting for every launch enqueued so far.  A
    // query has no launch slot, so it leaves one event of its own for that wait; a query on another
    // stream first waits for the previous one's event, so the one event stands for them all.
    std::lock_guard<std::mutex> lock(mds->mu);
    if (!mds->query_done) HIPCHK(hipEventCreateWithFlags(&mds->query_done, hipEventDisableTiming));
    if (mds->query_used && mds->query_stream != st) HIPCHK(hipStreamWaitEvent(st, mds->query_done, 0));
    HIPCHK(gs_query_launch(ds->feat, mode == GS_QUERY_ANY, ds->dev, ds->tquads, ds->thr_root, d_rays, (uint32_t)n, seed,
                           d_hits, d_counts, st));
    HIPCHK(hipEventRecord(mds->query_done, st));
    mds->query_used = true;
    mds->query_stream = st;
    return GS_OK;
}

gs_status gs_query_rays(const gs_device_scene* ds, const gs_ray* rays, int64_t n, int32_t mode, uint64_t seed,
                        gs_ray_hit* hits, uint32_t* counts) {
    gs_status e = check_args("gs_query_rays", ds, rays, n, mode, hits);
    if (e != GS_OK) return e;
    if (n == 0) return GS_OK;
    const size_t rb = (size_t)n * sizeof(gs_ray), hb = (size_t)n * sizeof(gs_ray_hit), cb = counts ? (size_t)n * 32 : 0;
    // one allocation: rays, hits, counts (each a multiple of 8 B; the rays' size keeps 8-B alignment)
    char* d = nullptr;
    if (hipMalloc((void**)&d, rb + hb + cb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GS_ERR_OOM, "gs_query_rays: hipMalloc of the ray and result buffers failed");
    }
    gs_ray* d_rays = (gs_ray*)d;
    gs_ray_hit* d_hits = (gs_ray_hit*)(d + rb);
    uint32_t* d_counts = counts ? (uint32_t*)(d + rb + hb) : nullptr;
    hipError_t h = hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice);
    if (h == hipSuccess) {
        e = gs_query_rays_async(ds, d_rays, n, mode, seed, d_hits, d_counts, nullptr);
        if (e == GS_OK) h = hipStreamSynchronize(nullptr);
        if (e == GS_OK && h == hipSuccess) h = hipMemcpy(hits, d_hits, hb, hipMemcpyDeviceToHost);
        if (e == GS_OK && h == hipSuccess && counts) h = hipMemcpy(counts, d_counts, cb, hipMemcpyDeviceToHost);
    }
    const hipError_t f = hipFree(d);
    if (e != GS_OK) return e;
    if (h != hipSuccess) return fail(GS_ERR_HIP, std::string("gs_query_rays: ") + hipGetErrorString(h));
    if (f != hipSuccess) return fail(GS_ERR_HIP, std::string("gs_query_rays: hipFree: ") + hipGetErrorString(f));
    return GS_OK;
}

gs_status gs_debug_set_radiance_batch(int32_t shade_batch) {
    if (shade_batch < 0 || shade_batch > 64)
        return fail(GS_ERR_ARG, "gs_debug_set_radiance_batch: shade_batch must be in [0, 64] (0: the default)");
    g_radiance_batch.store(shade_batch ? shade_batch : GS_RADIANCE_SHADE_BATCH);
    return GS_OK;
}

int64_t gs_query_radiance_scratch_bytes(int64_t n, uint32_t samples, uint32_t chunk) {
    uint32_t c = 0, chunks = 0;
    if (!radiance_items(n, samples, chunk, c, chunks)) return -1;
    return chunks > 1u ? n * (int64_t)chunks * (int64_t)sizeof(gs_ray_radiance) : 0;
}

// The checks both radiance forms share, on the arguments alone (nothing of the scene is read).
static gs_status check_radiance(const char* who, const gs_device_scene* ds, const void* rays, int64_t n, uint32_t samples,
                                uint32_t chunk, const void* out, uint32_t& c, uint32_t& chunks) {
    if (!ds || !rays || !out) return fail(GS_ERR_ARG, std::string(who) + ": null argument");
    if (n < 0) return fail(GS_ERR_ARG, std::string(who) + ": n must not be negative");
    if (samples == 0) return fail(GS_ERR_ARG, std::string(who) + ": samples must be at least 1");
    if (!radiance_items(n, samples, chunk, c, chunks))
        return fail(GS_ERR_ARG, std::string(who) + ": n * ceil(samples / chunk) must be below 2^31");
    return GS_OK;
}

gs_status gs_query_radiance_async(const gs_device_scene* ds, const gs_ray* d_rays, int64_t n, uint32_t samples,
                                  uint32_t chunk, uint32_t max_depth, uint64_t seed, const uint64_t* d_states,
                                  gs_ray_radiance* d_out, gs_counters* d_counters, void* d_scratch, int64_t scratch_bytes,
                                  void* stream) {
    uint32_t c = 0, chunks = 0;
    gs_status e = check_radiance("gs_query_radiance_async", ds, d_rays, n, samples, chunk, d_out, c, chunks);
    if (e != GS_OK) return e;
    const int64_t need = chunks > 1u ? n * (int64_t)chunks * (int64_t)sizeof(gs_ray_radiance) : 0;
    if (need > 0 && (!d_scratch || scratch_bytes < need))
        return fail(GS_ERR_ARG, "gs_query_radiance_async: scratch is null or smaller than gs_query_radiance_scratch_bytes");
    if (n == 0) return GS_OK;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev != ds->device) return fail(GS_ERR_ARG, "scene lives on another device");
    const hipStream_t st = (hipStream_t)stream;
    gs_device_scene* mds = const_cast<gs_device_scene*>(ds);
    // Under the scene's mutex with the ray queries' one event (gs_query_rays_async): the placement
    // pilot's end waits for it before it rewrites the threaded records.
    std::lock_guard<std::mutex> lock(mds->mu);
    if (!mds->query_done) HIPCHK(hipEventCreateWithFlags(&mds->query_done, hipEventDisableTiming));
    if (mds->query_used && mds->query_stream != st) HIPCHK(hipStreamWaitEvent(st, mds->query_done, 0));
    HIPCHK(gs_radiance_launch(ds->feat, ds->dev, ds->tquads, ds->thr_root, d_rays, (uint32_t)n, samples, c, chunks,
                              max_depth, seed, d_states, d_out, (gs_ray_radiance*)d_scratch,
                              (unsigned long long*)d_counters, (uint32_t)g_radiance_batch.load(), st));
    HIPCHK(hipEventRecord(mds->query_done, st));
    mds->query_used = true;
    mds->query_stream = st;
    return GS_OK;
}

gs_status gs_query_radiance(const gs_device_scene* ds, const gs_ray* rays, int64_t n, uint32_t samples, uint32_t chunk,
                            uint32_t max_depth, uint64_t seed, const uint64_t* states, gs_ray_radiance* out,
                            gs_counters* counters) {
    uint32_t c = 0, chunks = 0;
    gs_status e = check_radiance("gs_query_radiance", ds, rays, n, samples, chunk, out, c, chunks);
    if (e != GS_OK) return e;
    if (n == 0) return GS_OK;
    {  // (the last check, before the buffers are allocated: nothing is copied for a scene elsewhere)
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        if (dev != ds->device) return fail(GS_ERR_ARG, "scene lives on another device");
    }
    const size_t rb = (size_t)n * sizeof(gs_ray), sb = states ? (size_t)n * samples * 8 : 0;
    const size_t ob = (size_t)n * sizeof(gs_ray_radiance), cb = counters ? sizeof(gs_counters) : 0;
    const size_t pb = chunks > 1u ? (size_t)n * chunks * sizeof(gs_ray_radiance) : 0;
    // one allocation: rays, states, out, counters, scratch (each a multiple of 8 B)
    char* d = nullptr;
    if (hipMalloc((void**)&d, rb + sb + ob + cb + pb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GS_ERR_OOM, "gs_query_radiance: hipMalloc of the ray and result buffers failed");
    }
    gs_ray* d_rays = (gs_ray*)d;
    uint64_t* d_states = states ? (uint64_t*)(d + rb) : nullptr;
    gs_ray_radiance* d_out = (gs_ray_radiance*)(d + rb + sb);
    gs_counters* d_cnt = counters ? (gs_counters*)(d + rb + sb + ob) : nullptr;
    void* d_part = pb ? (void*)(d + rb + sb + ob + cb) : nullptr;
    gs_counters got = {};
    hipError_t h = hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice);
    if (h == hipSuccess && states) h = hipMemcpy(d_states, states, sb, hipMemcpyHostToDevice);
    if (h == hipSuccess && counters) h = hipMemset(d_cnt, 0, cb);
    if (h == hipSuccess) {
        e = gs_query_radiance_async(ds, d_rays, n, samples, chunk, max_depth, seed, d_states, d_out, d_cnt, d_part,
                                    (int64_t)pb, nullptr);
        if (e == GS_OK) h = hipStreamSynchronize(nullptr);
        if (e == GS_OK && h == hipSuccess) h = hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost);
        if (e == GS_OK && h == hipSuccess && counters) h = hipMemcpy(&got, d_cnt, cb, hipMemcpyDeviceToHost);
    }
    const hipError_t f = hipFree(d);
    if (e != GS_OK) return e;
    if (h != hipSuccess) return fail(GS_ERR_HIP, std::string("gs_query_radiance: ") + hipGetErrorString(h));
    if (f != hipSuccess) return fail(GS_ERR_HIP, std::string("gs_query_radiance: hipFree: ") + hipGetErrorString(f));
    if (counters) {  // accumulated into, as the device form
        uint64_t* dst = reinterpret_cast<uint64_t*>(counters);
        const uint64_t* src = reinterpret_cast<const uint64_t*>(&got);
        for (size_t k = 0; k < sizeof(gs_counters) / 8; k++) dst[k] += src[k];
    }
    return GS_OK;
}

// The checks both generated forms share, on the arguments alone: the item count, the chunking and
// the generator as the launch takes it (a camera's dimensions copied to width and height).
static gs_status check_radiance_gen(const char* who, const gs_device_scene* ds, const gs_raygen* gen, const void* points,
                                    uint32_t samples, uint32_t first_sample, uint32_t chunk, const void* out, int64_t& n,
                                    uint32_t& c, uint32_t& chunks, gs_raygen& g) {
    if (!ds || !gen || !out) return fail(GS_ERR_ARG, std::string(who) + ": null argument");
    if (gen->kind < GS_GEN_CAMERA || gen->kind > GS_GEN_HEMISPHERE)
        return fail(GS_ERR_ARG, std::string(who) + ": kind must be one of the four GS_GEN_ generators");
    g = *gen;
    if (g.kind == GS_GEN_CAMERA) {
        g.width = g.cam.image_width;
        g.height = g.cam.image_height;
    }
    if (g.width < 1 || g.height < 1 || (g.kind == GS_GEN_HEMISPHERE && g.height != 1))
        return fail(GS_ERR_ARG, std::string(who) + ": width and height must be at least 1 (GS_GEN_HEMISPHERE: height 1)");
    if (g.kind == GS_GEN_HEMISPHERE && !points)
        return fail(GS_ERR_ARG, std::string(who) + ": GS_GEN_HEMISPHERE needs its points");
    if (samples == 0) return fail(GS_ERR_ARG, std::string(who) + ": samples must be at least 1");
    if ((uint64_t)first_sample + samples > ((uint64_t)1 << 32))
        return fail(GS_ERR_ARG, std::string(who) + ": first_sample + samples must not exceed 2^32");
    n = (int64_t)g.width * g.height;
    if (!radiance_items(n, samples, chunk, c, chunks))
        return fail(GS_ERR_ARG, std::string(who) + ": width * height * ceil(samples / chunk) must be below 2^31");
    return GS_OK;
}

gs_status gs_query_radiance_gen_async(const gs_device_scene* ds, const gs_raygen* gen, const gs_ray* d_points,
                                      uint32_t samples, uint32_t first_sample, uint32_t chunk, uint32_t max_depth,
                                      uint64_t seed, gs_ray_radiance* d_out, gs_counters* d_counters, gs_ray* d_rays_out,
                                      uint64_t* d_states_out, void* d_scratch, int64_t scratch_bytes, void* stream) {
    int64_t n = 0;
    uint32_t c = 0, chunks = 0;
    gs_raygen g;
    gs_status e = check_radiance_gen("gs_query_radiance_gen_async", ds, gen, d_points, samples, first_sample, chunk, d_out,
                                     n, c, chunks, g);
    if (e != GS_OK) return e;
    const int64_t need = chunks > 1u ? n * (int64_t)chunks * (int64_t)sizeof(gs_ray_radiance) : 0;
    if (need > 0 && (!d_scratch || scratch_bytes < need))
        return fail(GS_ERR_ARG,
                    "gs_query_radiance_gen_async: scratch is null or smaller than gs_query_radiance_scratch_bytes");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev != ds->device) return fail(GS_ERR_ARG, "scene lives on another device");
    const hipStream_t st = (hipStream_t)stream;
    gs_device_scene* mds = const_cast<gs_device_scene*>(ds);
    // Under the scene's mutex with the ray queries' one event, as gs_query_radiance_async.
    std::lock_guard<std::mutex> lock(mds->mu);
    if (!mds->query_done) HIPCHK(hipEventCreateWithFlags(&mds->query_done, hipEventDisableTiming));
    if (mds->query_used && mds->query_stream != st) HIPCHK(hipStreamWaitEvent(st, mds->query_done, 0));
    HIPCHK(gs_raygen_launch(ds->feat, ds->dev, ds->tquads, ds->thr_root, g, g.kind == GS_GEN_HEMISPHERE ? d_points : nullptr,
                            (uint32_t)n, samples, first_sample, c, chunks, max_depth, seed, d_out,
                            (gs_ray_radiance*)d_scratch, (unsigned long long*)d_counters, d_rays_out, d_states_out,
                            (uint32_t)g_radiance_batch.load(), st));
    HIPCHK(hipEventRecord(mds->query_done, st));
    mds->query_used = true;
    mds->query_stream = st;
    return GS_OK;
}

gs_status gs_query_radiance_gen(const gs_device_scene* ds, const gs_raygen* gen, const gs_ray* points, uint32_t samples,
                                uint32_t first_sample, uint32_t chunk, uint32_t max_depth, uint64_t seed,
                                gs_ray_radiance* out, gs_counters* counters, gs_ray* rays_out, uint64_t* states_out) {
    int64_t n = 0;
    uint32_t c = 0, chunks = 0;
    gs_raygen g;
    gs_status e = check_radiance_gen("gs_query_radiance_gen", ds, gen, points, samples, first_sample, chunk, out, n, c,
                                     chunks, g);
    if (e != GS_OK) return e;
    // the host arrays' sizes must be countable: n * samples gs_ray (n < 2^31, samples < 2^32: the product fits 64 bits)
    if ((rays_out || states_out) && (uint64_t)n * samples > (uint64_t)(SIZE_MAX / 2) / sizeof(gs_ray))
        return fail(GS_ERR_ARG, "gs_query_radiance_gen: width * height * samples rays_out / states_out do not fit memory");
    {  // (the last check, before the buffers are allocated: nothing is copied for a scene elsewhere)
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        if (dev != ds->device) return fail(GS_ERR_ARG, "scene lives on another device");
    }
    const bool hemi = g.kind == GS_GEN_HEMISPHERE;
    const size_t pb = hemi ? (size_t)n * sizeof(gs_ray) : 0, ob = (size_t)n * sizeof(gs_ray_radiance);
    const size_t cb = counters ? sizeof(gs_counters) : 0;
    const size_t rb = rays_out ? (size_t)n * samples * sizeof(gs_ray) : 0, sb = states_out ? (size_t)n * samples * 8 : 0;
    const size_t xb = chunks > 1u ? (size_t)n * chunks * sizeof(gs_ray_radiance) : 0;
    // one allocation: points, out, counters, rays out, states out, scratch (each a multiple of 8 B)
    char* d = nullptr;
    if (hipMalloc((void**)&d, pb + ob + cb + rb + sb + xb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GS_ERR_OOM, "gs_query_radiance_gen: hipMalloc of the point and result buffers failed");
    }
    gs_ray* d_points = hemi ? (gs_ray*)d : nullptr;
    gs_ray_radiance* d_out = (gs_ray_radiance*)(d + pb);
    gs_counters* d_cnt = counters ? (gs_counters*)(d + pb + ob) : nullptr;
    gs_ray* d_rays = rays_out ? (gs_ray*)(d + pb + ob + cb) : nullptr;
    uint64_t* d_states = states_out ? (uint64_t*)(d + pb + ob + cb + rb) : nullptr;
    void* d_part = xb ? (void*)(d + pb + ob + cb + rb + sb) : nullptr;
    gs_counters got = {};
    hipError_t h = hemi ? hipMemcpy(d_points, points, pb, hipMemcpyHostToDevice) : hipSuccess;
    if (h == hipSuccess && counters) h = hipMemset(d_cnt, 0, cb);
    // (max_depth 0 writes no ray and no state: the caller's arrays then come back zeroed, not stale)
    if (h == hipSuccess && rb + sb) h = hipMemset(d + pb + ob + cb, 0, rb + sb);
    if (h == hipSuccess) {
        e = gs_query_radiance_gen_async(ds, gen, d_points, samples, first_sample, chunk, max_depth, seed, d_out, d_cnt,
                                        d_rays, d_states, d_part, (int64_t)xb, nullptr);
        if (e == GS_OK) h = hipStreamSynchronize(nullptr);
        if (e == GS_OK && h == hipSuccess) h = hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost);
        if (e == GS_OK && h == hipSuccess && counters) h = hipMemcpy(&got, d_cnt, cb, hipMemcpyDeviceToHost);
        if (e == GS_OK && h == hipSuccess && rays_out) h = hipMemcpy(rays_out, d_rays, rb, hipMemcpyDeviceToHost);
        if (e == GS_OK && h == hipSuccess && states_out) h = hipMemcpy(states_out, d_states, sb, hipMemcpyDeviceToHost);
    }
    const hipError_t f = hipFree(d);
    if (e != GS_OK) return e;
    if (h != hipSuccess) return fail(GS_ERR_HIP, std::string("gs_query_radiance_gen: ") + hipGetErrorString(h));
    if (f != hipSuccess) return fail(GS_ERR_HIP, std::string("gs_query_radiance_gen: hipFree: ") + hipGetErrorString(f));
    if (counters) {  // accumulated into, as the device form
        uint64_t* dst = reinterpret_cast<uint64_t*>(counters);
        const uint64_t* src = reinterpret_cast<const uint64_t*>(&got);
        for (size_t k = 0; k < sizeof(gs_counters) / 8; k++) dst[k] += src[k];
    }
    return GS_OK;
}

}  // extern "C"
