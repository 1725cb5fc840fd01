// query.cpp — the host side of the ray queries (gs_query_rays_async, gs_query_rays): the argument
// checks, the scene's mutex around the one launch, and the synchronous form's copies.  The kernel
// and its instantiation table are csrc/device/query.hip's.
#include <hip/hip_runtime_api.h>

#include <mutex>
#include <string>

#include "render_host.hpp"

hipError_t gs_query_launch(int feat, int any, const DevScene& sc, const TQuad* tquads, uint32_t root, const gs_ray* rays,
                           uint32_t n, uint64_t seed, gs_ray_hit* hits, uint32_t* counts, hipStream_t st);

static_assert(sizeof(gs_ray) == 72 && sizeof(gs_ray_hit) == 104, "gs_ray / gs_ray_hit layout (grayshift_gpu.h)");

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

}  // extern "C"
