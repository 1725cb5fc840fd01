// multi_gpu.cpp — the frame context behind the synchronous C-ABI calls: gs_multi_* (one
// world on N GPUs, many frames), and gs_render_multi / gs_render / gs_render_ppm on top.
//
// Replaces the reference's whole pixel loop, camera.rs:105-114 (pixel list, rayon
// `par_iter` over every pixel, `collect_into_vec`), across the GPUs of one node from a
// single host thread: at creation the scene is uploaded to every device and one RCCL
// communicator is built (ncclCommInitAll, N > 1); per frame the image is cut into tiles
// (cost-balanced plan from a 1-spp pilot on the first device, kept while the camera is
// unchanged, or round-robin), every device renders its tiles into a packed buffer on its
// own stream, one grouped RCCL gather over xGMI brings the packed buffers to the first
// device, which unpacks them into the frame (and, optionally, formats the PPM text,
// camera.rs:101-103,116-118).  Pixels carry their own RNG streams, so the frame is the
// same for any device count.
//
// RCCL is resolved at run time (dlopen), so single-GPU users never load it, and the copy
// that matches the process's HIP runtime is used (torch bundles both: one HIP runtime
// per process).
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/grayshift_gpu.h"
#include "internal.hpp"

namespace {

gs_status fail(gs_status code, const std::string& msg) {
    gs_set_last_error(msg.c_str());
    return code;
}

struct Rccl {
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclCommAbort) comm_abort = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGather) gather = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    std::string path, error;
    bool ok = false;
};

// The RCCL next to the HIP runtime this process uses first (torch/lib/librccl.so beside
// torch's libamdhip64), then the loader's search path, then /opt/rocm.
const Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<std::string> cands;
        Dl_info info{};
        if (dladdr((const void*)&hipRuntimeGetVersion, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t k = dir.find_last_of('/');
            if (k != std::string::npos) {
                dir.resize(k);
                cands.push_back(dir + "/librccl.so");
                cands.push_back(dir + "/librccl.so.1");
            }
        }
        cands.push_back("librccl.so.1");
        cands.push_back("/opt/rocm/lib/librccl.so.1");
        void* h = nullptr;
        for (const auto& c : cands)
            if ((h = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL)) != nullptr) {
                r.path = c;
                break;
            }
        if (!h) {
            r.error = "librccl not found";
            return;
        }
        r.comm_init_all = (decltype(r.comm_init_all))dlsym(h, "ncclCommInitAll");
        r.comm_destroy = (decltype(r.comm_destroy))dlsym(h, "ncclCommDestroy");
        r.comm_abort = (decltype(r.comm_abort))dlsym(h, "ncclCommAbort");
        r.group_start = (decltype(r.group_start))dlsym(h, "ncclGroupStart");
        r.group_end = (decltype(r.group_end))dlsym(h, "ncclGroupEnd");
        r.gather = (decltype(r.gather))dlsym(h, "ncclGather");
        r.error_string = (decltype(r.error_string))dlsym(h, "ncclGetErrorString");
        r.ok = r.comm_init_all && r.comm_destroy && r.comm_abort && r.group_start && r.group_end && r.gather &&
               r.error_string;
        if (!r.ok) r.error = r.path + " lacks ncclCommInitAll/ncclCommAbort/ncclGather";
    });
    return r;
}

// SURVEY.md §8d algorithmic bytes per counted event (the same table as bench.py BYTES).
uint64_t algorithmic_bytes(const gs_counters& c) {
    return 56 * c.node_visits + 40 * c.sphere_tests + 64 * c.msphere_tests + 136 * c.quad_tests + 104 * c.tri_tests +
           32 * c.instance_tests + 16 * c.medium_tests + 32 * c.hits + 3 * c.image_texels + 12 * c.hdri_texels +
           12 * c.pixels + 168 * c.noise_evals;
}

void add_counters(gs_counters& a, const gs_counters& b) {
    const uint64_t* pb = (const uint64_t*)&b;
    uint64_t* pa = (uint64_t*)&a;
    for (size_t k = 0; k < sizeof(gs_counters) / sizeof(uint64_t); k++) pa[k] += pb[k];
}

// A device buffer grown on demand (contents not kept).
struct DBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t need) {
        if (bytes >= need && p) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        if (hipMalloc(&p, need + 16) != hipSuccess) return false;
        bytes = need;
        return true;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct Device {
    int id = 0;
    gs_device_scene* scene = nullptr;
    hipStream_t stream = nullptr;
    // render start / end, megakernel start / end, gather + unpack start / end
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DBuf order, packed, packed8, cnt;
    // an open accumulation (gs_multi_accum_*): the rank's running sums (cap * 3 f64, packed
    // order) and the last pass's per-block change, with its pinned host copy
    DBuf sums, delta;
    double* h_delta = nullptr;
    // an open adaptation (gs_multi_adapt_*): the rank's round state (launch.cpp's blob), the two
    // maps in packed order (cap u32, cap f32) and the pinned copy of the blob's summary words
    DBuf rstate, map_samples, map_error;
    unsigned long long* h_summary = nullptr;
    uint64_t ad_paths = 0;  // this rank's paths so far in the adaptation's device counters
    // the frame's counters, copied back on the stream behind the frame's last work, so the
    // host's wait is the only synchronisation (a synchronous copy after it cost C1 ~25 us)
    gs_counters* h_cnt = nullptr;  // pinned
};

#define HIPOK(x)                                                                                     \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) return fail(GS_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define GROW(buf, n)                                                                                            \
    do {                                                                                                        \
        if (!(buf).ensure((size_t)(n)))                                                                         \
            return fail(GS_ERR_OOM, "hipMalloc of " + std::to_string((long long)(n)) + " bytes failed");       \
    } while (0)

// Restores the caller's current device on every exit path.
struct DeviceGuard {
    int saved = 0;
    DeviceGuard() { (void)hipGetDevice(&saved); }
    ~DeviceGuard() { (void)hipSetDevice(saved); }
};

// The settings rules of an adaptation, on the arguments alone.
gs_status adapt_settings_check(const gs_sample_settings* ss) {
    if (ss->batch_size == 0) return fail(GS_ERR_ARG, "batch_size 0 never terminates (camera.rs:137)");
    if (ss->max_samples < ss->batch_size)
        return fail(GS_ERR_ARG, "the settings run one batch (max_samples < batch_size): a fixed-spp frame has its "
                                "passes in gs_multi_accum_begin");
    if ((uint64_t)ss->max_samples / ss->batch_size + 1u > 65536u)
        return fail(GS_ERR_ARG, "more than 65536 batches (max_samples / batch_size + 1): no round form");
    return GS_OK;
}

int g_collective_always = 0;  // gs_debug_set_multi_collective
int g_same_device = 0;        // gs_debug_set_multi_same_device

}  // namespace

struct gs_multi {
    std::vector<Device> dev;
    std::vector<int> ids;
    std::vector<ncclComm_t> comms;  // one rank per device (N > 1, or forced by the test hook)
    // gs_debug_set_multi_same_device: N ranks on one device list that may repeat a device, the
    // gather done by device copies on the ranks' streams instead of RCCL (N > 1, no comms)
    bool copy_gather = false;
    bool comms_broken = false;      // a collective failed: the communicators were aborted
    int32_t tw = 64, th = 64;
    bool plan = false;
    mutable std::mutex mu;  // one frame at a time; guards every field below and comms_broken
    // tile partition of the last camera (plan or round-robin)
    bool part_ready = false, part_rr = false;  // (part_rr: cut round-robin for a views call)
    gs_camera part_cam{};
    std::vector<int32_t> order;  // empty: round-robin
    int32_t slots = 0;
    int64_t cap = 0;  // packed pixels per rank
    // the first device's gather and frame buffers
    DBuf gathered, gathered8, frame, frame8, text, scratch, len;
    bool have_rgb = false, have_rgb8 = false;
    int32_t frame_w = 0, frame_h = 0;
    // The open accumulation (gs_multi_accum_begin .. _end): camera, seed and chunk are fixed,
    // the tile plan is the one computed at its start, and acc_samples samples of every pixel
    // are in the ranks' sums.
    bool acc_open = false;
    gs_camera acc_cam{};
    uint64_t acc_seed = 0, acc_samples = 0;
    uint32_t acc_chunk = 0, acc_passes = 0;
    double acc_last_delta = 0.0;
    gs_counters acc_counters{};
    // The open adaptation (gs_multi_adapt_begin .. _end): camera, settings and seed are fixed, the
    // tile plan is the one computed at its start, and ad_rounds rounds are in the ranks' state.
    bool ad_open = false;
    gs_camera ad_cam{};
    gs_sample_settings ad_ss{};
    uint64_t ad_seed = 0, ad_active = 0, ad_samples_total = 0, ad_samples_max = 0;
    uint32_t ad_rounds = 0, ad_R = 0;
    // The ranks' device counters run on from pass to pass (gs_round_params_kernel sizes a round's
    // items by the rays per path so far, as in a one-shot launch): zeroed by the first pass after
    // _begin / _upload (ad_fresh), their sum over the ranks so far in ad_dev, and ad_counters =
    // ad_base (an upload's) + ad_dev.
    bool ad_fresh = true;
    gs_counters ad_counters{}, ad_base{}, ad_dev{};
    // The open views accumulation (gs_multi_views_accum_begin .. _end): the views and the chunk are
    // fixed, the tall frame is cut round-robin into tw x va_th tiles (`th` holds va_th while it is
    // open, th_ctx the context's own), view v's sums hold va_samples[v] samples.  The ranks' sums
    // and change partials are the accumulation's buffers (Device::sums, delta: one per tile slot),
    // acc_cam the tall frame's camera (permute_sums).
    bool va_open = false;
    int32_t th_ctx = 64;
    std::vector<gs_view> va_views;
    gs_camera va_tall{};
    uint32_t va_chunk = 0, va_passes = 0;
    std::vector<uint32_t> va_samples;
    std::vector<double> va_delta;
    gs_counters va_counters{};
    // The open views adaptation (gs_multi_views_adapt_begin .. _end): an adaptation (ad_open and
    // every ad_* field above) whose camera is the tall frame's, cut round-robin into tw x
    // gs_views_tile_h tiles like a views accumulation (`th`, th_ctx), with the views' records.
    bool vd_open = false;
    std::vector<gs_view> vd_views;

    ~gs_multi() {
        DeviceGuard g;
        if (!comms_broken)
            for (auto& d : dev) {
                (void)hipSetDevice(d.id);
                if (d.stream) (void)hipStreamSynchronize(d.stream);
            }
        if (!comms.empty() && rccl().ok)
            for (auto c : comms)
                if (c) (comms_broken ? rccl().comm_abort(c) : rccl().comm_destroy(c));
        for (auto& d : dev) {
            (void)hipSetDevice(d.id);
            for (auto e : d.ev)
                if (e) (void)hipEventDestroy(e);
            d.order.release();
            d.packed.release();
            d.packed8.release();
            d.cnt.release();
            d.sums.release();
            d.delta.release();
            d.rstate.release();
            d.map_samples.release();
            d.map_error.release();
            if (d.h_delta) (void)hipHostFree(d.h_delta);
            if (d.h_summary) (void)hipHostFree(d.h_summary);
            if (d.h_cnt) (void)hipHostFree(d.h_cnt);
            if (d.scene) gs_device_scene_destroy(d.scene);
            if (d.stream) (void)hipStreamDestroy(d.stream);
        }
        if (!dev.empty()) {
            (void)hipSetDevice(dev[0].id);
            for (DBuf* b : {&gathered, &gathered8, &frame, &frame8, &text, &scratch, &len}) b->release();
        }
    }

    // Abort the communicators after a failed collective: its peers may never join, so the
    // streams holding it must not be waited on (destroy skips the stream syncs).
    gs_status collective_failed(const std::string& what) {
        if (rccl().ok)
            for (auto& c : comms)
                if (c) rccl().comm_abort(c);
        comms.clear();
        comms_broken = true;
        return fail(GS_ERR_HIP, what);
    }

    // round_robin: no cost plan whatever `plan` says (a views call's tall frame)
    gs_status partition(const gs_camera* cam, uint64_t seed, double* plan_ms, bool round_robin = false);
    // pass_samples != 0: a pass of the open accumulation (cam, ss and seed are then its own)
    // adapt: a pass of the open adaptation, of adapt_rounds rounds (0: resolve the state as it stands)
    // vw: a views call (cam is then the tall frame's camera, ss one batch of its samples; the
    // views' own seeds)
    struct ViewsCall {
        const gs_view* views;
        uint32_t n, chunk;
    };
    // vp: a pass of the open views accumulation (with vw: its views), over the views `selected`
    // (NULL: all), which all hold `base` samples
    struct ViewsPass {
        const uint8_t* selected;
        uint32_t base;
    };
    gs_status render(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed, const gs_multi_outputs* out,
                     gs_stats* stats, uint32_t pass_samples = 0, bool adapt = false, uint32_t adapt_rounds = 0,
                     const ViewsCall* vw = nullptr, const ViewsPass* vp = nullptr);
    gs_status views_accum_begin(const gs_view* views, uint32_t n_views, uint32_t chunk);
    void views_accum_end();
    gs_status accum_begin(const gs_camera* cam, uint64_t seed, uint32_t chunk);
    void accum_end();
    // The tile (or -1) of rank `rank`'s slot `slot`, and the slots the rank holds.
    int64_t rank_slots(int rank) const;
    int32_t slot_tile(int rank, int64_t slot) const;
    // Moves the sums between the ranks' packed buffers and an [H][W][3] image (to_image or back).
    gs_status permute_sums(double* image, bool to_image);
    // views: a views adaptation (cam is then the tall frame's camera; the arguments are checked by
    // the caller, gs_views_check)
    gs_status adapt_begin(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                          const gs_view* views = nullptr, uint32_t n_views = 0);
    gs_status adapt_open(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed, bool round_robin);
    void adapt_end();
    // What gs_multi_adapt_* and gs_multi_views_adapt_* share, on the open adaptation's frame (the
    // tall one for views): a pass, the maps, the state down (sums may be NULL) and, behind
    // adapt_begin, the state up.
    gs_status adapt_pass(uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats);
    gs_status adapt_maps(uint32_t* samples, float* rel_error);
    gs_status adapt_download(double* sums, uint32_t* state);
    gs_status adapt_fill(uint32_t rounds_done, const double* sums, const uint32_t* state, const gs_counters* counters);
    // The packed pixels of rank `rank` as its launches see them (gs_partition_capacity): `cap` under
    // a plan, fewer for the later ranks of a round-robin partition -- the size the rank's round
    // state is laid out for.
    int64_t rank_cap(int rank, const gs_camera& cam) const {
        if (!order.empty()) return cap;
        gs_partition p{rank, (int32_t)dev.size(), tw, th, nullptr, 0, 0};
        return std::max<int64_t>(0, gs_partition_capacity(&cam, &p));
    }
    bool adapt_finished() const { return ad_rounds > 0 && (ad_active == 0 || ad_rounds >= ad_R); }
    // Rank `rank`'s packed array of `elem`-byte records <-> the [H][W] image of them (to_image or
    // back; going back, slots outside the image keep what `packed` holds).
    void permute_rank(int rank, const gs_camera& cam, uint8_t* image, uint8_t* packed, size_t elem, bool to_image) const;
};

gs_status gs_multi::partition(const gs_camera* cam, uint64_t seed, double* plan_ms, bool round_robin) {
    if (part_ready && part_rr == round_robin && std::memcmp(&part_cam, cam, sizeof(gs_camera)) == 0) return GS_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int n = (int)dev.size();
    part_ready = false;
    order.clear();
    slots = 0;
    if (plan && n > 1 && !round_robin) {
        HIPOK(hipSetDevice(dev[0].id));
        gs_status s = gs_plan_tiles(dev[0].scene, cam, seed, n, tw, th, nullptr, 0, &slots);
        if (s != GS_OK) return s;
        order.resize((size_t)slots * n);
        s = gs_plan_tiles(dev[0].scene, cam, seed, n, tw, th, order.data(), (int64_t)order.size(), &slots);
        if (s != GS_OK) return s;
        for (auto& d : dev) {
            HIPOK(hipSetDevice(d.id));
            GROW(d.order, order.size() * sizeof(int32_t));
            HIPOK(hipMemcpy(d.order.p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        cap = (int64_t)slots * tw * th;
    } else {
        gs_partition p0{0, n, tw, th, nullptr, 0, 0};
        cap = gs_partition_capacity(cam, &p0);  // rank 0 holds the most tiles
        if (cap < 0) return fail(GS_ERR_ARG, "bad partition");
    }
    part_cam = *cam;
    part_rr = round_robin;
    part_ready = true;
    *plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GS_OK;
}

gs_status gs_multi::render(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                           const gs_multi_outputs* out, gs_stats* stats, uint32_t pass_samples, bool adapt,
                           uint32_t adapt_rounds, const ViewsCall* vw, const ViewsPass* vp) {
    if (!cam || !ss) return fail(GS_ERR_ARG, "null argument");
    if (out && !out->rgb && !out->rgb8 && !out->ppm_text) return fail(GS_ERR_ARG, "no output requested");
    if (out && out->ppm_text && !out->ppm_len) return fail(GS_ERR_ARG, "ppm_text without ppm_len");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    if (out && out->ppm_text && out->ppm_capacity < gs_ppm_max_bytes(cam->image_width, cam->image_height))
        return fail(GS_ERR_ARG, "ppm_capacity below gs_ppm_max_bytes");
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    if (acc_open && !pass_samples)  // (a new plan would invalidate the packed sums)
        return fail(GS_ERR_ARG, "an accumulation is open: gs_multi_accum_end first");
    if (ad_open && !adapt)  // (likewise: the round state is in the plan's packed order)
        return fail(GS_ERR_ARG, vd_open ? "a views adaptation is open: gs_multi_views_adapt_end first"
                                        : "an adaptation is open: gs_multi_adapt_end first");
    if (va_open && !vp)  // (likewise: the views' sums are in the packed order of its own tile height)
        return fail(GS_ERR_ARG, "a views accumulation is open: gs_multi_views_accum_end first");
    DeviceGuard guard;
    const auto t0 = std::chrono::steady_clock::now();
    const int n = (int)dev.size();
    double plan_ms = 0.0;
    gs_status s = partition(cam, seed, &plan_ms, vw != nullptr);
    if (s != GS_OK) return s;
    {
        // The scenes' placement pilots (first frame, launch.cpp, run before the first launch):
        // launched on every device before any is waited for, outside the timed render.
        std::vector<gs_device_scene*> sc(n);
        std::vector<void*> st(n);
        for (int i = 0; i < n; i++) sc[i] = dev[i].scene, st[i] = dev[i].stream;
        const auto tp = std::chrono::steady_clock::now();
        int ran = 0;
        // (a views call: view 0's own camera and frame)
        s = gs_placement_prepare(sc.data(), ids.data(), st.data(), n, vw ? &vw->views[0].cam : cam, ss, &ran);
        if (s != GS_OK) return s;
        if (ran) plan_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
    }
    const bool want_rgb = !out || out->rgb;
    const bool want8 = out && (out->rgb8 || out->ppm_text);
    const int64_t W = cam->image_width, H = cam->image_height;
    have_rgb = have_rgb8 = false;

    // One device and no collective: the render writes the frame itself (no packed tiles,
    // no unpack: C1 saved the unpack kernel and a stream gap, ~20 us of a 0.9 ms frame).
    const bool direct = n == 1 && comms.empty();
    Device& d0 = dev[0];
    HIPOK(hipSetDevice(d0.id));
    if (want_rgb) GROW(frame, W * H * 12);
    if (want8) GROW(frame8, W * H * 3);

    // Render: every device its own tiles, concurrently (launches are asynchronous).
    for (int i = 0; i < n; i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        if (want_rgb && !direct) GROW(d.packed, cap * 12);
        if (want8 && !direct) GROW(d.packed8, cap * 3);
        GROW(d.cnt, sizeof(gs_counters));  // (zeroed by the launch's parameter kernel)
        gs_partition p{i, n, tw, th, order.empty() ? nullptr : (const int32_t*)d.order.p, slots, 0};
        gs_render_outputs o{want_rgb ? (float*)(direct ? frame.p : d.packed.p) : nullptr,
                            want8 ? (uint8_t*)(direct ? frame8.p : d.packed8.p) : nullptr, nullptr};
        HIPOK(hipEventRecord(d.ev[0], d.stream));
        if (adapt) {
            const gs_round_outputs ro{o.rgb, o.rgb8, (uint32_t*)d.map_samples.p, (float*)d.map_error.p};
            s = vw ? gs_render_tiles_views_rounds_timed_async(d.scene, vw->views, vw->n, ss, &p, ad_rounds, adapt_rounds,
                                                              d.rstate.p, (int64_t)d.rstate.bytes, &ro,
                                                              (gs_counters*)d.cnt.p, d.stream, d.ev[2], d.ev[3], direct,
                                                              ad_fresh)
                   : gs_render_tiles_rounds_timed_async(d.scene, cam, ss, seed, &p, ad_rounds, adapt_rounds, d.rstate.p,
                                                        (int64_t)d.rstate.bytes, &ro, (gs_counters*)d.cnt.p, d.stream,
                                                        d.ev[2], d.ev[3], direct, ad_fresh);
        } else if (pass_samples) {
            HIPOK(hipMemsetAsync(d.delta.p, 0, (size_t)gs_pass_delta_blocks(cap) * 8, d.stream));
            s = gs_render_tiles_pass_timed_async(d.scene, cam, pass_samples, seed, &p, (uint32_t)acc_samples, acc_chunk,
                                                 (double*)d.sums.p, (double*)d.delta.p, &o, (gs_counters*)d.cnt.p,
                                                 d.stream, d.ev[2], d.ev[3], direct, true);
        } else if (vp) {  // (every slot's partial is written by the pass's combine: no memset)
            s = gs_render_tiles_views_pass_timed_async(d.scene, vw->views, vw->n, va_samples.data(), vp->selected,
                                                       ss->batch_size, vw->chunk, &p, (double*)d.sums.p, &o,
                                                       (double*)d.delta.p, (gs_counters*)d.cnt.p, d.stream, d.ev[2],
                                                       d.ev[3], direct, true);
        } else if (vw) {
            s = gs_render_tiles_views_timed_async(d.scene, vw->views, vw->n, ss->batch_size, vw->chunk, &p, &o,
                                                  (gs_counters*)d.cnt.p, d.stream, d.ev[2], d.ev[3], direct, true);
        } else {
            s = gs_render_tiles_timed_async(d.scene, cam, ss, seed, &p, &o, (gs_counters*)d.cnt.p, d.stream, d.ev[2],
                                            d.ev[3], direct, true);
        }
        if (s != GS_OK) return s;
        HIPOK(hipEventRecord(d.ev[1], d.stream));
    }
    HIPOK(hipSetDevice(d0.id));
    const void* src = want_rgb ? d0.packed.p : nullptr;
    const void* src8 = want8 ? d0.packed8.p : nullptr;
    if (!comms.empty()) {
        // One grouped RCCL gather of the packed tiles to the first device (rank-major, as
        // gs_unpack_tiles_part_async reads them).
        if (want_rgb) GROW(gathered, (int64_t)n * cap * 12);
        if (want8) GROW(gathered8, (int64_t)n * cap * 3);
        const Rccl& R = rccl();
        for (int i = 0; i < n; i++) {
            HIPOK(hipSetDevice(dev[i].id));
            HIPOK(hipEventRecord(dev[i].ev[4], dev[i].stream));
        }
        if (R.group_start() != ncclSuccess) return collective_failed("ncclGroupStart failed");
        ncclResult_t rc = ncclSuccess;
        for (int i = 0; i < n && rc == ncclSuccess; i++) {
            Device& d = dev[i];
            (void)hipSetDevice(d.id);
            if (want_rgb)
                rc = R.gather(d.packed.p, i == 0 ? gathered.p : nullptr, (size_t)cap * 3, ncclFloat32, 0, comms[i],
                              d.stream);
            if (rc == ncclSuccess && want8)
                rc = R.gather(d.packed8.p, i == 0 ? gathered8.p : nullptr, (size_t)cap * 3, ncclUint8, 0, comms[i],
                              d.stream);
        }
        const ncclResult_t rc2 = R.group_end();
        if (rc != ncclSuccess || rc2 != ncclSuccess)
            return collective_failed(std::string("ncclGather: ") + R.error_string(rc != ncclSuccess ? rc : rc2));
        HIPOK(hipSetDevice(d0.id));
        src = gathered.p;
        src8 = gathered8.p;
    } else if (copy_gather) {
        // The test mode's gather (gs_debug_set_multi_same_device): each rank's packed tiles
        // copied on its own stream into its rank-major slot of the first device's buffer,
        // which ncclGather would fill the same way; the first device's stream waits for all.
        if (want_rgb) GROW(gathered, (int64_t)n * cap * 12);
        if (want8) GROW(gathered8, (int64_t)n * cap * 3);
        for (int i = 0; i < n; i++) {
            Device& d = dev[i];
            HIPOK(hipSetDevice(d.id));
            if (want_rgb)
                HIPOK(hipMemcpyAsync((char*)gathered.p + (size_t)i * cap * 12, d.packed.p, (size_t)cap * 12,
                                     hipMemcpyDeviceToDevice, d.stream));
            if (want8)
                HIPOK(hipMemcpyAsync((char*)gathered8.p + (size_t)i * cap * 3, d.packed8.p, (size_t)cap * 3,
                                     hipMemcpyDeviceToDevice, d.stream));
            HIPOK(hipEventRecord(d.ev[4], d.stream));
        }
        HIPOK(hipSetDevice(d0.id));
        for (int i = 1; i < n; i++) HIPOK(hipStreamWaitEvent(d0.stream, dev[i].ev[4], 0));
        src = gathered.p;
        src8 = gathered8.p;
    }  // (no collective: the unpack is timed from the render's end event, ev[1])
    gs_partition pu{0, n, tw, th, order.empty() ? nullptr : (const int32_t*)d0.order.p, slots, 0};
    if (want_rgb && !direct) {
        s = gs_unpack_tiles_part_async(cam, &pu, cap, src, frame.p, 12, d0.stream);
        if (s != GS_OK) return s;
    }
    if (want8 && !direct) {
        s = gs_unpack_tiles_part_async(cam, &pu, cap, src8, frame8.p, 3, d0.stream);
        if (s != GS_OK) return s;
    }
    if (out && out->ppm_text) {
        const int64_t need = gs_ppm_max_bytes(cam->image_width, cam->image_height);
        const int64_t sb = gs_ppm_scratch_bytes(cam->image_width, cam->image_height);
        GROW(text, need);
        GROW(scratch, sb);
        GROW(len, 8);
        s = gs_ppm_encode_async((const uint8_t*)frame8.p, cam->image_width, cam->image_height, (char*)text.p, need,
                                (int64_t*)len.p, scratch.p, sb, d0.stream);
        if (s != GS_OK) return s;
    }
    // (direct without PPM text: nothing after the render to time, one stream marker fewer)
    const bool timed_tail = !direct || (out && out->ppm_text);
    if (timed_tail) HIPOK(hipEventRecord(d0.ev[5], d0.stream));
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipMemcpyAsync(d.h_cnt, d.cnt.p, sizeof(gs_counters), hipMemcpyDeviceToHost, d.stream));
        if (adapt)  // (the active count the next pass's clip needs: the pass's one read-back)
            HIPOK(hipMemcpyAsync(d.h_summary, (const char*)d.rstate.p + gs_round_layout(0, ad_R).summary,
                                 kRoundSummaryWords * 8, hipMemcpyDeviceToHost, d.stream));
        if (pass_samples)
            HIPOK(hipMemcpyAsync(d.h_delta, d.delta.p, (size_t)gs_pass_delta_blocks(cap) * 8, hipMemcpyDeviceToHost,
                                 d.stream));
        if (vp)
            HIPOK(hipMemcpyAsync(d.h_delta, d.delta.p, (size_t)(cap / ((int64_t)tw * th)) * 8, hipMemcpyDeviceToHost,
                                 d.stream));
    }
    // Wait, then results.
    gs_counters total{};
    double rmax = 0.0, rmin = 1e300, kmax = 0.0, kmin = 1e300;
    for (int i = 0; i < n; i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        add_counters(total, *d.h_cnt);
        float ms = 0.0f, kms = 0.0f;
        HIPOK(hipEventElapsedTime(&ms, d.ev[0], d.ev[1]));
        HIPOK(hipEventElapsedTime(&kms, d.ev[2], d.ev[3]));
        const uint64_t paths_before = adapt && !ad_fresh ? d.ad_paths : 0u;  // (an adaptation's counters run on)
        gs_device_scene_note_frame(d.scene, (double)kms, d.h_cnt->paths - paths_before);
        d.ad_paths = d.h_cnt->paths;
        rmax = std::max(rmax, (double)ms);
        rmin = std::min(rmin, (double)ms);
        kmax = std::max(kmax, (double)kms);
        kmin = std::min(kmin, (double)kms);
    }
    HIPOK(hipSetDevice(d0.id));
    float gms = 0.0f;
    if (timed_tail) HIPOK(hipEventElapsedTime(&gms, comms.empty() && !copy_gather ? d0.ev[1] : d0.ev[4], d0.ev[5]));
    have_rgb = want_rgb;
    have_rgb8 = want8;
    frame_w = cam->image_width;
    frame_h = cam->image_height;
    if (out && out->rgb) HIPOK(hipMemcpy(out->rgb, frame.p, (size_t)(W * H * 12), hipMemcpyDeviceToHost));
    if (out && out->rgb8) HIPOK(hipMemcpy(out->rgb8, frame8.p, (size_t)(W * H * 3), hipMemcpyDeviceToHost));
    if (out && out->ppm_text) {
        int64_t l = 0;
        HIPOK(hipMemcpy(&l, len.p, 8, hipMemcpyDeviceToHost));
        if (l <= 0 || l > out->ppm_capacity) return fail(GS_ERR_HIP, "PPM encoder returned a bad length");
        HIPOK(hipMemcpy(out->ppm_text, text.p, (size_t)l, hipMemcpyDeviceToHost));
        *out->ppm_len = l;
    }
    if (pass_samples) {
        // the pass's change: every rank's per-block partials in index order, the ranks in rank order
        double change = 0.0;
        const int64_t nb = gs_pass_delta_blocks(cap);
        for (int i = 0; i < n; i++)
            for (int64_t b = 0; b < nb; b++) change += dev[i].h_delta[b];
        acc_last_delta = change / ((double)W * (double)H * 3.0);
        gs_counters add = total;
        if (acc_samples != 0) add.pixels = 0;  // (the kernel counts a pixel at chunk 0 of every pass)
        add_counters(acc_counters, add);
        acc_samples += pass_samples;
        acc_passes += 1;
    }
    if (vp) {
        // the selected views' change: a view's per-slot partials rank after rank, each rank's in
        // slot order (round-robin: rank i's slot sl holds tile i + sl n, which lies in one view)
        const int64_t vh = va_views[0].cam.image_height, tx = (W + tw - 1) / tw, nt = tx * (H / th);
        std::vector<double> change(vw->n, 0.0);
        for (int i = 0; i < n; i++) {
            const int64_t ns = rank_cap(i, *cam) / ((int64_t)tw * th);
            for (int64_t sl = 0; sl < ns; sl++) {
                const int64_t tile = i + sl * n;
                if (tile < nt) change[(size_t)((tile / tx) * th / vh)] += dev[i].h_delta[sl];
            }
        }
        for (uint32_t v = 0; v < vw->n; v++)
            if (!vp->selected || vp->selected[v]) {
                va_delta[v] = change[v] / ((double)W * (double)vh * 3.0);
                va_samples[v] += ss->batch_size;
            }
        gs_counters add = total;
        // (the kernel counts the selected views' pixels at chunk 0 of every pass; they all start
        // at sample 0 or none does)
        if (vp->base != 0) add.pixels = 0;
        add_counters(va_counters, add);
        va_passes += 1;
    }
    if (adapt) {
        ad_active = ad_samples_total = ad_samples_max = 0;
        for (int i = 0; i < n; i++) {
            ad_active += dev[i].h_summary[0];
            ad_samples_total += dev[i].h_summary[1];
            ad_samples_max = std::max<uint64_t>(ad_samples_max, dev[i].h_summary[2]);
        }
        // this pass alone: the ranks' running counters minus their sum after the last pass
        const gs_counters before = ad_fresh ? gs_counters{} : ad_dev;
        ad_dev = total;
        ad_counters = ad_base;
        add_counters(ad_counters, ad_dev);
        const uint64_t* pb = (const uint64_t*)&before;
        uint64_t* pt = (uint64_t*)&total;
        for (size_t k = 0; k < sizeof(gs_counters) / sizeof(uint64_t); k++) pt[k] -= pb[k];
        ad_fresh = false;
        ad_rounds += adapt_rounds;
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->counters = total;
        stats->setup_ms = plan_ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        stats->render_ms_max = rmax;
        stats->render_ms_min = rmin;
        stats->kernel_ms_max = kmax;
        stats->kernel_ms_min = kmin;
        stats->gather_ms = gms;
        stats->algorithmic_bytes = algorithmic_bytes(total);
        stats->gathered_bytes =
            comms.empty() && !copy_gather ? 0 : (uint64_t)n * (uint64_t)cap * ((want_rgb ? 12u : 0u) + (want8 ? 3u : 0u));
        stats->num_gpus = n;
    }
    return GS_OK;
}

// ---------------------------------------------------------------- progressive accumulation
int64_t gs_multi::rank_slots(int rank) const {
    if (!order.empty()) return slots;
    gs_partition p{rank, (int32_t)dev.size(), tw, th, nullptr, 0, 0};
    return gs_partition_capacity(&acc_cam, &p) / ((int64_t)tw * th);
}

int32_t gs_multi::slot_tile(int rank, int64_t slot) const {
    const int64_t pos = rank + slot * (int64_t)dev.size();
    return order.empty() ? (int32_t)pos : order[(size_t)pos];
}

gs_status gs_multi::accum_begin(const gs_camera* cam, uint64_t seed, uint32_t chunk) {
    if (acc_open) return fail(GS_ERR_ARG, "an accumulation is already open: gs_multi_accum_end first");
    if (vd_open) return fail(GS_ERR_ARG, "a views adaptation is open: gs_multi_views_adapt_end first");
    if (ad_open) return fail(GS_ERR_ARG, "an adaptation is open: gs_multi_adapt_end first");
    if (va_open) return fail(GS_ERR_ARG, "a views accumulation is open: gs_multi_views_accum_end first");
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    DeviceGuard guard;
    double plan_ms = 0.0;
    gs_status s = partition(cam, seed, &plan_ms);
    if (s != GS_OK) return s;
    if (cap <= 0 || cap >= (int64_t)0xFFFFFFFFll) return fail(GS_ERR_ARG, "bad partition");
    const size_t nb = (size_t)gs_pass_delta_blocks(cap);
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        GROW(d.sums, cap * 24);
        GROW(d.delta, nb * 8);
        HIPOK(hipMemsetAsync(d.sums.p, 0, (size_t)cap * 24, d.stream));
        if (d.h_delta) (void)hipHostFree(d.h_delta);
        d.h_delta = nullptr;
        if (hipHostMalloc((void**)&d.h_delta, nb * 8, hipHostMallocDefault) != hipSuccess)
            return fail(GS_ERR_OOM, "hipHostMalloc of the pass's change failed");
        HIPOK(hipStreamSynchronize(d.stream));
    }
    acc_cam = *cam;
    acc_seed = seed;
    acc_chunk = chunk ? chunk : 16u;
    acc_samples = 0;
    acc_passes = 0;
    acc_last_delta = 0.0;
    acc_counters = gs_counters{};
    acc_open = true;
    return GS_OK;
}

void gs_multi::accum_end() {
    DeviceGuard guard;
    for (auto& d : dev) {
        (void)hipSetDevice(d.id);
        if (d.stream && !comms_broken) (void)hipStreamSynchronize(d.stream);
        d.sums.release();
        d.delta.release();
        if (d.h_delta) (void)hipHostFree(d.h_delta);
        d.h_delta = nullptr;
    }
    acc_open = false;
}

// Checkpoints are not hot: each rank's packed sums cross to the host whole, and the tile
// permutation runs there.
gs_status gs_multi::permute_sums(double* image, bool to_image) {
    DeviceGuard guard;
    const int64_t W = acc_cam.image_width, H = acc_cam.image_height, tpx = (int64_t)tw * th;
    const int64_t tx = (W + tw - 1) / tw, nt = tx * ((H + th - 1) / th);
    std::vector<double> packed((size_t)cap * 3);
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        if (to_image)
            HIPOK(hipMemcpy(packed.data(), d.sums.p, packed.size() * 8, hipMemcpyDeviceToHost));
        else
            std::fill(packed.begin(), packed.end(), 0.0);
        const int64_t ns = std::min<int64_t>(rank_slots(i), cap / tpx);
        for (int64_t sl = 0; sl < ns; sl++) {
            const int64_t tile = slot_tile(i, sl);
            if (tile < 0 || tile >= nt) continue;
            const int64_t x0 = (tile % tx) * tw, y0 = (tile / tx) * th;
            for (int64_t y = 0; y < th && y0 + y < H; y++) {
                const int64_t nx = std::min<int64_t>(tw, W - x0);
                double* img = image + ((y0 + y) * W + x0) * 3;
                double* pk = packed.data() + (sl * tpx + y * tw) * 3;
                if (to_image)
                    std::memcpy(img, pk, (size_t)nx * 24);
                else
                    std::memcpy(pk, img, (size_t)nx * 24);
            }
        }
        if (!to_image) HIPOK(hipMemcpy(d.sums.p, packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
    }
    return GS_OK;
}

// ---------------------------------------------------------------- progressive views
// (the arguments are checked by the caller: gs_views_check)
gs_status gs_multi::views_accum_begin(const gs_view* views, uint32_t n_views, uint32_t chunk) {
    if (va_open) return fail(GS_ERR_ARG, "a views accumulation is already open: gs_multi_views_accum_end first");
    if (acc_open) return fail(GS_ERR_ARG, "an accumulation is open: gs_multi_accum_end first");
    if (vd_open) return fail(GS_ERR_ARG, "a views adaptation is open: gs_multi_views_adapt_end first");
    if (ad_open) return fail(GS_ERR_ARG, "an adaptation is open: gs_multi_adapt_end first");
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    gs_scene_info si{};
    gs_status s = gs_device_scene_info(dev[0].scene, &si);
    if (s != GS_OK) return s;
    if (si.feat & 512)
        return fail(GS_ERR_UNSUPPORTED, "the scene needs the catch-all kernel, which has no views form");
    gs_camera tall = views[0].cam;
    tall.image_height = (int32_t)(n_views * (uint32_t)views[0].cam.image_height);
    DeviceGuard guard;
    // the accumulation's own tile height, so that no tile straddles two views; the cut is redone
    // whatever camera the last frame had (the partition's cache does not know the tile height)
    th_ctx = th;
    th = gs_views_tile_h(views[0].cam.image_height, th_ctx);
    part_ready = false;
    double plan_ms = 0.0;
    s = partition(&tall, 0, &plan_ms, true);
    if (s == GS_OK && (cap <= 0 || cap >= (int64_t)0xFFFFFFFFll)) s = fail(GS_ERR_ARG, "bad partition");
    const size_t nb = s == GS_OK ? (size_t)(cap / ((int64_t)tw * th)) : 0;
    for (size_t i = 0; s == GS_OK && i < dev.size(); i++) {
        Device& d = dev[i];
        if (hipSetDevice(d.id) != hipSuccess || !d.sums.ensure((size_t)cap * 24) || !d.delta.ensure(nb * 8)) {
            s = fail(GS_ERR_OOM, "hipMalloc of the views' sums failed");
            break;
        }
        if (d.h_delta) (void)hipHostFree(d.h_delta);
        d.h_delta = nullptr;
        if (hipHostMalloc((void**)&d.h_delta, nb * 8, hipHostMallocDefault) != hipSuccess)
            s = fail(GS_ERR_OOM, "hipHostMalloc of the pass's change failed");
        else if (hipMemsetAsync(d.sums.p, 0, (size_t)cap * 24, d.stream) != hipSuccess ||
                 hipStreamSynchronize(d.stream) != hipSuccess)
            s = fail(GS_ERR_HIP, "zeroing the views' sums failed");
    }
    va_open = true;  // (views_accum_end undoes a partial begin)
    if (s != GS_OK) {
        views_accum_end();
        return s;
    }
    va_views.assign(views, views + n_views);
    va_tall = tall;
    acc_cam = tall;  // (permute_sums, rank_slots)
    va_chunk = chunk ? chunk : 16u;
    va_passes = 0;
    va_samples.assign(n_views, 0u);
    va_delta.assign(n_views, 0.0);
    va_counters = gs_counters{};
    return GS_OK;
}

void gs_multi::views_accum_end() {
    DeviceGuard guard;
    for (auto& d : dev) {
        (void)hipSetDevice(d.id);
        if (d.stream && !comms_broken) (void)hipStreamSynchronize(d.stream);
        d.sums.release();
        d.delta.release();
        if (d.h_delta) (void)hipHostFree(d.h_delta);
        d.h_delta = nullptr;
    }
    th = th_ctx;
    part_ready = false;
    va_open = false;
}

// ---------------------------------------------------------------- progressive adaptation
gs_status gs_multi::adapt_begin(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                                const gs_view* views, uint32_t n_views) {
    if (!views) return adapt_open(cam, ss, seed, false);
    if (vd_open || ad_open || acc_open || va_open) return adapt_open(cam, ss, seed, true);  // (its refusal)
    gs_scene_info si{};
    const gs_status si_s = gs_device_scene_info(dev[0].scene, &si);
    if (si_s != GS_OK) return si_s;
    if (si.feat & 512) return fail(GS_ERR_UNSUPPORTED, "the scene needs the catch-all kernel, which has no views form");
    // the batch's own tile height, so that no tile straddles two views; the cut is redone whatever
    // camera the last frame had (the partition's cache does not know the tile height)
    const int32_t th_was = th;
    th = gs_views_tile_h(views[0].cam.image_height, th_was);
    part_ready = false;
    const gs_status s = adapt_open(cam, ss, seed, true);
    if (s != GS_OK) {
        th = th_was;
        part_ready = false;
        return s;
    }
    th_ctx = th_was;
    vd_views.assign(views, views + n_views);
    vd_open = true;
    return GS_OK;
}

gs_status gs_multi::adapt_open(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed, bool round_robin) {
    if (vd_open) return fail(GS_ERR_ARG, "a views adaptation is open: gs_multi_views_adapt_end first");
    if (ad_open) return fail(GS_ERR_ARG, "an adaptation is already open: gs_multi_adapt_end first");
    if (acc_open) return fail(GS_ERR_ARG, "an accumulation is open: gs_multi_accum_end first");
    if (va_open) return fail(GS_ERR_ARG, "a views accumulation is open: gs_multi_views_accum_end first");
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    gs_status s = adapt_settings_check(ss);
    if (s != GS_OK) return s;
    const uint64_t R = (uint64_t)ss->max_samples / ss->batch_size + 1u;
    DeviceGuard guard;
    double plan_ms = 0.0;
    s = partition(cam, seed, &plan_ms, round_robin);
    if (s != GS_OK) return s;
    if (cap <= 0 || cap >= (int64_t)0xFFFFFFFFll) return fail(GS_ERR_ARG, "bad partition");
    const GsRoundLayout l = gs_round_layout((uint64_t)cap, R);
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        GROW(d.rstate, l.bytes);
        GROW(d.map_samples, cap * 4);
        GROW(d.map_error, cap * 4);
        HIPOK(hipMemsetAsync(d.rstate.p, 0, l.bytes, d.stream));
        HIPOK(hipMemsetAsync(d.map_samples.p, 0, (size_t)cap * 4, d.stream));
        HIPOK(hipMemsetAsync(d.map_error.p, 0, (size_t)cap * 4, d.stream));
        if (!d.h_summary &&
            hipHostMalloc((void**)&d.h_summary, kRoundSummaryWords * 8, hipHostMallocDefault) != hipSuccess)
            return fail(GS_ERR_OOM, "hipHostMalloc of the round summary failed");
        HIPOK(hipStreamSynchronize(d.stream));
    }
    ad_cam = *cam;
    ad_ss = *ss;
    ad_seed = seed;
    ad_R = (uint32_t)R;
    ad_rounds = 0;
    ad_active = (uint64_t)cam->image_width * (uint64_t)cam->image_height;
    ad_samples_total = ad_samples_max = 0;
    ad_counters = ad_base = ad_dev = gs_counters{};
    ad_fresh = true;
    ad_open = true;
    return GS_OK;
}

void gs_multi::adapt_end() {
    DeviceGuard guard;
    for (auto& d : dev) {
        (void)hipSetDevice(d.id);
        if (d.stream && !comms_broken) (void)hipStreamSynchronize(d.stream);
        d.rstate.release();
        d.map_samples.release();
        d.map_error.release();
    }
    if (vd_open) {  // (the context's own tile height again)
        th = th_ctx;
        part_ready = false;
        vd_open = false;
    }
    ad_open = false;
}

gs_status gs_multi::adapt_pass(uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats) {
    if (rounds == 0) return fail(GS_ERR_ARG, "a pass of 0 rounds");
    const uint32_t todo = adapt_finished() ? 0u : std::min(rounds, ad_R - ad_rounds);
    if (!vd_open) return render(&ad_cam, &ad_ss, ad_seed, out, stats, 0, true, todo);
    if (out && out->ppm_text) return fail(GS_ERR_ARG, "a views pass writes no PPM text");
    const ViewsCall vw{vd_views.data(), (uint32_t)vd_views.size(), 0};
    return render(&ad_cam, &ad_ss, 0, out, stats, 0, true, todo, &vw);
}

gs_status gs_multi::adapt_maps(uint32_t* samples, float* rel_error) {
    DeviceGuard guard;
    std::vector<uint8_t> packed((size_t)cap * 4);
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        if (samples) {
            HIPOK(hipMemcpy(packed.data(), d.map_samples.p, packed.size(), hipMemcpyDeviceToHost));
            permute_rank(i, ad_cam, (uint8_t*)samples, packed.data(), 4, true);
        }
        if (rel_error) {
            HIPOK(hipMemcpy(packed.data(), d.map_error.p, packed.size(), hipMemcpyDeviceToHost));
            permute_rank(i, ad_cam, (uint8_t*)rel_error, packed.data(), 4, true);
        }
    }
    return GS_OK;
}

gs_status gs_multi::adapt_download(double* sums, uint32_t* state) {
    DeviceGuard guard;
    std::vector<uint8_t> packed((size_t)cap * 40);
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        const size_t rc = (size_t)rank_cap(i, ad_cam);
        const GsRoundLayout l = gs_round_layout(rc, ad_R);
        if (rc == 0) continue;
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        if (sums) {
            HIPOK(hipMemcpy(packed.data(), (const char*)d.rstate.p + l.pstate, rc * 40, hipMemcpyDeviceToHost));
            permute_rank(i, ad_cam, (uint8_t*)sums, packed.data(), 40, true);
        }
        HIPOK(hipMemcpy(packed.data(), (const char*)d.rstate.p + l.batches, rc * 4, hipMemcpyDeviceToHost));
        permute_rank(i, ad_cam, (uint8_t*)state, packed.data(), 4, true);
    }
    return GS_OK;
}

// Behind adapt_begin: the state of a checkpoint into the ranks' blobs (closes the adaptation again
// when it cannot).
gs_status gs_multi::adapt_fill(uint32_t rounds_done, const double* sums, const uint32_t* state,
                               const gs_counters* counters) {
    const gs_camera* cam = &ad_cam;
    const gs_sample_settings* ss = &ad_ss;
    auto bail = [&](gs_status st) {
        adapt_end();
        return st;
    };
    if (rounds_done > ad_R) return bail(fail(GS_ERR_ARG, "rounds_done exceeds the settings' rounds"));
    // every pixel's word against rounds_done: an active pixel has taken every round so far, a
    // stopped one at least one and no more than that
    const uint64_t npx = (uint64_t)cam->image_width * (uint64_t)cam->image_height;
    uint64_t active = 0, total = 0, most = 0;
    for (uint64_t k = 0; k < npx; k++) {
        const uint32_t nb = state[k] & ~GS_ADAPT_STOPPED;
        const bool stopped = (state[k] & GS_ADAPT_STOPPED) != 0;
        if (stopped ? (nb < 1 || nb > rounds_done) : (nb != rounds_done || (rounds_done == ad_R && rounds_done)))
            return bail(fail(GS_ERR_ARG, "a pixel's state disagrees with rounds_done"));
        active += stopped ? 0u : 1u;
        total += (uint64_t)nb * ss->batch_size;
        most = std::max<uint64_t>(most, (uint64_t)nb * ss->batch_size);
    }
    if (rounds_done == 0) {  // (nothing to fill: the first pass initialises the state)
        ad_counters = ad_base = *counters;
        return GS_OK;
    }
    DeviceGuard guard;
    std::vector<double> psums((size_t)this->cap * 5);
    std::vector<uint32_t> words((size_t)this->cap), list;
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        const size_t cap = (size_t)rank_cap(i, *cam);  // (the rank's own: its launches lay the state out for it)
        const GsRoundLayout l = gs_round_layout(cap, ad_R);
        if (cap == 0) continue;
        std::fill(psums.begin(), psums.end(), 0.0);
        std::fill(words.begin(), words.end(), GS_ADAPT_STOPPED);  // (padding: never active)
        permute_rank(i, *cam, (uint8_t*)const_cast<double*>(sums), (uint8_t*)psums.data(), 40, false);
        permute_rank(i, *cam, (uint8_t*)const_cast<uint32_t*>(state), (uint8_t*)words.data(), 4, false);
        // the round's active list, rebuilt in packed order (its order is scheduling only)
        list.clear();
        for (size_t k = 0; k < cap; k++) {
            if (!(words[k] & GS_ADAPT_STOPPED)) list.push_back((uint32_t)k);
            if (words[k] == GS_ADAPT_STOPPED) words[k] = 0u;
        }
        const uint32_t n_act = (uint32_t)list.size();
        char* blob = (char*)d.rstate.p;
        if (hipSetDevice(d.id) != hipSuccess ||
            hipMemcpy(blob + l.pstate, psums.data(), cap * 40, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(blob + l.batches, words.data(), cap * 4, hipMemcpyHostToDevice) != hipSuccess ||
            (n_act && hipMemcpy(blob + l.list[rounds_done & 1u], list.data(), (size_t)n_act * 4, hipMemcpyHostToDevice) !=
                          hipSuccess) ||
            hipMemcpy(blob + l.counts + (size_t)rounds_done * 4, &n_act, 4, hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(GS_ERR_HIP, "uploading the round state failed"));
    }
    ad_rounds = rounds_done;
    ad_active = active;
    ad_samples_total = total;
    ad_samples_max = most;
    ad_counters = ad_base = *counters;
    return GS_OK;
}

void gs_multi::permute_rank(int rank, const gs_camera& cam, uint8_t* image, uint8_t* packed, size_t elem,
                            bool to_image) const {
    const int64_t W = cam.image_width, H = cam.image_height, tpx = (int64_t)tw * th;
    const int64_t tx = (W + tw - 1) / tw, nt = tx * ((H + th - 1) / th);
    int64_t ns = cap / tpx;
    if (order.empty()) {
        gs_partition p{rank, (int32_t)dev.size(), tw, th, nullptr, 0, 0};
        ns = std::min<int64_t>(ns, gs_partition_capacity(&cam, &p) / tpx);
    }
    for (int64_t sl = 0; sl < ns; sl++) {
        const int64_t tile = slot_tile(rank, sl);
        if (tile < 0 || tile >= nt) continue;
        const int64_t x0 = (tile % tx) * tw, y0 = (tile / tx) * th;
        const int64_t nx = std::min<int64_t>(tw, W - x0);
        for (int64_t y = 0; y < th && y0 + y < H; y++) {
            uint8_t* img = image + (size_t)((y0 + y) * W + x0) * elem;
            uint8_t* pk = packed + (size_t)(sl * tpx + y * tw) * elem;
            if (to_image)
                std::memcpy(img, pk, (size_t)nx * elem);
            else
                std::memcpy(pk, img, (size_t)nx * elem);
        }
    }
}

extern "C" {

gs_status gs_multi_adapt_begin(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed) {
    if (!m || !cam || !ss) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return m->adapt_begin(cam, ss, seed);
}

gs_status gs_multi_adapt_pass(gs_multi* m, uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->ad_open || m->vd_open) return fail(GS_ERR_ARG, "no adaptation is open: gs_multi_adapt_begin first");
    return m->adapt_pass(rounds, out, stats);
}

gs_status gs_multi_adapt_info(const gs_multi* m, gs_adapt_info* info) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->ad_open || m->vd_open) return fail(GS_ERR_ARG, "no adaptation is open");
    std::memset(info, 0, sizeof(*info));
    info->width = m->ad_cam.image_width;
    info->height = m->ad_cam.image_height;
    info->batch = m->ad_ss.batch_size;
    info->rounds = m->ad_rounds;
    info->max_rounds = m->ad_R;
    info->finished = m->adapt_finished() ? 1u : 0u;
    info->seed = m->ad_seed;
    info->active_pixels = m->ad_active;
    info->samples_total = m->ad_samples_total;
    info->samples_max = m->ad_samples_max;
    info->counters = m->ad_counters;
    return GS_OK;
}

gs_status gs_multi_adapt_maps(gs_multi* m, uint32_t* samples, float* rel_error) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->ad_open || m->vd_open) return fail(GS_ERR_ARG, "no adaptation is open");
    return m->adapt_maps(samples, rel_error);
}

gs_status gs_multi_adapt_download(gs_multi* m, double* sums, uint32_t* state) {
    if (!m || !sums || !state) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->ad_open || m->vd_open) return fail(GS_ERR_ARG, "no adaptation is open");
    return m->adapt_download(sums, state);
}

gs_status gs_multi_adapt_upload(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                                uint32_t rounds_done, const double* sums, const uint32_t* state,
                                const gs_counters* counters) {
    if (!m || !cam || !ss || !sums || !state || !counters) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    gs_status s = m->adapt_begin(cam, ss, seed);
    if (s != GS_OK) return s;
    return m->adapt_fill(rounds_done, sums, state, counters);
}

gs_status gs_multi_adapt_end(gs_multi* m) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->ad_open || m->vd_open) return fail(GS_ERR_ARG, "no adaptation is open");
    m->adapt_end();
    return GS_OK;
}

// ---- adaptive views: the adaptation's calls on the tall frame
// The views' rules and the settings' rules, on the arguments alone; the tall frame's camera.
static gs_status views_adapt_check(const gs_multi* m, const gs_view* views, uint32_t n_views,
                                   const gs_sample_settings* ss, gs_camera* tall) {
    if (!ss) return fail(GS_ERR_ARG, "null argument");
    gs_status s = gs_views_check(m->dev[0].scene, views, n_views, 1, 1, tall);  // (one chunk: the views' own rules)
    if (s == GS_OK) s = adapt_settings_check(ss);
    return s;
}

gs_status gs_multi_views_adapt_begin(gs_multi* m, const gs_view* views, uint32_t n_views, const gs_sample_settings* ss) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    gs_camera tall;
    const gs_status s = views_adapt_check(m, views, n_views, ss, &tall);
    if (s != GS_OK) return s;
    return m->adapt_begin(&tall, ss, 0, views, n_views);
}

gs_status gs_multi_views_adapt_pass(gs_multi* m, uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->vd_open) return fail(GS_ERR_ARG, "no views adaptation is open: gs_multi_views_adapt_begin first");
    return m->adapt_pass(rounds, out, stats);
}

gs_status gs_multi_views_adapt_info(gs_multi* m, gs_views_adapt_info* info, uint64_t* view_active_out) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->vd_open) return fail(GS_ERR_ARG, "no views adaptation is open");
    const uint32_t nv = (uint32_t)m->vd_views.size();
    std::memset(info, 0, sizeof(*info));
    info->width = m->ad_cam.image_width;
    info->height = m->vd_views[0].cam.image_height;
    info->n_views = nv;
    info->tile_h = m->th;
    info->batch = m->ad_ss.batch_size;
    info->rounds = m->ad_rounds;
    info->max_rounds = m->ad_R;
    info->finished = m->adapt_finished() ? 1u : 0u;
    info->active_pixels = m->ad_active;
    info->samples_total = m->ad_samples_total;
    info->samples_max = m->ad_samples_max;
    info->counters = m->ad_counters;
    if (view_active_out) {  // (not hot: the state words cross to the host)
        const size_t vpx = (size_t)info->width * (size_t)info->height;
        if (m->ad_rounds == 0) {
            for (uint32_t v = 0; v < nv; v++) view_active_out[v] = vpx;
            return GS_OK;
        }
        std::vector<uint32_t> state(vpx * nv);
        const gs_status s = m->adapt_download(nullptr, state.data());
        if (s != GS_OK) return s;
        for (uint32_t v = 0; v < nv; v++) {
            uint64_t act = 0;
            for (size_t k = 0; k < vpx; k++) act += (state[v * vpx + k] & GS_ADAPT_STOPPED) ? 0u : 1u;
            view_active_out[v] = act;
        }
    }
    return GS_OK;
}

gs_status gs_multi_views_adapt_maps(gs_multi* m, uint32_t* samples, float* rel_error) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->vd_open) return fail(GS_ERR_ARG, "no views adaptation is open");
    return m->adapt_maps(samples, rel_error);
}

gs_status gs_multi_views_adapt_download(gs_multi* m, double* sums, uint32_t* state) {
    if (!m || !sums || !state) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->vd_open) return fail(GS_ERR_ARG, "no views adaptation is open");
    return m->adapt_download(sums, state);
}

gs_status gs_multi_views_adapt_upload(gs_multi* m, const gs_view* views, uint32_t n_views, const gs_sample_settings* ss,
                                      uint32_t rounds_done, const double* sums, const uint32_t* state,
                                      const gs_counters* counters) {
    if (!m || !sums || !state || !counters) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    gs_camera tall;
    gs_status s = views_adapt_check(m, views, n_views, ss, &tall);
    if (s == GS_OK) s = m->adapt_begin(&tall, ss, 0, views, n_views);
    if (s != GS_OK) return s;
    return m->adapt_fill(rounds_done, sums, state, counters);
}

gs_status gs_multi_views_adapt_end(gs_multi* m) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->vd_open) return fail(GS_ERR_ARG, "no views adaptation is open");
    m->adapt_end();
    return GS_OK;
}

gs_status gs_multi_accum_begin(gs_multi* m, const gs_camera* cam, uint64_t seed, uint32_t chunk) {
    if (!m || !cam) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return m->accum_begin(cam, seed, chunk);
}

gs_status gs_multi_accum_pass(gs_multi* m, uint32_t samples, const gs_multi_outputs* out, gs_stats* stats) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->acc_open) return fail(GS_ERR_ARG, "no accumulation is open: gs_multi_accum_begin first");
    const uint32_t c = m->acc_chunk;
    if (samples == 0 || samples % c != 0 || samples / c > 64u)
        return fail(GS_ERR_ARG, "a pass is 1 to 64 whole chunks of samples");
    if (m->acc_samples + samples > 0xFFFFFFFFull) return fail(GS_ERR_ARG, "the frame's samples overflow 32 bits");
    const gs_sample_settings ss{0.0, 0.0, samples, 0};
    return m->render(&m->acc_cam, &ss, m->acc_seed, out, stats, samples);
}

gs_status gs_multi_accum_info(const gs_multi* m, gs_accum_info* info) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->acc_open) return fail(GS_ERR_ARG, "no accumulation is open");
    std::memset(info, 0, sizeof(*info));
    info->width = m->acc_cam.image_width;
    info->height = m->acc_cam.image_height;
    info->chunk = m->acc_chunk;
    info->passes = m->acc_passes;
    info->seed = m->acc_seed;
    info->samples = m->acc_samples;
    info->last_delta = m->acc_last_delta;
    info->counters = m->acc_counters;
    return GS_OK;
}

gs_status gs_multi_accum_download(gs_multi* m, double* sums) {
    if (!m || !sums) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->acc_open) return fail(GS_ERR_ARG, "no accumulation is open");
    return m->permute_sums(sums, true);
}

gs_status gs_multi_accum_upload(gs_multi* m, const gs_camera* cam, uint64_t seed, uint32_t chunk, uint64_t samples,
                                const double* sums, const gs_counters* counters) {
    if (!m || !cam || !sums || !counters) return fail(GS_ERR_ARG, "null argument");
    const uint32_t c = chunk ? chunk : 16u;
    if (samples % c != 0 || samples > 0xFFFFFFFFull)
        return fail(GS_ERR_ARG, "a checkpoint's samples are whole chunks, below 2^32");
    std::lock_guard<std::mutex> lock(m->mu);
    gs_status s = m->accum_begin(cam, seed, chunk);
    if (s != GS_OK) return s;
    s = m->permute_sums(const_cast<double*>(sums), false);
    if (s != GS_OK) {
        m->accum_end();
        return s;
    }
    m->acc_samples = samples;
    m->acc_counters = *counters;
    return GS_OK;
}

gs_status gs_multi_accum_end(gs_multi* m) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->acc_open) return fail(GS_ERR_ARG, "no accumulation is open");
    m->accum_end();
    return GS_OK;
}

const char* gs_rccl_library(void) {
    const Rccl& r = rccl();
    return r.ok ? r.path.c_str() : nullptr;
}

gs_status gs_multi_create(const gs_flat_scene* scene, const gs_launch* launch, gs_multi** out) {
    if (!scene || !launch || !out) return fail(GS_ERR_ARG, "null argument");
    *out = nullptr;
    if (launch->num_gpus <= 0 && launch->devices)
        return fail(GS_ERR_ARG, "num_gpus <= 0 (every visible device) with a device list");
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible == 0) return fail(GS_ERR_NO_DEVICE, "no HIP device visible");
    const int n = launch->num_gpus > 0 ? launch->num_gpus : visible;
    if (n > visible && !(g_same_device && launch->devices))  // (the test hook's lists may repeat a device)
        return fail(GS_ERR_ARG, "num_gpus " + std::to_string(n) + " > visible devices " + std::to_string(visible));
    std::vector<int> ids(n);
    for (int i = 0; i < n; i++) {
        ids[i] = launch->devices ? launch->devices[i] : i;
        if (ids[i] < 0 || ids[i] >= visible) return fail(GS_ERR_ARG, "bad device id");
        for (int j = 0; j < i && !g_same_device; j++)
            if (ids[j] == ids[i]) return fail(GS_ERR_ARG, "device listed twice (one communicator rank per device)");
    }
    if (launch->tile_w < 0 || launch->tile_h < 0) return fail(GS_ERR_ARG, "negative tile size");
    const bool copy_gather = g_same_device && n > 1;
    const bool collective = !copy_gather && (n > 1 || g_collective_always);
    if (collective && !rccl().ok) return fail(GS_ERR_UNSUPPORTED, "RCCL unavailable: " + rccl().error);
    DeviceGuard guard;
    auto m = new gs_multi();
    m->ids = ids;
    m->tw = launch->tile_w > 0 ? launch->tile_w : 64;
    m->th = launch->tile_h > 0 ? launch->tile_h : m->tw;
    m->plan = launch->plan != 0;
    m->dev.resize(n);
    m->copy_gather = copy_gather;
    auto bail = [&](gs_status st) {
        delete m;
        return st;
    };
    for (int i = 0; i < n; i++) {
        Device& d = m->dev[i];
        d.id = ids[i];
        if (hipSetDevice(d.id) != hipSuccess) return bail(fail(GS_ERR_HIP, "hipSetDevice failed"));
        const gs_status s = gs_device_scene_create(scene, &d.scene);
        if (s != GS_OK) return bail(s);
        if (hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess)
            return bail(fail(GS_ERR_HIP, "hipStreamCreateWithFlags failed"));
        for (auto& e : d.ev)
            if (hipEventCreate(&e) != hipSuccess) return bail(fail(GS_ERR_HIP, "hipEventCreate failed"));
        if (hipHostMalloc((void**)&d.h_cnt, sizeof(gs_counters), hipHostMallocDefault) != hipSuccess)
            return bail(fail(GS_ERR_OOM, "hipHostMalloc of the counters failed"));
    }
    if (collective) {  // one communicator rank per device, rank i = device i of the list
        m->comms.assign(n, nullptr);
        const ncclResult_t rc = rccl().comm_init_all(m->comms.data(), n, ids.data());
        if (rc != ncclSuccess) {
            m->comms.clear();
            return bail(fail(GS_ERR_HIP, std::string("ncclCommInitAll: ") + rccl().error_string(rc)));
        }
    }
    *out = m;
    return GS_OK;
}

gs_status gs_multi_render(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                          const gs_multi_outputs* out, gs_stats* stats) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    return m->render(cam, ss, seed, out, stats);
}

gs_status gs_multi_render_views(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t samples, uint32_t chunk,
                                const gs_multi_outputs* out, gs_stats* stats) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (out && out->ppm_text) return fail(GS_ERR_ARG, "a views call writes no PPM text");
    const uint32_t c = chunk ? chunk : 16u;
    gs_camera tall;
    gs_status s = gs_views_check(m->dev[0].scene, views, n_views, samples, c, &tall);
    if (s != GS_OK) return s;
    // (rank 0 holds the most tiles of the round-robin cut: its share bounds every rank's)
    const gs_partition p0{0, (int32_t)m->dev.size(), m->tw, m->th, nullptr, 0, 0};
    s = gs_views_check_cap(gs_partition_capacity(&tall, &p0), samples, c);
    if (s != GS_OK) return s;
    const gs_sample_settings ss{0.0, 0.0, samples, 0};
    const gs_multi::ViewsCall vw{views, n_views, c};
    return m->render(&tall, &ss, 0, out, stats, 0, false, 0, &vw);
}

// ---- progressive views
gs_status gs_multi_views_accum_begin(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t chunk) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    const uint32_t c = chunk ? chunk : 16u;
    gs_camera tall;
    gs_status s = gs_views_check(m->dev[0].scene, views, n_views, c, c, &tall);  // (one chunk: the views' own rules)
    if (s != GS_OK) return s;
    return m->views_accum_begin(views, n_views, chunk);
}

gs_status gs_multi_views_accum_pass(gs_multi* m, uint32_t samples, const uint8_t* selected, const gs_multi_outputs* out,
                                    gs_stats* stats) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->va_open) return fail(GS_ERR_ARG, "no views accumulation is open: gs_multi_views_accum_begin first");
    if (out && out->ppm_text) return fail(GS_ERR_ARG, "a views pass writes no PPM text");
    const uint32_t c = m->va_chunk, nv = (uint32_t)m->va_views.size();
    if (samples == 0 || samples % c != 0 || samples / c > 64u)
        return fail(GS_ERR_ARG, "a pass is 1 to 64 whole chunks of samples");
    uint32_t base = 0;
    gs_status s = gs_views_pass_check(nv, m->va_samples.data(), selected, samples, c, &base);
    if (s != GS_OK) return s;
    // (rank 0 holds the most tiles of the round-robin cut: its share bounds every rank's)
    const gs_partition p0{0, (int32_t)m->dev.size(), m->tw, m->th, nullptr, 0, 0};
    s = gs_views_check_cap(gs_partition_capacity(&m->va_tall, &p0), samples, c);
    if (s != GS_OK) return s;
    const gs_sample_settings ss{0.0, 0.0, samples, 0};
    const gs_multi::ViewsCall vw{m->va_views.data(), nv, c};
    const gs_multi::ViewsPass vp{selected, base};
    return m->render(&m->va_tall, &ss, 0, out, stats, 0, false, 0, &vw, &vp);
}

gs_status gs_multi_views_accum_info(const gs_multi* m, gs_views_accum_info* info, uint32_t* view_samples_out,
                                    double* delta_out) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->va_open) return fail(GS_ERR_ARG, "no views accumulation is open");
    std::memset(info, 0, sizeof(*info));
    info->width = m->va_views[0].cam.image_width;
    info->height = m->va_views[0].cam.image_height;
    info->n_views = (uint32_t)m->va_views.size();
    info->chunk = m->va_chunk;
    info->passes = m->va_passes;
    info->tile_h = m->th;
    info->counters = m->va_counters;
    if (view_samples_out) std::memcpy(view_samples_out, m->va_samples.data(), m->va_samples.size() * sizeof(uint32_t));
    if (delta_out) std::memcpy(delta_out, m->va_delta.data(), m->va_delta.size() * sizeof(double));
    return GS_OK;
}

gs_status gs_multi_views_accum_download(gs_multi* m, double* sums) {
    if (!m || !sums) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->va_open) return fail(GS_ERR_ARG, "no views accumulation is open");
    return m->permute_sums(sums, true);
}

gs_status gs_multi_views_accum_upload(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t chunk,
                                      const uint32_t* view_samples, const double* sums, const gs_counters* counters) {
    if (!m || !view_samples || !sums || !counters) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    const uint32_t c = chunk ? chunk : 16u;
    gs_camera tall;
    gs_status s = gs_views_check(m->dev[0].scene, views, n_views, c, c, &tall);
    if (s != GS_OK) return s;
    for (uint32_t v = 0; v < n_views; v++)
        if (view_samples[v] % c != 0)
            return fail(GS_ERR_ARG, "a checkpoint's samples are whole chunks (view " + std::to_string(v) + ")");
    s = m->views_accum_begin(views, n_views, chunk);
    if (s != GS_OK) return s;
    s = m->permute_sums(const_cast<double*>(sums), false);
    if (s != GS_OK) {
        m->views_accum_end();
        return s;
    }
    m->va_samples.assign(view_samples, view_samples + n_views);
    m->va_counters = *counters;
    return GS_OK;
}

gs_status gs_multi_views_accum_end(gs_multi* m) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->va_open) return fail(GS_ERR_ARG, "no views accumulation is open");
    m->views_accum_end();
    return GS_OK;
}

gs_status gs_multi_frame(const gs_multi* m, const float** d_rgb, const uint8_t** d_rgb8, int32_t* device) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);  // (a frame being rendered replaces these)
    if (d_rgb) *d_rgb = m->have_rgb ? (const float*)m->frame.p : nullptr;
    if (d_rgb8) *d_rgb8 = m->have_rgb8 ? (const uint8_t*)m->frame8.p : nullptr;
    if (device) *device = m->dev[0].id;
    return GS_OK;
}

gs_status gs_multi_devices(const gs_multi* m, int32_t* num_gpus, int32_t* devices, int32_t capacity) {
    if (!m || !num_gpus) return fail(GS_ERR_ARG, "null argument");
    *num_gpus = (int32_t)m->ids.size();
    if (devices)
        for (int32_t i = 0; i < *num_gpus && i < capacity; i++) devices[i] = m->ids[i];
    return GS_OK;
}

gs_status gs_multi_scene(const gs_multi* m, int32_t rank, const gs_device_scene** scene) {
    if (!m || !scene) return fail(GS_ERR_ARG, "null argument");
    if (rank < 0 || rank >= (int32_t)m->dev.size()) return fail(GS_ERR_ARG, "rank out of range");
    *scene = m->dev[rank].scene;
    return GS_OK;
}

gs_status gs_debug_set_multi_collective(int32_t always) {
    g_collective_always = always ? 1 : 0;
    return GS_OK;
}

gs_status gs_debug_set_multi_same_device(int32_t on) {
    if (on != 0 && on != 1) return fail(GS_ERR_ARG, "same-device mode is 0 or 1");
    g_same_device = on;
    return GS_OK;
}

gs_status gs_multi_destroy(gs_multi* m) {
    delete m;
    return GS_OK;
}

gs_status gs_render_multi(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                          const gs_launch* launch, const gs_multi_outputs* out, gs_stats* stats) {
    if (!scene || !cam || !ss || !launch || !out) return fail(GS_ERR_ARG, "null argument");
    const auto t0 = std::chrono::steady_clock::now();
    gs_multi* m = nullptr;
    gs_status s = gs_multi_create(scene, launch, &m);
    if (s != GS_OK) return s;
    const auto t1 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lock(m->mu);
        s = m->render(cam, ss, seed, out, stats);
    }
    gs_multi_destroy(m);
    if (s == GS_OK && stats) {
        stats->setup_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return s;
}

// The one-device, one-frame calls: a context on the current device, no collective.
static gs_status render_here(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss,
                             uint64_t seed, const gs_multi_outputs* out, gs_stats* stats) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(GS_ERR_NO_DEVICE, "no HIP device visible");
    const int32_t ids[1] = {dev};
    gs_launch l{1, 64, 64, 0, ids};
    return gs_render_multi(scene, cam, ss, seed, &l, out, stats);
}

gs_status gs_render(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                    float* out_rgb, gs_stats* stats) {
    if (!scene || !cam || !ss || !out_rgb) return fail(GS_ERR_ARG, "null argument");
    gs_multi_outputs o{out_rgb, nullptr, nullptr, 0, nullptr};
    return render_here(scene, cam, ss, seed, &o, stats);
}

gs_status gs_render_ppm(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                        char* out_text, int64_t text_capacity, int64_t* out_len, gs_stats* stats) {
    if (!scene || !cam || !ss || !out_text || !out_len) return fail(GS_ERR_ARG, "null argument");
    const int64_t need = gs_ppm_max_bytes(cam->image_width, cam->image_height);
    if (need < 0) return fail(GS_ERR_ARG, "bad image size");
    if (text_capacity < need) return fail(GS_ERR_ARG, "text capacity below gs_ppm_max_bytes");
    gs_multi_outputs o{nullptr, nullptr, out_text, text_capacity, out_len};
    return render_here(scene, cam, ss, seed, &o, stats);
}

}  // extern "C"
