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
//
// Layout: a context holds at most one open session (Session), whose record (AccumState,
// ViewsAccumState, AdaptState) and per-device buffers (AccumBufs, AdaptBufs) live from its begin to
// close_session; gs_multi::admit alone decides which call may run under which session.
// gs_multi::render draws a Frame (a one-shot frame or a pass of the open session) in stages, one
// function each; the sessions differ in three spots (launch_rank, read_back_session, note_pass).
// The tile partition is cached by camera, kind and tile height: a views session cuts at its own.
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
        release();
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

// One device's buffers of an open accumulation, plain or of views: the rank's running sums (cap * 3
// f64, packed order) and the last pass's change partials, with their pinned host copy.
struct AccumBufs {
    DBuf sums, delta;
    double* h_delta = nullptr;
    void release() {
        for (DBuf* b : {&sums, &delta}) b->release();
        if (h_delta) (void)hipHostFree(h_delta);
        h_delta = nullptr;
    }
};

// One device's buffers of an open adaptation, plain or of views: the rank's round state (launch.cpp's
// blob), the two maps in packed order (cap u32, cap f32), the pinned copy of the blob's summary
// words, and the rank's paths so far in the adaptation's device counters.  The summary's 24 pinned
// bytes stay from the first adaptation to the context's end (pinning them anew costs every adaptation).
struct AdaptBufs {
    DBuf rstate, map_samples, map_error;
    unsigned long long* h_summary = nullptr;
    uint64_t paths = 0;
    void release(bool context_ends = false) {
        for (DBuf* b : {&rstate, &map_samples, &map_error}) b->release();
        if (h_summary && context_ends) (void)hipHostFree(h_summary), h_summary = nullptr;
        paths = 0;
    }
};

struct Device {
    int id = 0;
    gs_device_scene* scene = nullptr;
    hipStream_t stream = nullptr;
    // render start / end, megakernel start / end, gather + unpack start / end
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    DBuf order, packed, packed8, cnt;
    AccumBufs acc;  // (only one of the two is in use: the open session's)
    AdaptBufs ad;
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

// At most one session is open on a context (gs_multi_*_begin .. _end): its camera(s), seed(s) and
// settings are fixed, and so is the tile partition computed at its begin, in whose packed order
// the ranks' session buffers are.  What a call needs of it (gs_multi::admit): Begin opens session
// s, so none may be open; Frame renders a frame of s (None: a one-shot frame), Pass and Other are
// s's own calls, so s must be the open one.
enum class Session { None, Accum, ViewsAccum, Adapt, ViewsAdapt };
enum class Call { Begin, Frame, Pass, Other };

// An open accumulation: `samples` samples of every pixel are in the ranks' sums.
struct AccumState {
    gs_camera cam{};
    uint64_t seed = 0, samples = 0;
    uint32_t chunk = 0, passes = 0;
    double last_delta = 0.0;
    gs_counters counters{};
};

// An open views accumulation: the tall frame is cut round-robin into tw x th tiles (gs_views_tile_h: no
// tile straddles two views), view v's sums hold samples[v] samples, the change partials are one a tile slot.
struct ViewsAccumState {
    std::vector<gs_view> views;
    gs_camera tall{};
    int32_t th = 0;
    uint32_t chunk = 0, passes = 0;
    std::vector<uint32_t> samples;
    std::vector<double> delta;
    gs_counters counters{};
};

// An open adaptation: `rounds` rounds are in the ranks' state.  With `views` a views adaptation: cam
// is then the tall frame's, cut round-robin into tw x th tiles like a views accumulation.
struct AdaptState {
    gs_camera cam{};
    gs_sample_settings ss{};
    int32_t th = 0;
    uint64_t seed = 0, active = 0, samples_total = 0, samples_max = 0;
    uint32_t rounds = 0, R = 0;
    // The ranks' device counters run on from pass to pass (gs_round_params_kernel sizes a round's
    // items by the rays per path so far, as in a one-shot launch): zeroed by the first pass after
    // _begin / _upload (fresh), their sum so far in `dev`, and counters = base (an upload's) + dev.
    bool fresh = true;
    gs_counters counters{}, base{}, dev{};
    std::vector<gs_view> views;
    bool finished() const { return rounds > 0 && (active == 0 || rounds >= R); }
};

// What one render() draws: a one-shot frame (session None) or a pass of the open session.  (Any frame
// has the first five, given in this order; the rest are set by name.)
struct Frame {
    Session session = Session::None;
    const gs_camera* cam = nullptr;  // (a views frame: the tall frame's camera)
    const gs_sample_settings* ss = nullptr;  // (an accumulation's pass: batch_size is its samples)
    uint64_t seed = 0;               // (a views frame: unused, the views have their own)
    int32_t th = 0;                  // the tile height of its partition
    const gs_view* views = nullptr;  // a views frame: cut round-robin whatever `plan` says
    uint32_t n_views = 0, chunk = 0, rounds = 0;  // (rounds: an adaptation's pass; 0 resolves the state as it stands)
    const uint8_t* selected = nullptr;  // a views accumulation's pass: over these views (NULL: all),
    uint32_t base = 0;                  // which all hold `base` samples
};

// One render() in flight: what its stages hand on.
struct Shot {
    const Frame& f;
    const gs_multi_outputs* out;
    bool want_rgb, want8, direct, timed_tail;
    int64_t W, H;
    const void *src = nullptr, *src8 = nullptr;  // what the unpack reads: packed or gathered tiles
    gs_stats st{};  // (its counters: the ranks' sum, made the pass's own by note_pass)
};

}  // namespace

struct gs_multi {
    std::vector<Device> dev;
    std::vector<int> ids;
    std::vector<ncclComm_t> comms;  // one rank per device (N > 1, or forced by the test hook)
    // gs_debug_set_multi_same_device: N ranks on one device list that may repeat a device, the
    // gather done by device copies on the ranks' streams instead of RCCL (N > 1, no comms)
    bool copy_gather = false;
    bool comms_broken = false;      // a collective failed: the communicators were aborted
    int32_t tw = 64, th = 64;       // (th: a views session cuts its frame at its own)
    bool plan = false;
    mutable std::mutex mu;  // one frame at a time; guards every field below and comms_broken
    // tile partition of the last frame (plan or round-robin), kept while camera, kind and tile height are
    bool part_ready = false, part_rr = false;  // (part_rr: cut round-robin for a views frame)
    gs_camera part_cam{};
    int32_t part_th = 0;
    std::vector<int32_t> order;  // empty: round-robin
    int32_t slots = 0;
    int64_t cap = 0;  // packed pixels per rank
    // the first device's gather and frame buffers
    DBuf gathered, gathered8, frame, frame8, text, scratch, len;
    bool have_rgb = false, have_rgb8 = false;
    int32_t frame_w = 0, frame_h = 0;
    // the open session and its record (the other records are empty)
    Session open = Session::None;
    AccumState acc;
    ViewsAccumState va;
    AdaptState ad;

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
            for (DBuf* b : {&d.order, &d.packed, &d.packed8, &d.cnt}) b->release();
            d.acc.release();
            d.ad.release(true);
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

    gs_status admit(Call call, Session s) const;
    // Ends the open session or undoes a failed begin: waits, frees its buffers, empties the records.
    void close_session();
    // round_robin: no cost plan whatever `plan` says (a views frame); plan_ms (nullable): a new cut's cost
    gs_status partition(const gs_camera* cam, uint64_t seed, double* plan_ms, bool round_robin, int32_t tile_h);
    // A frame, and its stages in their order (prepare: partition, placement pilots, buffers; gather: RCCL,
    // device copies or none; unpack: PPM text and the queued read-backs too; wait: then counters and outputs).
    gs_status render(const Frame& f, const gs_multi_outputs* out, gs_stats* stats);
    gs_status check_frame(const Frame& f, const gs_multi_outputs* out) const;
    gs_status prepare(Shot& c);
    gs_status launch(Shot& c);
    gs_status gather(Shot& c);
    gs_status unpack(Shot& c);
    gs_status wait(Shot& c);
    // ... and the three spots where the sessions differ:
    gs_status launch_rank(const Frame& f, Device& d, const gs_partition& p, const gs_render_outputs& o, bool direct);
    gs_status read_back_session(const Frame& f, Device& d);
    void note_pass(Shot& c);

    gs_status views_form_check() const {  // (a views session's scene)
        gs_scene_info si{};
        const gs_status s = gs_device_scene_info(dev[0].scene, &si);
        if (s != GS_OK || !(si.feat & 512)) return s;
        return fail(GS_ERR_UNSUPPORTED, "the scene needs the catch-all kernel, which has no views form");
    }
    gs_status accum_begin(const gs_camera* cam, uint64_t seed, uint32_t chunk);
    gs_status accum_alloc();
    // (views: checked by the caller, gs_views_check, which gives the tall frame's camera: `tall`, or `cam`)
    gs_status views_accum_begin(const gs_camera& tall, const gs_view* views, uint32_t n_views, uint32_t chunk);
    gs_status adapt_begin(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                          const gs_view* views = nullptr, uint32_t n_views = 0);
    gs_status adapt_alloc(const GsRoundLayout& l);
    // What gs_multi_adapt_* and gs_multi_views_adapt_* share, on the open adaptation's frame (the tall one
    // for views): a pass, the maps, the state down (sums may be NULL) and, behind adapt_begin, the state up.
    gs_status adapt_pass(uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats);
    gs_status adapt_maps(uint32_t* samples, float* rel_error);
    gs_status adapt_download(double* sums, uint32_t* state);
    gs_status adapt_fill(uint32_t rounds_done, const double* sums, const uint32_t* state, const gs_counters* counters);

    // The packed pixels of rank `rank` as its launches see them (gs_partition_capacity): `cap` under
    // a plan, fewer for the later ranks of a round-robin partition -- the size the rank's round
    // state is laid out for, and tw * part_th times the tile slots it holds.
    int64_t rank_cap(int rank, const gs_camera& cam) const {
        const gs_partition p = part(rank);
        return order.empty() ? std::max<int64_t>(0, gs_partition_capacity(&cam, &p)) : cap;
    }
    gs_partition part(int rank) const {  // rank's share of the cached partition, as its launches take it
        return {rank, (int32_t)dev.size(), tw, part_th, order.empty() ? nullptr : (const int32_t*)dev[rank].order.p, slots, 0};
    }
    // Rank `rank`'s packed array of `elem`-byte records <-> the [H][W] image of them (to_image or
    // back; going back, slots outside the image keep what `packed` holds).
    void permute_rank(int rank, const gs_camera& cam, uint8_t* image, uint8_t* packed, size_t elem, bool to_image) const;
    // An accumulation's sums: the ranks' packed buffers <-> the [H][W][3] image of frame `cam`.
    gs_status permute_sums(const gs_camera& cam, double* image, bool to_image);
};

// The one place that decides whether a call may proceed under the open session, and refuses it.
gs_status gs_multi::admit(Call call, Session s) const {
    if (call != Call::Begin && open == s) return GS_OK;
    if (call == Call::Pass || call == Call::Other) {
        static const char* const what[] = {"", "accumulation", "views accumulation", "adaptation", "views adaptation"};
        static const char* const begin[] = {"", "gs_multi_accum_begin", "gs_multi_views_accum_begin",
                                            "gs_multi_adapt_begin", "gs_multi_views_adapt_begin"};
        std::string msg = std::string("no ") + what[(int)s] + " is open";
        if (call == Call::Pass) msg += std::string(": ") + begin[(int)s] + " first";
        return fail(GS_ERR_ARG, msg);
    }
    // A begin or a one-shot frame: nothing may be open (a new partition would invalidate what the session
    // holds in packed order: the sums, the round state, the views' sums at their own tile height).
    static const char* const refusal[] = {"", "an accumulation is open: gs_multi_accum_end first",
                                          "a views accumulation is open: gs_multi_views_accum_end first",
                                          "an adaptation is open: gs_multi_adapt_end first",
                                          "a views adaptation is open: gs_multi_views_adapt_end first"};
    if (open == Session::None) return GS_OK;
    std::string msg = refusal[(int)open];
    // (opened twice: "already"; a views adaptation begins as an adaptation: over one it is told
    // "already" too, and over itself the plain refusal)
    const bool twice = open == s || (open == Session::Adapt && s == Session::ViewsAdapt);
    if (call == Call::Begin && twice && open != Session::ViewsAdapt) msg.insert(msg.find("open"), "already ");
    return fail(GS_ERR_ARG, msg);
}

void gs_multi::close_session() {
    DeviceGuard guard;
    for (auto& d : dev) {
        (void)hipSetDevice(d.id);
        if (d.stream && !comms_broken) (void)hipStreamSynchronize(d.stream);
        d.acc.release();
        d.ad.release();
    }
    acc = AccumState{};
    va = ViewsAccumState{};
    ad = AdaptState{};
    open = Session::None;
}

gs_status gs_multi::partition(const gs_camera* cam, uint64_t seed, double* plan_ms, bool round_robin, int32_t tile_h) {
    if (part_ready && part_rr == round_robin && part_th == tile_h && std::memcmp(&part_cam, cam, sizeof(gs_camera)) == 0)
        return GS_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int n = (int)dev.size();
    part_ready = false;
    order.clear();
    slots = 0;
    if (plan && n > 1 && !round_robin) {
        HIPOK(hipSetDevice(dev[0].id));
        gs_status s = gs_plan_tiles(dev[0].scene, cam, seed, n, tw, tile_h, nullptr, 0, &slots);
        if (s != GS_OK) return s;
        order.resize((size_t)slots * n);
        s = gs_plan_tiles(dev[0].scene, cam, seed, n, tw, tile_h, order.data(), (int64_t)order.size(), &slots);
        if (s != GS_OK) return s;
        for (auto& d : dev) {
            HIPOK(hipSetDevice(d.id));
            GROW(d.order, order.size() * sizeof(int32_t));
            HIPOK(hipMemcpy(d.order.p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        cap = (int64_t)slots * tw * tile_h;
    } else {
        gs_partition p0{0, n, tw, tile_h, nullptr, 0, 0};
        cap = gs_partition_capacity(cam, &p0);  // rank 0 holds the most tiles
        if (cap < 0) return fail(GS_ERR_ARG, "bad partition");
    }
    part_cam = *cam;
    part_rr = round_robin;
    part_th = tile_h;
    part_ready = true;
    if (plan_ms) *plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GS_OK;
}

// ---------------------------------------------------------------- a frame, stage by stage
gs_status gs_multi::render(const Frame& f, const gs_multi_outputs* out, gs_stats* stats) {
    gs_status s = check_frame(f, out);
    if (s != GS_OK) return s;
    DeviceGuard guard;
    const auto t0 = std::chrono::steady_clock::now();
    const int n = (int)dev.size();
    Shot c{f, out};
    c.st.render_ms_min = c.st.kernel_ms_min = 1e300;
    c.want_rgb = !out || out->rgb;
    c.want8 = out && (out->rgb8 || out->ppm_text);
    c.W = f.cam->image_width, c.H = f.cam->image_height;
    // One device and no collective: the render writes the frame itself (no packed tiles,
    // no unpack: C1 saved the unpack kernel and a stream gap, ~20 us of a 0.9 ms frame).
    c.direct = n == 1 && comms.empty();
    // (direct without PPM text: nothing after the render to time, one stream marker fewer)
    c.timed_tail = !c.direct || (out && out->ppm_text);
    if ((s = prepare(c)) != GS_OK || (s = launch(c)) != GS_OK || (s = gather(c)) != GS_OK ||
        (s = unpack(c)) != GS_OK || (s = wait(c)) != GS_OK)
        return s;
    note_pass(c);
    c.st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c.st.algorithmic_bytes = algorithmic_bytes(c.st.counters);
    c.st.gathered_bytes = comms.empty() && !copy_gather
                              ? 0
                              : (uint64_t)n * (uint64_t)cap * ((c.want_rgb ? 12u : 0u) + (c.want8 ? 3u : 0u));
    c.st.num_gpus = n;
    if (stats) *stats = c.st;
    return GS_OK;
}

gs_status gs_multi::check_frame(const Frame& f, const gs_multi_outputs* out) const {
    const gs_camera* cam = f.cam;
    if (!cam || !f.ss) return fail(GS_ERR_ARG, "null argument");
    if (out && !out->rgb && !out->rgb8 && !out->ppm_text) return fail(GS_ERR_ARG, "no output requested");
    if (out && out->ppm_text && !out->ppm_len) return fail(GS_ERR_ARG, "ppm_text without ppm_len");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    if (out && out->ppm_text && out->ppm_capacity < gs_ppm_max_bytes(cam->image_width, cam->image_height))
        return fail(GS_ERR_ARG, "ppm_capacity below gs_ppm_max_bytes");
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    return admit(Call::Frame, f.session);
}

gs_status gs_multi::prepare(Shot& c) {
    const Frame& f = c.f;
    const int n = (int)dev.size();
    gs_status s = partition(f.cam, f.seed, &c.st.setup_ms, f.views != nullptr, f.th);
    if (s != GS_OK) return s;
    // The scenes' placement pilots (first frame, launch.cpp, run before the first launch):
    // launched on every device before any is waited for, outside the timed render.
    std::vector<gs_device_scene*> sc(n);
    std::vector<void*> st(n);
    for (int i = 0; i < n; i++) sc[i] = dev[i].scene, st[i] = dev[i].stream;
    const auto tp = std::chrono::steady_clock::now();
    int ran = 0;
    // (a views frame: view 0's own camera and frame)
    s = gs_placement_prepare(sc.data(), ids.data(), st.data(), n, f.views ? &f.views[0].cam : f.cam, f.ss, &ran);
    if (s != GS_OK) return s;
    if (ran) c.st.setup_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
    // the first device's frame and every rank's packed tiles and counters
    have_rgb = have_rgb8 = false;
    HIPOK(hipSetDevice(dev[0].id));
    if (c.want_rgb) GROW(frame, c.W * c.H * 12);
    if (c.want8) GROW(frame8, c.W * c.H * 3);
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        if (c.want_rgb && !c.direct) GROW(d.packed, cap * 12);
        if (c.want8 && !c.direct) GROW(d.packed8, cap * 3);
        GROW(d.cnt, sizeof(gs_counters));  // (zeroed by the launch's parameter kernel)
    }
    return GS_OK;
}

// Render: every device its own tiles, concurrently (launches are asynchronous).
gs_status gs_multi::launch(Shot& c) {
    const int n = (int)dev.size();
    for (int i = 0; i < n; i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        const gs_partition p = part(i);
        const gs_render_outputs o{c.want_rgb ? (float*)(c.direct ? frame.p : d.packed.p) : nullptr,
                                  c.want8 ? (uint8_t*)(c.direct ? frame8.p : d.packed8.p) : nullptr, nullptr};
        HIPOK(hipEventRecord(d.ev[0], d.stream));
        const gs_status s = launch_rank(c.f, d, p, o, c.direct);
        if (s != GS_OK) return s;
        HIPOK(hipEventRecord(d.ev[1], d.stream));
    }
    return GS_OK;
}

gs_status gs_multi::gather(Shot& c) {
    const int n = (int)dev.size();
    const bool want_rgb = c.want_rgb, want8 = c.want8;
    Device& d0 = dev[0];
    HIPOK(hipSetDevice(d0.id));
    c.src = want_rgb ? d0.packed.p : nullptr;
    c.src8 = want8 ? d0.packed8.p : nullptr;
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
        c.src = gathered.p;
        c.src8 = gathered8.p;
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
        c.src = gathered.p;
        c.src8 = gathered8.p;
    }  // (no collective: the unpack is timed from the render's end event, ev[1])
    return GS_OK;
}

// (on the first device, which the gather leaves current)
gs_status gs_multi::unpack(Shot& c) {
    const gs_camera* cam = c.f.cam;
    Device& d0 = dev[0];
    const gs_partition pu = part(0);
    gs_status s = GS_OK;
    if (c.want_rgb && !c.direct) s = gs_unpack_tiles_part_async(cam, &pu, cap, c.src, frame.p, 12, d0.stream);
    if (s != GS_OK) return s;
    if (c.want8 && !c.direct) s = gs_unpack_tiles_part_async(cam, &pu, cap, c.src8, frame8.p, 3, d0.stream);
    if (s != GS_OK) return s;
    if (c.out && c.out->ppm_text) {
        const int64_t need = gs_ppm_max_bytes(cam->image_width, cam->image_height);
        const int64_t sb = gs_ppm_scratch_bytes(cam->image_width, cam->image_height);
        GROW(text, need);
        GROW(scratch, sb);
        GROW(len, 8);
        s = gs_ppm_encode_async((const uint8_t*)frame8.p, cam->image_width, cam->image_height, (char*)text.p, need,
                                (int64_t*)len.p, scratch.p, sb, d0.stream);
        if (s != GS_OK) return s;
    }
    // ... and behind the frame the read-backs, so that the host's wait is the only synchronisation
    if (c.timed_tail) HIPOK(hipEventRecord(d0.ev[5], d0.stream));
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipMemcpyAsync(d.h_cnt, d.cnt.p, sizeof(gs_counters), hipMemcpyDeviceToHost, d.stream));
        if ((s = read_back_session(c.f, d)) != GS_OK) return s;
    }
    return GS_OK;
}

// Wait, then the counters and the timings.
gs_status gs_multi::wait(Shot& c) {
    // (an adaptation's counters run on from pass to pass)
    const bool running = (c.f.session == Session::Adapt || c.f.session == Session::ViewsAdapt) && !ad.fresh;
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        add_counters(c.st.counters, *d.h_cnt);
        float ms = 0.0f, kms = 0.0f;
        HIPOK(hipEventElapsedTime(&ms, d.ev[0], d.ev[1]));
        HIPOK(hipEventElapsedTime(&kms, d.ev[2], d.ev[3]));
        gs_device_scene_note_frame(d.scene, (double)kms, d.h_cnt->paths - (running ? d.ad.paths : 0u));
        d.ad.paths = d.h_cnt->paths;
        c.st.render_ms_max = std::max(c.st.render_ms_max, (double)ms);
        c.st.render_ms_min = std::min(c.st.render_ms_min, (double)ms);
        c.st.kernel_ms_max = std::max(c.st.kernel_ms_max, (double)kms);
        c.st.kernel_ms_min = std::min(c.st.kernel_ms_min, (double)kms);
    }
    Device& d0 = dev[0];
    HIPOK(hipSetDevice(d0.id));
    float gms = 0.0f;
    if (c.timed_tail) HIPOK(hipEventElapsedTime(&gms, comms.empty() && !copy_gather ? d0.ev[1] : d0.ev[4], d0.ev[5]));
    c.st.gather_ms = gms;
    // the host outputs
    const gs_multi_outputs* out = c.out;
    have_rgb = c.want_rgb;
    have_rgb8 = c.want8;
    frame_w = (int32_t)c.W;
    frame_h = (int32_t)c.H;
    if (out && out->rgb) HIPOK(hipMemcpy(out->rgb, frame.p, (size_t)(c.W * c.H * 12), hipMemcpyDeviceToHost));
    if (out && out->rgb8) HIPOK(hipMemcpy(out->rgb8, frame8.p, (size_t)(c.W * c.H * 3), hipMemcpyDeviceToHost));
    if (out && out->ppm_text) {
        int64_t l = 0;
        HIPOK(hipMemcpy(&l, len.p, 8, hipMemcpyDeviceToHost));
        if (l <= 0 || l > out->ppm_capacity) return fail(GS_ERR_HIP, "PPM encoder returned a bad length");
        HIPOK(hipMemcpy(out->ppm_text, text.p, (size_t)l, hipMemcpyDeviceToHost));
        *out->ppm_len = l;
    }
    return GS_OK;
}

// ---------------------------------------------------------------- where the sessions differ
// One rank's launch, between its render events.
gs_status gs_multi::launch_rank(const Frame& f, Device& d, const gs_partition& p, const gs_render_outputs& o,
                                bool direct) {
    gs_counters* cnt = (gs_counters*)d.cnt.p;
    switch (f.session) {
    case Session::None:
        return f.views ? gs_render_tiles_views_timed_async(d.scene, f.views, f.n_views, f.ss->batch_size, f.chunk, &p, &o,
                                                           cnt, d.stream, d.ev[2], d.ev[3], direct, true)
                       : gs_render_tiles_timed_async(d.scene, f.cam, f.ss, f.seed, &p, &o, cnt, d.stream, d.ev[2],
                                                     d.ev[3], direct, true);
    case Session::Accum:
        HIPOK(hipMemsetAsync(d.acc.delta.p, 0, (size_t)gs_pass_delta_blocks(cap) * 8, d.stream));
        return gs_render_tiles_pass_timed_async(d.scene, f.cam, f.ss->batch_size, f.seed, &p, (uint32_t)acc.samples,
                                                acc.chunk, (double*)d.acc.sums.p, (double*)d.acc.delta.p, &o, cnt,
                                                d.stream, d.ev[2], d.ev[3], direct, true);
    case Session::ViewsAccum:  // (every slot's partial is written by the pass's combine: no memset)
        return gs_render_tiles_views_pass_timed_async(d.scene, f.views, f.n_views, va.samples.data(), f.selected,
                                                      f.ss->batch_size, f.chunk, &p, (double*)d.acc.sums.p, &o,
                                                      (double*)d.acc.delta.p, cnt, d.stream, d.ev[2], d.ev[3], direct,
                                                      true);
    case Session::Adapt:
    case Session::ViewsAdapt: {
        const gs_round_outputs ro{o.rgb, o.rgb8, (uint32_t*)d.ad.map_samples.p, (float*)d.ad.map_error.p};
        return f.views ? gs_render_tiles_views_rounds_timed_async(d.scene, f.views, f.n_views, f.ss, &p, ad.rounds,
                                                                  f.rounds, d.ad.rstate.p, (int64_t)d.ad.rstate.bytes,
                                                                  &ro, cnt, d.stream, d.ev[2], d.ev[3], direct, ad.fresh)
                       : gs_render_tiles_rounds_timed_async(d.scene, f.cam, f.ss, f.seed, &p, ad.rounds, f.rounds,
                                                            d.ad.rstate.p, (int64_t)d.ad.rstate.bytes, &ro, cnt,
                                                            d.stream, d.ev[2], d.ev[3], direct, ad.fresh);
    }
    }
    return GS_OK;
}

// One rank's read-backs behind the frame's counters: what note_pass reads after the wait.
gs_status gs_multi::read_back_session(const Frame& f, Device& d) {
    switch (f.session) {
    case Session::None: break;
    case Session::Accum:
        HIPOK(hipMemcpyAsync(d.acc.h_delta, d.acc.delta.p, (size_t)gs_pass_delta_blocks(cap) * 8,
                             hipMemcpyDeviceToHost, d.stream));
        break;
    case Session::ViewsAccum:
        HIPOK(hipMemcpyAsync(d.acc.h_delta, d.acc.delta.p, (size_t)(cap / ((int64_t)tw * part_th)) * 8,
                             hipMemcpyDeviceToHost, d.stream));
        break;
    case Session::Adapt:
    case Session::ViewsAdapt:  // (the active count the next pass's clip needs: the pass's one read-back)
        HIPOK(hipMemcpyAsync(d.ad.h_summary, (const char*)d.ad.rstate.p + gs_round_layout(0, ad.R).summary,
                             kRoundSummaryWords * 8, hipMemcpyDeviceToHost, d.stream));
        break;
    }
    return GS_OK;
}

// The open session's bookkeeping after a pass (c.st.counters: the ranks' counters, made this pass's own).
void gs_multi::note_pass(Shot& c) {
    const Frame& f = c.f;
    const int n = (int)dev.size();
    switch (f.session) {
    case Session::None: break;
    case Session::Accum: {
        // the pass's change: every rank's per-block partials in index order, the ranks in rank order
        double change = 0.0;
        const int64_t nb = gs_pass_delta_blocks(cap);
        for (int i = 0; i < n; i++)
            for (int64_t b = 0; b < nb; b++) change += dev[i].acc.h_delta[b];
        acc.last_delta = change / ((double)c.W * (double)c.H * 3.0);
        gs_counters add = c.st.counters;
        if (acc.samples != 0) add.pixels = 0;  // (the kernel counts a pixel at chunk 0 of every pass)
        add_counters(acc.counters, add);
        acc.samples += f.ss->batch_size;
        acc.passes += 1;
        break;
    }
    case Session::ViewsAccum: {
        // the selected views' change: a view's per-slot partials rank after rank, each rank's in
        // slot order (round-robin: rank i's slot sl holds tile i + sl n, which lies in one view)
        const int64_t tpx = (int64_t)tw * part_th, vh = va.views[0].cam.image_height, tx = (c.W + tw - 1) / tw;
        const int64_t nt = tx * (c.H / part_th);
        std::vector<double> change(f.n_views, 0.0);
        for (int i = 0; i < n; i++) {
            const int64_t ns = rank_cap(i, *f.cam) / tpx;
            for (int64_t sl = 0; sl < ns; sl++) {
                const int64_t tile = i + sl * n;
                if (tile < nt) change[(size_t)((tile / tx) * part_th / vh)] += dev[i].acc.h_delta[sl];
            }
        }
        for (uint32_t v = 0; v < f.n_views; v++)
            if (!f.selected || f.selected[v]) {
                va.delta[v] = change[v] / ((double)c.W * (double)vh * 3.0);
                va.samples[v] += f.ss->batch_size;
            }
        gs_counters add = c.st.counters;
        // (the kernel counts the selected views' pixels at chunk 0 of every pass; they all start
        // at sample 0 or none does)
        if (f.base != 0) add.pixels = 0;
        add_counters(va.counters, add);
        va.passes += 1;
        break;
    }
    case Session::Adapt:
    case Session::ViewsAdapt: {
        ad.active = ad.samples_total = ad.samples_max = 0;
        for (int i = 0; i < n; i++) {
            ad.active += dev[i].ad.h_summary[0];
            ad.samples_total += dev[i].ad.h_summary[1];
            ad.samples_max = std::max<uint64_t>(ad.samples_max, dev[i].ad.h_summary[2]);
        }
        // this pass alone: the ranks' running counters minus their sum after the last pass
        const gs_counters before = ad.fresh ? gs_counters{} : ad.dev;
        ad.dev = c.st.counters;
        ad.counters = ad.base;
        add_counters(ad.counters, ad.dev);
        const uint64_t* pb = (const uint64_t*)&before;
        uint64_t* pt = (uint64_t*)&c.st.counters;
        for (size_t k = 0; k < sizeof(gs_counters) / sizeof(uint64_t); k++) pt[k] -= pb[k];
        ad.fresh = false;
        ad.rounds += f.rounds;
        break;
    }
    }
}

void gs_multi::permute_rank(int rank, const gs_camera& cam, uint8_t* image, uint8_t* packed, size_t elem,
                            bool to_image) const {
    const int64_t W = cam.image_width, H = cam.image_height, tpx = (int64_t)tw * part_th;
    const int64_t tx = (W + tw - 1) / tw, nt = tx * ((H + part_th - 1) / part_th);
    const int64_t ns = std::min(cap, rank_cap(rank, cam)) / tpx;
    for (int64_t sl = 0; sl < ns; sl++) {
        const int64_t pos = rank + sl * (int64_t)dev.size(), tile = order.empty() ? pos : order[(size_t)pos];
        if (tile < 0 || tile >= nt) continue;
        const int64_t x0 = (tile % tx) * tw, y0 = (tile / tx) * part_th;
        const int64_t nx = std::min<int64_t>(tw, W - x0);
        for (int64_t y = 0; y < part_th && y0 + y < H; y++) {
            uint8_t* img = image + (size_t)((y0 + y) * W + x0) * elem;
            uint8_t* pk = packed + (size_t)(sl * tpx + y * tw) * elem;
            std::memcpy(to_image ? img : pk, to_image ? pk : img, (size_t)nx * elem);
        }
    }
}

// Checkpoints are not hot: each rank's packed sums cross to the host whole and are permuted there.
gs_status gs_multi::permute_sums(const gs_camera& cam, double* image, bool to_image) {
    DeviceGuard guard;
    std::vector<double> packed((size_t)cap * 3);
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        if (to_image)
            HIPOK(hipMemcpy(packed.data(), d.acc.sums.p, packed.size() * 8, hipMemcpyDeviceToHost));
        else
            std::fill(packed.begin(), packed.end(), 0.0);
        permute_rank(i, cam, (uint8_t*)image, (uint8_t*)packed.data(), 24, to_image);
        if (!to_image) HIPOK(hipMemcpy(d.acc.sums.p, packed.data(), packed.size() * 8, hipMemcpyHostToDevice));
    }
    return GS_OK;
}

// ---------------------------------------------------------------- progressive accumulation
gs_status gs_multi::accum_begin(const gs_camera* cam, uint64_t seed, uint32_t chunk) {
    gs_status s = admit(Call::Begin, Session::Accum);
    if (s != GS_OK) return s;
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    DeviceGuard guard;
    if ((s = partition(cam, seed, nullptr, false, th)) != GS_OK) return s;
    if (cap <= 0 || cap >= (int64_t)0xFFFFFFFFll) return fail(GS_ERR_ARG, "bad partition");
    if ((s = accum_alloc()) != GS_OK) return close_session(), s;
    acc.cam = *cam;
    acc.seed = seed;
    acc.chunk = chunk ? chunk : 16u;
    open = Session::Accum;
    return GS_OK;
}

gs_status gs_multi::accum_alloc() {
    const size_t nb = (size_t)gs_pass_delta_blocks(cap);
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        GROW(d.acc.sums, cap * 24);
        GROW(d.acc.delta, nb * 8);
        HIPOK(hipMemsetAsync(d.acc.sums.p, 0, (size_t)cap * 24, d.stream));
        if (hipHostMalloc((void**)&d.acc.h_delta, nb * 8, hipHostMallocDefault) != hipSuccess)
            return fail(GS_ERR_OOM, "hipHostMalloc of the pass's change failed");
        HIPOK(hipStreamSynchronize(d.stream));
    }
    return GS_OK;
}

gs_status gs_multi::views_accum_begin(const gs_camera& tall, const gs_view* views, uint32_t n_views, uint32_t chunk) {
    gs_status s = admit(Call::Begin, Session::ViewsAccum);
    if (s != GS_OK) return s;
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    if ((s = views_form_check()) != GS_OK) return s;
    DeviceGuard guard;
    // the accumulation's own tile height, so that no tile straddles two views
    const int32_t vth = gs_views_tile_h(views[0].cam.image_height, th);
    s = partition(&tall, 0, nullptr, true, vth);
    if (s == GS_OK && (cap <= 0 || cap >= (int64_t)0xFFFFFFFFll)) s = fail(GS_ERR_ARG, "bad partition");
    const size_t nb = s == GS_OK ? (size_t)(cap / ((int64_t)tw * vth)) : 0;
    for (size_t i = 0; s == GS_OK && i < dev.size(); i++) {
        Device& d = dev[i];
        if (hipSetDevice(d.id) != hipSuccess || !d.acc.sums.ensure((size_t)cap * 24) || !d.acc.delta.ensure(nb * 8))
            s = fail(GS_ERR_OOM, "hipMalloc of the views' sums failed");
        else if (hipHostMalloc((void**)&d.acc.h_delta, nb * 8, hipHostMallocDefault) != hipSuccess)
            s = fail(GS_ERR_OOM, "hipHostMalloc of the pass's change failed");
        else if (hipMemsetAsync(d.acc.sums.p, 0, (size_t)cap * 24, d.stream) != hipSuccess ||
                 hipStreamSynchronize(d.stream) != hipSuccess)
            s = fail(GS_ERR_HIP, "zeroing the views' sums failed");
    }
    if (s != GS_OK) return close_session(), s;
    va.views.assign(views, views + n_views);
    va.tall = tall;
    va.th = vth;
    va.chunk = chunk ? chunk : 16u;
    va.samples.assign(n_views, 0u);
    va.delta.assign(n_views, 0.0);
    open = Session::ViewsAccum;
    return GS_OK;
}

// ---------------------------------------------------------------- progressive adaptation, plain and of views
gs_status gs_multi::adapt_begin(const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                                const gs_view* views, uint32_t n_views) {
    const Session kind = views ? Session::ViewsAdapt : Session::Adapt;
    gs_status s = admit(Call::Begin, kind);
    if (s != GS_OK) return s;
    if (views && (s = views_form_check()) != GS_OK) return s;
    if (comms_broken) return fail(GS_ERR_HIP, "the context's communicator was aborted after a failed collective");
    if (cam->image_width <= 0 || cam->image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    if ((s = adapt_settings_check(ss)) != GS_OK) return s;
    const uint64_t R = (uint64_t)ss->max_samples / ss->batch_size + 1u;
    DeviceGuard guard;
    // (views: the batch's own tile height, so that no tile straddles two views)
    const int32_t ath = views ? gs_views_tile_h(views[0].cam.image_height, th) : th;
    if ((s = partition(cam, seed, nullptr, views != nullptr, ath)) != GS_OK) return s;
    if (cap <= 0 || cap >= (int64_t)0xFFFFFFFFll) return fail(GS_ERR_ARG, "bad partition");
    if ((s = adapt_alloc(gs_round_layout((uint64_t)cap, R))) != GS_OK) return close_session(), s;
    ad.cam = *cam;
    ad.ss = *ss;
    ad.th = ath;
    ad.seed = seed;
    ad.R = (uint32_t)R;
    ad.active = (uint64_t)cam->image_width * (uint64_t)cam->image_height;
    if (views) ad.views.assign(views, views + n_views);
    open = kind;
    return GS_OK;
}

gs_status gs_multi::adapt_alloc(const GsRoundLayout& l) {
    for (auto& d : dev) {
        HIPOK(hipSetDevice(d.id));
        GROW(d.ad.rstate, l.bytes);
        GROW(d.ad.map_samples, cap * 4);
        GROW(d.ad.map_error, cap * 4);
        HIPOK(hipMemsetAsync(d.ad.rstate.p, 0, l.bytes, d.stream));
        HIPOK(hipMemsetAsync(d.ad.map_samples.p, 0, (size_t)cap * 4, d.stream));
        HIPOK(hipMemsetAsync(d.ad.map_error.p, 0, (size_t)cap * 4, d.stream));
        if (!d.ad.h_summary &&
            hipHostMalloc((void**)&d.ad.h_summary, kRoundSummaryWords * 8, hipHostMallocDefault) != hipSuccess)
            return fail(GS_ERR_OOM, "hipHostMalloc of the round summary failed");
        HIPOK(hipStreamSynchronize(d.stream));
    }
    return GS_OK;
}

gs_status gs_multi::adapt_pass(uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats) {
    if (rounds == 0) return fail(GS_ERR_ARG, "a pass of 0 rounds");
    if (open == Session::ViewsAdapt && out && out->ppm_text) return fail(GS_ERR_ARG, "a views pass writes no PPM text");
    Frame f{open, &ad.cam, &ad.ss, ad.seed, ad.th};
    f.views = ad.views.empty() ? nullptr : ad.views.data();
    f.n_views = (uint32_t)ad.views.size();
    f.rounds = ad.finished() ? 0u : std::min(rounds, ad.R - ad.rounds);
    return render(f, out, stats);
}

gs_status gs_multi::adapt_maps(uint32_t* samples, float* rel_error) {
    DeviceGuard guard;
    std::vector<uint8_t> packed((size_t)cap * 4);
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        if (samples) {
            HIPOK(hipMemcpy(packed.data(), d.ad.map_samples.p, packed.size(), hipMemcpyDeviceToHost));
            permute_rank(i, ad.cam, (uint8_t*)samples, packed.data(), 4, true);
        }
        if (rel_error) {
            HIPOK(hipMemcpy(packed.data(), d.ad.map_error.p, packed.size(), hipMemcpyDeviceToHost));
            permute_rank(i, ad.cam, (uint8_t*)rel_error, packed.data(), 4, true);
        }
    }
    return GS_OK;
}

gs_status gs_multi::adapt_download(double* sums, uint32_t* state) {
    DeviceGuard guard;
    std::vector<uint8_t> packed((size_t)cap * 40);
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        const size_t rc = (size_t)rank_cap(i, ad.cam);
        const GsRoundLayout l = gs_round_layout(rc, ad.R);
        if (rc == 0) continue;
        HIPOK(hipSetDevice(d.id));
        HIPOK(hipStreamSynchronize(d.stream));
        if (sums) {
            HIPOK(hipMemcpy(packed.data(), (const char*)d.ad.rstate.p + l.pstate, rc * 40, hipMemcpyDeviceToHost));
            permute_rank(i, ad.cam, (uint8_t*)sums, packed.data(), 40, true);
        }
        HIPOK(hipMemcpy(packed.data(), (const char*)d.ad.rstate.p + l.batches, rc * 4, hipMemcpyDeviceToHost));
        permute_rank(i, ad.cam, (uint8_t*)state, packed.data(), 4, true);
    }
    return GS_OK;
}

// Behind adapt_begin: a checkpoint's state into the ranks' blobs (closes the adaptation when it cannot).
gs_status gs_multi::adapt_fill(uint32_t rounds_done, const double* sums, const uint32_t* state,
                               const gs_counters* counters) {
    const gs_camera* cam = &ad.cam;
    const uint64_t batch = ad.ss.batch_size;
    auto bail = [&](gs_status st) { return close_session(), st; };
    if (rounds_done > ad.R) return bail(fail(GS_ERR_ARG, "rounds_done exceeds the settings' rounds"));
    // every pixel's word against rounds_done: an active pixel has taken every round so far, a
    // stopped one at least one and no more than that
    const uint64_t npx = (uint64_t)cam->image_width * (uint64_t)cam->image_height;
    uint64_t active = 0, total = 0, most = 0;
    for (uint64_t k = 0; k < npx; k++) {
        const uint32_t nb = state[k] & ~GS_ADAPT_STOPPED;
        const bool stopped = (state[k] & GS_ADAPT_STOPPED) != 0;
        if (stopped ? (nb < 1 || nb > rounds_done) : (nb != rounds_done || (rounds_done == ad.R && rounds_done)))
            return bail(fail(GS_ERR_ARG, "a pixel's state disagrees with rounds_done"));
        active += stopped ? 0u : 1u;
        total += nb * batch;
        most = std::max(most, nb * batch);
    }
    if (rounds_done == 0) {  // (nothing to fill: the first pass initialises the state)
        ad.counters = ad.base = *counters;
        return GS_OK;
    }
    DeviceGuard guard;
    std::vector<double> psums((size_t)this->cap * 5);
    std::vector<uint32_t> words((size_t)this->cap), list;
    for (int i = 0; i < (int)dev.size(); i++) {
        Device& d = dev[i];
        const size_t cap = (size_t)rank_cap(i, *cam);  // (the rank's own: its launches lay the state out for it)
        const GsRoundLayout l = gs_round_layout(cap, ad.R);
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
        char* blob = (char*)d.ad.rstate.p;
        if (hipSetDevice(d.id) != hipSuccess ||
            hipMemcpy(blob + l.pstate, psums.data(), cap * 40, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(blob + l.batches, words.data(), cap * 4, hipMemcpyHostToDevice) != hipSuccess ||
            (n_act && hipMemcpy(blob + l.list[rounds_done & 1u], list.data(), (size_t)n_act * 4, hipMemcpyHostToDevice) !=
                          hipSuccess) ||
            hipMemcpy(blob + l.counts + (size_t)rounds_done * 4, &n_act, 4, hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(GS_ERR_HIP, "uploading the round state failed"));
    }
    ad.rounds = rounds_done;
    ad.active = active;
    ad.samples_total = total;
    ad.samples_max = most;
    ad.counters = ad.base = *counters;
    return GS_OK;
}

namespace {

// A session's own call: the context, its lock, the session open, then the call itself.
template <class M, class F>
gs_status in_session(M* m, Session s, Call call, F body) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    const gs_status st = m->admit(call, s);
    return st != GS_OK ? st : body();
}

// What gs_adapt_info and gs_views_adapt_info share.
template <class Info>
void adapt_info_fill(const AdaptState& a, Info* info) {
    std::memset(info, 0, sizeof(*info));
    info->width = a.cam.image_width;
    info->batch = a.ss.batch_size;
    info->rounds = a.rounds;
    info->max_rounds = a.R;
    info->finished = a.finished() ? 1u : 0u;
    info->active_pixels = a.active;
    info->samples_total = a.samples_total;
    info->samples_max = a.samples_max;
    info->counters = a.counters;
}

}  // namespace

extern "C" {

// ---- progressive accumulation
gs_status gs_multi_accum_begin(gs_multi* m, const gs_camera* cam, uint64_t seed, uint32_t chunk) {
    if (!m || !cam) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return m->accum_begin(cam, seed, chunk);
}

gs_status gs_multi_accum_pass(gs_multi* m, uint32_t samples, const gs_multi_outputs* out, gs_stats* stats) {
    return in_session(m, Session::Accum, Call::Pass, [&]() -> gs_status {
        const uint32_t c = m->acc.chunk;
        if (samples == 0 || samples % c != 0 || samples / c > 64u)
            return fail(GS_ERR_ARG, "a pass is 1 to 64 whole chunks of samples");
        if (m->acc.samples + samples > 0xFFFFFFFFull) return fail(GS_ERR_ARG, "the frame's samples overflow 32 bits");
        const gs_sample_settings ss{0.0, 0.0, samples, 0};
        return m->render(Frame{Session::Accum, &m->acc.cam, &ss, m->acc.seed, m->th}, out, stats);
    });
}

gs_status gs_multi_accum_info(const gs_multi* m, gs_accum_info* info) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::Accum, Call::Other, [&]() -> gs_status {
        std::memset(info, 0, sizeof(*info));
        info->width = m->acc.cam.image_width;
        info->height = m->acc.cam.image_height;
        info->chunk = m->acc.chunk;
        info->passes = m->acc.passes;
        info->seed = m->acc.seed;
        info->samples = m->acc.samples;
        info->last_delta = m->acc.last_delta;
        info->counters = m->acc.counters;
        return GS_OK;
    });
}

gs_status gs_multi_accum_download(gs_multi* m, double* sums) {
    if (!m || !sums) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::Accum, Call::Other, [&] { return m->permute_sums(m->acc.cam, sums, true); });
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
    s = m->permute_sums(m->acc.cam, const_cast<double*>(sums), false);
    if (s != GS_OK) return m->close_session(), s;
    m->acc.samples = samples;
    m->acc.counters = *counters;
    return GS_OK;
}

gs_status gs_multi_accum_end(gs_multi* m) {
    return in_session(m, Session::Accum, Call::Other, [&] { return m->close_session(), GS_OK; });
}

// ---- progressive views
gs_status gs_multi_views_accum_begin(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t chunk) {
    if (!m) return fail(GS_ERR_ARG, "null context");
    std::lock_guard<std::mutex> lock(m->mu);
    const uint32_t c = chunk ? chunk : 16u;
    gs_camera tall;
    gs_status s = gs_views_check(m->dev[0].scene, views, n_views, c, c, &tall);  // (one chunk: the views' own rules)
    if (s != GS_OK) return s;
    return m->views_accum_begin(tall, views, n_views, chunk);
}

gs_status gs_multi_views_accum_pass(gs_multi* m, uint32_t samples, const uint8_t* selected, const gs_multi_outputs* out,
                                    gs_stats* stats) {
    return in_session(m, Session::ViewsAccum, Call::Pass, [&]() -> gs_status {
        const ViewsAccumState& va = m->va;
        if (out && out->ppm_text) return fail(GS_ERR_ARG, "a views pass writes no PPM text");
        const uint32_t c = va.chunk, nv = (uint32_t)va.views.size();
        if (samples == 0 || samples % c != 0 || samples / c > 64u)
            return fail(GS_ERR_ARG, "a pass is 1 to 64 whole chunks of samples");
        Frame f{Session::ViewsAccum, &va.tall, nullptr, 0, va.th};
        f.views = va.views.data();
        f.n_views = nv;
        f.chunk = c;
        f.selected = selected;
        gs_status s = gs_views_pass_check(nv, va.samples.data(), selected, samples, c, &f.base);
        if (s != GS_OK) return s;
        // (rank 0 holds the most tiles of the round-robin cut: its share bounds every rank's)
        s = gs_views_check_cap(m->rank_cap(0, va.tall), samples, c);
        if (s != GS_OK) return s;
        const gs_sample_settings ss{0.0, 0.0, samples, 0};
        f.ss = &ss;
        return m->render(f, out, stats);
    });
}

gs_status gs_multi_views_accum_info(const gs_multi* m, gs_views_accum_info* info, uint32_t* view_samples_out,
                                    double* delta_out) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::ViewsAccum, Call::Other, [&]() -> gs_status {
        const ViewsAccumState& va = m->va;
        std::memset(info, 0, sizeof(*info));
        info->width = va.views[0].cam.image_width;
        info->height = va.views[0].cam.image_height;
        info->n_views = (uint32_t)va.views.size();
        info->chunk = va.chunk;
        info->passes = va.passes;
        info->tile_h = va.th;
        info->counters = va.counters;
        if (view_samples_out) std::memcpy(view_samples_out, va.samples.data(), va.samples.size() * sizeof(uint32_t));
        if (delta_out) std::memcpy(delta_out, va.delta.data(), va.delta.size() * sizeof(double));
        return GS_OK;
    });
}

gs_status gs_multi_views_accum_download(gs_multi* m, double* sums) {
    if (!m || !sums) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::ViewsAccum, Call::Other, [&] { return m->permute_sums(m->va.tall, sums, true); });
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
    s = m->views_accum_begin(tall, views, n_views, chunk);
    if (s != GS_OK) return s;
    s = m->permute_sums(m->va.tall, const_cast<double*>(sums), false);
    if (s != GS_OK) return m->close_session(), s;
    m->va.samples.assign(view_samples, view_samples + n_views);
    m->va.counters = *counters;
    return GS_OK;
}

gs_status gs_multi_views_accum_end(gs_multi* m) {
    return in_session(m, Session::ViewsAccum, Call::Other, [&] { return m->close_session(), GS_OK; });
}

// ---- progressive adaptation
gs_status gs_multi_adapt_begin(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed) {
    if (!m || !cam || !ss) return fail(GS_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    return m->adapt_begin(cam, ss, seed);
}

gs_status gs_multi_adapt_pass(gs_multi* m, uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats) {
    return in_session(m, Session::Adapt, Call::Pass, [&] { return m->adapt_pass(rounds, out, stats); });
}

gs_status gs_multi_adapt_info(const gs_multi* m, gs_adapt_info* info) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::Adapt, Call::Other, [&]() -> gs_status {
        adapt_info_fill(m->ad, info);
        info->height = m->ad.cam.image_height;
        info->seed = m->ad.seed;
        return GS_OK;
    });
}

gs_status gs_multi_adapt_maps(gs_multi* m, uint32_t* samples, float* rel_error) {
    return in_session(m, Session::Adapt, Call::Other, [&] { return m->adapt_maps(samples, rel_error); });
}

gs_status gs_multi_adapt_download(gs_multi* m, double* sums, uint32_t* state) {
    if (!m || !sums || !state) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::Adapt, Call::Other, [&] { return m->adapt_download(sums, state); });
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
    return in_session(m, Session::Adapt, Call::Other, [&] { return m->close_session(), GS_OK; });
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
    return in_session(m, Session::ViewsAdapt, Call::Pass, [&] { return m->adapt_pass(rounds, out, stats); });
}

gs_status gs_multi_views_adapt_info(gs_multi* m, gs_views_adapt_info* info, uint64_t* view_active_out) {
    if (!m || !info) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::ViewsAdapt, Call::Other, [&]() -> gs_status {
        const uint32_t nv = (uint32_t)m->ad.views.size();
        adapt_info_fill(m->ad, info);
        info->height = m->ad.views[0].cam.image_height;
        info->n_views = nv;
        info->tile_h = m->ad.th;
        if (view_active_out) {  // (not hot: the state words cross to the host)
            const size_t vpx = (size_t)info->width * (size_t)info->height;
            if (m->ad.rounds == 0) {
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
    });
}

gs_status gs_multi_views_adapt_maps(gs_multi* m, uint32_t* samples, float* rel_error) {
    return in_session(m, Session::ViewsAdapt, Call::Other, [&] { return m->adapt_maps(samples, rel_error); });
}

gs_status gs_multi_views_adapt_download(gs_multi* m, double* sums, uint32_t* state) {
    if (!m || !sums || !state) return fail(GS_ERR_ARG, "null argument");
    return in_session(m, Session::ViewsAdapt, Call::Other, [&] { return m->adapt_download(sums, state); });
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
    return in_session(m, Session::ViewsAdapt, Call::Other, [&] { return m->close_session(), GS_OK; });
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
    return m->render(Frame{Session::None, cam, ss, seed, m->th}, out, stats);
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
    Frame f{Session::None, &tall, &ss, 0, m->th};
    f.views = views;
    f.n_views = n_views;
    f.chunk = c;
    return m->render(f, out, stats);
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
        s = m->render(Frame{Session::None, cam, ss, seed, m->th}, out, stats);
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
