// launch.cpp — a device scene becomes launches: the process knobs and their setters, the work
// plan that cuts a frame into items, the LDS mirror fit, the launch slots, `launch` itself, the
// placement pilot, gs_plan_tiles and the small device-memory entry points.  Plain C++ over the
// HIP runtime API; the kernels are enqueued through render.hip's launchers (kernels.hpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "../device/kernels.hpp"
#include "render_host.hpp"

static thread_local std::string tl_err;
// Process-wide tuning (the gs_set_* / gs_debug_set_* setters).  Atomics: a setter may run
// while another thread launches; each launch reads every value once (read_knobs), so
// one launch never mixes two settings of the same knob.
static std::atomic<int32_t> g_shade_batch{0};   // 0: the scene's own (52, or GS_KIND_SHADE_BATCH with BVHs under instances);  // swept on MI355X C4 (chunked, uniform loop): 48 -> 3502, 52 -> 3535-3568, 56 -> 3506-3536 Msamples/s
static std::atomic<int32_t> g_blocks_per_cu{0};  // 0 = occupancy query
static std::atomic<int32_t> g_node_steps{0};  // 0: the scene's own (gs_device_scene.node_steps)
// leaf batch: 0 = the scene's choice (12: swept on MI355X C4 with leaf runs: 8 -> 4586, 10 ->
// 4632, 12 -> 4648-4651, 14 -> 4624, 16 -> 4592; GS_KIND_LEAF_BATCH for kind-batched kernels)
static std::atomic<int32_t> g_leaf_batch{0};
static std::atomic<int32_t> g_cam_batch{0};  // 0: the scene's own (gs_set_camera_batch)
static std::atomic<int32_t> g_tail_pct{0};  // guided tail (gs_debug_set_guided_tail): 0 = default
// -1 auto, 0 never split a pixel's samples.  Swept on MI355X with batched queue claims,
// C4 rank 0 / rank 3 of N (tools/rank_sim.py; ms): N=1: 4 -> 658.4, 8 -> 658.7,
// 16 -> 648.3, 32 -> 647.3; N=8: 4 -> 89.6, 8 -> 89.6, 16 -> 89.7, 32 -> 95.8 (max of the
// two ranks).  16 is within noise of the best at both ends.
static std::atomic<int32_t> g_sample_chunk{-1};
static std::atomic<int32_t> g_placement{1};  // 1: placement pilot at a scene's first launch; 0: the static estimate only
static std::atomic<uint64_t> g_partial_budget{4ull << 30};  // auto chunks: at most 4 GiB of chunk sums (per launch slot)
// Adaptive settings (more than one batch): 1 = batch rounds (gs_round_*_kernel), 0 = the
// per-lane loop (one work item per pixel running every batch).  Bit-identical results.
static std::atomic<int32_t> g_adaptive_rounds{1};  // 1 auto (GS_ROUND_MIN_CAP), 2 always rounds, 0 never
// Work items of a round: 0 split (default; measured on MI355X, A2 cornell_box 1024^2: split
// 7520, whole-batch items while the active pixels fill the lanes twice 5910 Msamples/s;
// A1 hdri 19738 vs 18124), 1 whole-batch items, -1 whole while the active pixels fill the
// lanes twice.
static std::atomic<int32_t> g_round_whole{0};
// Auto mode: batch rounds when a pixel can take at least this many samples ((max_samples /
// batch + 1) x batch): the per-lane loop's tail is up to that many samples in one lane.
// MI355X: A2 cornell_box (cap 1024) rounds 7520 vs per-lane 5394 Msamples/s; A1 hdri (cap
// 256) rounds 19738 vs per-lane 24582 -- its pixels stop after one or two batches, and the
// rounds' per-sample colours and launches cost more than its short tail.
#ifndef GS_ROUND_MIN_CAP
#define GS_ROUND_MIN_CAP 512
#endif
static const uint64_t kMaxRounds = 1u << 16;  // more batches than this: the per-lane loop
static std::atomic<int32_t> g_cube_lists{1};  // gs_debug_set_cube_lists
static std::atomic<int32_t> g_cert_boxes{1};  // gs_debug_set_cert_boxes
static std::atomic<int64_t> g_mirror_budget{-1};  // gs_debug_set_mirror_budget
static std::atomic<int32_t> g_max_blocks{0};  // gs_debug_set_max_blocks: 0 = no limit of its own

Knobs read_knobs() {
    const auto rlx = std::memory_order_relaxed;
    Knobs k;
    k.shade_batch = g_shade_batch.load(rlx);
    k.blocks_per_cu = g_blocks_per_cu.load(rlx);
    k.node_steps = g_node_steps.load(rlx);
    k.leaf_batch = g_leaf_batch.load(rlx);
    k.cam_batch = g_cam_batch.load(rlx);
    k.tail_pct = g_tail_pct.load(rlx);
    k.sample_chunk = g_sample_chunk.load(rlx);
    k.placement = g_placement.load(rlx);
    k.partial_budget = g_partial_budget.load(rlx);
    k.adaptive_rounds = g_adaptive_rounds.load(rlx);
    k.round_whole = g_round_whole.load(rlx);
    k.cube_lists = g_cube_lists.load(rlx);
    k.cert_boxes = g_cert_boxes.load(rlx);
    k.mirror_budget = g_mirror_budget.load(rlx);
    k.max_blocks = g_max_blocks.load(rlx);
    return k;
}

int32_t launch_node_steps(const gs_device_scene* ds, const Knobs& k) {
    return std::max(1, std::min<int32_t>(unroll_steps(ds->feat), k.node_steps > 0 ? k.node_steps : ds->node_steps));
}

extern "C" void gs_set_last_error(const char* msg) { tl_err = msg ? msg : ""; }
gs_status fail(gs_status code, const std::string& msg) {
    tl_err = msg;
    return code;
}

extern "C" {

const char* gs_last_error(void) { return tl_err.c_str(); }
int32_t gs_version(void) { return GS_ABI_VERSION; }

gs_status gs_set_node_steps(int32_t node_steps) {
    if (node_steps < 0 || node_steps > GS_NODE_STEPS) return fail(GS_ERR_ARG, "node_steps outside [0, GS_NODE_STEPS]");
    g_node_steps = node_steps;
    return GS_OK;
}

gs_status gs_set_camera_batch(int32_t cam_batch) {
    if (cam_batch < 0 || cam_batch > 64) return fail(GS_ERR_ARG, "camera batch outside [0, 64]");
    g_cam_batch = cam_batch;
    return GS_OK;
}

gs_status gs_set_tuning(int32_t shade_batch, int32_t blocks_per_cu, int32_t leaf_batch, int32_t sample_chunk) {
    if (shade_batch < 0 || shade_batch > 64 || blocks_per_cu < 0 || blocks_per_cu > 8 || leaf_batch < 0 ||
        leaf_batch > 64 || sample_chunk < -1)
        return fail(GS_ERR_ARG, "bad tuning");
    g_sample_chunk = sample_chunk;
    g_leaf_batch = leaf_batch;
    g_shade_batch = shade_batch;
    g_blocks_per_cu = blocks_per_cu;
    return GS_OK;
}

gs_status gs_set_placement(int32_t mode) {
    if (mode != 0 && mode != 1) return fail(GS_ERR_ARG, "placement mode is 0 or 1");
    g_placement = mode;
    return GS_OK;
}

gs_status gs_set_adaptive_mode(int32_t mode) {
    if (mode < 0 || mode > 2)
        return fail(GS_ERR_ARG, "adaptive mode is 0 (per-lane loop), 1 (auto) or 2 (batch rounds)");
    g_adaptive_rounds = mode;
    return GS_OK;
}

gs_status gs_debug_set_round_items(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(GS_ERR_ARG, "round item mode is -1 (auto), 0 (split) or 1 (whole)");
    g_round_whole = mode;
    return GS_OK;
}

gs_status gs_debug_set_cube_lists(int32_t on) {
    if (on != 0 && on != 1) return fail(GS_ERR_ARG, "cube lists are 0 (the list loop) or 1 (cube_test)");
    g_cube_lists = on;
    return GS_OK;
}

gs_status gs_debug_set_cert_boxes(int32_t on) {
    if (on != 0 && on != 1) return fail(GS_ERR_ARG, "cert boxes are 1 (the 1e15 rule decides) or 0 (the f64 box test)");
    g_cert_boxes = on;
    return GS_OK;
}

gs_status gs_debug_set_mirror_budget(int64_t bytes) {
    if (bytes < -1) return fail(GS_ERR_ARG, "the mirror budget is -1 (the block's own) or a byte count >= 0");
    g_mirror_budget = bytes;
    return GS_OK;
}

gs_status gs_debug_set_max_blocks(int32_t blocks) {
    if (blocks < 0) return fail(GS_ERR_ARG, "the block limit is 0 (none) or a count >= 1");
    g_max_blocks = blocks;
    return GS_OK;
}

gs_status gs_debug_set_partial_budget(uint64_t bytes) {
    g_partial_budget.store(bytes ? bytes : (4ull << 30));
    return GS_OK;
}

gs_status gs_debug_set_guided_tail(int32_t fine_chunk, int32_t tail_pct) {
    if (fine_chunk < 0 || tail_pct < 0) return fail(GS_ERR_ARG, "fine_chunk and tail_pct are >= 0 (0: the default)");
    // (the tail's items are single samples, which the combine regroups into the coarse chunks:
    // other sizes would make the association depend on which tiles run in the tail)
    if (fine_chunk > 1) return fail(GS_ERR_ARG, "fine_chunk is 0 or 1 (1-sample tail items)");
    g_tail_pct.store(tail_pct);
    return GS_OK;
}

#ifndef GS_SHORT_SAMPLE_LANE_US
#define GS_SHORT_SAMPLE_LANE_US 50.0
#endif
// Compute units of a device (cached: the attribute query costs ~0.5 ms).
static int device_cus(int dev) {
    static std::atomic<int> cache[64];
    if (dev < 0 || dev >= 64) return 256;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

void gs_device_scene_note_frame(gs_device_scene* ds, double kernel_ms, uint64_t samples) {
    if (!ds || !(kernel_ms > 0.0) || samples == 0) return;
    const double lanes = (double)device_cus(ds->device) * GS_BLOCK;
    const double lus = kernel_ms * 1e3 * lanes / (double)samples;
    ds->lane_us_per_sample.store(lus, std::memory_order_relaxed);
    if (lus > GS_SHORT_SAMPLE_LANE_US) ds->long_samples.store(true, std::memory_order_relaxed);
}

static bool part_ok(const gs_camera* cam, const gs_partition* p) {
    return cam && p && cam->image_width > 0 && cam->image_height > 0 && p->world_size >= 1 && p->rank >= 0 &&
           p->rank < p->world_size && p->tile_w > 0 && p->tile_h > 0 && (int64_t)p->tile_w * p->tile_h <= (1 << 20) &&
           (!p->d_tile_order || p->slots_per_rank > 0);
}

int64_t gs_partition_capacity(const gs_camera* cam, const gs_partition* p) {
    if (!part_ok(cam, p)) return -1;
    if (p->d_tile_order) return (int64_t)p->slots_per_rank * p->tile_w * p->tile_h;
    int64_t tx = (cam->image_width + p->tile_w - 1) / p->tile_w;
    int64_t ty = (cam->image_height + p->tile_h - 1) / p->tile_h;
    int64_t nt = tx * ty;
    int64_t mine = nt > p->rank ? (nt - p->rank + p->world_size - 1) / p->world_size : 0;
    return mine * p->tile_w * p->tile_h;
}

gs_status gs_render_tiles_async(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                uint64_t seed, const gs_partition* part, float* d_out, gs_counters* d_counters,
                                void* stream) {
    if (!d_out) return fail(GS_ERR_ARG, "null argument");
    gs_render_outputs o{d_out, nullptr, nullptr};
    return gs_render_tiles_ex_async(ds, cam, ss, seed, part, &o, d_counters, stream);
}

gs_status gs_render_tiles_debug_async(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                      uint64_t seed, const gs_partition* part, float* d_out,
                                      gs_counters* d_counters, uint32_t* d_item_visits, void* stream) {
    if (!d_out) return fail(GS_ERR_ARG, "null argument");
    gs_render_outputs o{d_out, nullptr, d_item_visits};
    return gs_render_tiles_ex_async(ds, cam, ss, seed, part, &o, d_counters, stream);
}

gs_status gs_render_tiles_ex_async(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                   uint64_t seed, const gs_partition* part, const gs_render_outputs* outs,
                                   gs_counters* d_counters, void* stream) {
    return gs_render_tiles_timed_async(ds, cam, ss, seed, part, outs, d_counters, stream, nullptr, nullptr);
}

}  // extern "C"

// A GS_FEAT_VISITS launch's count buffer: node record positions, then leaf positions.
struct VisitArgs {
    uint32_t* visits;
    uint32_t leaf_base;
};
// A progressive pass (gs_render_tiles_pass_async): the launch renders samples [sample_base,
// sample_base + ss->batch_size) in chunks of `chunk`, and gs_accumulate_kernel adds them to d_sums.
struct PassArgs {
    uint32_t sample_base, chunk;
    double* d_sums;
    double* d_delta;  // [gs_accum_blocks(capacity)], nullable
};
// A progressive adaptive pass (gs_render_tiles_rounds_async): the launch renders rounds
// [first_round, first_round + rounds) on the round state in the caller's blob, in split items,
// gs_round_fold_kernel after each; gs_round_resolve_kernel ends it.
struct RoundArgs {
    uint32_t first_round, rounds, R;
    uint8_t* d_state;
    uint32_t* map_samples;
    float* map_error;
};
// A views launch (gs_render_tiles_views_async): `cam` is the tall frame's camera, the camera-ray
// step reads `views` (host; uploaded to the slot by the launch), the coarse chunk as given.
struct ViewsArgs {
    const gs_view* views;
    uint32_t n, chunk;
    // A progressive views pass (gs_render_tiles_views_pass_async; with PassArgs): the per-view
    // records (host, n of them; null for a plain views launch) and the per-slot change partials.
    const GsViewState* vstate = nullptr;
    double* d_vdelta = nullptr;
};
static gs_status launch(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                        const gs_partition* part, const gs_render_outputs* outs, gs_counters* d_counters, void* stream,
                        hipEvent_t k_begin, hipEvent_t k_end, const VisitArgs* va, bool direct = false,
                        bool zero_counters = false, const PassArgs* pass = nullptr, const RoundArgs* ra = nullptr,
                        const ViewsArgs* vw = nullptr);
static gs_status ensure_placement(gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                  void* stream);

gs_status gs_render_tiles_timed_async(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                      uint64_t seed, const gs_partition* part, const gs_render_outputs* outs,
                                      gs_counters* d_counters, void* stream, hipEvent_t k_begin, hipEvent_t k_end,
                                      bool direct, bool zero_counters) {
    if (!ds || !cam) return fail(GS_ERR_ARG, "null argument");
    gs_status e = ensure_placement(const_cast<gs_device_scene*>(ds), cam, ss, stream);
    if (e != GS_OK) return e;
    return launch(ds, cam, ss, seed, part, outs, d_counters, stream, k_begin, k_end, nullptr, direct, zero_counters);
}

// The checks of a progressive pass, all on the arguments alone: nothing here reads the scene or
// touches a device.
static gs_status check_pass(const gs_device_scene* ds, const gs_camera* cam, uint32_t samples, const gs_partition* part,
                            uint32_t sample_base, uint32_t c, const double* d_sums, const gs_render_outputs* outs) {
    if (!ds || !cam || !part || !d_sums || !outs || (!outs->rgb && !outs->rgb8)) return fail(GS_ERR_ARG, "null argument");
    if (samples == 0) return fail(GS_ERR_ARG, "a pass of 0 samples");
    if (samples % c != 0) return fail(GS_ERR_ARG, "samples is not a multiple of the chunk");
    if (sample_base % c != 0) return fail(GS_ERR_ARG, "sample_base is not a multiple of the chunk");
    if (samples / c > 64u) return fail(GS_ERR_ARG, "more than 64 chunks in one pass");
    if ((uint64_t)sample_base + samples > 0xFFFFFFFFull) return fail(GS_ERR_ARG, "sample_base + samples overflows 32 bits");
    const int64_t cap = gs_partition_capacity(cam, part);
    if (cap < 0) return fail(GS_ERR_ARG, "bad partition / image size");
    if ((uint64_t)cap * (samples / c) * 24u > read_knobs().partial_budget)
        return fail(GS_ERR_ARG, "the pass's chunk sums exceed the partial budget: fewer samples per pass");
    return GS_OK;
}

gs_status gs_render_tiles_pass_timed_async(const gs_device_scene* ds, const gs_camera* cam, uint32_t samples,
                                           uint64_t seed, const gs_partition* part, uint32_t sample_base,
                                           uint32_t chunk, double* d_sums, double* d_delta,
                                           const gs_render_outputs* outs, gs_counters* d_counters, void* stream,
                                           hipEvent_t k_begin, hipEvent_t k_end, bool direct, bool zero_counters) {
    const uint32_t c = chunk ? chunk : 16u;
    gs_status e = check_pass(ds, cam, samples, part, sample_base, c, d_sums, outs);
    if (e != GS_OK) return e;
    const gs_sample_settings ss{0.0, 0.0, samples, 0};  // one batch of `samples` (max_samples < batch_size)
    e = ensure_placement(const_cast<gs_device_scene*>(ds), cam, &ss, stream);
    if (e != GS_OK) return e;
    const PassArgs pa{sample_base, c, d_sums, d_delta};
    return launch(ds, cam, &ss, seed, part, outs, d_counters, stream, k_begin, k_end, nullptr, direct, zero_counters, &pa);
}

extern "C" gs_status gs_render_tiles_pass_async(const gs_device_scene* ds, const gs_camera* cam, uint32_t samples,
                                                uint64_t seed, const gs_partition* part, uint32_t sample_base,
                                                uint32_t chunk, double* d_sums, const gs_render_outputs* outs,
                                                gs_counters* d_counters, void* stream) {
    return gs_render_tiles_pass_timed_async(ds, cam, samples, seed, part, sample_base, chunk, d_sums, nullptr, outs,
                                            d_counters, stream, nullptr, nullptr, false, false);
}

// ---------------------------------------------------------------- views
// The checks of a views call that need no partition, all on the arguments alone: nothing here
// reads the scene or touches a device.
gs_status gs_views_check(const gs_device_scene* ds, const gs_view* views, uint32_t n_views, uint32_t samples, uint32_t c,
                         gs_camera* tall) {
    if (!ds || !views || !tall) return fail(GS_ERR_ARG, "null argument");
    if (n_views == 0) return fail(GS_ERR_ARG, "a views call of 0 views");
    const gs_camera& c0 = views[0].cam;
    if (c0.image_width <= 0 || c0.image_height <= 0) return fail(GS_ERR_ARG, "bad image size");
    for (uint32_t v = 0; v < n_views; v++) {
        if (views[v].cam.image_width != c0.image_width || views[v].cam.image_height != c0.image_height)
            return fail(GS_ERR_ARG, "view " + std::to_string(v) + " differs from view 0 in width or height");
        if (views[v].cam.max_depth == 0) return fail(GS_ERR_ARG, "view " + std::to_string(v) + " has max_depth 0");
    }
    if (samples == 0) return fail(GS_ERR_ARG, "a views call of 0 samples");
    if (samples % c != 0) return fail(GS_ERR_ARG, "samples is not a multiple of the chunk");
    if (samples / c > 64u) return fail(GS_ERR_ARG, "more than 64 chunks per pixel");
    // (the tall frame's pixel ids are u32, its height an i32)
    if ((uint64_t)n_views * (uint64_t)c0.image_width * (uint64_t)c0.image_height >= 0xFFFFFFFFull ||
        (uint64_t)n_views * (uint64_t)c0.image_height > 0x7FFFFFFFull)
        return fail(GS_ERR_ARG, "views x width x height does not fit 32-bit pixel ids");
    *tall = c0;
    tall->image_height = (int32_t)(n_views * (uint32_t)c0.image_height);
    return GS_OK;
}

// ... and those of one rank's share of the tall frame, `cap` packed pixels.
gs_status gs_views_check_cap(int64_t cap, uint32_t samples, uint32_t c) {
    if (cap < 0) return fail(GS_ERR_ARG, "bad partition / image size");
    if ((uint64_t)cap * (samples / c) >= 0xFFFFFFFFull) return fail(GS_ERR_ARG, "too many work items for the 32-bit work queue");
    if ((uint64_t)cap * (samples / c) * 24u > read_knobs().partial_budget)
        return fail(GS_ERR_ARG, "the views' chunk sums exceed the partial budget: fewer views per call");
    return GS_OK;
}
static gs_status check_views_part(const gs_camera& tall, const gs_partition* part, uint32_t samples, uint32_t c,
                                  const gs_render_outputs* outs) {
    if (!part || !outs || (!outs->rgb && !outs->rgb8)) return fail(GS_ERR_ARG, "null argument");
    if (outs->item_visits) return fail(GS_ERR_ARG, "a views call has no per-pixel visit output");
    return gs_views_check_cap(gs_partition_capacity(&tall, part), samples, c);
}

gs_status gs_render_tiles_views_timed_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                            uint32_t samples, uint32_t chunk, const gs_partition* part,
                                            const gs_render_outputs* outs, gs_counters* d_counters, void* stream,
                                            hipEvent_t k_begin, hipEvent_t k_end, bool direct, bool zero_counters) {
    const uint32_t c = chunk ? chunk : 16u;
    gs_camera tall;
    gs_status e = gs_views_check(ds, views, n_views, samples, c, &tall);
    if (e == GS_OK) e = check_views_part(tall, part, samples, c, outs);
    if (e != GS_OK) return e;
    if (!has_views(ds->feat))
        return fail(GS_ERR_UNSUPPORTED, "the scene needs the catch-all kernel, which has no views form");
    const gs_sample_settings ss{0.0, 0.0, samples, 0};  // one batch of `samples` (max_samples < batch_size)
    e = ensure_placement(const_cast<gs_device_scene*>(ds), &views[0].cam, &ss, stream);  // (view 0's own frame)
    if (e != GS_OK) return e;
    const ViewsArgs vw{views, n_views, c};
    return launch(ds, &tall, &ss, 0, part, outs, d_counters, stream, k_begin, k_end, nullptr, direct, zero_counters,
                  nullptr, nullptr, &vw);
}

extern "C" gs_status gs_render_tiles_views_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                                 uint32_t samples, uint32_t chunk, const gs_partition* part,
                                                 const gs_render_outputs* outs, gs_counters* d_counters, void* stream) {
    return gs_render_tiles_views_timed_async(ds, views, n_views, samples, chunk, part, outs, d_counters, stream, nullptr,
                                             nullptr, false, false);
}

// ---------------------------------------------------------------- progressive views
extern "C" int32_t gs_views_tile_h(int32_t height, int32_t tile_h) {
    if (height <= 0 || tile_h <= 0) return 0;
    int32_t t = std::min(height, tile_h);
    while (height % t != 0) t--;
    return t;
}

// The checks of a views pass's selection, on the arguments alone: the selected views' common
// sample count into *base.  selected NULL: every view.
gs_status gs_views_pass_check(uint32_t n_views, const uint32_t* view_samples, const uint8_t* selected, uint32_t samples,
                              uint32_t c, uint32_t* base) {
    if (!view_samples || !base) return fail(GS_ERR_ARG, "null argument");
    bool any = false;
    uint32_t b = 0;
    for (uint32_t v = 0; v < n_views; v++) {
        if (view_samples[v] % c != 0)
            return fail(GS_ERR_ARG, "view " + std::to_string(v) + "'s samples are not a multiple of the chunk");
        if (selected && !selected[v]) continue;
        if (any && view_samples[v] != b)
            return fail(GS_ERR_ARG, "the selected views hold different sample counts (view " + std::to_string(v) +
                                        "): one pass per count");
        b = view_samples[v];
        any = true;
    }
    if (!any) return fail(GS_ERR_ARG, "an empty selection: no view to render");
    if ((uint64_t)b + samples > 0xFFFFFFFFull) return fail(GS_ERR_ARG, "a view's samples overflow 32 bits");
    *base = b;
    return GS_OK;
}

gs_status gs_render_tiles_views_pass_timed_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                                 const uint32_t* view_samples, const uint8_t* selected, uint32_t samples,
                                                 uint32_t chunk, const gs_partition* part, double* d_sums,
                                                 const gs_render_outputs* outs, double* d_delta_partials,
                                                 gs_counters* d_counters, void* stream, hipEvent_t k_begin,
                                                 hipEvent_t k_end, bool direct, bool zero_counters) {
    const uint32_t c = chunk ? chunk : 16u;
    gs_camera tall;
    gs_status e = gs_views_check(ds, views, n_views, samples, c, &tall);
    if (e != GS_OK) return e;
    if (!d_sums) return fail(GS_ERR_ARG, "null argument");
    uint32_t base = 0;
    e = gs_views_pass_check(n_views, view_samples, selected, samples, c, &base);
    if (e == GS_OK) e = check_views_part(tall, part, samples, c, outs);
    if (e != GS_OK) return e;
    if (views[0].cam.image_height % part->tile_h != 0)
        return fail(GS_ERR_ARG, "tile_h does not divide the views' height (gs_views_tile_h): a tile would straddle two views");
    if (!has_views(ds->feat))
        return fail(GS_ERR_UNSUPPORTED, "the scene needs the catch-all kernel, which has no views form");
    const gs_sample_settings ss{0.0, 0.0, samples, 0};  // one batch of `samples` (max_samples < batch_size)
    e = ensure_placement(const_cast<gs_device_scene*>(ds), &views[0].cam, &ss, stream);  // (view 0's own frame)
    if (e != GS_OK) return e;
    std::vector<GsViewState> vs(n_views);
    for (uint32_t v = 0; v < n_views; v++) vs[v] = GsViewState{view_samples[v], (!selected || selected[v]) ? 1u : 0u};
    const PassArgs pa{base, c, d_sums, nullptr};
    ViewsArgs vw{views, n_views, c};
    vw.vstate = vs.data();
    vw.d_vdelta = d_delta_partials;
    return launch(ds, &tall, &ss, 0, part, outs, d_counters, stream, k_begin, k_end, nullptr, direct, zero_counters, &pa,
                  nullptr, &vw);
}

extern "C" gs_status gs_render_tiles_views_pass_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                                      const uint32_t* view_samples, const uint8_t* selected,
                                                      uint32_t samples, uint32_t chunk, const gs_partition* part,
                                                      double* d_sums, const gs_render_outputs* outs,
                                                      double* d_delta_partials, gs_counters* d_counters, void* stream) {
    return gs_render_tiles_views_pass_timed_async(ds, views, n_views, view_samples, selected, samples, chunk, part, d_sums,
                                                  outs, d_delta_partials, d_counters, stream, nullptr, nullptr, false, false);
}

// ---------------------------------------------------------------- progressive adaptive passes
static_assert(kRoundSummaryWords == GS_ROUND_SUMMARY_WORDS, "the summary words of internal.hpp and kernel_abi.hpp");
GsRoundLayout gs_round_layout(uint64_t cap, uint64_t R) {
    const auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    GsRoundLayout l{};
    l.hint = 0;
    l.summary = 16;
    l.counts = 16 + GS_ROUND_SUMMARY_WORDS * 8;
    l.list[0] = al(l.counts + (size_t)(R + 2) * 4);
    l.list[1] = l.list[0] + al((size_t)cap * 4);
    l.pstate = l.list[1] + al((size_t)cap * 4);
    l.batches = l.pstate + al((size_t)cap * 5 * sizeof(double));
    l.bytes = l.batches + al((size_t)cap * 4);
    return l;
}

// Pixels per segment of a round: as many as the partial budget holds a batch's colours for.
static uint64_t round_seg_px(uint64_t cap, const gs_sample_settings& ss, const Knobs& k) {
    uint64_t sp = std::min<uint64_t>(cap, k.partial_budget / ((uint64_t)ss.batch_size * 24u));
    return std::min<uint64_t>(sp, (0x7FFFFFFFull - 1u) / ss.batch_size);  // (sp * bs < 2^31: the queue's items)
}

// The checks of a progressive adaptive pass, all on the arguments alone: nothing here reads the
// scene or touches a device.  zero_rounds: the library's own resolve-only form.
static gs_status check_rounds(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                              const gs_partition* part, uint32_t first_round, uint32_t rounds, const void* d_state,
                              int64_t state_bytes, const gs_round_outputs* out, bool zero_rounds) {
    if (!ds || !cam || !ss || !part || !d_state || !out || (!out->rgb && !out->rgb8))
        return fail(GS_ERR_ARG, "null argument");
    const int64_t cap = gs_partition_capacity(cam, part);
    if (cap < 0 || cap >= (int64_t)0xFFFFFFFFll) return fail(GS_ERR_ARG, "bad partition / image size");
    if (rounds == 0 && !zero_rounds) return fail(GS_ERR_ARG, "a pass of 0 rounds");
    if (ss->batch_size == 0) return fail(GS_ERR_ARG, "batch_size 0 never terminates (camera.rs:137)");
    if (ss->max_samples < ss->batch_size)
        return fail(GS_ERR_ARG, "the settings run one batch (max_samples < batch_size): a fixed-spp frame has its "
                                "passes in gs_render_tiles_pass_async");
    const uint64_t R = (uint64_t)ss->max_samples / ss->batch_size + 1u;
    if (R > kMaxRounds) return fail(GS_ERR_ARG, "more than 65536 batches (max_samples / batch_size + 1): no round form");
    if ((uint64_t)first_round + rounds > R)
        return fail(GS_ERR_ARG, "first_round + rounds exceeds the settings' " + std::to_string(R) + " rounds");
    if (state_bytes < 0 || (uint64_t)state_bytes < gs_round_layout((uint64_t)cap, R).bytes)
        return fail(GS_ERR_ARG, "state_bytes below gs_round_state_bytes");
    if (cap > 0 && round_seg_px((uint64_t)cap, *ss, read_knobs()) < 1)
        return fail(GS_ERR_ARG, "one pixel's batch exceeds the partial budget");
    return GS_OK;
}

gs_status gs_render_tiles_rounds_timed_async(const gs_device_scene* ds, const gs_camera* cam,
                                             const gs_sample_settings* ss, uint64_t seed, const gs_partition* part,
                                             uint32_t first_round, uint32_t rounds, void* d_state, int64_t state_bytes,
                                             const gs_round_outputs* out, gs_counters* d_counters, void* stream,
                                             hipEvent_t k_begin, hipEvent_t k_end, bool direct, bool zero_counters) {
    gs_status e = check_rounds(ds, cam, ss, part, first_round, rounds, d_state, state_bytes, out, true);
    if (e != GS_OK) return e;
    e = ensure_placement(const_cast<gs_device_scene*>(ds), cam, ss, stream);
    if (e != GS_OK) return e;
    const RoundArgs ra{first_round, rounds, ss->max_samples / ss->batch_size + 1u, (uint8_t*)d_state, out->samples,
                       out->rel_error};
    const gs_render_outputs o{out->rgb, out->rgb8, nullptr};
    return launch(ds, cam, ss, seed, part, &o, d_counters, stream, k_begin, k_end, nullptr, direct, zero_counters,
                  nullptr, &ra);
}

// ---------------------------------------------------------------- adaptive views
// A views adaptation's pass: the views' rules and the rounds' rules on the tall frame, all on the
// arguments alone, then the round pass with the views' records (launch: RoundArgs and ViewsArgs).
static gs_status check_views_rounds(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                    const gs_sample_settings* ss, const gs_partition* part, uint32_t first_round,
                                    uint32_t rounds, const void* d_state, int64_t state_bytes,
                                    const gs_round_outputs* out, bool zero_rounds, gs_camera* tall) {
    gs_status e = gs_views_check(ds, views, n_views, 1, 1, tall);  // (one sample, one chunk: the views' own rules)
    if (e == GS_OK) e = check_rounds(ds, tall, ss, part, first_round, rounds, d_state, state_bytes, out, zero_rounds);
    if (e != GS_OK) return e;
    if (views[0].cam.image_height % part->tile_h != 0)
        return fail(GS_ERR_ARG, "tile_h does not divide the views' height (gs_views_tile_h): a tile would straddle two views");
    return GS_OK;
}

gs_status gs_render_tiles_views_rounds_timed_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                                   const gs_sample_settings* ss, const gs_partition* part,
                                                   uint32_t first_round, uint32_t rounds, void* d_state,
                                                   int64_t state_bytes, const gs_round_outputs* out,
                                                   gs_counters* d_counters, void* stream, hipEvent_t k_begin,
                                                   hipEvent_t k_end, bool direct, bool zero_counters) {
    gs_camera tall;
    gs_status e = check_views_rounds(ds, views, n_views, ss, part, first_round, rounds, d_state, state_bytes, out, true, &tall);
    if (e != GS_OK) return e;
    if (!has_views_rounds(ds->feat))
        return fail(GS_ERR_UNSUPPORTED, "the scene needs the catch-all kernel, which has no views form");
    e = ensure_placement(const_cast<gs_device_scene*>(ds), &views[0].cam, ss, stream);  // (view 0's own frame)
    if (e != GS_OK) return e;
    const RoundArgs ra{first_round, rounds, ss->max_samples / ss->batch_size + 1u, (uint8_t*)d_state, out->samples,
                       out->rel_error};
    const ViewsArgs vw{views, n_views, 0};
    const gs_render_outputs o{out->rgb, out->rgb8, nullptr};
    return launch(ds, &tall, ss, 0, part, &o, d_counters, stream, k_begin, k_end, nullptr, direct, zero_counters, nullptr,
                  &ra, &vw);
}

extern "C" gs_status gs_render_tiles_views_rounds_async(const gs_device_scene* ds, const gs_view* views,
                                                        uint32_t n_views, const gs_sample_settings* ss,
                                                        const gs_partition* part, uint32_t first_round,
                                                        uint32_t rounds, void* d_state, int64_t state_bytes,
                                                        const gs_round_outputs* out, gs_counters* d_counters,
                                                        void* stream) {
    gs_camera tall;
    gs_status e = check_views_rounds(ds, views, n_views, ss, part, first_round, rounds, d_state, state_bytes, out, false, &tall);
    if (e != GS_OK) return e;
    return gs_render_tiles_views_rounds_timed_async(ds, views, n_views, ss, part, first_round, rounds, d_state,
                                                    state_bytes, out, d_counters, stream, nullptr, nullptr, false, false);
}

extern "C" int64_t gs_round_state_bytes(const gs_camera* cam, const gs_partition* part, const gs_sample_settings* ss) {
    if (!cam || !part || !ss || ss->batch_size == 0 || ss->max_samples < ss->batch_size) return -1;
    const int64_t cap = gs_partition_capacity(cam, part);
    const uint64_t R = (uint64_t)ss->max_samples / ss->batch_size + 1u;
    if (cap < 0 || cap >= (int64_t)0xFFFFFFFFll || R > kMaxRounds) return -1;
    return (int64_t)gs_round_layout((uint64_t)cap, R).bytes;
}

extern "C" gs_status gs_render_tiles_rounds_async(const gs_device_scene* ds, const gs_camera* cam,
                                                  const gs_sample_settings* ss, uint64_t seed,
                                                  const gs_partition* part, uint32_t first_round, uint32_t rounds,
                                                  void* d_state, int64_t state_bytes, const gs_round_outputs* out,
                                                  gs_counters* d_counters, void* stream) {
    gs_status e = check_rounds(ds, cam, ss, part, first_round, rounds, d_state, state_bytes, out, false);
    if (e != GS_OK) return e;
    return gs_render_tiles_rounds_timed_async(ds, cam, ss, seed, part, first_round, rounds, d_state, state_bytes, out,
                                              d_counters, stream, nullptr, nullptr, false, false);
}

int64_t gs_pass_delta_blocks(int64_t capacity) {
    return capacity <= 0 || capacity >= 0xFFFFFFFFll ? 1 : (int64_t)gs_accum_blocks((uint32_t)capacity);
}

// ---------------------------------------------------------------- the work plan
// How a launch's samples are cut into work items.
struct WorkPlan {
    // Sample chunks (single-batch settings; KParams::chunk): chunk == 0 is one item per pixel
    uint32_t chunk = 0, cpp = 1;
    // Guided tail: the packed pixels from fine_px on run in fine_chunk-sample items (fine_px ==
    // the capacity: no tail)
    uint32_t fine_px = 0, fine_chunk = 1, fine_cpp = 1;
    // Batch rounds (adaptive settings): n_rounds != 0, in n_segs segments of at most seg_px pixels
    uint32_t n_rounds = 0, seg_px = 0, n_segs = 0;
    uint32_t n_items(uint32_t cap) const { return fine_px * cpp + (cap - fine_px) * fine_cpp; }
};

// What the frame's bits depend on (round 6): a pixel's
// colour is ((0 + C_0) + C_1) + ... over its chunks of c samples, each C_k = ((0 + s) + s)
// + ... in sample order, so the association is fixed by c alone -- and c is a function of
// the frame (W x H), the settings, the scene's flags and the process's knobs: never of the
// rank's capacity, the device count, the device's CUs or a timing.  How the samples are
// cut into work items is scheduling: the guided tail's 1-sample items (gs_combine_kernel
// re-forms their chunks of c: a 1-sample chunk sum is 0 + s = s, bit for bit, so the
// regrouped sum is the coarse chunk's) may sit on any tiles, sized by the rank's capacity,
// this device's lanes and the scene's measured cost, without changing a bit.
// This function's parameters are that rule: it sees nothing else.
struct CoarseChunk {
    uint32_t c;
    bool small;  // the small-frame rule applied (such a frame takes no tail while its samples are short)
};
static CoarseChunk coarse_chunk(uint64_t frame_px, const gs_sample_settings& ss, int feat, const Knobs& k) {
    const uint32_t bs = ss.batch_size;
    uint32_t c = k.sample_chunk > 0 ? (uint32_t)k.sample_chunk : std::max<uint32_t>(16u, (bs + 63u) / 64u);
    if ((bs + c - 1) / c > 64u) c = (bs + 63u) / 64u;  // at most 64 chunks per pixel
    if (k.sample_chunk < 0)  // (the whole frame's sums: the same c on every rank)
        while (c < bs && frame_px * ((bs + c - 1) / c) * 24u > k.partial_budget) c *= 2u;
    // A small frame -- at most twice the default tail's samples on a 256-CU device -- of a
    // scene whose samples are alike (no media, no BVHs under instances, no staged shading)
    // runs in chunks of 4 samples: there the items' fixed costs (claims, refills, chunk
    // sums) outweigh the last chunk's length.  MI355X C1 (400x225 x 100 spp, earth + sky):
    // 16-sample chunks with a 2-sample tail on 21 of 28 tiles 14 727, a 4-sample tail 16 579,
    // every tile in 4-sample chunks 18 104 Msamples/s; 3, 5, 6 samples 15 977-17 205
    // (profiles/r05/sweep_C1_guided_tail*.txt).  (A fixed lane count, not this device's:
    // the chunk size is part of what the bits depend on.)
    const bool simple = (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_MIXED)) == 0;
    const bool small = k.sample_chunk < 0 && k.tail_pct == 0 && simple &&
                       frame_px * bs <= 4ull * (256ull * GS_BLOCK) * std::min(c, bs);
    if (small) c = std::min<uint32_t>(4u, c);
    if (k.sample_chunk < 0 || k.tail_pct > 0) c = std::min(c, bs);  // (where a tail may follow)
    return CoarseChunk{c, small};
}

// Guided tail: a work item of c samples started just before the queue runs dry
// can keep its lane busy for c samples while every other lane idles, and a frame
// with few items per lane ends on them (MI355X final_scene 400x400 x 64 spp,
// every pixel in chunks of 16: 211 Msamples/s; of 1: 1007).  So the rank's last
// tiles in queue order run in 1-sample items: enough tiles for 2 x lanes x c
// samples, which keeps the other lanes busy while the last coarse items finish.
// A small frame (above) takes no tail while its samples are short: once a frame of
// the scene measured more than GS_SHORT_SAMPLE_LANE_US lane-microseconds a sample
// (the frame context, gs_device_scene_note_frame; sticky) it takes the tail too.
// 400-px reference scenes, tail off / on (profiles/r05/small_frame_rule_scenes.txt),
// Msamples/s: earth 17 317 / 8 725, hdri 13 956 / 7 100, triangles 14 582 / 8 465,
// quads 13 402 / 11 088 (17-34 lane-us a sample) -- but checkered_spheres 10 523 /
// 14 047, cornell_box 8 272 / 8 918, perlin_spheres 1 524 / 3 320, simple_light
// 1 056 / 2 762 (77-391 lane-us: their last 4-sample items drag the frame).  Being
// scheduling only, neither the timing nor the device's lanes change a bit.
// Sets the plan's fine region for the coarse chunk `cc`, which it cannot alter.
static void guided_tail(const CoarseChunk cc, uint32_t bs, uint32_t cap, uint64_t tile_px, uint64_t lanes,
                        bool long_samples, const Knobs& k, WorkPlan& w) {
    const uint32_t c = cc.c;
    const uint64_t slots = (uint64_t)cap / tile_px;
    const bool short_samples = !long_samples;
    if (c > 1 && slots > 0 && !(cc.small && short_samples)) {
        const uint64_t want = lanes * c * (uint64_t)(k.tail_pct > 0 ? k.tail_pct : 200) / 100u;  // samples
        const uint64_t ft = std::min<uint64_t>(slots, (want + tile_px * bs - 1) / (tile_px * bs));
        const uint32_t fpx = (uint32_t)((slots - ft) * tile_px);
        const uint64_t items = (uint64_t)fpx * ((bs + c - 1) / c) + ((uint64_t)cap - fpx) * bs;
        if (items * 24u <= k.partial_budget && items < 0xFFFFFFFFull) {
            w.fine_px = fpx;
            w.fine_chunk = 1;
            w.fine_cpp = bs;
        }
    }
}

// The plan for a launch of `cap` packed pixels.  lanes, long_samples: this device's lanes and
// the scene's measured cost, which only the guided tail reads.  allow_rounds: the launch has
// no per-item visit output (batch rounds do not fill it).
static WorkPlan plan_work(const gs_camera& cam, const gs_sample_settings& ss, const gs_partition& part, uint32_t cap,
                          int feat, const Knobs& k, uint64_t lanes, bool long_samples, bool allow_rounds) {
    WorkPlan w;
    w.fine_px = cap;
    // Split pixels into sample chunks only when the settings run exactly one batch:
    // max_samples < batch_size makes the first stop test (camera.rs:158) always true.
    if (k.sample_chunk != 0 && ss.max_samples < ss.batch_size) {
        const uint32_t bs = ss.batch_size;
        const uint64_t frame_px = (uint64_t)cam.image_width * (uint64_t)cam.image_height;
        const CoarseChunk cc = coarse_chunk(frame_px, ss, feat, k);
        if (k.sample_chunk < 0 || k.tail_pct > 0)  // (an explicit chunk with a tail: gs_debug_set_guided_tail)
            guided_tail(cc, bs, cap, (uint64_t)part.tile_w * part.tile_h, lanes, long_samples, k, w);
        if (cc.c < bs || w.fine_px < cap) {
            w.chunk = cc.c;
            w.cpp = (bs + cc.c - 1) / cc.c;
        }
    }
    if ((uint64_t)w.fine_px * w.cpp + ((uint64_t)cap - w.fine_px) * w.fine_cpp >= 0xFFFFFFFFull)
        w.chunk = 0, w.cpp = 1, w.fine_px = cap, w.fine_cpp = 1;
    if (!w.chunk) w.fine_px = cap, w.fine_chunk = 1, w.fine_cpp = 1;
    // Adaptive settings (more than one batch) in batch rounds: rounds = the most batches a
    // pixel can run (the loop ends once sample_count > max_samples, camera.rs:162), in
    // segments of at most seg_px active pixels whose per-sample colours fit the budget.
    if (k.adaptive_rounds && k.sample_chunk != 0 && ss.max_samples >= ss.batch_size && allow_rounds) {
        const uint64_t R = (uint64_t)ss.max_samples / ss.batch_size + 1u;
        const uint64_t sp = std::min<uint64_t>((uint64_t)cap, k.partial_budget / ((uint64_t)ss.batch_size * 24u));
        const bool want = k.adaptive_rounds == 2 || R * ss.batch_size >= GS_ROUND_MIN_CAP;
        if (want && R <= kMaxRounds && sp >= 1 && sp * ss.batch_size < 0x7FFFFFFFull) {
            w.n_rounds = (uint32_t)R;
            w.seg_px = (uint32_t)sp;
            w.n_segs = (uint32_t)(((uint64_t)cap + sp - 1) / sp);
            w.chunk = 0;  // (the adaptive lane layout: whole-batch rounds keep Σlum, Σlum², the count)
            w.cpp = 1;
            w.fine_px = cap, w.fine_chunk = 1, w.fine_cpp = 1;
        }
    }
    return w;
}

// The plan for a progressive pass: always chunked, the coarse chunk `c` as the caller gave it
// (coarse_chunk's frame- and size-dependent rules do not apply: every pass of the frame must
// cut its samples the same way).  The guided tail, being scheduling only, is sized as usual;
// a small frame of a simple scene takes none while its samples are short (coarse_chunk's
// small-frame rule, here deciding the tail alone).
static WorkPlan plan_pass(const gs_camera& cam, uint32_t bs, const gs_partition& part, uint32_t cap, uint32_t c,
                          int feat, const Knobs& k, uint64_t lanes, bool long_samples) {
    WorkPlan w;
    w.fine_px = cap;
    w.chunk = c;
    w.cpp = bs / c;
    const uint64_t frame_px = (uint64_t)cam.image_width * (uint64_t)cam.image_height;
    const bool simple = (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_MIXED)) == 0;
    const bool small = k.tail_pct == 0 && simple && frame_px * bs <= 4ull * (256ull * GS_BLOCK) * c;
    guided_tail(CoarseChunk{c, small}, bs, cap, (uint64_t)part.tile_w * part.tile_h, lanes, long_samples, k, w);
    if ((uint64_t)w.fine_px * w.cpp + ((uint64_t)cap - w.fine_px) * w.fine_cpp >= 0xFFFFFFFFull)
        w.fine_px = cap, w.fine_chunk = 1, w.fine_cpp = 1;
    return w;
}

// The coarse chunk of a one-shot fixed-spp render of `cam`'s own frame: plan_work's, with a
// render that leaves its pixels whole (c >= samples, or the never-split knob) as one chunk.
extern "C" uint32_t gs_views_chunk(const gs_device_scene* ds, const gs_camera* cam, uint32_t samples) {
    if (!cam || samples == 0 || cam->image_width <= 0 || cam->image_height <= 0) {
        (void)fail(GS_ERR_ARG, "bad argument");
        return 0;
    }
    const Knobs k = read_knobs();
    if (k.sample_chunk == 0) return samples;
    const gs_sample_settings ss{0.0, 0.0, samples, 0};
    const uint64_t frame_px = (uint64_t)cam->image_width * (uint64_t)cam->image_height;
    // (no scene: the rule for one whose samples are alike -- no media, BVHs under instances or staged shading)
    return std::min(coarse_chunk(frame_px, ss, ds ? ds->feat : 0, k).c, samples);
}

// ---------------------------------------------------------------- the launch shape
// The launch shape of one instantiation (gs_device_scene::lcfg; lc.want, lc.views_round and
// lc.chunked say which): the mirror takes what the block's LDS limit leaves after the launched
// kernel's static LDS and its lane state (any prefix of either record array is a valid mirror).
// The lane state is the launched kernel's own -- none in LDS for the fixed-spp sphere-leaf
// kernels (lane_state_in_regs), while the loop's kernel of the same scene keeps its fields
// there -- so the static-LDS check, the lane bytes and the occupancy all ask that kernel.
static gs_status fit_mirror(gs_device_scene* ds, int dev, gs_device_scene::LaunchCfg& lc) {
    HIPCHK(hipDeviceGetAttribute(&ds->cus, hipDeviceAttributeMultiprocessorCount, dev));
    int max_lds = 0;
    HIPCHK(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    const bool chunked = lc.chunked;
    // (a views round's table has exact entries only: the word is the instantiation's own)
    auto kernel = [&](int f) { return lc.views_round ? views_round_kernel_for(f) : kernel_for(f); };
    auto own_feat = [&](int f) { return lc.views_round ? f : kernel_feat(f); };
    // Without GS_FEAT_LDSTREE the launch takes another instantiation: fitted again should that
    // one's lane state differ (none of the product kernels' does: the layout ignores the flag).
    for (int f = lc.want;;) {
        void (*kn)(KArgs) = kernel(f);
        if (!kn) return fail(GS_ERR_UNSUPPORTED, "no views form of the scene's round kernel in this build");
        const int kf = own_feat(f);
        hipFuncAttributes fa{};
        HIPCHK(hipFuncGetAttributes(&fa, (const void*)kn));
        // The node mirror must start at LDS address 0 (load_tnode): no static LDS.
        if (fa.sharedSizeBytes != 0) return fail(GS_ERR_UNSUPPORTED, "render kernel with static LDS");
        MirrorPrefix m = ds->mirror;
        // (the nested walk's save slots too, when they displace no mirror record; else they
        // stay in global memory: final_scene, whose mirror wants more than the 24 KiB the
        // slots would leave, lost 5% with them in LDS -- profiles/r06/ab_nest_save_lds.txt)
        uint32_t nsave = nest_save_lds(kf);
        if ((int64_t)max_lds - (int64_t)lane_lds_bytes(chunked, kf, nsave) < m.bytes()) nsave = 0;
        const int64_t room = (int64_t)max_lds - (int64_t)lane_lds_bytes(chunked, kf, nsave);
        if (room < 0) return fail(GS_ERR_UNSUPPORTED, "lane state exceeds the device's LDS per block");
        // shrink the least valuable prefix first: cubes, quads, then all
        while (m.bytes() > room && m.cubes) m.cubes = m.cubes - 1 - m.cubes / 16;
        while (m.bytes() > room && m.quads) m.quads = m.quads - 1 - m.quads / 16;
        while (m.bytes() > room) {
            if (m.nodes) m.nodes = m.nodes - 1 - m.nodes / 16;  // shrink the prefixes until they fit
            if (m.leaves) m.leaves = m.leaves - 1 - m.leaves / 16;
        }
        int f2 = f;
        if (m.nodes < ds->node_records || m.leaves < ds->leaf_records) f2 &= ~GS_FEAT_LDSTREE;
        if (f2 != f && kernel(f2) &&
            (lane_lds_bytes(chunked, own_feat(f2), nest_save_lds(own_feat(f2))) != lane_lds_bytes(chunked, kf, nest_save_lds(kf)))) {
            f = f2;
            continue;
        }
        lc.mirror = m;
        lc.lds = lane_lds_bytes(chunked, kf, nsave) + (size_t)m.bytes();
        lc.nest_lds = nsave;
        lc.lane_nd = lane_nd(chunked, kf) + nsave;
        lc.feat = f2;
        break;
    }
    void (*kn)(KArgs) = kernel(lc.feat);
    if (!kn) return fail(GS_ERR_UNSUPPORTED, "no views form of the scene's round kernel in this build");
    int occ = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)kn, GS_BLOCK, lc.lds));
    lc.per_cu = occ < 1 ? 1 : (occ > 8 ? 8 : occ);
    return GS_OK;
}

// The shape for a launch of `want` (cached per scene; the caller holds the scene's mutex).
static gs_status launch_shape(gs_device_scene* ds, int dev, int want, bool views_round, bool chunked,
                              const gs_device_scene::LaunchCfg** out) {
    for (const auto& c : ds->lcfg)
        if (c.want == want && c.views_round == views_round && c.chunked == chunked) {
            *out = &c;
            return GS_OK;
        }
    gs_device_scene::LaunchCfg lc;
    lc.want = want;
    lc.views_round = views_round;
    lc.chunked = chunked;
    gs_status e = fit_mirror(ds, dev, lc);
    if (e != GS_OK) return e;
    ds->lcfg.push_back(lc);
    *out = &ds->lcfg.back();
    return GS_OK;
}

// What a launch was asked for (the arguments of gs_render_tiles_timed_async, checked).
struct LaunchReq {
    const gs_camera* cam;
    const gs_sample_settings* ss;
    uint64_t seed;
    const gs_partition* part;
    const gs_render_outputs* outs;
    gs_counters* d_counters;
    const VisitArgs* va;
    bool direct, zero_counters;
    uint32_t cap;  // packed pixel slots of this rank (gs_partition_capacity)
};

// The launch's parameter block for a grid of `blocks` blocks: everything but the slot's
// buffers (bind_slot).
static KParams fill_params(const gs_device_scene* ds, const LaunchReq& q, const WorkPlan& w, int64_t blocks) {
    const gs_camera* cam = q.cam;
    const gs_partition* part = q.part;
    KParams kp{};
    kp.sc = ds->dev;
    kp.cam = *cam;
    kp.ss = *q.ss;
    kp.seed = q.seed;
    kp.rank = part->rank;
    kp.world_size = part->world_size;
    kp.tile_w = part->tile_w;
    kp.tile_h = part->tile_h;
    kp.tiles_x = (cam->image_width + part->tile_w - 1) / part->tile_w;
    kp.capacity = q.cap;
    kp.order = part->d_tile_order;
    kp.per_sample = w.n_rounds ? 1u : 0u;
    kp.rounds = w.n_rounds ? 1u : 0u;
    kp.chunk = w.chunk;
    kp.cpp = w.cpp;
    kp.fine_px = w.fine_px;
    kp.fine_base = w.fine_px * w.cpp;
    kp.fine_chunk = w.fine_chunk;
    kp.fine_cpp = w.fine_cpp;
    kp.n_items = w.n_items(q.cap);
    kp.u_cpp = gsd::udiv_make(w.cpp);
    kp.u_fcpp = gsd::udiv_make(w.fine_cpp);
    kp.u_tpx = gsd::udiv_make((uint32_t)(part->tile_w * part->tile_h));
    kp.u_bpr = gsd::udiv_make(std::max<uint32_t>(1, (uint32_t)part->tile_w >> 3));
    kp.u_tw = gsd::udiv_make((uint32_t)part->tile_w);
    kp.u_tx = gsd::udiv_make((uint32_t)kp.tiles_x);
    kp.u_w = gsd::udiv_make((uint32_t)cam->image_width);
    kp.out = q.outs->rgb;
    kp.out8 = q.outs->rgb8;
    kp.direct = q.direct ? 1u : 0u;
    kp.zero_counters = q.zero_counters && q.d_counters ? 1u : 0u;
    kp.counters = (unsigned long long*)q.d_counters;
    kp.item_visits = q.outs->item_visits;
    kp.visits = q.va ? q.va->visits : nullptr;
    kp.visit_leaf_base = q.va ? q.va->leaf_base : 0u;
    // Items per queue claim: about 1/8 of a wave's share of the items, at most 32 (a wave
    // ends holding at most one partly used reserve), at least 1.
    const uint64_t waves = (uint64_t)blocks * (GS_BLOCK / 64);
    kp.waves = (uint32_t)waves;
    kp.lanes = (uint32_t)(blocks * GS_BLOCK);
    // (coarse items of at most 4 samples -- a small frame's chunks -- claim like the tail's: the
    // one queue counter serialises claims of 32; MI355X C1, 4-sample items: 32 -> 1.15 ms, 128 ->
    // 0.57 ms a frame)
    const uint64_t claim_cap = kp.chunk && kp.chunk <= 4u ? (uint64_t)GS_CLAIM_FINE : 32u;
    kp.claim = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(claim_cap, (uint64_t)kp.n_items / waves / GS_CLAIM_DIV));
    kp.claim_fine = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(GS_CLAIM_FINE, (uint64_t)kp.n_items / waves / GS_CLAIM_DIV));
    return kp;
}

// The hot kernel arguments (P: the slot's parameter block, set by the caller).
static KArgs fill_args(const gs_device_scene* ds, const gs_device_scene::LaunchCfg& lc, const Knobs& k) {
    KArgs a{};
    a.tnodes = ds->dev.tnodes;
    a.tboxes = ds->dev.tboxes;
    a.tleaves = ds->dev.tleaves;
    a.tquads = ds->tquads;
    a.root = ds->thr_root;
    a.cert_boxes = ds->cert_boxes ? 1 : 0;
    a.shade_batch = k.shade_batch > 0 ? k.shade_batch : ds->shade_batch;
    a.leaf_batch = std::max<int32_t>(1, k.leaf_batch > 0 ? k.leaf_batch : ds->leaf_batch);  // (0 would never step a node)
    a.node_steps = launch_node_steps(ds, k);
    a.cam_batch = std::max<int32_t>(1, k.cam_batch > 0 ? k.cam_batch : ds->cam_batch);
    a.lds_nodes = lc.mirror.nodes;
    a.lds_leaves = lc.mirror.leaves;
    a.lds_quads = lc.mirror.quads;
    a.lds_cubes = lc.mirror.cubes;
    a.cubes = ds->dev.cubes;
    a.lane_nd = lc.lane_nd;
    a.nest_lds = lc.nest_lds;
    return a;
}

// ---------------------------------------------------------------- launch slots
// This launch's slot.  A slot whose last launch ran on this very stream is reused first:
// stream order already puts the new launch behind the old one, so one caller on one
// stream keeps one slot (and one chunk-sum buffer) however many launches it queues.
// Otherwise a slot whose launch has finished, preferring one whose chunk sums are big
// enough; otherwise the next in turn, behind a stream wait on its previous launch.
static int pick_slot(gs_device_scene* ds, hipStream_t st, size_t need_partial) {
    for (int k = 0; k < kLaunchSlots; k++)
        if (ds->slots[k].used && ds->slots[k].stream == st) return k;
    int idle = -1;
    for (int k = 0; k < kLaunchSlots; k++) {
        LaunchSlot& c = ds->slots[k];
        if (c.used && hipEventQuery(c.done) != hipSuccess) continue;
        if (c.partial_bytes >= need_partial) return k;
        if (idle < 0) idle = k;
    }
    return idle >= 0 ? idle : (int)(ds->next_slot++ % kLaunchSlots);
}

// Grows one of a slot's device buffers to `need` bytes (contents are not kept); `what` names
// it in the error text.  *grew (nullable) is set when a new buffer was allocated.
template <class T>
static gs_status grow_buffer(LaunchSlot& sl, T*& buf, size_t& have, size_t need, const char* what, bool* grew = nullptr) {
    if (have >= need) return GS_OK;
    if (sl.used) HIPCHK(hipEventSynchronize(sl.done));  // nothing in flight reads it
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    have = 0;
    if (hipMalloc((void**)&buf, need) != hipSuccess)
        return fail(GS_ERR_OOM, "hipMalloc of " + std::to_string(need) + " bytes of " + what + " failed");
    have = need;
    if (grew) *grew = true;
    return GS_OK;
}

// Sizes the slot's buffers for the launch and points the parameter block at them.
// (own_rounds: the round state is the slot's; a progressive adaptive pass brings its own)
static gs_status bind_slot(LaunchSlot& sl, hipStream_t st, const WorkPlan& w, int feat, int64_t blocks, size_t need_partial, KParams& kp,
                           bool own_rounds = true) {
    if (w.chunk || w.n_rounds) {
        gs_status e = grow_buffer(sl, sl.partial, sl.partial_bytes, need_partial, "chunk sums");
        if (e != GS_OK) return e;
        kp.partial = sl.partial;
    }
    // batch rounds: [item-size hint, round counts][active list 0][active list 1][running sums],
    // 256-B aligned (the hint first: it outlives launches of other settings)
    if (w.n_rounds && own_rounds) {
        const size_t cap = kp.capacity;
        const size_t r_counts = ((size_t)(w.n_rounds + 2) * 4 + 16 + 255) & ~(size_t)255;
        const size_t r_list = (cap * 4 + 255) & ~(size_t)255;
        bool grew = false;
        gs_status e = grow_buffer(sl, sl.rbuf, sl.rbuf_bytes, r_counts + 2 * r_list + cap * 5 * sizeof(double),
                                  "batch-round state", &grew);
        if (e != GS_OK) return e;
        if (grew) HIPCHK(hipMemsetAsync(sl.rbuf, 0, 16, st));  // no item-size hint yet
        uint8_t* rb = (uint8_t*)sl.rbuf;
        kp.rpp_hint = (unsigned long long*)rb;
        kp.round_counts = (uint32_t*)(rb + 16);
        kp.active_buf[0] = (uint32_t*)(rb + r_counts);
        kp.active_buf[1] = (uint32_t*)(rb + r_counts + r_list);
        kp.pstate = (double*)(rb + r_counts + 2 * r_list);
    }
    if (feat & GS_FEAT_NESTED) {  // (and the pilot's instantiation, which has every path)
        gs_status e = grow_buffer(sl, sl.nest_save, sl.nest_save_bytes, (size_t)blocks * GS_BLOCK * 64u,
                                  "nested-walk save slots");
        if (e != GS_OK) return e;
        kp.nest_save = sl.nest_save;
    }
    kp.queue = sl.queue;
    return GS_OK;
}

// ---------------------------------------------------------------- the launches
#ifndef GS_USE_RSPLIT
#define GS_USE_RSPLIT 1  // (A/B: 0 runs split rounds on the generic instantiation)
#endif
#ifndef GS_USE_FIXED
#define GS_USE_FIXED 1  // (A/B: 0 launches the generic instantiation for fixed-spp frames too)
#endif
// The instantiation a launch asks for, from the scene's feature set `sf` (the shape then drops
// GS_FEAT_LDSTREE where the mirror is a strict prefix, fit_mirror).  It is chosen before the shape,
// because the shape follows it: the lane state, and with it the mirror, differs between a scene's
// loop kernel and its fixed-spp forms.
static int launch_word(int sf, const WorkPlan& w, const Knobs& k, const LaunchReq& r, bool round_pass, bool views) {
    if (round_pass) {
        // A progressive adaptive pass: always split items; paths that always trace a camera ray
        // take the fixed kernel's sample loop (GS_FEAT_RSPLIT).  (views: a views adaptation's pass,
        // in the views form of the round's kernel -- every view's max_depth > 0 -- views_round_kernel_for)
        const bool rsplit = GS_USE_RSPLIT && has_rsplit(sf) && r.cam->max_depth > 0;
        return (rsplit ? sf | GS_FEAT_FIXED | GS_FEAT_RSPLIT : sf) | (views ? GS_FEAT_VIEWS : 0);
    }
    if (w.n_rounds) {
        // Rounds whose items are surely split (gs_round_params_kernel: a requested chunk, a batch
        // above GS_ROUND_WHOLE_MAX_BATCH, or whole-batch items off -- the default) and whose
        // paths always trace a camera ray take the fixed kernel's sample loop too.
        const bool rsplit = GS_USE_RSPLIT && has_rsplit(sf) && r.cam->max_depth > 0 &&
                            (k.sample_chunk > 0 || r.ss->batch_size > GS_ROUND_WHOLE_MAX_BATCH || k.round_whole == 0);
        return rsplit ? sf | GS_FEAT_FIXED | GS_FEAT_RSPLIT : sf;
    }
    // (a views launch: always chunked, every view's max_depth > 0 -- the fixed kernel's views form)
    if (views) return sf | GS_FEAT_FIXED | GS_FEAT_VIEWS;
    if (r.va) return GS_FEAT_PILOT;
    // (a fixed-spp chunked launch takes the instantiation without the adaptive paths)
    const bool fixed = GS_USE_FIXED && w.chunk != 0 && r.cam->max_depth > 0;
    return sf | (fixed ? GS_FEAT_FIXED : 0);
}

// What the enqueue steps share: the stream, the grid and the timing events.
struct Enqueue {
    hipStream_t st;
    unsigned blocks;
    size_t lds;
    int feat;  // the word to launch: the shape's instantiation (LaunchCfg::feat)
    hipEvent_t k_begin, k_end;
    const gs_device_scene* ds;
    // kernel_for(f), noted for gs_debug_last_launch_feat
    void (*kernel(int f) const)(KArgs) {
        ds->last_launch_feat.store(f);
        return kernel_for(f);
    }
    // views_round_kernel_for(f), noted likewise when it exists
    void (*views_round_kernel(int f) const)(KArgs) {
        void (*kn)(KArgs) = views_round_kernel_for(f);
        if (kn) ds->last_launch_feat.store(f);
        return kn;
    }
};

// Batch rounds: init (every real packed pixel active), then per round and segment: parameters,
// the megakernel, the combine; all on the stream, no host synchronisation (a segment
// or round with no active pixel left launches and exits at once).
static gs_status enqueue_rounds(const Enqueue& q, const WorkPlan& w, const Knobs& k, const LaunchReq& r,
                                const KParams& kp, KParams* dP, const KArgs& a) {
    const hipStream_t st = q.st;
    HIPCHK(hipMemsetAsync(kp.round_counts, 0, (size_t)(w.n_rounds + 1) * 4, st));
    const unsigned g_init = (unsigned)std::min<int64_t>(((int64_t)r.cap + 255) / 256, 8192);
    HIPCHK(launch_round_init_kernel(st, g_init, dP));
    if (q.k_begin) HIPCHK(hipEventRecord(q.k_begin, st));
    const unsigned g_comb = (unsigned)std::min<int64_t>((w.seg_px + 255) / 256, 8192);
    void (*rkern)(KArgs) = q.kernel(q.feat);  // (launch_word: the split-round form where it applies)
    for (uint32_t rd = 0; rd < w.n_rounds; rd++)
        for (uint32_t sg = 0; sg < w.n_segs; sg++) {
            HIPCHK(launch_round_params_kernel(st, dP, rd, sg, w.seg_px, k.sample_chunk, k.round_whole));
            HIPCHK(launch_render_kernel(st, rkern, q.blocks, q.lds, a));
            HIPCHK(launch_round_combine_kernel(st, g_comb, dP, rd));
        }
    if (q.k_end) HIPCHK(hipEventRecord(q.k_end, st));
    return GS_OK;
}

// A progressive adaptive pass: enqueue_rounds over rounds [first_round, first_round + rounds) of
// the caller's state -- round_counts[first_round] is read on the device, so nothing here waits
// for an earlier pass -- always in split items (whole-batch items take the stop test in the
// megakernel, which does not write the persistent state), the fold in the combine's place;
// then the resolve over every packed pixel.
// views: a views adaptation's pass -- the same rounds on the tall frame, in the views form of the
// round's kernel (views_round_kernel_for; every view's max_depth > 0), which has no fallback.
static gs_status enqueue_round_pass(const Enqueue& q, const WorkPlan& w, const Knobs& k, const LaunchReq& r,
                                    const RoundArgs& ra, const KParams& kp, KParams* dP, const KArgs& a, bool views) {
    const hipStream_t st = q.st;
    void (*rkern)(KArgs) = views ? q.views_round_kernel(q.feat) : q.kernel(q.feat);
    if (!rkern) return fail(GS_ERR_UNSUPPORTED, "no views form of the scene's round kernel in this build");
    if (ra.first_round == 0 && ra.rounds) {
        const unsigned g_init = (unsigned)std::min<int64_t>(((int64_t)r.cap + 255) / 256, 8192);
        HIPCHK(launch_round_init_kernel(st, g_init, dP));
    }
    if (q.k_begin) HIPCHK(hipEventRecord(q.k_begin, st));
    const unsigned g_fold = (unsigned)std::min<int64_t>((w.seg_px + 255) / 256, 8192);
    for (uint32_t rd = ra.first_round; rd < ra.first_round + ra.rounds; rd++)
        for (uint32_t sg = 0; sg < w.n_segs; sg++) {
            HIPCHK(launch_round_params_kernel(st, dP, rd, sg, w.seg_px, k.sample_chunk, 0));
            HIPCHK(launch_render_kernel(st, rkern, q.blocks, q.lds, a));
            HIPCHK(launch_round_fold_kernel(st, g_fold, dP, rd));
        }
    if (q.k_end) HIPCHK(hipEventRecord(q.k_end, st));
    HIPCHK(hipMemsetAsync(kp.round_summary, 0, GS_ROUND_SUMMARY_WORDS * 8, st));
    HIPCHK(launch_round_resolve_kernel(st, dP, r.cap));
    return GS_OK;
}

// One megakernel launch, then the chunk combine when the pixels' samples were split.
static gs_status enqueue_frame(const Enqueue& q, const WorkPlan& w, const LaunchReq& r, const KParams* dP,
                               const KArgs& a, bool pass, bool views) {
    if (q.k_begin) HIPCHK(hipEventRecord(q.k_begin, q.st));
    HIPCHK(launch_render_kernel(q.st, q.kernel(q.feat), q.blocks, q.lds, a));
    if (q.k_end) HIPCHK(hipEventRecord(q.k_end, q.st));
    if (pass && views) {  // (a progressive views pass: one block per tile slot)
        HIPCHK(launch_views_accumulate_kernel(q.st, dP, r.cap / (uint32_t)(r.part->tile_w * r.part->tile_h)));
    } else if (pass) {  // (always chunked: the pass's sums join the frame's)
        HIPCHK(launch_accumulate_kernel(q.st, dP, r.cap));
    } else if (w.chunk) {
        const unsigned grid = (unsigned)std::min<int64_t>(((int64_t)r.cap + 255) / 256, 8192);
        HIPCHK(launch_combine_kernel(q.st, grid, dP));
    }
    return GS_OK;
}

// The launch behind gs_render_tiles_ex_async; k_begin / k_end (nullable, timing events of
// the stream's device) are recorded right around the megakernel, so a caller can time the
// dominant kernel alone (csrc/host/internal.hpp; the frame context's gs_stats.kernel_ms).
static gs_status launch(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                        const gs_partition* part, const gs_render_outputs* outs, gs_counters* d_counters, void* stream,
                        hipEvent_t k_begin, hipEvent_t k_end, const VisitArgs* va, bool direct, bool zero_counters,
                        const PassArgs* pass, const RoundArgs* ra, const ViewsArgs* vw) {
    if (!ds || !cam || !ss || !part || !outs || (!outs->rgb && !outs->rgb8)) return fail(GS_ERR_ARG, "null argument");
    if (!part_ok(cam, part)) return fail(GS_ERR_ARG, "bad partition / image size");
    if (ss->batch_size == 0) return fail(GS_ERR_ARG, "batch_size 0 never terminates (camera.rs:137)");
    const int64_t cap = gs_partition_capacity(cam, part);
    const hipStream_t st = (hipStream_t)stream;
    if (cap <= 0) {  // nothing to render; a frame context's counters still start from zero
        if (zero_counters && d_counters) HIPCHK(hipMemsetAsync(d_counters, 0, sizeof(gs_counters), st));
        if (ra) HIPCHK(hipMemsetAsync(ra->d_state + gs_round_layout(0, ra->R).summary, 0, GS_ROUND_SUMMARY_WORDS * 8, st));
        if (k_begin) HIPCHK(hipEventRecord(k_begin, st));  // (a caller times an empty kernel span)
        if (k_end) HIPCHK(hipEventRecord(k_end, st));
        return GS_OK;
    }
    if (cap >= (int64_t)0xFFFFFFFFll) return fail(GS_ERR_ARG, "partition too large");
    if ((int64_t)cam->image_width * cam->image_height >= (int64_t)0xFFFFFFFFll)
        return fail(GS_ERR_ARG, "image too large for 32-bit pixel ids");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev != ds->device) return fail(GS_ERR_ARG, "scene lives on another device");
    const LaunchReq req{cam, ss, seed, part, outs, d_counters, va, direct, zero_counters, (uint32_t)cap};
    const Knobs k = read_knobs();  // (the one read of the process knobs for this launch)
#if defined(GS_STAMPS) || defined(GS_CERT_CHECK)
    const bool visit_out = false;  // (those builds' item_visits is their record buffer: rounds allowed)
#else
    const bool visit_out = outs->item_visits != nullptr;
#endif
    const uint64_t lanes = (uint64_t)std::max(1, device_cus(dev)) * GS_BLOCK;
    const bool long_samples = ds->long_samples.load(std::memory_order_relaxed);
    // (a views launch: a pass's plan on the tall frame -- always chunked, the chunk as given)
    WorkPlan w;
    if (ra) {  // always batch rounds, whatever gs_set_adaptive_mode and the sample chunk say (plan_work's layout)
        w.n_rounds = ra->R;
        w.seg_px = (uint32_t)round_seg_px(req.cap, *ss, k);
        if (w.seg_px < 1) return fail(GS_ERR_ARG, "one pixel's batch exceeds the partial budget");
        w.n_segs = (uint32_t)(((uint64_t)req.cap + w.seg_px - 1) / w.seg_px);
        w.fine_px = req.cap;
    } else if (pass || vw) {
        w = plan_pass(*cam, ss->batch_size, *part, req.cap, pass ? pass->chunk : vw->chunk, ds->feat, k, lanes, long_samples);
    } else {
        w = plan_work(*cam, *ss, *part, req.cap, ds->feat, k, lanes, long_samples, !visit_out && !va);
    }
    // (under the scene's mutex from here: the placement pilot's end rewrites the records,
    // the root and the mirror prefixes under it, pilot_end)
    gs_device_scene* mds = const_cast<gs_device_scene*>(ds);
    std::lock_guard<std::mutex> lock(mds->mu);
    if (vw && !(ra ? has_views_rounds(ds->feat) : has_views(ds->feat)))
        return fail(GS_ERR_UNSUPPORTED, "no views form of the scene's kernel");
    const gs_device_scene::LaunchCfg* lcp = nullptr;
    {
        const int want = launch_word(ds->feat, w, k, req, ra != nullptr, vw != nullptr);
        gs_status e = launch_shape(mds, dev, want, ra && vw, w.chunk != 0, &lcp);
        if (e != GS_OK) return e;
    }
    const gs_device_scene::LaunchCfg& lc = *lcp;
    const int per_cu = k.blocks_per_cu > 0 ? k.blocks_per_cu : lc.per_cu;
    int64_t blocks = (int64_t)ds->cus * per_cu;
    // no more waves than work: one lane per item at most (a round's items: at most one per sample)
    const int64_t max_blocks =
        ((int64_t)(w.n_rounds ? (uint64_t)w.seg_px * ss->batch_size : w.n_items(req.cap)) + GS_BLOCK - 1) / GS_BLOCK;
    if (blocks > max_blocks) blocks = max_blocks;
    if (k.max_blocks > 0 && blocks > k.max_blocks) blocks = k.max_blocks;  // (test hook: lanes that run many items in turn)
    if (blocks < 1) blocks = 1;
    KParams kp = fill_params(ds, req, w, blocks);
    if (pass) {
        kp.sample_base = pass->sample_base;
        kp.accum = pass->d_sums;
        kp.delta = pass->d_delta;
    }
    // The u32 queue counter runs past n_items by at most one claim per wave (each wave's
    // last, failed claim): it must not wrap.
    if ((uint64_t)std::max<uint64_t>(kp.n_items, (uint64_t)w.seg_px * ss->batch_size) +
            (uint64_t)std::max<uint32_t>(GS_CLAIM_FINE, std::max(kp.claim, kp.claim_fine)) * ((uint64_t)kp.waves + 1) >= 0xFFFFFFFFull)
        return fail(GS_ERR_ARG, "too many work items for the 32-bit work queue");

    const size_t need_partial = w.n_rounds ? (size_t)w.seg_px * ss->batch_size * 3 * sizeof(double)
                                : w.chunk  ? (size_t)kp.n_items * 3 * sizeof(double) : 0;
    LaunchSlot& sl = mds->slots[pick_slot(mds, st, need_partial)];
    if (sl.used && sl.stream != st) HIPCHK(hipStreamWaitEvent(st, sl.done, 0));
    gs_status e = bind_slot(sl, st, w, ds->feat, blocks, need_partial, kp, ra == nullptr);
    if (e != GS_OK) return e;
    if (ra) {
        const GsRoundLayout l = gs_round_layout(req.cap, ra->R);
        if (ra->first_round == 0 && ra->rounds) HIPCHK(hipMemsetAsync(ra->d_state, 0, l.bytes, st));  // (no hint, no counts, no sums)
        kp.rpp_hint = (unsigned long long*)(ra->d_state + l.hint);
        kp.round_summary = (unsigned long long*)(ra->d_state + l.summary);
        kp.round_counts = (uint32_t*)(ra->d_state + l.counts);
        kp.active_buf[0] = (uint32_t*)(ra->d_state + l.list[0]);
        kp.active_buf[1] = (uint32_t*)(ra->d_state + l.list[1]);
        kp.pstate = (double*)(ra->d_state + l.pstate);
        kp.pbatches = (uint32_t*)(ra->d_state + l.batches);
        kp.map_samples = ra->map_samples;
        kp.map_error = ra->map_error;
    }
    if (vw) {  // the views' records into the slot's array, behind the slot's previous launch on the stream
        e = grow_buffer(sl, sl.views, sl.views_bytes, (size_t)vw->n * sizeof(gs_view), "views");
        if (e != GS_OK) return e;
        for (uint32_t first = 0; first < vw->n; first += GS_VIEW_BATCH) {
            ViewBatch vb{};
            vb.first = first;
            vb.n = std::min<uint32_t>(GS_VIEW_BATCH, vw->n - first);
            std::memcpy(vb.v, vw->views + first, (size_t)vb.n * sizeof(gs_view));
            HIPCHK(launch_views_kernel(st, vb, sl.views));
        }
        kp.views = sl.views;
        kp.u_vpx = gsd::udiv_make((uint32_t)cam->image_width * (uint32_t)vw->views[0].cam.image_height);
    }
    // (a progressive views pass: the per-view records likewise, and room for the pass's own tile
    // order, which gs_views_order_kernel writes behind the parameter kernel)
    const uint32_t vp_pos = vw && vw->vstate ? req.cap / (uint32_t)(part->tile_w * part->tile_h) * (uint32_t)part->world_size : 0u;
    if (vp_pos) {
        e = grow_buffer(sl, sl.vstate, sl.vstate_bytes, (size_t)vw->n * sizeof(GsViewState), "view states");
        if (e == GS_OK) e = grow_buffer(sl, sl.vorder, sl.vorder_bytes, (size_t)vp_pos * sizeof(int32_t), "the pass's tile order");
        if (e != GS_OK) return e;
        for (uint32_t first = 0; first < vw->n; first += GS_VSTATE_BATCH) {
            ViewStateBatch vb{};
            vb.first = first;
            vb.n = std::min<uint32_t>(GS_VSTATE_BATCH, vw->n - first);
            std::memcpy(vb.s, vw->vstate + first, (size_t)vb.n * sizeof(GsViewState));
            HIPCHK(launch_view_state_kernel(st, vb, sl.vstate));
        }
        kp.vstate = sl.vstate;
        kp.vorder = part->d_tile_order;
        kp.order = sl.vorder;
        kp.vdelta = vw->d_vdelta;
    }
    KArgs a = fill_args(ds, lc, k);
    a.P = sl.params;
    if (outs->item_visits) HIPCHK(hipMemsetAsync(outs->item_visits, 0, (size_t)cap * sizeof(uint32_t), st));
    HIPCHK(launch_params_kernel(st, kp, sl.params));  // (zeroes the queue)
    if (vp_pos) HIPCHK(launch_views_order_kernel(st, sl.params, sl.vorder, vp_pos, (uint32_t)vw->views[0].cam.image_height));
    const Enqueue q{st, (unsigned)blocks, lc.lds, lc.feat, k_begin, k_end, ds};
    e = ra ? enqueue_round_pass(q, w, k, req, *ra, kp, sl.params, a, vw != nullptr)
        : w.n_rounds ? enqueue_rounds(q, w, k, req, kp, sl.params, a)
                     : enqueue_frame(q, w, req, sl.params, a, pass != nullptr, vw != nullptr);
    if (e != GS_OK) return e;
    HIPCHK(hipEventRecord(sl.done, st));
    sl.used = true;
    sl.stream = st;
    return GS_OK;
}

// Placement pilot.  Before a scene's first launch, when its threaded records do not all
// fit the LDS mirror: render the launch's camera at 1 spp on a grid of every k-th pixel
// (k chosen for ~64 k pilot pixels) with the GS_FEAT_VISITS instantiation, which counts
// the tests of every node and leaf record, then re-place the records by measured visits
// per byte (place_records) and upload them again.  The static estimate ranks records by
// geometry alone and misses where the camera's rays actually go (MI355X C4: its mirror
// served 90.8% of node visits and 50.2% of leaf tests; the measured order of the same
// bytes serves 99.6% and 96.0%, tools/visitmap.py).  Placement never changes a result
// (links are explicit), and the pilot is deterministic, so every device of a multi-GPU
// render places its copy identically.
// The pilot in two halves, so a multi-GPU frame issues every device's pilot before it waits
// for any (pilot_begin launches it on the stream, pilot_end waits, reads the counts back and
// re-places the records).
struct PilotRun {
    std::chrono::steady_clock::time_point t0;
    float* d_rgb = nullptr;
    uint32_t* d_vis = nullptr;
    hipStream_t st = nullptr;
    bool launched = false;
};

// The pilot's camera: every k-th pixel of the launch's (~64 k pixels), 1 spp.
static gs_camera pilot_camera(const gs_camera* cam) {
    const int64_t px = (int64_t)cam->image_width * cam->image_height;
    const int32_t k = std::max<int32_t>(1, (int32_t)std::sqrt((double)px / 65536.0));
    gs_camera pc = *cam;
    pc.image_width = (cam->image_width + k - 1) / k;
    pc.image_height = (cam->image_height + k - 1) / k;
    for (int a = 0; a < 3; a++) {
        pc.pixel_delta_u[a] = cam->pixel_delta_u[a] * (double)k;
        pc.pixel_delta_v[a] = cam->pixel_delta_v[a] * (double)k;
    }
    return pc;
}

static gs_status pilot_begin(gs_device_scene* ds, const gs_camera* cam, void* stream, PilotRun& pr) {
    pr.t0 = std::chrono::steady_clock::now();
    const gs_camera pc = pilot_camera(cam);
    gs_partition part{0, 1, 64, 64, nullptr, 0, 0};
    const int64_t cap = gs_partition_capacity(&pc, &part);
    const uint32_t nn = ds->node_records, nl = ds->leaf_records;
    if (hipMalloc(&pr.d_rgb, (size_t)cap * 12 + 16) != hipSuccess ||
        hipMalloc(&pr.d_vis, ((size_t)nn + nl) * 4 + 16) != hipSuccess) {
        if (pr.d_rgb) (void)hipFree(pr.d_rgb);
        pr.d_rgb = nullptr;
        return fail(GS_ERR_OOM, "hipMalloc of the placement pilot's buffers failed");
    }
    pr.st = (hipStream_t)stream;
    gs_sample_settings one{0.0, 0.0, 1, 0};  // one sample per pixel (camera.rs:158: max_samples < batch)
    gs_render_outputs o{pr.d_rgb, nullptr, nullptr};
    VisitArgs va{pr.d_vis, nn};
    hipError_t e = hipMemsetAsync(pr.d_vis, 0, ((size_t)nn + nl) * 4, pr.st);
    gs_status r = e == hipSuccess ? launch(ds, &pc, &one, 1, &part, &o, nullptr, stream, nullptr, nullptr, &va)
                                  : fail(GS_ERR_HIP, hipGetErrorString(e));
    pr.launched = r == GS_OK;
    return r;
}

static gs_status pilot_end(gs_device_scene* ds, PilotRun& pr) {
    const uint32_t nn = ds->node_records, nl = ds->leaf_records;
    std::vector<uint32_t> vis((size_t)nn + nl);
    gs_status r = GS_OK;
    if (pr.launched) {
        hipError_t e = hipStreamSynchronize(pr.st);
        if (e == hipSuccess) e = hipMemcpy(vis.data(), pr.d_vis, vis.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = fail(GS_ERR_HIP, std::string("placement pilot: ") + hipGetErrorString(e));
    }
    if (pr.d_rgb) (void)hipFree(pr.d_rgb);
    if (pr.d_vis) (void)hipFree(pr.d_vis);
    pr.d_rgb = nullptr;
    pr.d_vis = nullptr;
    if (!pr.launched) return fail(GS_ERR_HIP, "placement pilot not launched");
    if (r != GS_OK) return r;
    const ThreadedTree& t = ds->tree;
    std::vector<uint64_t> counts(t.rec.size());
    for (size_t i = 0; i < t.rec.size(); i++) counts[i] = t.leaf[i] ? vis[(size_t)nn + ds->pos[i]] : vis[ds->pos[i]];
    Placed pl = place_records(ds, &counts);
    if (pl.tnodes.size() != nn || pl.tleaves.size() != nl) return fail(GS_ERR_HIP, "placement changed the record counts");
    {
        // The arrays are rewritten in place, so nothing of this scene may be running: the
        // pilot is not always the scene's first launch (pilot_due defers it past small ones,
        // which may still be in flight on other streams).  Every launch records its slot's
        // `done` event under `mu` before it returns, so with `mu` held every launch enqueued
        // so far has an event to wait for, and none can start until the records and the
        // launch shape below agree again.
        std::lock_guard<std::mutex> lock(ds->mu);
        for (int k = 0; k < kLaunchSlots; k++)
            if (ds->slots[k].used) HIPCHK(hipEventSynchronize(ds->slots[k].done));
        if (ds->query_used) HIPCHK(hipEventSynchronize(ds->query_done));  // (ray queries read the records too)
        HIPCHK(hipMemcpy(const_cast<TNode*>(ds->dev.tnodes), pl.tnodes.data(), pl.tnodes.size() * sizeof(TNode),
                         hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(const_cast<TBox*>(ds->dev.tboxes), pl.tboxes.data(), pl.tboxes.size() * sizeof(TBox),
                         hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(const_cast<TLeaf*>(ds->dev.tleaves), pl.tleaves.data(), pl.tleaves.size() * sizeof(TLeaf),
                         hipMemcpyHostToDevice));
        if (!pl.nroots.empty())
            HIPCHK(hipMemcpy(ds->nroots, pl.nroots.data(), pl.nroots.size() * 4, hipMemcpyHostToDevice));
        adopt_placement(ds, pl);
    }
    ds->pilot_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pr.t0).count();
    ds->tree = ThreadedTree{};  // not needed again
    ds->placement.store(2, std::memory_order_release);
    return GS_OK;
}

// Does this launch run the scene's pending pilot?  Not when placement is settled, or every
// record is mirrored anyway (then it is settled as static), and not yet when the launch is
// small next to the pilot: a pilot of ~64 k pixel samples before a launch of fewer than
// 16 x as many samples costs more than a better mirror can save there (a one-shot 4-spp
// frame of <= 64 k pixels would pay a full-frame pass, +25%), so it waits for a bigger one.
static bool pilot_due(gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss) {
    if (ds->placement.load(std::memory_order_acquire) != 0) return false;
    const bool all_mirrored = ds->mirror.nodes == ds->node_records && ds->mirror.leaves == ds->leaf_records;
    // (scenes of the catch-all kernel keep the static placement: the pilot's instantiation does
    // not walk their compositions)
    if (!read_knobs().placement || all_mirrored || !cam || cam->image_width <= 0 || cam->image_height <= 0 ||
        (ds->feat & GS_FEAT_GENERAL)) {
        ds->placement.store(1, std::memory_order_release);
        return false;
    }
    const gs_camera pc = pilot_camera(cam);
    const uint64_t pilot_samples = (uint64_t)pc.image_width * (uint64_t)pc.image_height;
    const uint64_t samples = (uint64_t)cam->image_width * (uint64_t)cam->image_height * (ss ? ss->batch_size : 1u);
    return samples >= 16u * pilot_samples;
}

static gs_status ensure_placement(gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                  void* stream) {
    if (ds->placement.load(std::memory_order_acquire) != 0) return GS_OK;
    std::lock_guard<std::mutex> g(ds->place_mu);
    if (!pilot_due(ds, cam, ss)) return GS_OK;
    PilotRun pr;
    gs_status r = pilot_begin(ds, cam, stream, pr);
    const gs_status r2 = pilot_end(ds, pr);  // (frees the buffers either way; tried again at the next launch)
    return r != GS_OK ? r : r2;
}

// The frame context's first frame (and camera changes): every device's pending pilot is
// launched before any is waited for, so N devices pilot concurrently (internal.hpp).
gs_status gs_placement_prepare(gs_device_scene* const* scenes, const int* devices, void* const* streams, int n,
                               const gs_camera* cam, const gs_sample_settings* ss, int* ran) {
    *ran = 0;
    std::vector<std::unique_lock<std::mutex>> locks;
    std::vector<PilotRun> runs(n);
    std::vector<int> due(n, 0);
    gs_status r = GS_OK;
    for (int i = 0; i < n && r == GS_OK; i++) {
        gs_device_scene* ds = scenes[i];
        if (ds->placement.load(std::memory_order_acquire) != 0) continue;
        locks.emplace_back(ds->place_mu);
        if (!pilot_due(ds, cam, ss)) continue;
        if (hipSetDevice(devices[i]) != hipSuccess) {
            r = fail(GS_ERR_HIP, "hipSetDevice failed");
            break;
        }
        due[i] = 1;
        *ran = 1;
        r = pilot_begin(ds, cam, streams[i], runs[i]);
    }
    for (int i = 0; i < n; i++) {
        if (!due[i]) continue;
        (void)hipSetDevice(devices[i]);
        const gs_status e = pilot_end(scenes[i], runs[i]);
        if (r == GS_OK) r = e;
    }
    return r;
}

extern "C" {

gs_status gs_plan_tiles(const gs_device_scene* ds, const gs_camera* cam, uint64_t seed, int32_t world,
                        int32_t tile_w, int32_t tile_h, int32_t* order_out, int64_t order_cap,
                        int32_t* slots_per_rank) {
    if (!ds || !cam || !slots_per_rank || world < 1 || tile_w < 1 || tile_h < 1)
        return fail(GS_ERR_ARG, "bad argument");
    gs_partition all{0, 1, tile_w, tile_h, nullptr, 0, 0};
    if (!part_ok(cam, &all)) return fail(GS_ERR_ARG, "bad partition / image size");
    const int32_t tx = (cam->image_width + tile_w - 1) / tile_w, ty = (cam->image_height + tile_h - 1) / tile_h;
    const int32_t nt = tx * ty;
    const int32_t slots = (nt + world - 1) / world;  // LPT below never gives a rank more (see the cap)
    if (!order_out) {
        *slots_per_rank = slots;
        return GS_OK;
    }
    // 1-spp pilot over the whole frame: per-pixel BVH node visits (deterministic).
    const int64_t cap = gs_partition_capacity(cam, &all);
    float* d_rgb = nullptr;
    uint32_t* d_vis = nullptr;
    if (hipMalloc(&d_rgb, (size_t)cap * 12 + 16) != hipSuccess || hipMalloc(&d_vis, (size_t)cap * 4 + 16) != hipSuccess) {
        if (d_rgb) (void)hipFree(d_rgb);
        return fail(GS_ERR_OOM, "hipMalloc failed");
    }
    gs_sample_settings one{0.0, 0.0, 1, 0};
    gs_render_outputs o{d_rgb, nullptr, d_vis};
    gs_status r = gs_render_tiles_ex_async(ds, cam, &one, seed, &all, &o, nullptr, nullptr);
    std::vector<uint32_t> vis((size_t)cap);
    if (r == GS_OK) {
        hipError_t e = hipStreamSynchronize(nullptr);  // (the launch's stream: this device's alone)
        if (e == hipSuccess) e = hipMemcpy(vis.data(), d_vis, (size_t)cap * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = fail(GS_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d_rgb);
    (void)hipFree(d_vis);
    if (r != GS_OK) return r;
    // Tile cost: node visits + a per-path constant (shading, camera ray), over real pixels.
    const int64_t tpx = (int64_t)tile_w * tile_h;
    std::vector<double> cost(nt, 0.0);
    for (int32_t t = 0; t < nt; t++) {
        const int32_t x0 = (t % tx) * tile_w, y0 = (t / tx) * tile_h;
        for (int32_t y = 0; y < tile_h; y++)
            for (int32_t x = 0; x < tile_w; x++)
                if (x0 + x < cam->image_width && y0 + y < cam->image_height)
                    cost[t] += 16.0 + (double)vis[(size_t)t * tpx + (size_t)y * tile_w + x];
    }
    // Longest processing time first: the costliest tile to the least-loaded rank (ties:
    // lowest rank) among ranks with a free slot.
    std::vector<int32_t> idx(nt);
    for (int32_t t = 0; t < nt; t++) idx[t] = t;
    std::stable_sort(idx.begin(), idx.end(), [&](int32_t a, int32_t b) { return cost[a] > cost[b]; });
    std::vector<double> load(world, 0.0);
    std::vector<std::vector<int32_t>> lists(world);
    for (int32_t t : idx) {
        int32_t best = -1;
        for (int32_t rk = 0; rk < world; rk++)
            if ((int32_t)lists[rk].size() < slots && (best < 0 || load[rk] < load[best])) best = rk;
        lists[best].push_back(t);
        load[best] += cost[t];
    }
    // Each rank walks its tiles in frame order: measured on MI355X (C4, 8 ranks) frame
    // order beat descending cost (max rank 87.6 vs 88.0 ms, mean 85.0 vs 86.5): locality
    // between neighbouring tiles outweighs ending the queue on cheap tiles.
    for (auto& l : lists) std::sort(l.begin(), l.end());
    if (order_cap < (int64_t)slots * world) return fail(GS_ERR_ARG, "order_out too small");
    for (int32_t sl = 0; sl < slots; sl++)
        for (int32_t rk = 0; rk < world; rk++)
            order_out[(size_t)sl * world + rk] = sl < (int32_t)lists[rk].size() ? lists[rk][sl] : -1;
    *slots_per_rank = slots;
    return GS_OK;
}

gs_status gs_debug_record_visits(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                 uint64_t seed, const gs_partition* part, float* d_packed_rgb, uint32_t* d_visits,
                                 void* stream) {
    if (!ds || !cam || !d_packed_rgb || !d_visits) return fail(GS_ERR_ARG, "null argument");
    gs_status e = ensure_placement(const_cast<gs_device_scene*>(ds), cam, ss, stream);
    if (e != GS_OK) return e;
    HIPCHK(hipMemsetAsync(d_visits, 0, ((size_t)ds->node_records + ds->leaf_records) * 4, (hipStream_t)stream));
    gs_render_outputs o{d_packed_rgb, nullptr, nullptr};
    VisitArgs va{d_visits, ds->node_records};
    return launch(ds, cam, ss, seed, part, &o, nullptr, stream, nullptr, nullptr, &va);
}

gs_status gs_debug_last_launch_feat(const gs_device_scene* ds, int32_t* feat) {
    if (!ds || !feat) return fail(GS_ERR_ARG, "null argument");
    *feat = ds->last_launch_feat.load();
    return GS_OK;
}

gs_status gs_debug_device_scene_record(const gs_device_scene* ds, void* out, int64_t out_bytes) {
    if (!ds || !out) return fail(GS_ERR_ARG, "null argument");
    if (out_bytes != (int64_t)sizeof(DevScene))
        return fail(GS_ERR_ARG, "the device scene record is " + std::to_string(sizeof(DevScene)) + " bytes");
    std::memcpy(out, &ds->dev, sizeof(DevScene));
    return GS_OK;
}

gs_status gs_debug_leaf_stage_record(const gs_device_scene* ds, gs_debug_leaf_stage* out, int64_t out_bytes) {
    if (!ds || !out) return fail(GS_ERR_ARG, "null argument");
    if (out_bytes != (int64_t)sizeof(gs_debug_leaf_stage))
        return fail(GS_ERR_ARG, "the leaf stage record is " + std::to_string(sizeof(gs_debug_leaf_stage)) + " bytes");
    *out = gs_debug_leaf_stage{ds->tquads, ds->n_quads, ds->n_cubes, ds->mirror.quads, ds->mirror.cubes};
    return GS_OK;
}

gs_status gs_device_alloc(int64_t bytes, void** d_out) {
    if (!d_out || bytes < 0) return fail(GS_ERR_ARG, "bad argument");
    *d_out = nullptr;
    if (hipMalloc(d_out, (size_t)std::max<int64_t>(bytes, 1)) != hipSuccess) return fail(GS_ERR_OOM, "hipMalloc failed");
    return GS_OK;
}
gs_status gs_device_free(void* d) {
    if (d) HIPCHK(hipFree(d));
    return GS_OK;
}
gs_status gs_device_upload(void* d_dst, const void* src, int64_t bytes) {
    if (!d_dst || !src || bytes < 0) return fail(GS_ERR_ARG, "bad argument");
    HIPCHK(hipMemcpy(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return GS_OK;
}
gs_status gs_device_download(void* dst, const void* d_src, int64_t bytes) {
    if (!dst || !d_src || bytes < 0) return fail(GS_ERR_ARG, "bad argument");
    HIPCHK(hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return GS_OK;
}

}  // extern "C"
