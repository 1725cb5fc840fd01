// internal.hpp — library-internal entry points shared by the host files (launch.cpp, multi_gpu.cpp)
// (not part of the C-ABI in include/).
#pragma once
#include <hip/hip_runtime_api.h>

#include "../../../include/grayshift_gpu.h"

extern "C" void gs_set_last_error(const char* msg);

// gs_render_tiles_ex_async with two optional timing events (of the stream's device)
// recorded right before and after the megakernel itself, so the frame context can report
// the dominant kernel's time apart from the parameter, queue and chunk-combine launches.
// direct: outs->rgb / rgb8 are the W x H frame itself (image pixel j * W + i; padding slots
// not written), so a one-device frame needs no unpack.  zero_counters: d_counters is set to
// zero by the launch's first kernel instead of accumulated into (no memset before it).
gs_status gs_render_tiles_timed_async(const gs_device_scene* ds, const gs_camera* cam, const gs_sample_settings* ss,
                                      uint64_t seed, const gs_partition* part, const gs_render_outputs* outs,
                                      gs_counters* d_counters, void* stream, hipEvent_t k_begin, hipEvent_t k_end,
                                      bool direct = false, bool zero_counters = false);

// gs_render_tiles_pass_async with the same extras, and the pass's change: d_delta (nullable)
// receives gs_pass_delta_blocks(capacity) per-block sums of |colour after - colour before| over
// this rank's real pixels and channels (f64 colours; before = 0 when sample_base is 0), to be
// added in index order.  The block count depends on the capacity alone.
gs_status gs_render_tiles_pass_timed_async(const gs_device_scene* ds, const gs_camera* cam, uint32_t samples,
                                           uint64_t seed, const gs_partition* part, uint32_t sample_base,
                                           uint32_t chunk, double* d_sums, double* d_delta,
                                           const gs_render_outputs* outs, gs_counters* d_counters, void* stream,
                                           hipEvent_t k_begin, hipEvent_t k_end, bool direct, bool zero_counters);
int64_t gs_pass_delta_blocks(int64_t capacity);

// gs_render_tiles_views_async with the same extras (direct: outs are the [V][H][W][3] frames).
gs_status gs_render_tiles_views_timed_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                            uint32_t samples, uint32_t chunk, const gs_partition* part,
                                            const gs_render_outputs* outs, gs_counters* d_counters, void* stream,
                                            hipEvent_t k_begin, hipEvent_t k_end, bool direct, bool zero_counters);
// gs_render_tiles_views_pass_async with the same extras.
gs_status gs_render_tiles_views_pass_timed_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                                 const uint32_t* view_samples, const uint8_t* selected, uint32_t samples,
                                                 uint32_t chunk, const gs_partition* part, double* d_sums,
                                                 const gs_render_outputs* outs, double* d_delta_partials,
                                                 gs_counters* d_counters, void* stream, hipEvent_t k_begin,
                                                 hipEvent_t k_end, bool direct, bool zero_counters);
// The checks of a views pass's selection (all on the arguments alone): view_samples whole chunks
// of c, a selection (NULL: every view) that is not empty and whose views hold one count, *base.
gs_status gs_views_pass_check(uint32_t n_views, const uint32_t* view_samples, const uint8_t* selected, uint32_t samples,
                              uint32_t c, uint32_t* base);
// The checks of a views call that need no partition (all on the arguments alone), and the tall
// frame's camera: view 0's with image_height = V H.  c: the chunk, resolved (never 0).
gs_status gs_views_check(const gs_device_scene* ds, const gs_view* views, uint32_t n_views, uint32_t samples, uint32_t c,
                         gs_camera* tall);
// ... and those of one rank's share of the tall frame, `cap` packed pixels (gs_partition_capacity).
gs_status gs_views_check_cap(int64_t cap, uint32_t samples, uint32_t c);

// gs_render_tiles_rounds_async with the same extras.  rounds == 0 (this form only) renders
// nothing and resolves the state as it stands.  After the call's work the blob's summary words
// (GsRoundLayout::summary) hold this rank's active pixels, Σ samples and max samples of a pixel.
gs_status gs_render_tiles_rounds_timed_async(const gs_device_scene* ds, const gs_camera* cam,
                                             const gs_sample_settings* ss, uint64_t seed, const gs_partition* part,
                                             uint32_t first_round, uint32_t rounds, void* d_state, int64_t state_bytes,
                                             const gs_round_outputs* out, gs_counters* d_counters, void* stream,
                                             hipEvent_t k_begin, hipEvent_t k_end, bool direct, bool zero_counters);
// gs_render_tiles_views_rounds_async with the same extras (rounds == 0, this form only: resolve
// the state as it stands; direct: out->rgb / rgb8 are the [V][H][W][3] frames).
gs_status gs_render_tiles_views_rounds_timed_async(const gs_device_scene* ds, const gs_view* views, uint32_t n_views,
                                                   const gs_sample_settings* ss, const gs_partition* part,
                                                   uint32_t first_round, uint32_t rounds, void* d_state,
                                                   int64_t state_bytes, const gs_round_outputs* out,
                                                   gs_counters* d_counters, void* stream, hipEvent_t k_begin,
                                                   hipEvent_t k_end, bool direct, bool zero_counters);
// The round-state blob of `cap` packed pixels and R rounds, byte offsets (256-B aligned but the
// first three): the item-size hint, the summary (4 u64), round_counts[R + 2], the two active
// lists (cap u32 each), pstate (cap * 5 f64), the batches words (cap u32).  Private to the
// library: the frame context fills and reads it for checkpoints.
static const int kRoundSummaryWords = 4;  // (kernel_abi.hpp GS_ROUND_SUMMARY_WORDS)
struct GsRoundLayout {
    size_t hint, summary, counts, list[2], pstate, batches, bytes;
};
GsRoundLayout gs_round_layout(uint64_t cap, uint64_t R);

// The placement pilots still pending for a launch of `cam` / `ss` on n devices (scenes[i] on
// devices[i], its stream streams[i]): every device's pilot is launched before any is waited
// for, so the first frame of an N-GPU context pilots concurrently (launch.cpp).  *ran: whether
// any pilot ran.  Leaves the current device changed.
gs_status gs_placement_prepare(gs_device_scene* const* scenes, const int* devices, void* const* streams, int n,
                               const gs_camera* cam, const gs_sample_settings* ss, int* ran);

// A timed frame of the scene on its device: its megakernel time and samples (paths), which
// set the scene's per-sample cost that the guided tail's small-frame rule reads (launch.cpp).
extern "C" void gs_device_scene_note_frame(gs_device_scene* ds, double kernel_ms, uint64_t samples);
