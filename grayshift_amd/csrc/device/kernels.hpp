// kernels.hpp — what render.hip offers the host files (csrc/host/scene.cpp, launch.cpp): which
// gs_render_kernel instantiations exist, and one launcher per kernel.  Kernel pointers feed
// hipFuncGetAttributes and the occupancy query on the host side; only render.hip launches.
#pragma once
#include "kernel_abi.hpp"

// The instantiation for a feature set (gs_render_kernel<0> when there is none for it).
void (*kernel_for(int feat))(KArgs);
// That instantiation's own feature word (0 for the fallback; `feat` itself where kernel_for gives
// null): what its lane-state layout follows (kernel_abi.hpp: lane_nd, lane_ni, lane_lds_bytes).
int kernel_feat(int feat);
// A split batch round may take the (feat | GS_FEAT_FIXED | GS_FEAT_RSPLIT) instantiation.
bool has_rsplit(int feat);
// A views launch may take the (feat | GS_FEAT_FIXED | GS_FEAT_VIEWS) instantiation (for such a
// feature set kernel_for returns null when there is none: a views launch has no fallback).
bool has_views(int feat);
// The split batch round of a views adaptation: the (feat | GS_FEAT_FIXED | GS_FEAT_RSPLIT |
// GS_FEAT_VIEWS) instantiation where has_rsplit(feat), else (feat | GS_FEAT_VIEWS), the loop's
// kernel with per-sample items; null for any other word (no fallback).  has_views_rounds: the
// feature set has one of the two.
void (*views_round_kernel_for(int feat))(KArgs);
bool has_views_rounds(int feat);

// Each enqueues one kernel on `st` and returns that launch's error (hipGetLastError()).
hipError_t launch_params_kernel(hipStream_t st, const KParams& kp, KParams* dst);  // (zeroes the queue)
hipError_t launch_views_kernel(hipStream_t st, const ViewBatch& vb, gs_view* dst);  // (vb.n records to dst + vb.first)
hipError_t launch_combine_kernel(hipStream_t st, unsigned grid, const KParams* P);
// (a progressive pass's combine; its grid is gs_accum_blocks(capacity), the size of KParams::delta)
hipError_t launch_accumulate_kernel(hipStream_t st, const KParams* P, uint32_t capacity);
// (a progressive views pass: vb.n per-view records to dst + vb.first; the pass's tile order, n_pos
// positions, written to dst after the parameter kernel -- it reads P; the pass's combine, one block
// per tile slot of the rank, the size of KParams::vdelta)
hipError_t launch_view_state_kernel(hipStream_t st, const ViewStateBatch& vb, GsViewState* dst);
hipError_t launch_views_order_kernel(hipStream_t st, const KParams* P, int32_t* dst, uint32_t n_pos, uint32_t view_h);
hipError_t launch_views_accumulate_kernel(hipStream_t st, const KParams* P, uint32_t slots);
hipError_t launch_round_init_kernel(hipStream_t st, unsigned grid, const KParams* P);
hipError_t launch_round_params_kernel(hipStream_t st, KParams* P, uint32_t round, uint32_t seg, uint32_t seg_px,
                                      int32_t chunk_req, int32_t whole_mode);
hipError_t launch_round_combine_kernel(hipStream_t st, unsigned grid, const KParams* P, uint32_t round);
// (a progressive adaptive pass: the fold after each (round, segment) launch, the resolve at the
// pass's end on gs_accum_blocks(capacity) blocks)
hipError_t launch_round_fold_kernel(hipStream_t st, unsigned grid, const KParams* P, uint32_t round);
hipError_t launch_round_resolve_kernel(hipStream_t st, const KParams* P, uint32_t capacity);
hipError_t launch_render_kernel(hipStream_t st, void (*kernel)(KArgs), unsigned blocks, size_t lds, const KArgs& a);
