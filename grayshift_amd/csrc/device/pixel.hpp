// pixel.hpp — the stage that turns samples into pixels: packed_pixel (packed slot -> image pixel
// through the tile order), gs_combine_kernel and gs_accumulate_kernel (a pixel's chunk sums added
// in chunk order, the guided tail's 1-sample sums re-formed into chunks first; the pass's change
// folded in a fixed tree), gs_views_order_kernel and gs_views_accumulate_kernel (the same for a
// pass over a subset of a batch of views), and the adaptive batch rounds outside the megakernel:
// gs_round_init_kernel, gs_round_params_kernel (a launch's share of the active list and its item
// size), gs_round_combine_kernel and gs_round_fold_kernel (a batch folded in sample order, the
// reference's stop test, the active list compacted with ballots) and gs_round_resolve_kernel.
// Included by render.hip; tests/hip/kat_device.hip includes it too, so the known-answer tests
// launch these very kernels.  Written in namespace gsd's names (color_byte, sat_u64, udiv, ...):
// an includer says `using namespace gsd;` before it includes this file, as both do (as leaf.hpp).
//
// Two halves under include guards of their own: the combine and accumulate kernels, then the
// views and rounds kernels.  An includer gets both at once.  render.hip alone takes them one at a
// time (GS_PIXEL_FIRST_HALF set for its first include), because a code object lists its kernels in
// definition order and render.hip's gs_view_state_kernel stands between the two: moved past them,
// the library's code-object hash (grayshift_amd/codeobj.py) would change with no kernel changed.
#ifndef GS_PIXEL_HPP_PASSES
#define GS_PIXEL_HPP_PASSES
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../../include/grayshift_gpu.h"
#include "kernel_abi.hpp"
#include "devmath.hpp"

// (GS_ROUND_PIXEL_MAJOR, the layout of a split round's per-sample colours: kernel_abi.hpp, since
// the megakernel, which writes them, stands above this header in render.hip)

// Chunked single-batch renders: a pixel's colour is the sum of its chunks' Σrgb, taken
// in chunk (= sample) order, over the batch size (camera.rs:142-160 with one batch).
// Padding slots of partial tiles get zeros.
// Packed pixel k of this rank -> its image pixel (pi, pj); false for a padding slot (an empty
// tile slot of the plan, or outside the image).
__device__ __forceinline__ bool packed_pixel(const KParams* __restrict__ P, uint32_t k, uint32_t& pi, uint32_t& pj) {
    const uint32_t tile_px = (uint32_t)(P->tile_w * P->tile_h);
    const uint32_t slot = k / tile_px, w = k % tile_px;
    const uint32_t pos = (uint32_t)P->rank + slot * (uint32_t)P->world_size;
    const uint32_t tile = P->order ? (uint32_t)P->order[pos] : pos;  // -1: empty slot
    if (tile == 0xFFFFFFFFu) return false;
    pi = (tile % (uint32_t)P->tiles_x) * (uint32_t)P->tile_w + w % (uint32_t)P->tile_w;
    pj = (tile / (uint32_t)P->tiles_x) * (uint32_t)P->tile_h + w / (uint32_t)P->tile_w;
    return pi < (uint32_t)P->cam.image_width && pj < (uint32_t)P->cam.image_height;
}

__global__ void gs_combine_kernel(const KParams* __restrict__ P) {
    const uint32_t cpp = P->cpp;
    const double scount = 0.0 + (double)P->ss.batch_size;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < P->capacity; k += gridDim.x * blockDim.x) {
        uint32_t pi = 0, pj = 0;
        const bool real = packed_pixel(P, k, pi, pj);
        const size_t oi = P->direct ? (size_t)pj * (uint32_t)P->cam.image_width + pi : (size_t)k;
        float* o = P->out ? P->out + oi * 3 : nullptr;
        uint8_t* o8 = P->out8 ? P->out8 + oi * 3 : nullptr;
        if (!real) {
            if (P->direct) continue;
            if (o) {
                o[0] = 0.0f;
                o[1] = 0.0f;
                o[2] = 0.0f;
            }
            if (o8) {
                o8[0] = 0;
                o8[1] = 0;
                o8[2] = 0;
            }
            continue;
        }
        const bool fine = k >= P->fine_px;
        // chunk-major sums: consecutive lanes read consecutive 24-B sums of each chunk
        const size_t stride = (size_t)(fine ? P->capacity - P->fine_px : P->fine_px) * 3;
        const double* p = P->partial + (fine ? (size_t)P->fine_base + (k - P->fine_px) : (size_t)k) * 3;
        double r = 0.0, g = 0.0, b = 0.0;
        if (!fine) {
            for (uint32_t c = 0; c < cpp; c++, p += stride) {
                r += p[0];
                g += p[1];
                b += p[2];
            }
        } else {
            // 1-sample items (fine_chunk 1: each sum is 0 + s = s), re-formed into the coarse
            // chunks of P->chunk samples and added in order: the coarse pixels' association,
            // so a pixel's bits do not depend on whether its tile ran in the tail
            const uint32_t bs = P->ss.batch_size, c = P->chunk;
            for (uint32_t s0 = 0; s0 < bs; s0 += c) {
                const uint32_t e = min(bs, s0 + c);
                double cr = 0.0, cg = 0.0, cb = 0.0;
                for (uint32_t s = s0; s < e; s++, p += stride) {
                    cr += p[0];
                    cg += p[1];
                    cb += p[2];
                }
                r += cr;
                g += cg;
                b += cb;
            }
        }
        const double cr = r / scount, cg = g / scount, cb = b / scount;
        if (o) {
            o[0] = (float)cr;
            o[1] = (float)cg;
            o[2] = (float)cb;
        }
        if (o8) {
            o8[0] = color_byte(cr);
            o8[1] = color_byte(cg);
            o8[2] = color_byte(cb);
        }
    }
}

// Progressive passes: gs_combine_kernel for a launch that continues a frame.  The pass rendered
// samples [sample_base, sample_base + batch_size) of every pixel; a pixel's running sums
// (accum, f64, packed order) take the pass's chunk sums in chunk order -- the combine's own
// additions, the tail's 1-sample sums re-formed into chunks of P->chunk first -- so after K
// passes of n samples they hold ((0 + C_0) + C_1) + ... over all K n / c chunks: a one-shot
// K n-spp render's sums, bit for bit, and sums / (K n) is its colour.
// The pass's change, Σ over real pixels and channels of |colour after - colour before| (the
// f64 colours; before = 0 for the first pass): each thread adds its pixels' terms in pixel
// order, the block folds its 256 values through LDS in a fixed tree, and block b's sum goes
// to delta[b] -- no float atomics, and the grid is gs_accum_blocks(capacity), so the values
// depend on the capacity alone.  The host adds the partials in index order.
__global__ __launch_bounds__(256) void gs_accumulate_kernel(const KParams* __restrict__ P) {
    __shared__ double s_red[256];
    const uint32_t cpp = P->cpp;
    const uint32_t base = P->sample_base, bs = P->ss.batch_size;
    const double n_before = (double)base, n_after = (double)(base + bs);
    double change = 0.0;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < P->capacity; k += gridDim.x * blockDim.x) {
        uint32_t pi = 0, pj = 0;
        const bool real = packed_pixel(P, k, pi, pj);
        const size_t oi = P->direct ? (size_t)pj * (uint32_t)P->cam.image_width + pi : (size_t)k;
        float* o = P->out ? P->out + oi * 3 : nullptr;
        uint8_t* o8 = P->out8 ? P->out8 + oi * 3 : nullptr;
        if (!real) {
            if (P->direct) continue;
            if (o) {
                o[0] = 0.0f;
                o[1] = 0.0f;
                o[2] = 0.0f;
            }
            if (o8) {
                o8[0] = 0;
                o8[1] = 0;
                o8[2] = 0;
            }
            continue;
        }
        const bool fine = k >= P->fine_px;
        // chunk-major sums: consecutive lanes read consecutive 24-B sums of each chunk
        const size_t stride = (size_t)(fine ? P->capacity - P->fine_px : P->fine_px) * 3;
        const double* p = P->partial + (fine ? (size_t)P->fine_base + (k - P->fine_px) : (size_t)k) * 3;
        double* acc = P->accum + (size_t)k * 3;
        const double r0 = acc[0], g0 = acc[1], b0 = acc[2];
        double r = r0, g = g0, b = b0;
        if (!fine) {
            for (uint32_t c = 0; c < cpp; c++, p += stride) {
                r += p[0];
                g += p[1];
                b += p[2];
            }
        } else {
            const uint32_t c = P->chunk;  // (bs is a multiple of c: gs_render_tiles_pass_async)
            for (uint32_t s0 = 0; s0 < bs; s0 += c) {
                const uint32_t e = min(bs, s0 + c);
                double cr = 0.0, cg = 0.0, cb = 0.0;
                for (uint32_t s = s0; s < e; s++, p += stride) {
                    cr += p[0];
                    cg += p[1];
                    cb += p[2];
                }
                r += cr;
                g += cg;
                b += cb;
            }
        }
        acc[0] = r;
        acc[1] = g;
        acc[2] = b;
        const double cr = r / n_after, cg = g / n_after, cb = b / n_after;
        if (o) {
            o[0] = (float)cr;
            o[1] = (float)cg;
            o[2] = (float)cb;
        }
        if (o8) {
            o8[0] = color_byte(cr);
            o8[1] = color_byte(cg);
            o8[2] = color_byte(cb);
        }
        const double pr = base ? r0 / n_before : 0.0, pg = base ? g0 / n_before : 0.0, pb = base ? b0 / n_before : 0.0;
        change += fabs(cr - pr);
        change += fabs(cg - pg);
        change += fabs(cb - pb);
    }
    s_red[threadIdx.x] = change;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) s_red[threadIdx.x] += s_red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0 && P->delta) P->delta[blockIdx.x] = s_red[0];
}

#endif  // GS_PIXEL_HPP_PASSES
#if !defined(GS_PIXEL_HPP_VIEWS_ROUNDS) && !defined(GS_PIXEL_FIRST_HALF)
#define GS_PIXEL_HPP_VIEWS_ROUNDS

// Progressive views: a pass's tile order: dst[pos] = the tile of position pos (P->vorder, or pos itself),
// or -1 when that tile's view is not selected (or the position holds no tile of the frame).  A
// selected tile keeps its slot, so the packed sums never move.  view_h: the rows of one view, a
// multiple of tile_h.
__global__ void gs_views_order_kernel(const KParams* __restrict__ P, int32_t* __restrict__ dst, uint32_t n_pos,
                                      uint32_t view_h) {
    for (uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x; pos < n_pos; pos += gridDim.x * blockDim.x) {
        const int32_t tile = P->vorder ? P->vorder[pos] : (int32_t)pos;
        int32_t t = -1;
        if (tile >= 0) {
            const uint32_t row = ((uint32_t)tile / (uint32_t)P->tiles_x) * (uint32_t)P->tile_h;
            if (row < (uint32_t)P->cam.image_height && P->vstate[row / view_h].selected) t = tile;
        }
        dst[pos] = t;
    }
}

// Progressive views: gs_accumulate_kernel for a pass over a subset of a batch of views.  Block b
// takes tile slot b of this rank (its tile from P->vorder: P->order has the unselected views'
// tiles emptied), which lies in one view v.  A selected view's pixel takes exactly the accumulate
// kernel's additions -- the pass's chunk sums in chunk order, the tail's 1-sample sums re-formed
// into chunks of P->chunk first -- and resolves to sums / (double)(before + batch); an unselected
// view's pixel resolves again from its stored sums, sums / (double)before (0 while the view has
// no samples), so a buffer never seen before is filled whole.  The pass's change: each thread adds
// its pixels' terms in pixel order, the block folds its 256 values through LDS in a fixed tree
// and writes vdelta[b]: one partial per slot, a function of the capacity and the tile size alone.
__global__ __launch_bounds__(256) void gs_views_accumulate_kernel(const KParams* __restrict__ P) {
    __shared__ double s_red[256];
    const uint32_t tile_px = (uint32_t)(P->tile_w * P->tile_h);
    const uint32_t slot = blockIdx.x;
    const uint32_t pos = (uint32_t)P->rank + slot * (uint32_t)P->world_size;
    const uint32_t tile = P->vorder ? (uint32_t)P->vorder[pos] : pos;  // -1: empty slot
    const uint32_t W = (uint32_t)P->cam.image_width, H = (uint32_t)P->cam.image_height;
    const uint32_t x0 = (tile % (uint32_t)P->tiles_x) * (uint32_t)P->tile_w;
    const uint32_t y0 = (tile / (uint32_t)P->tiles_x) * (uint32_t)P->tile_h;
    const bool tile_real = tile != 0xFFFFFFFFu && y0 < H;
    GsViewState vs{0u, 0u};
    if (tile_real) vs = P->vstate[udiv(y0 * W, P->u_vpx)];
    const uint32_t cpp = P->cpp, bs = P->ss.batch_size;
    const uint32_t n_after_u = vs.selected ? vs.before + bs : vs.before;
    const double n_before = (double)vs.before, n_after = (double)n_after_u;
    double change = 0.0;
    for (uint32_t w = threadIdx.x; w < tile_px; w += blockDim.x) {
        const uint32_t k = slot * tile_px + w;
        const uint32_t pi = x0 + w % (uint32_t)P->tile_w, pj = y0 + w / (uint32_t)P->tile_w;
        const bool real = tile_real && pi < W && pj < H;
        const size_t oi = P->direct ? (size_t)pj * W + pi : (size_t)k;
        float* o = P->out ? P->out + oi * 3 : nullptr;
        uint8_t* o8 = P->out8 ? P->out8 + oi * 3 : nullptr;
        double cr = 0.0, cg = 0.0, cb = 0.0;
        if (!real) {
            if (P->direct) continue;
        } else {
            double* acc = P->accum + (size_t)k * 3;
            const double r0 = acc[0], g0 = acc[1], b0 = acc[2];
            double r = r0, g = g0, b = b0;
            if (vs.selected) {
                const bool fine = k >= P->fine_px;
                // chunk-major sums: consecutive lanes read consecutive 24-B sums of each chunk
                const size_t stride = (size_t)(fine ? P->capacity - P->fine_px : P->fine_px) * 3;
                const double* p = P->partial + (fine ? (size_t)P->fine_base + (k - P->fine_px) : (size_t)k) * 3;
                if (!fine) {
                    for (uint32_t c = 0; c < cpp; c++, p += stride) {
                        r += p[0];
                        g += p[1];
                        b += p[2];
                    }
                } else {
                    const uint32_t c = P->chunk;  // (bs is a multiple of c)
                    for (uint32_t s0 = 0; s0 < bs; s0 += c) {
                        const uint32_t e = min(bs, s0 + c);
                        double sr = 0.0, sg = 0.0, sb = 0.0;
                        for (uint32_t s = s0; s < e; s++, p += stride) {
                            sr += p[0];
                            sg += p[1];
                            sb += p[2];
                        }
                        r += sr;
                        g += sg;
                        b += sb;
                    }
                }
                acc[0] = r;
                acc[1] = g;
                acc[2] = b;
            }
            if (n_after_u) {
                cr = r / n_after;
                cg = g / n_after;
                cb = b / n_after;
            }
            if (vs.selected) {
                const double pr = vs.before ? r0 / n_before : 0.0, pg = vs.before ? g0 / n_before : 0.0,
                             pb = vs.before ? b0 / n_before : 0.0;
                change += fabs(cr - pr);
                change += fabs(cg - pg);
                change += fabs(cb - pb);
            }
        }
        if (o) {
            o[0] = (float)cr;
            o[1] = (float)cg;
            o[2] = (float)cb;
        }
        if (o8) {
            o8[0] = color_byte(cr);
            o8[1] = color_byte(cg);
            o8[2] = color_byte(cb);
        }
    }
    s_red[threadIdx.x] = change;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) s_red[threadIdx.x] += s_red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0 && P->vdelta) P->vdelta[slot] = s_red[0];
}

// ------------------------------------------------ adaptive sampling in batch rounds
// The reference's adaptive loop (camera.rs:135-165) runs a pixel's batches one after the
// other, each batch's stop test over the running sums.  Per-lane that puts up to
// max_samples + batch sequential samples of one pixel into one lane, and a frame ends on
// its slowest pixels (an all-black pixel never converges, camera.rs:156).  In rounds, round
// r renders batch r of every pixel still active, its samples split into work items like the
// fixed-spp chunks, each sample's colour kept; the combine then folds a pixel's batch into
// its sums in sample order and takes the stop test -- the same f64 operations in the same
// order as the sequential loop, so every stop decision and every output is bit-identical.

// Before round 0: padding slots get their zero output; every real packed pixel enters the
// first active list (one atomic per wave; the order inside a wave is kept).
__global__ void gs_round_init_kernel(const KParams* __restrict__ P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t cap = P->capacity;
    const uint32_t span = (cap + 63u) & ~63u;  // whole waves take every iteration (ballots)
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < span; k += gridDim.x * blockDim.x) {
        bool real = false;
        if (k < cap) {
            uint32_t pi = 0, pj = 0;
            real = packed_pixel(P, k, pi, pj);
            if (!real && !P->direct) {
                if (P->out) {
                    float* o = P->out + (size_t)k * 3;
                    o[0] = 0.0f;
                    o[1] = 0.0f;
                    o[2] = 0.0f;
                }
                if (P->out8) {
                    uint8_t* o8 = P->out8 + (size_t)k * 3;
                    o8[0] = 0;
                    o8[1] = 0;
                    o8[2] = 0;
                }
            }
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(real);
        if (m == 0) continue;
        const uint32_t leader = (uint32_t)__builtin_ctzll(m);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&P->round_counts[0], (uint32_t)__popcll(m));
        base = __shfl(base, (int)leader);
        if (real) P->active_buf[0][base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = k;
    }
}

// Before each (round, segment) launch: this launch's share of the round's active list, its
// chunking (finer when few pixels are left, so the round's samples still spread over the
// lanes), queue claim and cleared queue.
__global__ void gs_round_params_kernel(KParams* __restrict__ P, uint32_t round, uint32_t seg, uint32_t seg_px,
                                       int32_t chunk_req, int32_t whole_mode) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t n_act = P->round_counts[round];
    const uint32_t base = seg * seg_px;
    const uint32_t n_seg = n_act > base ? min(seg_px, n_act - base) : 0u;
    const uint32_t bs = P->ss.batch_size;
    // whole-batch items while the active pixels are at least twice the lanes (no per-sample
    // colours kept, no combine), split ones once few are left (their samples spread over the
    // lanes); a requested sample chunk always splits
    const bool whole = chunk_req <= 0 && bs <= GS_ROUND_WHOLE_MAX_BATCH &&
                       (whole_mode > 0 || (whole_mode < 0 && (uint64_t)n_seg >= 2ull * P->lanes));
    uint32_t csz;
    if (chunk_req > 0) {
        csz = min((uint32_t)chunk_req, bs);
    } else {
        // Scenes whose paths are long (>= 2 rays a path so far: the launch's counters from round
        // 1 on, before that the slot's last rounds) take 1-sample items: a round then ends on one
        // path, not on an item of several.  Round 6, MI355X A2 (cornell_box, 5.3 rays a path):
        // the rule below for every scene 9 553 Msamples/s; 16 / 32 / 64 / 128 items per lane
        // 10 216 / 10 767 / 10 955 / 10 954, the last two 1-sample items at A2's size.  Short
        // paths (A1's hdri, 1.1) keep the rule -- halve 16-sample items until the round has 8
        // items per lane: with 1-sample items A1 in rounds ran 10 968 instead of 23 729, each
        // item's fixed costs beside a one-ray path (profiles/r06/ab_A2_round_items.txt).
        // Item sizes are scheduling only: the combine folds every sample in order.
        unsigned long long rays = 0, paths = 0;
        if (round && P->counters) {
            rays = P->counters[C_RAYS];
            paths = P->counters[C_PATHS];
            P->rpp_hint[0] = rays;
            P->rpp_hint[1] = paths;
        } else if (!round) {
            rays = P->rpp_hint[0];
            paths = P->rpp_hint[1];
        }
        if (paths && rays >= 2ull * paths) {
            csz = 1u;
        } else {
            csz = min(16u, bs);
            while (csz > 1u && (uint64_t)n_seg * ((bs + csz - 1u) / csz) < 8ull * P->lanes) csz >>= 1;
        }
    }
    const uint32_t cpp = whole ? 1u : (bs + csz - 1u) / csz;
    P->per_sample = whole ? 0u : 1u;
    P->chunk = whole ? 0u : csz;
    P->round = round;
    P->cpp = cpp;
    P->u_cpp = udiv_make(cpp);
    P->n_items = n_seg * cpp;
    P->fine_base = 0xFFFFFFFFu;  // no fine region
    P->fine_px = P->capacity;
    // (items of a few samples claim more at a time, as fine chunks do: the one queue counter
    // serialises the claims, and a tail round runs millions of 1-sample items)
    P->claim = max(1u, min(whole || csz > 4u ? 32u : (uint32_t)GS_CLAIM_FINE,
                           P->n_items / max(1u, P->waves) / (uint32_t)GS_CLAIM_DIV));
    P->claim_fine = P->claim;
    P->round_base = round * bs;
    P->seg_base = base;
    P->seg_n = n_seg;
    P->active = P->active_buf[round & 1u];
    P->next_active = P->active_buf[(round & 1u) ^ 1u];
    *P->queue = 0u;
}

// After each (round, segment) launch: per active pixel, its batch folded into the running
// sums in sample order (camera.rs:142-146), then the stop test (:149-164) exactly as the
// per-lane loop takes it; a stopped pixel's colour (:167) is written, the rest go on.
__global__ void gs_round_combine_kernel(const KParams* __restrict__ P, uint32_t round) {
    if (!P->per_sample) return;  // a whole-batch round: the lanes took the stop test
    const uint32_t n = P->seg_n, bs = P->ss.batch_size, lane = threadIdx.x & 63u;
    const uint32_t span = (n + 63u) & ~63u;
    const double confidence_sq = P->ss.confidence * P->ss.confidence;
    const double tolerance_sq = P->ss.tolerance * P->ss.tolerance;
    // sample_count after this round's batch: 0.0 + bs + bs + ... (exact: integers < 2^53)
    const double scount = (double)((uint64_t)(round + 1u) * bs);
    for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < span; a += gridDim.x * blockDim.x) {
        bool go_on = false, stopped = false;
        uint32_t item = 0;
        if (a < n) {
            item = P->active[P->seg_base + a];
            double* ps = P->pstate + (size_t)item * 5;
            double r = 0.0, g = 0.0, b = 0.0, lsum = 0.0, lsq = 0.0;
            if (round) {
                r = ps[0];
                g = ps[1];
                b = ps[2];
                lsum = ps[3];
                lsq = ps[4];
            }
            const double* smp = P->partial + (size_t)a * (GS_ROUND_PIXEL_MAJOR ? bs : 1u) * 3;
            for (uint32_t j = 0; j < bs; j++, smp += (GS_ROUND_PIXEL_MAJOR ? 1u : (size_t)n) * 3) {
                const double cr = smp[0], cg = smp[1], cb = smp[2];
                r += cr;
                g += cg;
                b += cb;
                const double lum = 0.299 * cr + 0.587 * cg + 0.144 * cb;
                lsum += lum;
                lsq += lum * lum;
            }
            const double mean = lsum / scount;
            const double variance_sq = 1.0 / (scount - 1.0) * (lsq - lsum * lsum / scount);
            const double convergence_sq = confidence_sq * variance_sq / scount;
            bool stop = convergence_sq < (mean * mean * tolerance_sq);
            if (!stop) stop = (uint32_t)sat_u64(scount, 4294967295.0, 4294967295ull) > P->ss.max_samples;
            if (stop) {
                const double cr = r / scount, cg = g / scount, cb = b / scount;
                uint32_t pi = 0, pj = 0;
                if (P->direct) (void)packed_pixel(P, item, pi, pj);  // (an active pixel is real)
                const size_t oi = P->direct ? (size_t)pj * (uint32_t)P->cam.image_width + pi : (size_t)item;
                if (P->out) {
                    float* o = P->out + oi * 3;
                    o[0] = (float)cr;
                    o[1] = (float)cg;
                    o[2] = (float)cb;
                }
                if (P->out8) {
                    uint8_t* o8 = P->out8 + oi * 3;
                    o8[0] = color_byte(cr);
                    o8[1] = color_byte(cg);
                    o8[2] = color_byte(cb);
                }
                stopped = true;
            } else {
                ps[0] = r;
                ps[1] = g;
                ps[2] = b;
                ps[3] = lsum;
                ps[4] = lsq;
                go_on = true;
            }
        }
        const uint64_t mg = __builtin_amdgcn_ballot_w64(go_on), ms = __builtin_amdgcn_ballot_w64(stopped);
        if (mg != 0) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(mg);
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&P->round_counts[round + 1u], (uint32_t)__popcll(mg));
            base = __shfl(base, (int)leader);
            if (go_on) P->next_active[base + (uint32_t)__popcll(mg & ((1ull << lane) - 1ull))] = item;
        }
        if (ms != 0 && P->counters && lane == (uint32_t)__builtin_ctzll(ms))
            atomicAdd(&P->counters[C_PIX], (unsigned long long)__popcll(ms));
    }
}

// ------------------------------------------------ progressive adaptive passes
// A frame's rounds split over passes (gs_render_tiles_rounds_async): the round state lives in
// the caller's blob and every round has split items, so the megakernel never touches it.

// gs_round_combine_kernel for a pass: the same additions in the same order and the same stop
// test, but a stopped pixel's final sums are kept too, with its batches-taken word
// (GS_ADAPT_STOPPED set), and no colour is written: gs_round_resolve_kernel resolves every
// pixel from its sums at the end of the pass.
__global__ void gs_round_fold_kernel(const KParams* __restrict__ P, uint32_t round) {
    const uint32_t n = P->seg_n, bs = P->ss.batch_size, lane = threadIdx.x & 63u;
    const uint32_t span = (n + 63u) & ~63u;
    const double confidence_sq = P->ss.confidence * P->ss.confidence;
    const double tolerance_sq = P->ss.tolerance * P->ss.tolerance;
    const double scount = (double)((uint64_t)(round + 1u) * bs);
    for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < span; a += gridDim.x * blockDim.x) {
        bool go_on = false, stopped = false;
        uint32_t item = 0;
        if (a < n) {
            item = P->active[P->seg_base + a];
            double* ps = P->pstate + (size_t)item * 5;
            double r = 0.0, g = 0.0, b = 0.0, lsum = 0.0, lsq = 0.0;
            if (round) {
                r = ps[0];
                g = ps[1];
                b = ps[2];
                lsum = ps[3];
                lsq = ps[4];
            }
            const double* smp = P->partial + (size_t)a * (GS_ROUND_PIXEL_MAJOR ? bs : 1u) * 3;
            for (uint32_t j = 0; j < bs; j++, smp += (GS_ROUND_PIXEL_MAJOR ? 1u : (size_t)n) * 3) {
                const double cr = smp[0], cg = smp[1], cb = smp[2];
                r += cr;
                g += cg;
                b += cb;
                const double lum = 0.299 * cr + 0.587 * cg + 0.144 * cb;
                lsum += lum;
                lsq += lum * lum;
            }
            const double mean = lsum / scount;
            const double variance_sq = 1.0 / (scount - 1.0) * (lsq - lsum * lsum / scount);
            const double convergence_sq = confidence_sq * variance_sq / scount;
            bool stop = convergence_sq < (mean * mean * tolerance_sq);
            if (!stop) stop = (uint32_t)sat_u64(scount, 4294967295.0, 4294967295ull) > P->ss.max_samples;
            ps[0] = r;
            ps[1] = g;
            ps[2] = b;
            ps[3] = lsum;
            ps[4] = lsq;
            P->pbatches[item] = (round + 1u) | (stop ? GS_ADAPT_STOPPED : 0u);
            stopped = stop;
            go_on = !stop;
        }
        const uint64_t mg = __builtin_amdgcn_ballot_w64(go_on), ms = __builtin_amdgcn_ballot_w64(stopped);
        if (mg != 0) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(mg);
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&P->round_counts[round + 1u], (uint32_t)__popcll(mg));
            base = __shfl(base, (int)leader);
            if (go_on) P->next_active[base + (uint32_t)__popcll(mg & ((1ull << lane) - 1ull))] = item;
        }
        if (ms != 0 && P->counters && lane == (uint32_t)__builtin_ctzll(ms))
            atomicAdd(&P->counters[C_PIX], (unsigned long long)__popcll(ms));
    }
}

// The end of a pass, over every packed pixel of the rank: a pixel's colour is its Σrgb over the
// samples it has taken -- the combine's `r / scount` for a stopped pixel, the preview for an
// active one -- so an output buffer never seen before is filled whole; padding slots get zeros
// (`direct`: as gs_accumulate_kernel).  The maps, when asked for: the samples taken and the
// stop test's left side as a relative error, sqrt(confidence² · var / n / mean²), from the
// stored Σlum, Σlum².  The block folds its threads' active pixels, Σ samples and max samples
// through LDS in a fixed tree; thread 0 adds them to round_summary with integer atomics (the
// host zeroes it before the kernel), so the totals do not depend on any order.
__global__ __launch_bounds__(256) void gs_round_resolve_kernel(const KParams* __restrict__ P) {
    __shared__ uint32_t s_act[256];
    __shared__ unsigned long long s_sum[256], s_max[256];
    const uint32_t bs = P->ss.batch_size;
    const double confidence_sq = P->ss.confidence * P->ss.confidence;
    uint32_t n_act = 0;
    unsigned long long n_sum = 0, n_max = 0;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < P->capacity; k += gridDim.x * blockDim.x) {
        uint32_t pi = 0, pj = 0;
        const bool real = packed_pixel(P, k, pi, pj);
        const size_t oi = P->direct ? (size_t)pj * (uint32_t)P->cam.image_width + pi : (size_t)k;
        float* o = P->out ? P->out + oi * 3 : nullptr;
        uint8_t* o8 = P->out8 ? P->out8 + oi * 3 : nullptr;
        if (!real) {
            if (P->map_samples) P->map_samples[k] = 0u;
            if (P->map_error) P->map_error[k] = 0.0f;
            if (P->direct) continue;
            if (o) {
                o[0] = 0.0f;
                o[1] = 0.0f;
                o[2] = 0.0f;
            }
            if (o8) {
                o8[0] = 0;
                o8[1] = 0;
                o8[2] = 0;
            }
            continue;
        }
        const uint32_t word = P->pbatches[k];
        const unsigned long long taken = (unsigned long long)(word & ~GS_ADAPT_STOPPED) * bs;
        const double* ps = P->pstate + (size_t)k * 5;
        const double scount = (double)taken;
        const double cr = ps[0] / scount, cg = ps[1] / scount, cb = ps[2] / scount;
        if (o) {
            o[0] = (float)cr;
            o[1] = (float)cg;
            o[2] = (float)cb;
        }
        if (o8) {
            o8[0] = color_byte(cr);
            o8[1] = color_byte(cg);
            o8[2] = color_byte(cb);
        }
        if (P->map_samples) P->map_samples[k] = taken > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)taken;
        if (P->map_error) {
            const double lsum = ps[3], lsq = ps[4];
            const double mean = lsum / scount;
            const double var = 1.0 / (scount - 1.0) * (lsq - lsum * lsum / scount);
            P->map_error[k] = (float)sqrt(confidence_sq * var / scount / (mean * mean));
        }
        n_act += (word & GS_ADAPT_STOPPED) ? 0u : 1u;
        n_sum += taken;
        n_max = taken > n_max ? taken : n_max;
    }
    s_act[threadIdx.x] = n_act;
    s_sum[threadIdx.x] = n_sum;
    s_max[threadIdx.x] = n_max;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            s_act[threadIdx.x] += s_act[threadIdx.x + h];
            s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
            s_max[threadIdx.x] = s_max[threadIdx.x] > s_max[threadIdx.x + h] ? s_max[threadIdx.x] : s_max[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && P->round_summary) {
        atomicAdd(&P->round_summary[0], (unsigned long long)s_act[0]);
        atomicAdd(&P->round_summary[1], s_sum[0]);
        atomicMax(&P->round_summary[2], s_max[0]);
    }
}

#endif  // GS_PIXEL_HPP_VIEWS_ROUNDS
