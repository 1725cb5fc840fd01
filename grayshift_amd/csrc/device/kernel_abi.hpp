// kernel_abi.hpp — what the kernels (render.hip) and the host code that feeds them
// (csrc/host/scene.cpp, launch.cpp) must agree on: the feature flags, the tunables both sides
// read, the device records, the launch parameter blocks and the lane-state layout in LDS.
// No device builtins: HIP sources and plain C++ sources both compile it, and a variant build's
// -D flags reach both kinds, so they always see the same values.
#pragma once
#include <hip/hip_runtime_api.h>  // (plain C++: __host__ / __device__ expand to nothing)
#include <stddef.h>
#include <stdint.h>

#include "../../../include/grayshift_gpu.h"

// One 1024-lane block per CU (4 waves/SIMD): the block's LDS holds the lane state and
// the largest mirror of the tree's top records (1456 of them; measured on MI355X C4:
// 256-lane blocks with 352 mirrored records 4060, 1024-lane blocks 4150 Msamples/s).
#ifndef GS_BLOCK
#define GS_BLOCK 1024
#endif
// Measured on MI355X (C4): everything inlined with a 4-waves/SIMD register cap (128
// VGPRs; spills only in shading) beats out-of-line shading calls and 3 or 5 waves.
#ifndef GS_MIN_WAVES
#define GS_MIN_WAVES 4
#endif
// The longest Translate / RotateY chain (instances in a row, an outer chain -- a BVH's -- and an
// inner one -- a leaf's inside that BVH -- counted together; round 6: was 4).  reconstruct keeps
// the first 4 in registers and re-walks deeper ones.
#define GS_MAX_CHAIN 16
// Batch rounds (adaptive settings): whole-batch items only for batches up to this size
#ifndef GS_ROUND_WHOLE_MAX_BATCH
#define GS_ROUND_WHOLE_MAX_BATCH 256
#endif
// A split round's per-sample colours: entry a's sample j at j * n + a (sample-major: the
// combine's lanes read one contiguous run per sample), or at a * batch + j (pixel-major: a
// wave's 1-sample items write one contiguous run).  MI355X A2 (round 6): equal render time;
// fabric writes 20.1 vs 15.0 GB a frame, combine 4.2 vs 5.7 ms a frame (5.7 -> 6.2 ms with the
// pixels' samples staged through LDS); profiles/r06/ab_A2_round_items.txt.  The one default: the
// megakernel (render.hip) writes the layout and the pixel stage (pixel.hpp) folds it.
#ifndef GS_ROUND_PIXEL_MAJOR
#define GS_ROUND_PIXEL_MAJOR 0
#endif
#define GS_NESTED_STACK 32  // max depth of a BVH under a Translate/RotateY chain (a validation bound; the walk is stackless)
// Kernel feature flags (template argument): scenes without them compile the code out.
#define GS_FEAT_MEDIA 1   // ConstantMedium leaves (RNG draws inside traversal)
#define GS_FEAT_NESTED 2  // BVHs under Translate/RotateY (a second-level threaded walk)
#define GS_FEAT_LEAFRUN 4 // sphere leaves come in adjacent pairs: leaf passes test runs of them
#define GS_FEAT_LDSTREE 8 // every record of the threaded tree is in the LDS mirror: no global path
                          // (instantiated without media / nested BVHs only; C3 +1%, C5 +2.5%)
#define GS_FEAT_MIXED 16  // three or more of {sky, Lambertian, metal, dielectric, isotropic}:
                          // staged shading (shade), else one branch per case (shade_split);
                          // media / nested-BVH scenes always stage.  MI355X: C4 +2.2%, C5 +1.6%
                          // staged, C3 (Lambertian + light) -2.8% staged
#define GS_FEAT_VISITS 32 // count tests per threaded record (the placement pilot, run_pilot)
#define GS_FEAT_SPHLEAF 64 // every top-level leaf is a stationary sphere (no media / nested BVHs):
                           // leaf passes without the other kinds' code or the kind test
#define GS_FEAT_GENERAL 512 // compositions beyond the reference scenes' (round 6): Translate / RotateY chains
                            // deeper than 4, chains inside a BVH under a chain (two-chain hit records), a BVH
                            // as a ConstantMedium boundary, a medium as a medium's boundary.  One catch-all
                            // instantiation (with media, nested BVHs, leaf runs, staged shading); the other
                            // kernels keep the 4-deep single-chain hit record
#define GS_FEAT_PLAIN 256  // staged shading of sphere-only trees whose materials are all solid / two-solid
                           // checker Lambertians, metals and dielectrics with no uv: the hit record of a
                           // stationary sphere only, no texture, light or isotropic code (round 6; C4)
#define GS_FEAT_FIXED 128  // a fixed-spp launch in sample chunks (KParams.chunk != 0, no batch rounds,
                           // max_depth > 0): the adaptive loop's batch ends, stop test, Σlum / Σlum²
                           // and the rounds' per-sample colours are compiled out (round 6)
#define GS_FEAT_RSPLIT 1024  // with GS_FEAT_FIXED: a batch round of split items (KParams.per_sample,
                             // chunk != 0, max_depth > 0) -- the fixed kernel's sample loop, its items
                             // taken from the round's active list and each sample's colour written for
                             // the combine; no stop test, Σlum or batch end in the kernel (round 6)
#define GS_FEAT_VIEWS 2048   // a batch of cameras as one tall frame (KParams.views; the views calls,
                             // gs_render_tiles_views_async): the camera-ray step takes its camera, seed
                             // and max_depth from the record of the view the pixel lies in.  With
                             // GS_FEAT_FIXED (fixed spp), with GS_FEAT_FIXED | GS_FEAT_RSPLIT or alone (a
                             // views adaptation's split rounds: views_round_kernel_for)
#ifndef GS_NODE_STEPS
#define GS_NODE_STEPS 8  // node steps per unrolled node pass (the render kernel, below)
#endif
__host__ __device__ constexpr int unroll_steps(int feat) { return GS_NODE_STEPS; }
// The pilot's instantiation: every code path (any scene), plus the counts.
#define GS_FEAT_PILOT (GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_VISITS)
#define GS_FEAT_GENERAL_KERNEL (GS_FEAT_GENERAL | GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_LEAFRUN | GS_FEAT_MIXED)

// ---------------------------------------------------------------- device layout
// Internal layouts (may differ from the ABI records; converted at upload).
// Material record with the common texture cases folded in (64 B, one line): a
// Lambertian/DiffuseLight over a SolidColorTexture, or over a CheckeredTexture of two
// solids (the bouncing_spheres ground), reads no texture record at shading time.
enum {
    DM_LAMB_SOLID = 1,    // a = albedo
    DM_LAMB_CHECKER = 2,  // a = even, b = odd, param = scale_inv   (texture.rs:58-70)
    DM_LAMB_TEX = 3,      // generic texture tree: `texture`
    DM_METAL = 4,         // a = albedo, param = fuzz
    DM_DIELECTRIC = 5,    // param = refraction index
    DM_LIGHT_SOLID = 6,   // a = emitted colour
    DM_LIGHT_TEX = 7,     // `texture`
    DM_ISO_SOLID = 8,     // Isotropic over a solid: a = albedo  (material.rs:185-196)
    DM_ISO_TEX = 9        // Isotropic over `texture`
};

namespace gsd {

struct alignas(16) DNode {  // 64 B: box (f64, as AABB.rs) + children
    double mnx, mny, mnz, mxx, mxy, mxz;
    uint32_t left, right, pad0, pad1;
};
struct alignas(16) DSphere {  // 32 B: what Sphere::hit reads; material kept apart
    double cx, cy, cz, r;
};
struct alignas(16) TNode {  // 32 B record of the threaded tree: f32 box (paired for box_cert) + hit / miss links
    float mnx, mny, mxx, mxy, mnz, mxz;
    uint32_t hit, miss;
};
struct alignas(16) TLeaf {  // 48 B leaf record: a stationary sphere inline, next link, ABI ref
    // rr = radius * radius, Sphere::hit's `self.radius * self.radius` (sphere.rs:70) taken
    // once on the host: the same IEEE product the test would take per ray (round 5)
    double cx, cy, cz, rr;
    uint32_t next, ref, pad0, pad1;
};
struct alignas(16) TBox {  // 48 B: the node's f64 box (AABB.rs), for undecided and non-cert rays
    double mnx, mny, mnz, mxx, mxy, mxz;
};
// 128 B traversal copy of a quad (the ABI gs_quad, material aside), ordered by use: the
// plane (normal, D: 32 B) decides most tests; Q, u, v, w (96 B) are read only for a plane
// hit inside the interval.
struct alignas(16) TQuad {
    double nx, ny, nz, d;
    double qx, qy, qz, ux, uy, uz, vx, vy, vz, wx, wy, wz;
};

// Unsigned 32-bit division by a divisor fixed for a launch (image width, tiles per row,
// chunks per pixel, ...): the round-up multiply-shift method (Granlund & Montgomery
// 1994; Hacker's Delight 10-8), exact for every n < 2^32 and every d >= 1 -- 5 VALU
// instead of the ~18 of a division by a runtime value.  The host fills the magic.
struct UDiv {
    uint32_t d, m, s1, s2;
};
__host__ __device__ inline UDiv udiv_make(uint32_t d) {
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) l++;  // ceil(log2 d)
    UDiv u;
    u.d = d;
    u.m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    u.s1 = l < 1 ? l : 1;
    u.s2 = l < 1 ? 0 : l - 1;
    return u;
}

}  // namespace gsd

using gsd::DSphere;
using gsd::TBox;
using gsd::TLeaf;
using gsd::TNode;
using gsd::TQuad;
using gsd::UDiv;

struct alignas(16) DMaterial {
    uint32_t kind, texture, needs_uv, pad;
    double a[3];
    double param;
    double b[3];
    double pad2;
};

enum { C_RAYS = 0, C_NODES, C_SPH, C_MSPH, C_QUAD, C_TRI, C_INST, C_LIST, C_HITS, C_IMG, C_HDRI, C_PATHS, C_PIX, C_MED, C_NOISE, C_N };
#ifdef GS_CERT_CHECK
#define GS_CNT_SLOTS (C_N + 1)  // + slot 15: nested certified-decision mismatches
#else
#define GS_CNT_SLOTS C_N
#endif

struct DevScene {
    // BVHs under Translate/RotateY chains (GS_FEAT_NESTED): their records are threaded into
    // the node and leaf arrays with the top-level tree's; nroots[k] is the link of tree k's
    // root record (an instance whose chain ends in tree k has the child GS_REF_NODE | k).
    const uint32_t* nroots;
    const DSphere* spheres;
    const uint32_t* sphere_mat;
    const gs_msphere* mspheres;
    const gs_quad* quads;
    const gs_triangle* tris;
    const gs_list* lists;       // (a Quad::cube list: {cube index, GS_CUBE_FLAG | first quad}, cube_test)
    const uint32_t* list_refs;
    const double* cubes;        // GS_CUBE_DOUBLES per Quad::cube list (cube_test)
    const gs_instance* inst;
    const gs_medium* media;
    const uint8_t* noise_perm;  // 256 B, Perlin::default()'s table (NoiseTexture)
    const DMaterial* mats;
    const gs_texture* texs;
    const gs_image* images;
    const uint8_t* texels;
    const float* hdri;
    const uint32_t* hdri_rgbe;  // non-null when every texel round-trips through RGBE8
    gs_background bg;
    uint32_t root;
    // the threaded records (GS_FEAT_GENERAL: a BVH as a medium boundary is walked from global
    // memory by tree_test; the kernels' own walks read them through KArgs and the LDS mirror)
    const TNode* tnodes;
    const TBox* tboxes;
    const TLeaf* tleaves;
};

// One view of a progressive views pass (KParams::vstate): the samples its sums held before the
// pass, and whether the pass renders it (1) or only resolves it again (0).
struct GsViewState {
    uint32_t before, selected;
};

// Cold launch parameters: written to device memory per launch and read through a
// pointer at their (conditional) use sites, so they are not hoisted into SGPRs for
// the whole kernel (a by-value struct of this size spilled SGPRs into VGPR lanes,
// costing 16 v_readlane per traversal step).
struct KParams {
    DevScene sc;
    gs_camera cam;
    gs_sample_settings ss;
    uint64_t seed;
    int32_t rank, world_size, tile_w, tile_h, tiles_x, pad;
    uint32_t capacity;  // packed pixel slots of this rank
    // Sample chunking (single-batch settings only): work item q = (packed pixel q / cpp,
    // samples [(q % cpp) * chunk, +chunk)); each item leaves its Σrgb in `partial` and
    // gs_combine_kernel sums a pixel's chunks in chunk order.  chunk == 0: one item per
    // pixel running the reference's batch loop (camera.rs:135-165) to completion.
    // `partial` is chunk-major (round 5): chunk ck of coarse pixel k at ck * fine_px + k, of
    // fine pixel k at fine_base + ck * (capacity - fine_px) + k - fine_px, so the combine's
    // lanes (consecutive pixels) read consecutive sums.
    uint32_t chunk, cpp, n_items;
    // Guided tail: the packed pixels from fine_px on (the rank's last tiles in queue order)
    // run in smaller chunks (fine_chunk samples, fine_cpp per pixel), their items (and
    // sums) from fine_base = fine_px * cpp on, so the frame's last items are short (fine_px =
    // capacity: no fine region).
    uint32_t fine_px, fine_base, fine_chunk, fine_cpp;
    uint32_t claim;  // work items a wave claims per queue atomic (its private reserve)
#ifndef GS_CLAIM_DIV
// claims per wave's share of the items (MI355X C1, 25 4-sample chunks per pixel: 8 -> 18 035-
// 18 079, 4 -> 20 335, 2 -> 20 273 Msamples/s; C2, C4, A1, A2 within noise; the coarse
// claims' cap of 32 binds for large frames either way: profiles/r05/ab_claim_div.txt)
#define GS_CLAIM_DIV 4
#endif
#ifndef GS_CLAIM_FINE
// the claim's cap for items of a few samples: one queue counter serialises the claims (MI355X
// C1, 1-2 sample items: cap 32 -> 6786, 128 -> 12397, 512 -> 12559; perlin 3169, 3221, 2670)
#define GS_CLAIM_FINE 128
#endif
    uint32_t claim_fine;  // the same once the wave's claims reach the fine region
    // multiply-shift forms of the launch's fixed divisors (devmath.hpp UDiv): chunks per
    // pixel, tile pixels, 8x8 blocks per tile row, tile width, tiles per row, image width
    UDiv u_cpp, u_tpx, u_bpr, u_tw, u_tx, u_w, u_fcpp;
    const int32_t* order;  // position -> tile (gs_partition.d_tile_order), or null: tile = position
    double* partial;
    float* out;     // linear colour per packed pixel (nullable when out8 is set)
    uint8_t* out8;  // write_color bytes of the f64 colour per packed pixel (nullable)
    // 1: out / out8 are the W x H frame itself (image pixel j * W + i), padding slots are not
    // written -- the one-device frame context, which then needs no unpack (round 5)
    uint32_t direct;
    uint32_t zero_counters;  // 1: gs_params_kernel zeroes `counters` first (the frame context's own buffer)
    unsigned long long* counters;
    uint32_t* queue;
    uint32_t* item_visits;  // diagnostic: node visits per packed pixel (nullable)
    // GS_FEAT_VISITS launches (the placement pilot): tests per node record position, then
    // per leaf record position from visit_leaf_base
    uint32_t* visits;
    uint32_t visit_leaf_base, pad1;
    // Adaptive settings in batch rounds (rounds = 1; DESIGN.md §3.2 "Adaptive sampling in
    // batch rounds"): launch (round, segment) renders batch `round` of the active packed
    // pixels active[seg_base, seg_base + seg_n).  gs_round_params_kernel sets the per-round
    // fields from the device-side counts and picks one of two item forms:
    //  * whole (many pixels active): item = one pixel's whole batch, run in one lane from the
    //    pixel's running sums (pstate) exactly as the per-lane loop runs it, then the stop test
    //    (camera.rs:149-164) in the lane, which writes the colour or the sums and appends the
    //    pixel to the next round's list;
    //  * split (per_sample = 1, few pixels left): item q = (entry q / cpp, samples
    //    [(q % cpp) * chunk, +chunk) of the batch), every sample's colour to partial[(j *
    //    seg_n + entry) * 3] (sample-major: j = the sample's index in the batch); then
    //    gs_round_combine_kernel folds each pixel's batch into its sums in sample order
    //    (camera.rs:138-147) and takes the stop test.
    uint32_t per_sample, round_base, seg_base, seg_n;
    uint32_t waves, lanes, rounds, round;
    const uint32_t* active;    // this round's active packed pixels
    uint32_t* next_active;     // the next round's, appended by the combine
    uint32_t* active_buf[2];   // the two lists (rounds alternate)
    uint32_t* round_counts;    // [rounds + 1]: active pixels per round
    unsigned long long* rpp_hint;  // [2]: rays, paths of the slot's last split rounds (item sizes; kept across launches)
    double* pstate;            // per packed pixel: the running Σr, Σg, Σb, Σlum, Σlum² (camera.rs:131-146)
    // GS_FEAT_NESTED: per lane (block * GS_BLOCK + thread), the top-level ray while the lane
    // walks a BVH under an instance chain: o, d (6 doubles), the return link (u32), and (the
    // general kernel) a hit's outer chain -- slot k of lane g at [k * grid lanes + g]
    double* nest_save;
    // Progressive passes (gs_render_tiles_pass_async; DESIGN.md §3.2 "Progressive passes"):
    // this launch renders samples [sample_base, sample_base + ss.batch_size) of every pixel,
    // and gs_accumulate_kernel takes gs_combine_kernel's place: it adds the pass's chunk sums
    // to accum (capacity * 3 f64, packed order) and resolves accum / (sample_base + batch_size).
    // Every other launch has sample_base 0 and accum null.
    uint32_t sample_base, pad2;
    double* accum;
    // [gs_accum_blocks(capacity)] per-block sums of |colour after - colour before| (nullable)
    double* delta;
    // Progressive adaptive passes (gs_render_tiles_rounds_async; DESIGN.md §3.2 "Progressive
    // adaptive passes"): the round state (round_counts, the lists, pstate) lives in the caller's
    // blob, every round has split items, and gs_round_fold_kernel takes gs_round_combine_kernel's
    // place: it keeps a stopped pixel's final sums in pstate too and writes no colour.
    // gs_round_resolve_kernel ends the pass.  Every other launch leaves these null.
    uint32_t* pbatches;       // per packed pixel: batches taken, GS_ADAPT_STOPPED once it has stopped
    uint32_t* map_samples;    // per packed pixel: samples taken so far (nullable)
    float* map_error;         // per packed pixel: the stop test's relative error (nullable)
    unsigned long long* round_summary;  // [GS_ROUND_SUMMARY_WORDS]: active pixels, Σ samples, max samples, 0
    // Views (gs_render_tiles_views_async; DESIGN.md §3.2 "Views"): the launch's frame is V views
    // of W x H stacked into W x (V H), view v in rows [v H, (v + 1) H) -- `cam` holds that tall
    // frame's size (the packed-pixel validity test, the output index) and the tiles, chunks,
    // sums and combine run on it unchanged.  A GS_FEAT_VIEWS kernel's camera-ray step reads
    // views[pixel / (W H)] for the camera, the seed and max_depth, and seeds the stream with
    // the pixel's index inside its view.  Every other launch leaves these null / zero.
    const gs_view* views;  // [V] (device)
    UDiv u_vpx;            // W H, the pixels of one view
    // Progressive views (gs_render_tiles_views_pass_async; DESIGN.md §3.2 "Progressive views"): a
    // views launch that is also a pass, over a subset of the views.  `order` is then the launch's
    // own tile order, in which the tiles of unselected views are empty slots (the megakernel
    // retires their pixels without a ray), and gs_views_accumulate_kernel ends the pass: it finds
    // a packed pixel's tile in vorder (the caller's order, every tile in its slot; null: tile =
    // position) and its view's record in vstate.  Tiles do not straddle views (tile_h divides H),
    // so each tile slot belongs to one view, and vdelta takes one partial sum of the pass's change
    // per slot.  Every other launch leaves these null.
    const GsViewState* vstate;  // [V] (device)
    const int32_t* vorder;
    double* vdelta;  // [capacity / (tile_w tile_h)] (nullable)
};
#define GS_ROUND_SUMMARY_WORDS 4

// gs_view_state_kernel's argument: up to GS_VSTATE_BATCH of a views pass's per-view records by
// value, written to dst[first, first + n) of the slot's array.
#define GS_VSTATE_BATCH 256
struct ViewStateBatch {
    GsViewState s[GS_VSTATE_BATCH];
    uint32_t first, n;
};
static_assert(sizeof(GsViewState) == 8 && sizeof(ViewStateBatch) <= 3072, "gs_view_state_kernel copies 8-byte words of a small argument");

// gs_views_kernel's argument: up to GS_VIEW_BATCH of a views launch's records by value (a
// kernel's arguments hold 4 KiB), written to views[first, first + n) of the slot's array.
#define GS_VIEW_BATCH 16
struct ViewBatch {
    gs_view v[GS_VIEW_BATCH];
    uint32_t first, n;
};
static_assert(sizeof(gs_view) % 8 == 0 && sizeof(ViewBatch) <= 3072, "gs_views_kernel copies 8-byte words of a small argument");

// gs_accumulate_kernel's grid: one block of 256 per 256 packed pixels up to 2048 blocks (a
// grid-stride loop past that) -- a function of the capacity alone, so the per-block partial
// sums of the pass's change, and their sum in index order, do not depend on the device.
#define GS_ACCUM_MAX_BLOCKS 2048u
__host__ __device__ constexpr uint32_t gs_accum_blocks(uint32_t capacity) {
    return capacity == 0u ? 1u : ((capacity - 1u) / 256u + 1u < GS_ACCUM_MAX_BLOCKS ? (capacity - 1u) / 256u + 1u : GS_ACCUM_MAX_BLOCKS);
}
// gs_views_order_kernel's grid: one block of 256 per 256 positions up to 1024 blocks (a grid-stride
// loop past that).
__host__ __device__ constexpr uint32_t gs_views_order_blocks(uint32_t n_pos) {
    return (n_pos - 1u) / 256u + 1u < 1024u ? (n_pos - 1u) / 256u + 1u : 1024u;
}

// Hot kernel arguments: what the traversal loop reads every step.
struct KArgs {
    const TNode* tnodes;   // the threaded top-level tree: node records (f32 box, links)
    const TLeaf* tleaves;  // its leaf records
    const TBox* tboxes;    // the f64 box of each node record (undecided / non-cert rays)
    const TQuad* tquads;   // the quads' traversal records (gs_quad order)
    const KParams* P;
    uint32_t root;
    int32_t shade_batch;
    int32_t leaf_batch;  // >= 1: tracing lanes at a leaf before a wave runs a leaf pass
    int32_t node_steps;  // node steps per node pass, 1 .. GS_NODE_STEPS (per scene, see gs_set_node_steps)
    int32_t cam_batch;   // >= 1: lanes waiting for a camera ray before a wave generates them (gs_set_camera_batch)
    int32_t cert_boxes;  // every node coordinate |x| <= 1e15: cert rays may take box_cert
    uint32_t lds_nodes;  // node records [0, lds_nodes) are mirrored in each block's LDS,
    uint32_t lds_leaves; // then leaf records [0, lds_leaves)
    uint32_t lds_quads;  // then quad records [0, lds_quads)
    uint32_t lds_cubes;  // then the Quad::cube records [0, lds_cubes) (cube_test)
    const double* cubes; // (the mirror's source)
    uint32_t lane_nd;    // f64 lane-state fields in LDS: lane_nd(chunked) + nest_lds
    uint32_t nest_lds;   // of which the nested walk's save slots (0: in KParams::nest_save)
};

// DevScene::root in the two-child records' terms: a BVH node is its bare index (< 2^26),
// leaves keep their ABI tag (kind >= 2 in the top 4 bits), "none" is all ones.  (The
// kernels start at KArgs::root, the threaded tree's first link; this form is kept for the
// scene record only.)
#define DREF_NONE 0xFFFFFFFFu
#define DREF_LEAF (1u << GS_REF_SHIFT)
__host__ __device__ inline uint32_t device_ref(uint32_t abi_ref) {
    if (abi_ref == GS_REF_NONE) return DREF_NONE;
    if ((abi_ref >> GS_REF_SHIFT) == GS_REF_NODE) return abi_ref & GS_REF_MASK;
    return abi_ref;
}

// Threaded top-level tree.
// BVHNode::hit's left-first recursion (BVH.rs:69-90) visits the tree in pre-order, and a
// box miss skips exactly the node's subtree.  So the top-level tree is stored as its
// pre-order sequence of records — one per node AND one per leaf occurrence — where a node
// record holds its box, a hit link (the next record: its left child) and a miss link (the
// record after its subtree), and a leaf record holds the primitive's ABI ref, a stationary
// sphere's centre/radius inline, and its next link.  The walk is then `cur = hit ? hit_link
// : miss_link` with no stack: the same records tested in the same order with the same
// closest t, minus every push, pop and LDS stack slot.  Links are record indices, a leaf's
// tagged with THR_LEAF; THR_END ends the walk.
#define THR_END 0x7FFFFFFFu
#define THR_LEAF 0x80000000u
// The last links of a BVH under an instance chain (GS_FEAT_NESTED): "back to the top-level
// ray" -- a leaf-tagged value no leaf index reaches (< 2^26), so a lane there waits for a
// leaf pass like a lane at a leaf.
#define THR_RET 0xFFFFFFFFu
// A node's link is its record's byte offset (32-B TNode; render.hip, load_tnode).
__host__ __device__ constexpr uint32_t node_link(uint32_t pos) { return pos << 5; }

// The aligned form's tag (aligned_tquad, host: the cube records' derivation): a
// signalling-NaN first word carrying the axis code 2 a + o.  (Single quads in the aligned
// form, with per-lane selects or compile-time copies per axis code, were measured and
// dropped in round 4, profiles/r04/ab_aligned_quads.txt.)
#define GS_AQ_TAG 0xFFF4A5C0u
// A Quad::cube list's 96-B device record (render.hip, cube_test; built by the host's cube_record)
#define GS_CUBE_FLAG 0x80000000u
#define GS_CUBE_DOUBLES 12
__host__ __device__ constexpr int cube_code(int k) { return k == 0 || k == 2 ? 4 : (k == 1 || k == 3 ? 1 : 3); }
// face k's D', Q_iu, Q_iv, U_iu, V_iv, W' as (record index, sign): quad.rs:73-78 in order
__host__ __device__ constexpr int cube_src(int k, int f) {
    constexpr int t[6][6] = {{5, 0, 1, 6, 7, 9},    {3, 5, 1, -8, 7, -10}, {2, 3, 1, -6, 7, -9},
                             {0, 2, 1, 8, 7, 10},   {4, 0, 5, 6, -8, -11}, {1, 0, 2, 6, 8, 11}};
    return t[k][f];
}

// Per-lane pixel state lives in LDS ([field][lane], conflict-free), touched once per
// path; the mirror of the tree's top records follows it.
enum { L_CSR = 0, L_CSG, L_CSB, L_LSUM, L_LSQ, L_SCOUNT, L_ND };
enum { L_ITEM = 0, L_PIX, L_BLEFT, L_SAMPLE, L_DEPTH, L_HINST, L_NI };  // (sample, depth, hit
// instance: per-path state touched once per bounce, kept out of the traversal loop's VGPRs)

// Lane state plus the block's 64-bit counters (C_N of them, 128 B).  There is no static
// LDS: the dynamic LDS then starts at address 0, so a node's LDS address is its byte
// offset itself (node links are pre-shifted, below).
#ifdef GS_STAMPS
#define GS_STAMP_LDS ((GS_BLOCK / 64) * 16 * 8)
#else
#define GS_STAMP_LDS 0
#endif
// Fixed-spp (chunked) launches never reach the stop test, so their lanes keep only the
// three colour sums: the 24 KiB of Σlum / Σlum² / sample-count slots go to the mirror.
enum { L_ND_CHUNKED = L_LSUM };
// Media / nested-BVH kernels keep the path throughput (Tr, Tg, Tb: read and written only
// by the shade pass) in three more f64 lane fields (before those), out of the registers their
// leaf tests need (round 3: with them in VGPRs these instantiations spilled 52-76 B/lane).
// (not the placement pilot's counting kernel: it launches with the scene's own lane layout)
__host__ __device__ constexpr bool t_in_lds(int feat) {
    return (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED)) != 0 && (feat & GS_FEAT_VISITS) == 0;
}
// ... and, in kernels that walk BVHs under instances, the lane's save slots (the top-level
// ray, the return link and -- the general kernel -- a hit's outer chain, while the lane walks
// such a tree) in 7 or 8 more f64 fields at the end when the block's LDS has room for them
// beside the whole mirror (KArgs::nest_lds): written at each tree entry, read at its THR_RET.
// Else in global memory (KParams::nest_save, slot-major; also the pilot's counting kernel).
// Off by default: the one scene it helps by traffic (final_scene: 9x fewer fabric writes) lost
// 5% to the mirror records the slots displace, and the run-time choice between the two homes
// cost final_scene 2% more in the kernel that has both (profiles/r06/ab_nest_save_lds.txt).
#ifndef GS_NEST_SAVE_LDS
#define GS_NEST_SAVE_LDS 0
#endif
__host__ __device__ constexpr uint32_t nest_save_lds(int feat) {
    return (GS_NEST_SAVE_LDS && (feat & GS_FEAT_NESTED) != 0 && (feat & GS_FEAT_VISITS) == 0)
               ? ((feat & GS_FEAT_GENERAL) ? 8u : 7u)
               : 0u;
}
// The fixed-spp sphere-leaf kernels (GS_FEAT_FIXED && GS_FEAT_SPHLEAF, their views and split-round
// forms included: C1, C2, C4) keep the whole lane state in registers instead: three colour sums
// and five words, touched once per sample or per item, fit the VGPRs those instantiations leave
// idle under the 4-waves/SIMD cap (<468>: 104 of 128), and their 48 KiB of LDS go to the mirror,
// which is read at every node step.  `feat` is the launched instantiation's own word (the host:
// kernel_feat), not the scene's: the loop's kernel of the same scene keeps the LDS layout.
#ifndef GS_LANE_REGS
#define GS_LANE_REGS 1  // (A/B: 0 keeps every kernel's lane state in LDS)
#endif
__host__ __device__ constexpr bool lane_state_in_regs(int feat) {
    return GS_LANE_REGS && (feat & GS_FEAT_FIXED) != 0 && (feat & GS_FEAT_SPHLEAF) != 0 &&
           (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_GENERAL | GS_FEAT_VISITS)) == 0;
}
__host__ __device__ constexpr uint32_t lane_nd(bool chunked, int feat) {
    return lane_state_in_regs(feat) ? 0u : (chunked ? (uint32_t)L_ND_CHUNKED : (uint32_t)L_ND) + (t_in_lds(feat) ? 3u : 0u);
}
// ... and the hit primitive's ref (written by leaf tests, read by the shade pass) in one
// more u32 field, L_HREF.
enum { L_HREF = L_NI };
// ... and, in kernels that walk BVHs under instances (GS_FEAT_NESTED), the instance chain
// whose tree the lane walks (GS_REF_NONE at the top level) in one more, L_NINST (not the
// placement pilot's: it launches with the scene's own lane layout and keeps it in a register).
__host__ __device__ constexpr bool ninst_in_lds(int feat) {
    return (feat & GS_FEAT_NESTED) != 0 && (feat & GS_FEAT_VISITS) == 0;
}
__host__ __device__ constexpr uint32_t lane_ninst(int feat) { return (uint32_t)L_NI + (t_in_lds(feat) ? 1u : 0u); }
__host__ __device__ constexpr uint32_t lane_ni(int feat) {
    return lane_state_in_regs(feat) ? 0u : lane_ninst(feat) + (ninst_in_lds(feat) ? 1u : 0u);
}
__host__ __device__ constexpr size_t lane_lds_bytes(bool chunked, int feat, uint32_t nsave = 0) {
    return (size_t)GS_BLOCK * ((lane_nd(chunked, feat) + nsave) * 8 + lane_ni(feat) * 4) + 128 + GS_STAMP_LDS;
}
