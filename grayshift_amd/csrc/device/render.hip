// render.hip — persistent-wavefront path-tracing megakernel for gfx950 (MI355X), its helper
// kernels, the table of its instantiations and one launcher per kernel (kernels.hpp).  Device
// code only: the C-ABI of include/grayshift_gpu.h that feeds it is plain C++ in
// csrc/host/scene.cpp and launch.cpp, and what both sides agree on is kernel_abi.hpp.
//
// What it replaces: the reference's per-pixel loop camera.rs:105-114 →
// Camera::sample (camera.rs:125-171) → recursive Camera::ray_color (:174-202) →
// BVHNode::hit (BVH.rs:69-90) / AABB::hit (AABB.rs:58-113) / primitive hits →
// Material::scatter (material.rs) → Texture::value_at / HDRI::sample.
//
// Structure:
//  * a lane owns one work item — a pixel, or for single-batch settings a chunk of one
//    pixel's consecutive samples — and runs its samples in the reference's order, so
//    the per-pixel sums accumulate exactly as camera.rs:138-147 does (chunk sums are
//    added in order by gs_combine_kernel);
//  * a wave hands finished lanes items from its private reserve, refilled by one
//    atomicAdd of up to 32 items on the global queue, so sky pixels never wait for
//    busy ones;
//  * each lane runs a small state machine NEED → TRACE → SHADE → (TRACE | NEED):
//    the wave keeps stepping BVH traversal until `shade_batch` lanes have finished
//    their ray, then shades those lanes together (active-ray packing) while the
//    others keep their traversal state (one record index) for the next round;
//  * traversal is the reference's left-first DFS with a global closest-t, restated
//    over the tree's pre-order records with hit/miss links (no stack), identical in
//    node visits and primitive tests; the most-tested records are mirrored in LDS;
//  * the hit record is recomputed once per ray from (primitive, t) after traversal,
//    which yields the same values the reference computes at every accepted hit.
// All arithmetic is f64 with -ffp-contract=off, as the reference's Rust.

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "../../../include/grayshift_gpu.h"
#include "kernel_abi.hpp"
#include "kernels.hpp"
#include "devmath.hpp"
#include "geometry.hpp"
#include "perlin.hpp"

using namespace gsd;

// (everything inlined: GS_MIN_WAVES, kernel_abi.hpp)
#ifndef GS_NOINLINE
#define GS_NOINLINE __forceinline__
#endif
#ifndef GS_ROOT_RCP
#define GS_ROOT_RCP 1  // sphere roots divided through a refined reciprocal of a (sphere_root_take_ra; A/B: 0)
#endif
// A wave's issue priority raised (s_setprio level, back to 0 after) while it runs a node pass --
// a chain of dependent LDS reads and box tests, latency-bound per wave -- and, in kernels whose
// leaves are not all stationary spheres and whose leaf passes are not C5's mix (staged shading
// without media or nested BVHs), a leaf pass.  Round 6, MI355X (Msamples/s; none / node
// 1 / node 1 + leaf 1 / node 2 + leaf 1 / node 3): C4 8 773 / 8 971 / 8 886 / 8 911 / 8 962, C3
// 13 969 / 13 992 / 14 204 / 14 179 / 14 011, C2 38 267 / 38 279 / 38 385 / 38 365 / 38 450, C1
// 21 346 / 21 123 / 21 547 / 21 475 / 21 507; none / node 1 / node 1 + leaf 1: C5 7 129 / 7 164 /
// 7 057, final_scene 2 750 / 2 772 / 2 807, cornell_smoke 9 702 / 9 700 / 9 770, A2 11 074 / - /
// 11 333 (profiles/r06/ab_wave_priority.txt).  (FEAT: the kernel's template argument where the
// macros are used.)
#ifndef GS_PRIO_NODE
#define GS_PRIO_NODE 1
#endif
#ifndef GS_PRIO_LEAF
#define GS_PRIO_LEAF                                 \
    ((FEAT & GS_FEAT_SPHLEAF) == 0 &&                \
             ((FEAT & GS_FEAT_MIXED) == 0 || (FEAT & (GS_FEAT_MEDIA | GS_FEAT_NESTED)) != 0) \
         ? 1                                         \
         : 0)
#endif
#ifndef GS_PRIO_SHADE
#define GS_PRIO_SHADE 0
#endif
#define GS_PRIO_SET(lvl) do { if (lvl) __builtin_amdgcn_s_setprio(lvl); } while (0)
#define GS_PRIO_CLR(on) do { if (on) __builtin_amdgcn_s_setprio(0); } while (0)
// ISA census build only (-DGS_ISA_MARKS, tools/isa_census.py): assembler comments that
// delimit the node pass, its f64 fallback and the leaf pass in the generated code.
#ifdef GS_ISA_MARKS
#define GS_MARK(s) asm volatile(";; GS_MARK " s)
#else
#define GS_MARK(s) do { } while (0)
#endif


// S_CAM: the lane's next sample needs its camera ray (set by the refill for a new item and
// by the shade pass for a finished sample; one advance() at the loop head serves both).
enum { S_NEED = 0, S_TRACE = 1, S_SHADE = 2, S_DONE = 3, S_CAM = 4 };

// The leaf stage -- the LDS load types and scene loads, the quad source, the primitive, chain,
// list, cube and medium tests, leaf_other -- in a header of its own, which the known-answer
// harness (tests/hip/kat_device.hip) includes too.
#include "leaf.hpp"

// A node record (2 x 16 B) at byte offset `off`: a = (mnx, mny, mxx, mxy), b = (mnz, mxz,
// hit, miss).  (Offsets are u32: fewer than 2^26 records; leaf offsets i * 48 < 2^32.)
// (Bank-swizzled node and quad records were measured and dropped in round 3: C4 -1.4%,
// C5 -1.3%)
__device__ __forceinline__ uint32_t node_half_b(uint32_t off) { return off + 16u; }
__device__ __forceinline__ uint32_t node_global(uint32_t off) { return off; }
template <bool LDS_ONLY>
__device__ __forceinline__ void load_tnode(const uint8_t* s_nodes, const TNode* g, uint32_t off, uint32_t lds_bytes,
                                           u32x4& a, u32x4& b) {
    if (LDS_ONLY || off < lds_bytes) {
        // The kernel has no static LDS (checked at launch), so the node mirror's first byte
        // is LDS address 0 and `off` is the record's LDS address (no address arithmetic).
        a = *(lds_u32x4*)(uintptr_t)off;
        b = *(lds_u32x4*)(uintptr_t)node_half_b(off);
    } else {
        const u32x4* q = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(g) + node_global(off));
        a = q[0];
        b = q[1];
    }
}
// The same, for the node steps of a pass: when no active lane's record lies outside the
// mirror (the common case once the mirror holds the most-tested records) the wave takes
// a scalar branch straight to the LDS reads, with no exec-mask split and no wait on
// global loads; otherwise each lane reads its own record's memory.
template <bool LDS_ONLY>
__device__ __forceinline__ void load_tnode_w(const uint8_t* s_nodes, const TNode* g, uint32_t off, uint32_t lds_bytes,
                                             u32x4& a, u32x4& b) {
    if (LDS_ONLY || __builtin_expect(__builtin_amdgcn_ballot_w64(off >= lds_bytes) == 0, 1)) {
        a = *(lds_u32x4*)(uintptr_t)off;
        b = *(lds_u32x4*)(uintptr_t)node_half_b(off);
    } else {
        load_tnode<false>(s_nodes, g, off, lds_bytes, a, b);
    }
}
__device__ __forceinline__ d3 inv_cert(d3 d) {
    asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z));  // (as inv_of: not hoisted)
    return mk(rcp_cert(d.x), rcp_cert(d.y), rcp_cert(d.z));
}
// Chunk sums and per-sample colours (written once, read by the combine kernel).  (Non-temporal
// stores measured neutral, C4 +0.2%, final_scene +0.7%, and wrote as many fabric bytes: gfx950
// stores leave L2 whatever their flavour, MI355X_MICROARCH.md; profiles/r06/ab_nt_partial.txt.)
__device__ __forceinline__ void st_partial(double* o, double r, double g, double b) {
    o[0] = r;
    o[1] = g;
    o[2] = b;
}
// A leaf record: the sphere's centre and radius squared, its next link and its ABI ref.
template <bool LDS_ONLY>
__device__ __forceinline__ void load_tleaf(const uint8_t* s_leaves, const TLeaf* g, uint32_t i, uint32_t lds_l,
                                           double& cx, double& cy, double& cz, double& rr, uint32_t& next,
                                           uint32_t& ref) {
    u32x4 a, b;
    u32x2 d;
    // (as load_tnode_w: one scalar branch when every active lane's record is mirrored)
    if (LDS_ONLY || __builtin_expect(__builtin_amdgcn_ballot_w64(i >= lds_l) == 0, 1)) {
        const uint8_t* p = s_leaves + i * 48u;
        a = ((lds_u32x4*)p)[0];
        b = ((lds_u32x4*)p)[1];
        d = *(lds_u32x2*)(p + 32);
    } else if (i < lds_l) {
        const uint8_t* p = s_leaves + i * 48u;
        a = ((lds_u32x4*)p)[0];
        b = ((lds_u32x4*)p)[1];
        d = *(lds_u32x2*)(p + 32);
    } else {
        const char* p = reinterpret_cast<const char*>(g) + i * 48u;
        a = reinterpret_cast<const u32x4*>(p)[0];
        b = reinterpret_cast<const u32x4*>(p)[1];
        d = *reinterpret_cast<const u32x2*>(p + 32);
    }
    cx = lo_hi(a.x, a.y);
    cy = lo_hi(a.z, a.w);
    cz = lo_hi(b.x, b.y);
    rr = lo_hi(b.z, b.w);
    next = d.x;
    ref = d.y;
}

// The shading stage -- the HitRecord of an accepted hit, the textures, the sky, Material::emitted /
// scatter in their staged and split forms -- in a header of its own, which the known-answer
// harness (tests/hip/kat_device.hip) includes too.
#include "shading.hpp"


// The placement pilot's count (GS_FEAT_VISITS): one atomic per distinct record among the
// wave's active lanes (every ray of a pilot tests the root and the records below it: one
// atomic per lane on those addresses serialised the pilot, 111 ms on MI355X C4).
// The lead lane is retired every round whatever the ballot returns, so the loop ends
// after at most 64 rounds even if the mask it starts from held a lane that is not active
// here (the round-3 stamps-build hang: DESIGN.md §7); a lane outside `same` but in `m`
// is then counted by nobody, which the pilot's tests would show as a miscount.
__device__ __forceinline__ void count_visit(uint32_t* counts, uint32_t idx) {
    uint64_t m = __builtin_amdgcn_ballot_w64(true);
#pragma unroll 1
    while (m != 0) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(m);
        const uint32_t v = __builtin_amdgcn_readlane(idx, lead);
        const uint64_t same = __builtin_amdgcn_ballot_w64(idx == v);
        if ((threadIdx.x & 63u) == lead) atomicAdd(&counts[v], (uint32_t)__popcll(same));
        m &= ~(same | (1ull << lead));
    }
}

// Diagnostic build only (-DGS_STAMPS): per-wave shader-clock totals of the three loop
// phases, written to their own debug buffer (the d_item_visits pointer, reinterpreted
// as u64[3]) — never to an output.  The stamps' fences perturb scheduling, so only the
// shares are meaningful, not the absolute time.
#if defined(GS_STAMPS)
#define GS_STAMP(t) do { __builtin_amdgcn_sched_barrier(0); t = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
// Region timing inside divergent shading code: the first active lane adds the wave's
// elapsed clock to its wave's LDS slot (one count per wave, whatever the mask).
#define GS_REGION(k, t0) do { uint64_t t1_; GS_STAMP(t1_); \
    const uint64_t em_ = __builtin_amdgcn_read_exec(); \
    if (lane == (uint32_t)__builtin_ctzll(em_)) s_reg[(tid >> 6) * 16 + (k)] += t1_ - (t0); } while (0)
#else
#define GS_STAMP(t) do { } while (0)
#define GS_REGION(k, t0) do { } while (0)
#endif
// Diagnostic builds (-DGS_WATCHDOG=N; on in the stamps build): a wave whose traversal phase
// takes more than N passes, or whose loop more than 64 N iterations, prints every lane's
// state once (the first 4 such waves of the launch) and retires its lanes, so a loop that
// does not end names itself instead of running into the caller's time limit.
#if defined(GS_STAMPS) && !defined(GS_WATCHDOG)
#define GS_WATCHDOG (1 << 20)
#endif
#ifdef GS_WATCHDOG
__device__ unsigned int g_wd_trips;
#endif



template <int FEAT>
#ifdef GS_NUM_VGPR
__attribute__((amdgpu_num_vgpr(GS_NUM_VGPR)))
#endif
__global__ __launch_bounds__(GS_BLOCK, GS_MIN_WAVES) void gs_render_kernel(KArgs A) {
    extern __shared__ __align__(16) uint8_t smem[];
    // An empty batch round (adaptive settings: no active pixel left in this segment) has no
    // item to hand out: return before the mirror copy.
    if ((!(FEAT & GS_FEAT_FIXED) || (FEAT & GS_FEAT_RSPLIT)) && A.P->rounds && A.P->n_items == 0) return;

    // The records a ray most likely tests (placed first by the host) are mirrored in LDS;
    // a lane whose node / leaf index is below lds_nodes / lds_leaves reads it from there
    // (ds_read), the rest from global memory.  The node mirror starts the dynamic LDS, so
    // a node's LDS address is cur << 5 plus a constant the ds_read offset absorbs.
    uint8_t* s_nodes = smem;
    uint8_t* s_leaves = s_nodes + (size_t)A.lds_nodes * sizeof(TNode);
    uint8_t* s_quads = s_leaves + (size_t)A.lds_leaves * sizeof(TLeaf);
    {
        const uint4* src = reinterpret_cast<const uint4*>(A.tnodes);
        uint4* dst = reinterpret_cast<uint4*>(s_nodes);
        for (uint32_t k = threadIdx.x; k < A.lds_nodes * 2u; k += GS_BLOCK) dst[k] = src[k];
        src = reinterpret_cast<const uint4*>(A.tleaves);
        dst = reinterpret_cast<uint4*>(s_leaves);
        for (uint32_t k = threadIdx.x; k < A.lds_leaves * 3u; k += GS_BLOCK) dst[k] = src[k];
        src = reinterpret_cast<const uint4*>(A.tquads);
        dst = reinterpret_cast<uint4*>(s_quads);
        for (uint32_t k = threadIdx.x; k < A.lds_quads * 8u; k += GS_BLOCK) dst[k] = src[k];
        src = reinterpret_cast<const uint4*>(A.cubes);
        dst = reinterpret_cast<uint4*>(s_quads + (size_t)A.lds_quads * sizeof(TQuad));
        for (uint32_t k = threadIdx.x; k < A.lds_cubes * (GS_CUBE_DOUBLES / 2); k += GS_BLOCK) dst[k] = src[k];
    }
    uint8_t* s_cubes = s_quads + (size_t)A.lds_quads * sizeof(TQuad);
    const QuadSrc qs{s_quads, A.tquads, A.lds_quads, s_cubes, A.lds_cubes};
    // Per-lane pixel / path state after the mirror: [L_ND][GS_BLOCK] f64, [L_NI][GS_BLOCK] u32
    // (none of either in lane_state_in_regs kernels: the counters follow the mirror).
    double* s_d = (double*)(s_cubes + (size_t)A.lds_cubes * (GS_CUBE_DOUBLES * 8));
    uint32_t* s_i = (uint32_t*)(s_d + A.lane_nd * GS_BLOCK);
    unsigned long long* s_cnt = (unsigned long long*)(s_i + lane_ni(FEAT) * GS_BLOCK);
#ifdef GS_STAMPS
    unsigned long long* s_reg = s_cnt + 16;  // [(GS_BLOCK / 64) * 16]: shade regions 0-4, leaf kinds 8-15
    if (threadIdx.x < (GS_BLOCK / 64) * 16) s_reg[threadIdx.x] = 0;
#endif
    if (threadIdx.x < GS_CNT_SLOTS) s_cnt[threadIdx.x] = 0;
    __syncthreads();

    const KParams* __restrict__ P = A.P;
    const DevScene& sc = P->sc;
    const gs_camera& cam = P->cam;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t tid = threadIdx.x;
    const uint64_t flushers = __builtin_amdgcn_ballot_w64(tid < GS_CNT_SLOTS);  // the counters' flushing lanes
    const double tmin = 0.001;
    constexpr int kUnroll = unroll_steps(FEAT);  // node steps of an unrolled node pass
    // Every top-level leaf a stationary sphere: no instance is ever hit, so the hit's
    // instance (lane state L_HINST) stays GS_REF_NONE from the kernel's start.
    constexpr bool kSphLeaf = (FEAT & GS_FEAT_SPHLEAF) != 0;
    // A fixed-spp chunked launch (the host's choice, kernel_for): P->chunk != 0, no rounds, no
    // per-sample colours, max_depth > 0 -- a camera ray is always due when advance() runs.
    constexpr bool kFixed = (FEAT & GS_FEAT_FIXED) != 0;
    // ... or a batch round's split items in that form (GS_FEAT_RSPLIT: per-sample colours)
    constexpr bool kRsplit = kFixed && (FEAT & GS_FEAT_RSPLIT) != 0;
    constexpr bool kGeneral = (FEAT & GS_FEAT_GENERAL) != 0;
    // A batch of cameras stacked into one tall frame (GS_FEAT_VIEWS: KParams.views) -- of the fixed
    // kernel, of a split batch round in its form (with GS_FEAT_RSPLIT) or of one in the loop's
    // (without GS_FEAT_FIXED: views_round_kernel_for).  Only the camera-ray step reads it: the
    // claim block's bounds test and L_PIX are the tall frame's.
    constexpr bool kViews = (FEAT & GS_FEAT_VIEWS) != 0;
    // (t_in_lds kernels: the throughput's three fields first, at fixed offsets)
    // (lane_state_in_regs kernels: per-lane locals instead -- every index is a constant, so
    // the fields are plain VGPRs, and the ones a kernel never reads cost nothing)
    constexpr bool kLaneRegs = lane_state_in_regs(FEAT);
    double r_d[L_ND] = {};
    uint32_t r_i[L_NI] = {};
#define LD(k) (*(kLaneRegs ? &r_d[(k)] : &s_d[((k) + (t_in_lds(FEAT) ? 3 : 0)) * GS_BLOCK + tid]))
#define LI(k) (*(kLaneRegs ? &r_i[(k)] : &s_i[(k) * GS_BLOCK + tid]))
    if constexpr (kSphLeaf) LI(L_HINST) = GS_REF_NONE;
    // GS_FEAT_NESTED: the instance chain whose BVH the lane walks (GS_REF_NONE: the top level)
    constexpr bool kNested = (FEAT & GS_FEAT_NESTED) != 0;
    uint32_t ninst_ = GS_REF_NONE;
#define LNINST (*(ninst_in_lds(FEAT) ? &s_i[lane_ninst(FEAT) * GS_BLOCK + tid] : &ninst_))
    if constexpr (kNested) LNINST = GS_REF_NONE;
    // the lane's nested-walk save slot k: the last f64 lane fields (nest_save_lds), else the
    // slot-major global array (slot k of every lane of the grid contiguous)
    double* const s_save = s_d + (size_t)(A.lane_nd - A.nest_lds) * GS_BLOCK + tid;
    const size_t g_lanes = (size_t)gridDim.x * GS_BLOCK;
#define NSAVE(k)                                                                                   \
    (*(nest_save_lds(FEAT) && A.nest_lds ? &s_save[(size_t)(k) * GS_BLOCK]                         \
                                         : &P->nest_save[(size_t)(k) * g_lanes + (size_t)blockIdx.x * GS_BLOCK + tid]))

    uint32_t st = S_NEED;
    bool qdone = false;
    uint32_t res_base = 0, res_cnt = 0;  // the wave's reserve of claimed items (wave-uniform)
    // path state (registers)
    uint64_t rng = 0;
    // path throughput: registers, or the last three f64 lane fields (t_in_lds)
    constexpr bool kTLds = t_in_lds(FEAT);
    double Tr_ = 1, Tg_ = 1, Tb_ = 1;
#define GS_TP(reg, k) (*(kTLds ? &s_d[(k) * GS_BLOCK + tid] : &(reg)))
#define Tr GS_TP(Tr_, 0)
#define Tg GS_TP(Tg_, 1)
#define Tb GS_TP(Tb_, 2)
    Ray ray;
    ray.o = mk(0, 0, 0);
    ray.d = mk(0, 0, 0);
    ray.time = 0;
    RayCert rc{};  // the ray in the certified f32 slab test's terms (geometry.hpp)
    // traversal state
    uint32_t cur = THR_END, hit_ref_ = GS_REF_NONE;
    // the hit primitive's ref: a register, or the lane's L_HREF field (t_in_lds kernels)
    uint32_t& hit_ref = kTLds ? s_i[L_HREF * GS_BLOCK + tid] : hit_ref_;
    double closest = 0.0;
    float closest32 = 0.0f;  // f32(closest)
    const float tmin32 = 0.001f;  // f32(tmin)
    bool fast = false;  // a cert ray: nodes take box_cert (geometry.hpp)
    // The lane has a new ray in `ray` whose traversal state begin_ray has not set up yet:
    // camera rays (advance) and scattered rays (shade) meet in one begin_ray per phase, so
    // a wave pays for it once, not once per branch.
    bool fresh = false;
    // hot counters kept in registers, flushed per pixel
    uint32_t c_nodes = 0, c_sph = 0;  // (per lane: one VALU add beat a 64-bit SALU wave count)

    auto begin_ray = [&]() {
        // AABB::hit's `1.0 / ray.direction[axis]` (AABB.rs:64), hoisted per ray for the certified
        // f32 test's constants (rcp_cert: within 2^-52 of it; the f64 test takes inv_of's exact one)
        const d3 inv = inv_cert(ray.d);
        fast = A.cert_boxes && cert_ray_ok(ray.o, inv);
        rc = make_cert(ray.o, inv);
        cur = A.root;  // the root record's link (THR_*)
        closest = 1.7976931348623157e308;  // f64::MAX (camera.rs:177)
        closest32 = __builtin_inff();
        hit_ref = GS_REF_NONE;
        if constexpr (!kSphLeaf) LI(L_HINST) = GS_REF_NONE;  // (sphere-only trees: never set)
        atomicAdd(&s_cnt[C_RAYS], 1ull);
    };

    // camera.rs:142-146 for one finished sample of colour L
    auto add_sample = [&](double Lr, double Lg, double Lb) {
        if (kRsplit || (!kFixed && P->per_sample)) {  // batch rounds: the sample's colour, summed in order by the combine
            double* o = P->partial + (size_t)LI(L_ITEM) * 3;
            st_partial(o, Lr, Lg, Lb);
            LI(L_ITEM) += GS_ROUND_PIXEL_MAJOR ? 1u : P->seg_n;
        } else {
            LD(L_CSR) += Lr;
            LD(L_CSG) += Lg;
            LD(L_CSB) += Lb;
        }
        if (!kFixed && !P->chunk) {  // a chunk never reaches the stop test: Σlum, Σlum² unused
            double lum = 0.299 * Lr + 0.587 * Lg + 0.144 * Lb;
            LD(L_LSUM) += lum;
            LD(L_LSQ) += lum * lum;
        }
        LI(L_SAMPLE) += 1u;
        LI(L_BLEFT) -= 1u;
    };

    // Start samples until one needs tracing or the pixel is finished:
    // leaves st = S_TRACE (ray ready) or S_NEED (pixel written).
    // End of a chunk: its Σrgb, summed per pixel by gs_combine_kernel.
    // The lane's node-visit and sphere-test counts go to the block's counters at the end of
    // the kernel -- or at an item's end when the launch records per-item visits (the tile
    // plan's pilot), or before a count could overflow.  (Flushing at every item's end ran
    // the compiler's lane-serial reduction loop of two 64-bit atomics per chunk.)
    auto flush_counts = [&]() {
        atomicAdd(&s_cnt[C_NODES], (unsigned long long)c_nodes);
        atomicAdd(&s_cnt[C_SPH], (unsigned long long)c_sph);
        c_nodes = 0;
        c_sph = 0;
    };
    // a stationary-sphere test: a lane count (flushed with c_nodes), or in t_in_lds kernels
    // a wave-aggregated LDS atomic, as prim_test counts the other kinds (no register kept)
    auto count_sph = [&]() __attribute__((always_inline)) {
        if constexpr (kTLds) atomicAdd(&s_cnt[C_SPH], 1ull);
        else c_sph++;
    };
    auto end_chunk = [&]() {
        const uint32_t item = LI(L_ITEM);
        if (!kRsplit && (kFixed || !P->per_sample)) {
            double* o = P->partial + (size_t)item * 3;
            st_partial(o, LD(L_CSR), LD(L_CSG), LD(L_CSB));
        }
#if !defined(GS_STAMPS) && !defined(GS_CERT_CHECK)  // (those builds use item_visits as their record buffer)
        if (P->item_visits) {  // (the item's packed pixel, from its chunk-major sum slot)
            const uint32_t k = item < P->fine_base ? item % P->fine_px
                                                   : P->fine_px + (item - P->fine_base) % (P->capacity - P->fine_px);
            atomicAdd(&P->item_visits[k], c_nodes);
            flush_counts();
        }
#endif
        if ((c_nodes | c_sph) >= (1u << 30)) flush_counts();
        st = S_NEED;
    };

    auto advance = [&]() {
#pragma unroll 1
        for (;;) {
            // (fixed-spp launches: the shade pass ends a chunk at its last sample, so a lane
            // here always has a sample left and max_depth > 0 -- straight to get_ray)
            if (!kFixed && LI(L_BLEFT) == 0) {
                if (P->chunk) {
                    end_chunk();
                    return;
                }
                // end of a batch (camera.rs:149-164)
                const double scount = LD(L_SCOUNT), lsum = LD(L_LSUM), lsq = LD(L_LSQ);
                const double confidence_sq = P->ss.confidence * P->ss.confidence;
                const double tolerance_sq = P->ss.tolerance * P->ss.tolerance;
                double mean = lsum / scount;
                double variance_sq = 1.0 / (scount - 1.0) * (lsq - lsum * lsum / scount);
                double convergence_sq = confidence_sq * variance_sq / scount;
                bool stop = convergence_sq < (mean * mean * tolerance_sq);
                if (!stop) stop = (uint32_t)sat_u64(scount, 4294967295.0, 4294967295ull) > P->ss.max_samples;
                if (stop) {
                    const uint32_t item = LI(L_ITEM);
                    const size_t oi = P->direct ? (size_t)LI(L_PIX) : (size_t)item;
                    const double cr = LD(L_CSR) / scount, cg = LD(L_CSG) / scount, cb = LD(L_CSB) / scount;
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
                    atomicAdd(&s_cnt[C_PIX], 1ull);
#if !defined(GS_STAMPS) && !defined(GS_CERT_CHECK)
                    if (P->item_visits) {
                        P->item_visits[item] = c_nodes;
                        flush_counts();
                    }
#endif
                    if ((c_nodes | c_sph) >= (1u << 30)) flush_counts();
                    st = S_NEED;
                    return;
                }
                if (P->rounds) {  // batch rounds: the sums wait for the next round, maybe in another lane
                    const uint32_t item = LI(L_ITEM);
                    double* ps = P->pstate + (size_t)item * 5;
                    ps[0] = LD(L_CSR);
                    ps[1] = LD(L_CSG);
                    ps[2] = LD(L_CSB);
                    ps[3] = lsum;
                    ps[4] = lsq;
                    P->next_active[atomicAdd(&P->round_counts[P->round + 1u], 1u)] = item;
                    if ((c_nodes | c_sph) >= (1u << 30)) flush_counts();
                    st = S_NEED;
                    return;
                }
                LD(L_SCOUNT) = scount + (double)P->ss.batch_size;
                LI(L_BLEFT) = P->ss.batch_size;
            }
            // Camera::get_ray (camera.rs:204-221) on the seeded stream of this sample
            const uint32_t pix = LI(L_PIX);
            // (a views launch: the pixel of the tall frame lies in view pix / (W H); its index,
            // column and row there, that view's camera and seed -- lanes of a wave may differ)
            uint32_t vpix = pix;
            const gs_camera* vcam = &cam;
            uint64_t vseed = 0;
            if constexpr (kViews) {
                const uint32_t view = udiv(pix, P->u_vpx);
                vpix = pix - view * P->u_vpx.d;
                vcam = &P->views[view].cam;
                vseed = P->views[view].seed;
            }
            const gs_camera& cam = *vcam;  // (image_width: the same in every view and the tall frame)
            const uint32_t pj = udiv(vpix, P->u_w), pi = vpix - pj * (uint32_t)cam.image_width;
            rng = stream_seed(kViews ? vseed : P->seed, vpix, LI(L_SAMPLE));
            atomicAdd(&s_cnt[C_PATHS], 1ull);
            double offx = wy_f64(rng) - 0.5;
            double offy = wy_f64(rng) - 0.5;
            double si = (double)pi + offx, sj = (double)pj + offy;
            d3 ps = add(add(ld3(cam.starting_pixel_pos), muls(ld3(cam.pixel_delta_u), si)),
                        muls(ld3(cam.pixel_delta_v), sj));
            d3 org;
            if (cam.defocus_angle <= 0.0) {
                org = ld3(cam.center);
            } else {  // defocus_disk_sample (camera.rs:223-226, util.rs:36-46)
                double dx, dy;
#pragma unroll 1
                for (;;) {
                    dx = wy_f64(rng) * 2.0 + -1.0;
                    dy = wy_f64(rng) * 2.0 + -1.0;
                    if (dx * dx + dy * dy + 0.0 * 0.0 < 1.0) break;
                }
                org = add(add(ld3(cam.center), muls(ld3(cam.defocus_disk_u), dx)), muls(ld3(cam.defocus_disk_v), dy));
            }
            ray.o = org;
            ray.d = sub(ps, org);
            ray.time = wy_f64(rng);
#if defined(GS_DIAG_DUP) && (GS_DIAG_DUP & 4)
            {  // cost probe: get_ray's draws and arithmetic twice, plus begin_ray's reciprocals
                uint64_t g2 = stream_seed(P->seed, pix, LI(L_SAMPLE));
                asm volatile("" : "+v"(g2));
                double ox2 = wy_f64(g2) - 0.5, oy2 = wy_f64(g2) - 0.5;
                d3 ps2 = add(add(ld3(cam.starting_pixel_pos), muls(ld3(cam.pixel_delta_u), (double)pi + ox2)),
                             muls(ld3(cam.pixel_delta_v), (double)pj + oy2));
                d3 org2 = ld3(cam.center);
                if (cam.defocus_angle > 0.0) {
                    double dx, dy;
#pragma unroll 1
                    for (;;) {
                        dx = wy_f64(g2) * 2.0 + -1.0;
                        dy = wy_f64(g2) * 2.0 + -1.0;
                        if (dx * dx + dy * dy + 0.0 * 0.0 < 1.0) break;
                    }
                    org2 = add(add(ld3(cam.center), muls(ld3(cam.defocus_disk_u), dx)), muls(ld3(cam.defocus_disk_v), dy));
                }
                const d3 d2 = sub(ps2, org2);
                const double tm2 = wy_f64(g2);
                const d3 inv2 = mk(1.0 / d2.x, 1.0 / d2.y, 1.0 / d2.z);
                asm volatile("" ::"v"(inv2.x), "v"(inv2.y), "v"(inv2.z), "v"(tm2), "v"(org2.x), "v"(org2.y), "v"(org2.z));
            }
#endif
            Tr = Tg = Tb = 1.0;
            LI(L_DEPTH) = cam.max_depth;
            if (kFixed || cam.max_depth > 0) {
                fresh = true;  // begin_ray by the caller
                st = S_TRACE;
                return;
            }
            add_sample(0.0, 0.0, 0.0);  // ray_color(ray, 0) = 0 (camera.rs:175)
        }
    };

    uint64_t ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0, acc_refill = 0, acc_trav = 0, acc_shade = 0;
    uint64_t acc_node = 0, acc_leaf = 0;  // stamps build: wave clock in node / leaf passes
    uint64_t dist_ref = 0, dist_kind = 0;  // stamps build: distinct leaf refs / ref kinds per leaf pass
    uint64_t dist_bad = 0;                 // stamps build: those counts' loops that did not converge
    uint64_t it_all = 0, it_node = 0, it_leaf = 0, ln_node = 0, ln_leaf = 0, it_shade = 0, ln_shade = 0;
    uint64_t it_adv = 0, ln_adv = 0;  // stamps build: camera-ray (advance) executions and their lanes
    // stamps build: node steps (lanes) from global memory; wave node steps with any active lane,
    // with any lane reading its record from global memory; active lanes over those steps
    uint64_t d_gvis = 0, d_wsteps = 0, d_wsteps_g = 0, d_wlanes = 0;
#ifdef GS_WATCHDOG
    uint32_t wd_loop = 0;
    // prints the lane's state (once per tripped wave, the launch's first 4) and retires the lane
    auto wd_trip = [&](const char* where, uint32_t count) {
        uint32_t k = 0;
        if (lane == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) k = atomicAdd(&g_wd_trips, 1u);
        k = __builtin_amdgcn_readfirstlane(k);
        if (k < 4)
            printf("GS_WATCHDOG %s n=%u block=%u wave=%u lane=%u st=%u cur=%08x fast=%d closest=%g hit_ref=%08x "
                   "depth=%u bleft=%u item=%u sample=%u res_cnt=%u qdone=%d o=(%g %g %g) d=(%g %g %g)\n",
                   where, count, (unsigned)blockIdx.x, (unsigned)(tid >> 6), lane, st, cur, (int)fast, closest,
                   (uint32_t)hit_ref, LI(L_DEPTH), LI(L_BLEFT), LI(L_ITEM), LI(L_SAMPLE), res_cnt, (int)qdone, ray.o.x,
                   ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z);
        st = S_DONE;
        cur = THR_END;
        fresh = false;
        qdone = true;
    };
#endif
#pragma unroll 1
    for (;;) {
        // ---------------------------------------------------------- refill
        GS_STAMP(ts0);
#ifdef GS_WATCHDOG
        if (++wd_loop > 64u * (uint32_t)GS_WATCHDOG) {
            wd_trip("loop", wd_loop);
            break;
        }
#endif
        // Refill and camera rays: lanes without an item take one (S_NEED -> S_CAM), then every
        // lane whose next sample needs a camera ray -- a new item's first, or the next sample
        // after the shade pass finished one -- runs advance() together, once per loop
        // iteration (the wave pays for get_ray once, not once per refill and once per shade).
        // advance() hands back S_TRACE, or S_NEED when an item ends there (adaptive settings,
        // max_depth 0), which sends the lane round once more.
#pragma unroll 1
        for (;;) {
        uint64_t need = __builtin_amdgcn_ballot_w64(st == S_NEED);
#pragma unroll 1
        while (need != 0 && !qdone) {
            // Lanes take items from the wave's reserve; an empty reserve is refilled with
            // `claim` items by one atomic (a contended device-scope atomic per refill round
            // cost ~5% of wave time with 8-sample items).  Items are independent, so who
            // runs which one changes nothing in the result.
            if (res_cnt == 0) {
                const uint32_t leader = (uint32_t)__ffsll((long long)need) - 1;
                uint32_t base = 0;
                const uint32_t cl = res_base >= P->fine_base ? P->claim_fine : P->claim;
                if (lane == leader) base = atomicAdd(P->queue, cl);
                base = __builtin_amdgcn_readfirstlane(__shfl(base, leader));
                if (base >= P->n_items) {
                    qdone = true;
                    break;
                }
                res_base = base;
                res_cnt = min(cl, P->n_items - base);
            }
            const uint32_t n = (uint32_t)__popcll(need);
            const uint32_t take = min(n, res_cnt);
            const uint32_t base = res_base;
            res_base += take;
            res_cnt -= take;
            const uint32_t tile_px = (uint32_t)(P->tile_w * P->tile_h);
            const bool blocked8 = (P->tile_w % 8 == 0) && (P->tile_h % 8 == 0);
            // set bits of `need` below this lane (v_mbcnt: no 64-bit lane mask kept live)
            // (media / nested / sphere-only kernels; the others keep the popcount of the
            // masked ballot: C3 +0.6%, C5 +1.2%, C4 -0.3% the other way round)
#ifndef GS_RANK_MBCNT
#define GS_RANK_MBCNT ((FEAT & (GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_SPHLEAF)) != 0)
#endif
            const uint32_t rank =
                GS_RANK_MBCNT ? __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u))
                              : (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
            if (st == S_NEED && rank < take) {
                const uint64_t q = (uint64_t)base + (uint64_t)rank;
                if (q >= P->n_items) {
                    st = S_DONE;
                } else {
                    // work order: 8x8 blocks inside each tile (coherent primary rays), a
                    // pixel's chunks adjacent
                    const uint32_t q32 = (uint32_t)q;  // q < n_items < 2^32
                    const bool fine = q32 >= P->fine_base;
                    const uint32_t cpp = fine ? P->fine_cpp : P->cpp, csz = fine ? P->fine_chunk : P->chunk;
                    const uint32_t qr = fine ? q32 - P->fine_base : q32;
                    const uint32_t pr = udiv(qr, fine ? P->u_fcpp : P->u_cpp), ck = qr - pr * cpp;
                    uint32_t slot, x, y;
                    if (kRsplit || (!kFixed && P->rounds)) {  // batch rounds: the packed pixel of active entry pr
                        const uint32_t it = P->active[P->seg_base + pr];
                        slot = udiv(it, P->u_tpx);
                        const uint32_t w = it - slot * tile_px;
                        y = udiv(w, P->u_tw);
                        x = w - y * (uint32_t)P->tile_w;
                    } else {
                        const uint32_t pq = fine ? P->fine_px + pr : pr;
                        slot = udiv(pq, P->u_tpx);
                        const uint32_t w = pq - slot * tile_px;
                        if (blocked8) {
                            const uint32_t b = w >> 6, l = w & 63, bpr = (uint32_t)P->tile_w >> 3;
                            const uint32_t by = udiv(b, P->u_bpr);
                            x = (b - by * bpr) * 8 + (l & 7);
                            y = by * 8 + (l >> 3);
                        } else {
                            y = udiv(w, P->u_tw);
                            x = w - y * (uint32_t)P->tile_w;
                        }
                    }
                    const uint32_t item = slot * tile_px + y * (uint32_t)P->tile_w + x;
                    const uint32_t pos = (uint32_t)P->rank + slot * (uint32_t)P->world_size;
                    const uint32_t tile = P->order ? (uint32_t)P->order[pos] : pos;  // -1: empty slot
                    const uint32_t ty = udiv(tile, P->u_tx), tx = tile - ty * (uint32_t)P->tiles_x;
                    const uint32_t pi = tile == 0xFFFFFFFFu ? 0xFFFFFFFFu : tx * (uint32_t)P->tile_w + x;
                    const uint32_t pj = tile == 0xFFFFFFFFu ? 0xFFFFFFFFu : ty * (uint32_t)P->tile_h + y;
                    if (pi >= (uint32_t)cam.image_width || pj >= (uint32_t)cam.image_height) {
                        if (!kFixed && !P->chunk && !P->direct) {  // padding pixel (chunked: gs_combine_kernel writes it)
                            if (P->out) {
                                float* o = P->out + (size_t)item * 3;
                                o[0] = 0.0f;
                                o[1] = 0.0f;
                                o[2] = 0.0f;
                            }
                            if (P->out8) {
                                uint8_t* o8 = P->out8 + (size_t)item * 3;
                                o8[0] = 0;
                                o8[1] = 0;
                                o8[2] = 0;
                            }
                        }
                    } else {
                        LI(L_PIX) = pj * (uint32_t)cam.image_width + pi;
                        LD(L_CSR) = 0.0;
                        LD(L_CSG) = 0.0;
                        LD(L_CSB) = 0.0;
                        if (kRsplit || (!kFixed && P->per_sample)) {
                            // batch rounds: the sample slots of entry pr, samples ck * csz on
                            LI(L_ITEM) = GS_ROUND_PIXEL_MAJOR ? pr * P->ss.batch_size + ck * csz : ck * csz * P->seg_n + pr;
                            LI(L_SAMPLE) = P->round_base + ck * csz;
                            LI(L_BLEFT) = min(csz, P->ss.batch_size - ck * csz);
                        } else if (kFixed || P->chunk) {
                            // chunk sums, chunk-major: a coarse pixel's at ck * fine_px + item,
                            // a fine one's after every coarse pixel's (the packed pixel and its
                            // queue position share a tile, so both are in the fine region or neither)
                            LI(L_ITEM) = fine ? P->fine_base + ck * (P->capacity - P->fine_px) + (item - P->fine_px)
                                              : ck * P->fine_px + item;
                            LI(L_SAMPLE) = P->sample_base + ck * csz;  // (sample_base: a progressive pass's first sample, else 0)
                            LI(L_BLEFT) = min(csz, P->ss.batch_size - ck * csz);
                            if (ck == 0) atomicAdd(&s_cnt[C_PIX], 1ull);
                        } else if (P->rounds) {
                            // batch rounds, whole-batch items: the pixel's running sums (none
                            // before round 1), then batch `round` in this lane
                            if (P->round_base) {
                                const double* ps = P->pstate + (size_t)item * 5;
                                LD(L_CSR) = ps[0];
                                LD(L_CSG) = ps[1];
                                LD(L_CSB) = ps[2];
                                LD(L_LSUM) = ps[3];
                                LD(L_LSQ) = ps[4];
                            } else {
                                LD(L_LSUM) = 0.0;
                                LD(L_LSQ) = 0.0;
                            }
                            // sample_count after this batch: 0.0 + bs + ... (exact integers)
                            LD(L_SCOUNT) = (double)((uint64_t)P->round_base + P->ss.batch_size);
                            LI(L_ITEM) = item;
                            LI(L_BLEFT) = P->ss.batch_size;
                            LI(L_SAMPLE) = P->round_base;
                        } else {
                            LD(L_LSUM) = 0.0;
                            LD(L_LSQ) = 0.0;
                            // first batch starts (camera.rs:137)
                            LD(L_SCOUNT) = 0.0 + (double)P->ss.batch_size;
                            LI(L_ITEM) = item;
                            LI(L_BLEFT) = P->ss.batch_size;
                            LI(L_SAMPLE) = 0u;
                        }
                        st = S_CAM;
                    }
                }
            }
            need = __builtin_amdgcn_ballot_w64(st == S_NEED);
        }
        // Camera rays in batches (round 5): get_ray's draws, the defocus rejection loop and
        // the stream seed cost a wave as much for a few lanes as for all 64, and after a
        // shade pass only the lanes whose sample ended (~20 of 57 on C4) want one.  So a
        // wave waits until `cam_batch` lanes want a camera ray -- those lanes sit idle, like
        // finished lanes, meanwhile -- unless no lane has a ray to trace or the queue is
        // done.  Each lane's samples and draws are unchanged; only when they start moves.
        const uint64_t cam_m = __builtin_amdgcn_ballot_w64(st == S_CAM);
        if (cam_m != 0 && ((uint32_t)__popcll(cam_m) >= (uint32_t)A.cam_batch || qdone ||
                           __builtin_amdgcn_ballot_w64(st == S_TRACE) == 0)) {
#ifdef GS_STAMPS
            it_adv++;
            ln_adv += (uint64_t)__popcll(cam_m);
#endif
            if (st == S_CAM) {
                GS_MARK("adv_begin");
                advance();
                GS_MARK("adv_end");
            }
        }
        if (qdone || __builtin_amdgcn_ballot_w64(st == S_NEED) == 0) break;
        }
        if (fresh) {  // scattered rays (shade pass) and camera rays together
            begin_ray();
            fresh = false;
        }
        if (st == S_NEED) st = S_DONE;
        if (__builtin_amdgcn_ballot_w64(st == S_TRACE || st == S_SHADE) == 0) break;
        GS_STAMP(ts1);

        // ------------------------------------------------------- traverse
        // Within this phase a lane is TRACE, SHADE or DONE and rays do not change, so the
        // shade count and the slab flavour are wave-uniform SGPR facts: no per-iteration
        // ballot for the former, a scalar branch (no exec-mask juggling) for the latter.
        const uint64_t alive = __builtin_amdgcn_ballot_w64(st != S_DONE);
        // (GS_FEAT_NESTED: a lane's ray changes when it enters or leaves a BVH under an
        // instance, in a leaf pass: recomputed there)
        bool wave_fast = __builtin_amdgcn_ballot_w64(st == S_TRACE && !fast) == 0;
        // Invariant: cur != THR_END exactly for lanes whose ray is still being traced
        // (every other lane holds THR_END), so the loop reads lane states from `cur` alone
        // and only marks finished lanes S_SHADE once it ends.
#ifdef GS_WATCHDOG
        uint32_t wd_trav = 0;
#endif
#pragma unroll 1
        for (;;) {
#ifdef GS_WATCHDOG
            if (++wd_trav > (uint32_t)GS_WATCHDOG) {
                wd_trip("traverse", wd_trav);
                break;
            }
#endif
            const uint64_t tr = __builtin_amdgcn_ballot_w64(cur != THR_END);
            if (tr == 0) break;
            if ((uint32_t)__popcll(alive & ~tr) >= (uint32_t)A.shade_batch) break;
            // Leaf batching: step nodes until `leaf_batch` tracing lanes sit at a leaf (or all
            // do), then test those leaves together, so a wave pays for the node step and the
            // sphere test in different iterations instead of both in every one.  Each lane
            // still processes its refs in the reference's order.  The pass kind is uniform.
            const bool at_leaf = cur > THR_END;
            const uint64_t lm = __builtin_amdgcn_ballot_w64(at_leaf);
            const bool leaf_pass = lm == tr || (uint32_t)__popcll(lm) >= (uint32_t)A.leaf_batch;
#ifdef GS_STAMPS
            uint64_t tp0;
            GS_STAMP(tp0);
            it_all++;
            it_node += !leaf_pass;
            it_leaf += leaf_pass;
            ln_node += leaf_pass ? 0ull : (uint64_t)__popcll(tr & ~lm);
            ln_leaf += leaf_pass ? (uint64_t)__popcll(lm) : 0ull;
#endif
            if (!leaf_pass) {
                GS_MARK("node_begin"); GS_PRIO_SET(GS_PRIO_NODE);
// A node pass takes up to GS_NODE_STEPS node steps per lane, unrolled (the loop head's
// ballots, shade-count and pass-kind tests are paid once per pass, not per node):
// measured on MI355X C4 (leaf batch 12), Msamples/s: 1 step 5487, 2 5788, 4 6049, 8 6205;
// unrolled 4 6303, 6 6384, 8 6451-6456, 10 6417, 12 6334, 16 6378; a ballot to leave the
// pass early once no lane is at a node cost 6% (8 steps: 5833).
#ifndef GS_NODE_STEPS
#define GS_NODE_STEPS 8
#endif
                // FAST (compile time): the wave's rays are all cert rays (wave_fast, uniform
                // for the pass), so the 8 unrolled steps carry no per-step flavour test.
                // LDSP (compile time): no node lane of the wave sits at a record outside the
                // LDS mirror when the pass starts (always with the whole tree mirrored), so a
                // step's one compare, cur < lim, picks the lanes that step -- and reads LDS; a
                // lane whose walk leaves the mirror parks there until the next pass, which
                // then runs the mixed flavour (each step splitting its lanes by memory).
                const uint32_t lim = (FEAT & GS_FEAT_LDSTREE) != 0 ? (uint32_t)THR_END : A.lds_nodes << 5;
                auto node_step = [&](auto fast_tag, auto ldsp_tag) __attribute__((always_inline)) {
                constexpr bool FAST = decltype(fast_tag)::value;
                constexpr bool LDSP = decltype(ldsp_tag)::value;
#ifdef GS_STAMPS
                {
                    const bool glob = !((FEAT & GS_FEAT_LDSTREE) != 0) && cur < THR_END && cur >= (A.lds_nodes << 5);
                    const uint64_t act = __builtin_amdgcn_ballot_w64(LDSP ? cur < lim : cur < THR_END);
                    const uint64_t gl = __builtin_amdgcn_ballot_w64(glob && !LDSP);
                    d_gvis += glob && !LDSP;
                    d_wsteps += act != 0;
                    d_wsteps_g += gl != 0;
                    d_wlanes += (uint64_t)__popcll(act);
                }
#endif
                if (__builtin_expect(LDSP ? cur < lim : cur < THR_END, 1)) {
                    // One 32-B record (2 x 16 B; from LDS, offset = cur, or off the SGPR
                    // base), the box test, and the next record: the hit link or the miss link.
                    u32x4 ra, rb;
                    if constexpr (LDSP) {
                        ra = *(lds_u32x4*)(uintptr_t)cur;
                        rb = *(lds_u32x4*)(uintptr_t)node_half_b(cur);
                    } else {
                        load_tnode_w<(FEAT & GS_FEAT_LDSTREE) != 0>(s_nodes, A.tnodes, cur, A.lds_nodes << 5, ra, rb);
                    }
                    c_nodes++;
                    if constexpr ((FEAT & GS_FEAT_VISITS) != 0) {
                        if (P->visits) count_visit(P->visits, cur >> 5);
                    }
                    const uint32_t me = cur;  // this record
                    if constexpr (FAST) {
                        // the certified decision picks the link at once; lanes f32 cannot
                        // decide (rare) run the reference's f64 test out of line.  (Taking the
                        // link once after the join saves the copy of `cur` but puts the hit
                        // mask in an SGPR pair: VOP3 compare and select, +2 issue cycles.)
                        float d, thr;
                        bool h = box_cert_dt(__uint_as_float(ra.x), __uint_as_float(ra.y), __uint_as_float(rb.x),
                                             __uint_as_float(ra.z), __uint_as_float(ra.w), __uint_as_float(rb.y), rc,
                                             tmin32, closest32, d, thr);
                        cur = h ? rb.z : rb.w;
                        if (__builtin_expect(__builtin_fabsf(d) <= thr, 0)) {  // undecided by f32: the f64 test
                            GS_MARK("fallback_begin");
                            h = box_hit_fast(box64(A.tboxes[me >> 5]), ray.o, inv_of(ray.d), tmin, closest);
                            cur = h ? rb.z : rb.w;
                            GS_MARK("fallback_end");
                        }
#ifdef GS_CERT_CHECK
                        // Diagnostic build: every certified decision re-checked in f64; a
                        // mismatch is counted (counters[15]) and its first 64 cases recorded
                        // (item_visits as f64[64][16]: o, d, f64 box, tmin, closest, f32 verdict).
                        {
                            const TBox bx = A.tboxes[me >> 5];
                            const bool h64 = box_hit(box64(bx), ray.o, inv_of(ray.d), tmin, closest);
                            if (h64 != h) {
                                const unsigned long long k = atomicAdd(&P->counters[15], 1ull);
                                if (k < 64 && P->item_visits) {
                                    double* rec = reinterpret_cast<double*>(P->item_visits) + k * 16;
                                    const double v[16] = {ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, bx.mnx,
                                                          bx.mny, bx.mnz, bx.mxx, bx.mxy, bx.mxz, tmin, closest,
                                                          (double)h, (double)closest32};
                                    for (int q = 0; q < 16; q++) rec[q] = v[q];
                                }
                            }
                        }
#endif
                    } else {  // a wave with a non-cert ray: the f64 compare-select test
                        GS_MARK("slow_begin");
                        const bool h = box_hit(box64(A.tboxes[me >> 5]), ray.o, inv_of(ray.d), tmin, closest);
                        cur = h ? rb.z : rb.w;
                        GS_MARK("slow_end");
                    }
                }
                };
                // The scene's step count (gs_device_scene.node_steps): the full count as one
                // unrolled block (a runtime exit inside it keeps the loop rolled: -1.5% on C4),
                // fewer steps (trees of other-kind leaves) as a loop.  The mixed-memory flavour
                // (a node lane outside the mirror at the pass start: ~10% of C4's passes) and
                // waves holding a non-cert ray (rare) take rolled loops.
                using fast_t = std::integral_constant<bool, true>;
                using slow_t = std::integral_constant<bool, false>;
                using ldsp_t = std::integral_constant<bool, true>;
                using mixed_t = std::integral_constant<bool, false>;
                const bool lds_pass = (FEAT & GS_FEAT_LDSTREE) != 0 ||
                                      __builtin_amdgcn_ballot_w64(cur < THR_END && cur >= lim) == 0;
                if (wave_fast && lds_pass && A.node_steps >= kUnroll) {
#pragma unroll
                    for (int nstep = 0; nstep < kUnroll; nstep++) node_step(fast_t{}, ldsp_t{});
                } else if (wave_fast && lds_pass && A.node_steps == 1) {  // (trees of other-kind leaves, C3)
                    node_step(fast_t{}, ldsp_t{});
                } else if (wave_fast && lds_pass) {
#pragma unroll 1
                    for (int nstep = 0; nstep < A.node_steps; nstep++) node_step(fast_t{}, ldsp_t{});
                } else if (wave_fast) {
#pragma unroll 1
                    for (int nstep = 0; nstep < A.node_steps; nstep++) node_step(fast_t{}, mixed_t{});
                } else {
#pragma unroll 1
                    for (int nstep = 0; nstep < A.node_steps; nstep++) node_step(slow_t{}, mixed_t{});
                }
                GS_MARK("node_end"); GS_PRIO_CLR(GS_PRIO_NODE);
            } else if (kNested && __builtin_amdgcn_ballot_w64(cur == THR_RET) != 0) {
                // Return passes (GS_FEAT_NESTED): a lane whose walk of a BVH under an instance
                // chain ended (the tree's last links are THR_RET) takes back its top-level ray
                // and goes on at the record after the instance's leaf -- where BVHNode::hit's
                // recursion returns from the Translate / RotateY's hit (hittable.rs:107-211).
#ifdef GS_STAMPS
                uint64_t rt0_;
                GS_STAMP(rt0_);
#endif
                if (cur == THR_RET) {
                    ray.o = mk(NSAVE(0), NSAVE(1), NSAVE(2));
                    ray.d = mk(NSAVE(3), NSAVE(4), NSAVE(5));
                    cur = (uint32_t)__double_as_longlong(NSAVE(6));
                    LNINST = GS_REF_NONE;
                }
                GS_REGION(6, rt0_);  // (stamps: return passes)
            } else if (at_leaf) {
                GS_MARK("leaf_begin"); GS_PRIO_SET(GS_PRIO_LEAF);
                double scx, scy, scz, sr;
                uint32_t next, ref;
                load_tleaf<(FEAT & GS_FEAT_LDSTREE) != 0>(s_leaves, A.tleaves, cur & ~THR_LEAF, A.lds_leaves, scx, scy, scz, sr,
                                                         next, ref);
                // Kind-batched leaf passes (GS_LEAF_KIND_BATCH): besides stationary spheres, a
                // pass tests only the leaves of one other kind (the first such lane's); lanes
                // at other kinds keep their leaf for a later pass, so each kind's code runs
                // with its lanes together instead of every kind present running in turn.  On
                // for kernels with BVHs under instances or staged shading, where many kinds
                // meet: final_scene +8.5%, C5 +1.3%; off elsewhere (C3 -1.2%, cornell_smoke
                // -0.4%; profiles/r03/ab_leaf_kind_batch.txt).  Each lane still tests its own
                // leaves in its own order, so nothing it computes changes.
#ifndef GS_LEAF_KIND_BATCH
#define GS_LEAF_KIND_BATCH ((FEAT & (GS_FEAT_NESTED | GS_FEAT_MIXED)) != 0)
#endif
                bool take_leaf = true;
                if constexpr (GS_LEAF_KIND_BATCH && (FEAT & GS_FEAT_SPHLEAF) == 0) {
                    const uint32_t kind = ref >> GS_REF_SHIFT;
                    const uint64_t om = __builtin_amdgcn_ballot_w64(kind != GS_REF_SPHERE);
                    if (om != 0) {
                        const uint32_t k0 = __builtin_amdgcn_readlane(kind, (uint32_t)__builtin_ctzll(om));
                        take_leaf = kind == GS_REF_SPHERE || kind == k0;
                    }
                }
                if (take_leaf) {
                if constexpr ((FEAT & GS_FEAT_VISITS) != 0) {
                    if (P->visits) count_visit(P->visits, P->visit_leaf_base + (cur & ~THR_LEAF));
                }
#ifdef GS_STAMPS
                {  // counted by the pass's first active lane (summed over lanes at the end)
                    // The r03 hang of this build on media scenes was in these counts: its
                    // distinct-KIND loop took `readlane(ref, L) >> GS_REF_SHIFT`, and the builtin
                    // returns int, so the scalar shift was arithmetic while each lane's
                    // `ref >> GS_REF_SHIFT` was logical: a medium's ref (kind 8, bit 31) never
                    // matched its own lane and the mask never emptied (ISA:
                    // profiles/r05/ballot_anomaly_isa.txt).  The readlane results are uint32_t
                    // here, the kinds come from the ref loop, and the picked lane is retired
                    // whatever the ballot returns; dbg[23] counts passes whose ballot missed it.
                    const uint64_t act = __builtin_amdgcn_read_exec();
                    const bool first = __builtin_ctzll(act) == (uint32_t)lane;
                    bool bad = false;
                    uint32_t kinds = 0;
                    uint64_t m = act;
                    while (m) {
                        const uint32_t L = (uint32_t)__builtin_ctzll(m);
                        const uint32_t r0 = __builtin_amdgcn_readlane(ref, L);
                        const uint64_t same = __builtin_amdgcn_ballot_w64(ref == r0);
                        bad |= ((same >> L) & 1u) == 0;
                        kinds |= 1u << (r0 >> GS_REF_SHIFT);
                        m &= ~(same | (1ull << L));
                        dist_ref += first;
                    }
                    dist_kind += first ? (uint64_t)__builtin_popcount(kinds) : 0;
                    dist_bad += bad && first;
                }
#endif
                // a stationary sphere's test (sphere.rs:64-106); its root divisions through one
                // refined reciprocal of a when every active lane's a is in range (as the
                // sphere-only leaf runs below), else the f64 division
                auto sphere_test = [&](d3 c, double rr, double& t) __attribute__((always_inline)) {
                    const double a = len2(ray.d);
                    // (not in media / nested-BVH kernels: final_scene and cornell_smoke measured
                    // neutral, and the media kernel spilled 12 B/lane with it)
                    constexpr bool kRa = GS_ROOT_RCP && (FEAT & (GS_FEAT_MEDIA | GS_FEAT_NESTED)) == 0;
                    if (kRa && __builtin_amdgcn_ballot_w64(!(a >= 0x1p-900 && a <= 0x1p900)) == 0)
                        return sphere_accept_rr_ra(c, rr, ray, a, rcp_cert(a), tmin, closest, t);
                    return sphere_accept_rr(c, rr, ray, a, tmin, closest, t);
                };
                auto sphere_leaf = [&]() __attribute__((always_inline)) {  // a stationary sphere, inline
                    GS_MARK("sphere_begin");
                    count_sph();
                    double t;
                    if (sphere_test(mk(scx, scy, scz), sr, t)) {
                        closest = t;
                        closest32 = (float)t;
                        hit_ref = ref;
                        if constexpr (kNested) LI(L_HINST) = LNINST;  // (a sphere of the tree under LNINST)
                        else if constexpr (!kSphLeaf) LI(L_HINST) = GS_REF_NONE;
                    }
                    GS_MARK("sphere_end");
                };
                if constexpr ((FEAT & GS_FEAT_SPHLEAF) != 0) {
                    // Sphere-only trees: a leaf run's second sphere (the next record, when it
                    // is a leaf) is read right away and both discriminants are computed as two
                    // independent chains; the roots are then taken in order, the second sphere
                    // against the interval the first left (sphere.rs:64-89, BVH.rs:73-80).
                    const bool two = cur_next_is_leaf(next);
                    double s2x, s2y, s2z, s2r;
                    uint32_t next2, ref2;
                    load_tleaf<(FEAT & GS_FEAT_LDSTREE) != 0>(s_leaves, A.tleaves, two ? next & ~THR_LEAF : cur & ~THR_LEAF,
                                                             A.lds_leaves, s2x, s2y, s2z, s2r, next2, ref2);
                    const double a = len2(ray.d);
                    // Root rounds (round 5): the square root and the divisions run once for
                    // the lane's first sphere with a real discriminant (sphere 1, else sphere 2),
                    // then once more only for lanes where both were real.  Run per sphere, both
                    // root blocks executed in most passes (C4 traces: 86% and 76% of leaf passes;
                    // in rounds 97% and 19%).  MI355X C4: 8 025 -> 8 226 Msamples/s.  Order: a
                    // lane whose sphere 1 is real takes it against `closest`, then sphere 2
                    // against what it left; a lane whose sphere 1 is not real takes sphere 2
                    // first, as the reference, whose sphere-1 test changed nothing.
                    const SphereDisc q1 = sphere_disc_rr(mk(scx, scy, scz), sr, ray, a);
                    const SphereDisc q2 = sphere_disc_rr(mk(s2x, s2y, s2z), s2r, ray, a);
                    const bool real1 = !(q1.disc < 0.0), real2 = two && !(q2.disc < 0.0);
                    GS_MARK("sphere_begin");
                    double t;
                    // Root divisions by a from one refined reciprocal per pass (sphere_root_take_ra,
                    // bit-identical for a in [2^-900, 2^900]: a wave-uniform choice, else `/`)
                    const double ra = rcp_cert(a);
                    const bool wave_ra =
                        GS_ROOT_RCP && __builtin_amdgcn_ballot_w64(!(a >= 0x1p-900 && a <= 0x1p900)) == 0;
                    auto take = [&](double hh, double dd) __attribute__((always_inline)) {
                        return wave_ra ? sphere_root_take_ra(hh, dd, a, ra, tmin, closest, t)
                                       : sphere_root_take(hh, dd, a, tmin, closest, t);
                    };
                    if (real1 || real2) {
                        const double hA = real1 ? q1.h : q2.h, dA = real1 ? q1.disc : q2.disc;
                        if (take(hA, dA)) {
                            closest = t;
                            hit_ref = real1 ? ref : ref2;
                        }
                    }
                    if (real1 && real2) {
                        if (take(q2.h, q2.disc)) {
                            closest = t;
                            hit_ref = ref2;
                        }
                    }
                    if (two) {
                        if constexpr ((FEAT & GS_FEAT_VISITS) != 0) {
                            if (P->visits) count_visit(P->visits, P->visit_leaf_base + (next & ~THR_LEAF));
                        }
                        next = next2;
                    }
                    closest32 = (float)closest;
                    c_sph += 1u + (uint32_t)two;
                    GS_MARK("sphere_end");
                } else if ((FEAT & GS_FEAT_SPHLEAF) != 0 || (ref >> GS_REF_SHIFT) == GS_REF_SPHERE) {
#ifdef GS_STAMPS
                    uint64_t k0_;
                    GS_STAMP(k0_);
#endif
                    sphere_leaf();
                    GS_REGION(7 + GS_REF_SPHERE, k0_);
                } else if constexpr ((FEAT & GS_FEAT_SPHLEAF) == 0) {
                    GS_MARK("other_begin");
#ifdef GS_STAMPS
                    // (leaf-kind clock: the branch's first lane's ref kind, before any
                    // instance chain -- one kind per pass with kind-batched leaf passes)
                    uint64_t k0_;
                    GS_STAMP(k0_);
                    const uint32_t kk_ = __builtin_amdgcn_readfirstlane(ref >> GS_REF_SHIFT);
#endif
                    // A leaf pass whose other-kind lanes all sit at one leaf (the Cornell box:
                    // always, with single node steps) tests it with scalar loads.
                    const uint32_t r0 = __builtin_amdgcn_readfirstlane(ref);
                    const bool uni = __builtin_amdgcn_ballot_w64(ref != r0) == 0;
                    LeafHit lh;
                    Ray rl = ray;  // (the ray in the leaf's space after its instance chain)
                    if (uni) lh = leaf_other<FEAT, true>(sc, qs, r0, rl, tmin, closest, rng, s_cnt);
                    else lh = leaf_other<FEAT, false>(sc, qs, ref, rl, tmin, closest, rng, s_cnt);
                    if (lh.hit) {
                        closest = lh.t;
                        closest32 = (float)lh.t;
                        hit_ref = lh.ref;
                        // (a primitive or list in the tree under LNINST; an instance leaf's own chain;
                        // round 6: an instance leaf inside the tree under LNINST -- both chains, the
                        // outer one in the save slot, bit 31 on the inner one)
                        if constexpr (kNested && kGeneral) {
                            if (lh.inst != GS_REF_NONE && LNINST != GS_REF_NONE) {
                                NSAVE(7) = __longlong_as_double((long long)LNINST);
                                LI(L_HINST) = lh.inst | 0x80000000u;
                            } else {
                                LI(L_HINST) = lh.inst != GS_REF_NONE ? lh.inst : LNINST;
                            }
                        } else if constexpr (kNested) {
                            LI(L_HINST) = lh.inst != GS_REF_NONE ? lh.inst : LNINST;
                        } else {
                            LI(L_HINST) = lh.inst;
                        }
                    }
                    if constexpr (kNested) {
                        // The chain ended in a BVH (final_scene's box of balls): the lane walks
                        // the tree in the main loop's node and leaf passes, in the reference's
                        // order, with its ray in the tree's space; the top-level ray and the
                        // link after this leaf wait in the lane's save slot until THR_RET.
                        if (lh.enter) {
                            NSAVE(0) = ray.o.x;
                            NSAVE(1) = ray.o.y;
                            NSAVE(2) = ray.o.z;
                            NSAVE(3) = ray.d.x;
                            NSAVE(4) = ray.d.y;
                            NSAVE(5) = ray.d.z;
                            NSAVE(6) = __longlong_as_double((long long)next);
                            LNINST = ref;
                            ray.o = rl.o;
                            ray.d = rl.d;
                            next = sc.nroots[lh.enter - 1u];
                        }
                    }
                    GS_REGION(7 + (kk_ < 1u ? 1u : kk_ > 8u ? 8u : kk_), k0_);
                    GS_MARK("other_end");
                }
                cur = next;
#ifndef GS_LEAF_RUN
#define GS_LEAF_RUN 2
#endif
                // More leaves in the same pass while the next record is a leaf holding a
                // stationary sphere (the n == 2 leaves of BVH.rs:44-55 sit side by side):
                // up to GS_LEAF_RUN per pass, each tested in order with the updated closest.
                // A template feature: trees without such pairs (the Cornell box's quads and
                // instances) lose ~2% to the loop's mere presence (MI355X C3).
#pragma unroll 1
                for (int k = 1; (FEAT & GS_FEAT_LEAFRUN) && (FEAT & GS_FEAT_SPHLEAF) == 0 &&
                                k < GS_LEAF_RUN && cur > THR_END && (!kNested || cur != THR_RET); k++) {
                    load_tleaf<(FEAT & GS_FEAT_LDSTREE) != 0>(s_leaves, A.tleaves, cur & ~THR_LEAF, A.lds_leaves, scx, scy, scz, sr,
                                                         next, ref);
                    if ((FEAT & GS_FEAT_SPHLEAF) == 0 && (ref >> GS_REF_SHIFT) != GS_REF_SPHERE) break;
                    if constexpr ((FEAT & GS_FEAT_VISITS) != 0) {
                        if (P->visits) count_visit(P->visits, P->visit_leaf_base + (cur & ~THR_LEAF));
                    }
                    count_sph();
                    double t;
                    if (sphere_test(mk(scx, scy, scz), sr, t)) {
                        closest = t;
                        closest32 = (float)t;
                        hit_ref = ref;
                        if constexpr (kNested) LI(L_HINST) = LNINST;
                        else if constexpr (!kSphLeaf) LI(L_HINST) = GS_REF_NONE;
                    }
                    cur = next;
                }
                }  // take_leaf
                GS_MARK("leaf_end"); GS_PRIO_CLR(GS_PRIO_LEAF);
            }
            // Nested-BVH kernels and media kernels with sphere leaf runs: the certified test's
            // ray constants are recomputed after a leaf pass (the same function of the same
            // ray), so they are not live through leaf_other, whose medium and nested tests
            // need the registers (without it these spill 12-36 B/lane).  Media-only kernels
            // (cornell_smoke: a leaf pass after nearly every single node step) have the
            // registers and skip the recomputation (with it: -6.6%).
            // In nested-BVH kernels a lane's ray also changes in a leaf pass (entering or leaving a
            // BVH under an instance): its slab flavour is decided again, and the wave's.
            if constexpr ((FEAT & GS_FEAT_NESTED) != 0 ||
                          (FEAT & (GS_FEAT_MEDIA | GS_FEAT_LEAFRUN)) == (GS_FEAT_MEDIA | GS_FEAT_LEAFRUN)) {
                if (leaf_pass) {
#ifdef GS_STAMPS
                    uint64_t rc0_;
                    GS_STAMP(rc0_);
#endif
                    const d3 inv = inv_cert(ray.d);
                    rc = make_cert(ray.o, inv);
                    if constexpr (kNested) {
                        fast = A.cert_boxes && cert_ray_ok(ray.o, inv);
                        wave_fast = __builtin_amdgcn_ballot_w64(cur != THR_END && !fast) == 0;
                    }
                    GS_REGION(5, rc0_);  // (stamps: the recomputation's share of the leaf-pass clock)
                }
            }
#ifdef GS_STAMPS
            {
                uint64_t tp1;
                GS_STAMP(tp1);
                (leaf_pass ? acc_leaf : acc_node) += tp1 - tp0;
            }
#endif
        }
        if (st == S_TRACE && cur == THR_END) st = S_SHADE;

        // ---------------------------------------------------------- shade
        GS_STAMP(ts2);
#ifdef GS_STAMPS
        {
            const uint64_t sm = __builtin_amdgcn_ballot_w64(st == S_SHADE);
            it_shade += sm != 0;
            ln_shade += (uint64_t)__popcll(sm);
        }
#endif
        if (st == S_SHADE) {
            bool ends = true;
            double Lr = 0.0, Lg = 0.0, Lb = 0.0;
#ifdef GS_STAMPS
            uint64_t r0;
#endif
            if constexpr ((FEAT & (GS_FEAT_MIXED | GS_FEAT_MEDIA | GS_FEAT_NESTED)) != 0) {
                GS_STAMP(r0);
                GS_MARK("shade_begin"); GS_PRIO_SET(GS_PRIO_SHADE);
#if defined(GS_DIAG_DUP) && (GS_DIAG_DUP & 1)
                {  // cost probe: the shade work twice (the copy's results consumed, its counts double)
                    Ray r2 = ray;
                    uint64_t g2 = rng;
                    double c2 = closest;
                    asm volatile("" : "+v"(r2.d.x), "+v"(c2));
                    const ShadeOut s2 = shade<(FEAT & GS_FEAT_PLAIN) != 0, kSphLeaf, kGeneral>(sc, r2, c2, hit_ref, LI(L_HINST), g2, s_cnt);
                    asm volatile("" ::"v"(s2.col.x), "v"(s2.col.y), "v"(s2.col.z), "v"(s2.dir.x), "v"(s2.dir.y), "v"(s2.dir.z),
                                 "v"(r2.o.x), "v"(g2), "v"(s2.cont));
                }
#endif
                // (GS_FEAT_NESTED: a hit through a chain inside a BVH under another chain carries
                // bit 31 on its inner chain's ref, the outer chain in the lane's save slot 7)
                uint32_t hinst = (FEAT & GS_FEAT_PLAIN) ? GS_REF_NONE : LI(L_HINST), houter = GS_REF_NONE;
                if constexpr (kNested && kGeneral) {
                    if (hinst != GS_REF_NONE && (hinst >> 31)) {
                        houter = (uint32_t)__double_as_longlong(NSAVE(7));
                        hinst &= 0x7FFFFFFFu;
                    }
                }
                const ShadeOut s = shade<(FEAT & GS_FEAT_PLAIN) != 0, kSphLeaf, kGeneral>(sc, ray, closest, hit_ref, hinst,
                                                                                        rng, s_cnt, houter);
                GS_MARK("shade_end"); GS_PRIO_CLR(GS_PRIO_SHADE);
                GS_REGION(2, r0);
                if (s.cont) {
                    Tr = Tr * s.col.x;
                    Tg = Tg * s.col.y;
                    Tb = Tb * s.col.z;
                    const uint32_t depth = LI(L_DEPTH) - 1u;
                    LI(L_DEPTH) = depth;
                    if (depth > 0) {
                        ray.d = s.dir;  // (ray.o = p: set by shade)
                        fresh = true;
                        st = S_TRACE;
                        ends = false;
                    }  // else ray_color(.., 0) = 0 (camera.rs:175): black
                } else {
                    // sky (camera.rs:201), emitter (DiffuseLight never scatters) or absorbed (col = 0)
                    Lr = Tr * s.col.x;
                    Lg = Tg * s.col.y;
                    Lb = Tb * s.col.z;
                }
            } else {  // split: one branch per case
                if (hit_ref == GS_REF_NONE) {
                    // miss: sample_background (camera.rs:201); the path's only radiance
                    GS_STAMP(r0);
                    const d3 bg = background(sc, ray.d, s_cnt);
                    GS_REGION(0, r0);
                    Lr = Tr * bg.x;
                    Lg = Tg * bg.y;
                    Lb = Tb * bg.z;
                } else {
                    atomicAdd(&s_cnt[C_HITS], 1ull);
                    GS_STAMP(r0);
                    const HitRec h = kSphLeaf ? reconstruct_sphere<true>(sc, ray, closest, hit_ref)
                                              : reconstruct<false>(sc, ray, closest, hit_ref, LI(L_HINST));
                    GS_REGION(1, r0);
                    GS_STAMP(r0);
                    const Scatter s = scatter(sc, h, ray.d, rng, s_cnt);
                    GS_REGION(2, r0);
                    rng = s.rng;
                    if (s.cont) {
                        Tr = Tr * s.col.x;
                        Tg = Tg * s.col.y;
                        Tb = Tb * s.col.z;
                        const uint32_t depth = LI(L_DEPTH) - 1u;
                        LI(L_DEPTH) = depth;
                        if (depth > 0) {
                            ray.o = h.p;
                            ray.d = s.dir;
                            fresh = true;
                            st = S_TRACE;
                            ends = false;
                        }  // else ray_color(.., 0) = 0 (camera.rs:175): black
                    } else {
                        // emitter (DiffuseLight never scatters) or absorbed (col = 0)
                        Lr = Tr * s.col.x;
                        Lg = Tg * s.col.y;
                        Lb = Tb * s.col.z;
                    }
                }
            }
            if (ends) {  // the sample is done; its item's next camera ray comes at the loop head
                GS_STAMP(r0);
                add_sample(Lr, Lg, Lb);
                if ((kFixed || P->chunk) && LI(L_BLEFT) == 0) end_chunk();  // -> S_NEED
                else st = S_CAM;
                GS_REGION(4, r0);
            }
        }
#ifdef GS_STAMPS
        GS_STAMP(ts3);
        acc_refill += ts1 - ts0;
        acc_trav += ts2 - ts1;
        acc_shade += ts3 - ts2;
#endif
    }
#ifdef GS_STAMPS
    if (P->item_visits && (dist_ref || dist_kind || dist_bad)) {
        unsigned long long* dbg = (unsigned long long*)P->item_visits;
        atomicAdd(&dbg[17], (unsigned long long)dist_ref);
        atomicAdd(&dbg[18], (unsigned long long)dist_kind);
        atomicAdd(&dbg[23], (unsigned long long)dist_bad);
    }
    if (P->item_visits && d_gvis) atomicAdd(&((unsigned long long*)P->item_visits)[19], (unsigned long long)d_gvis);
    if (lane == 0 && P->item_visits) {
        unsigned long long* dbg = (unsigned long long*)P->item_visits;
        atomicAdd(&dbg[0], (unsigned long long)acc_refill);
        atomicAdd(&dbg[1], (unsigned long long)acc_trav);
        atomicAdd(&dbg[2], (unsigned long long)acc_shade);
        atomicAdd(&dbg[3], (unsigned long long)it_all);
        atomicAdd(&dbg[4], (unsigned long long)it_node);
        atomicAdd(&dbg[5], (unsigned long long)it_leaf);
        atomicAdd(&dbg[6], (unsigned long long)ln_node);
        atomicAdd(&dbg[7], (unsigned long long)ln_leaf);
        atomicAdd(&dbg[8], (unsigned long long)it_shade);
        atomicAdd(&dbg[9], (unsigned long long)ln_shade);
        for (int k = 0; k < 5; k++) atomicAdd(&dbg[10 + k], s_reg[(tid >> 6) * 16 + k]);
        for (int k = 0; k < 8; k++) atomicAdd(&dbg[24 + k], s_reg[(tid >> 6) * 16 + 8 + k]);
        for (int k = 5; k < 7; k++) atomicAdd(&dbg[29 + k], s_reg[(tid >> 6) * 16 + k]);  // dbg[34], dbg[35]
        atomicAdd(&dbg[15], (unsigned long long)acc_node);
        atomicAdd(&dbg[16], (unsigned long long)acc_leaf);
        atomicAdd(&dbg[20], (unsigned long long)d_wsteps);
        atomicAdd(&dbg[21], (unsigned long long)d_wsteps_g);
        atomicAdd(&dbg[22], (unsigned long long)d_wlanes);
        atomicAdd(&dbg[32], (unsigned long long)it_adv);
        atomicAdd(&dbg[33], (unsigned long long)ln_adv);

    }
#endif
#undef LD
#undef LI
#undef LNINST
#undef NSAVE
#undef Tr
#undef Tg
#undef Tb
#undef GS_TP

    // flush counters: LDS -> global, one atomic per counter per block
    atomicAdd(&s_cnt[C_NODES], (unsigned long long)c_nodes);
    atomicAdd(&s_cnt[C_SPH], (unsigned long long)c_sph);
    __syncthreads();
    // (the block's first C_N lanes: wave 0, where the lane is the thread index; the test is
    // a wave-uniform mask taken at the start, so no thread-index register is kept to here)
    const uint32_t lane_end = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (((flushers >> lane_end) & 1ull) && P->counters) atomicAdd(&P->counters[lane_end], s_cnt[lane_end]);
}

// Per-launch parameters reach device memory by a one-thread kernel on the caller's stream
// (not a pageable hipMemcpyAsync, which can block the host until earlier work drains and
// would need a host buffer that outlives the copy).
__global__ void gs_params_kernel(KParams kp, KParams* __restrict__ dst) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *dst = kp;
        *kp.queue = 0u;  // (here rather than a memset: one stream operation fewer per frame)
    }
    if (kp.zero_counters && blockIdx.x == 0 && threadIdx.x < sizeof(gs_counters) / 8) kp.counters[threadIdx.x] = 0ull;
}

// A views launch's records reach the slot's array the same way, GS_VIEW_BATCH per launch: one
// 8-byte word per thread (sizeof(gs_view) is a multiple of 8).
__global__ void gs_views_kernel(ViewBatch vb, gs_view* __restrict__ dst) {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(vb.v);
    uint64_t* out = reinterpret_cast<uint64_t*>(dst + vb.first);
    const uint32_t words = vb.n * (uint32_t)(sizeof(gs_view) / 8);
    for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) out[k] = src[k];
}

// The pixel stage -- packed_pixel, the combine and the accumulate kernels, the views pass's order
// and accumulate kernels, the batch rounds' init, params, combine, fold and resolve kernels -- in a
// header of its own, which the known-answer harness (tests/hip/kat_device.hip) includes too.
// (In two halves here, so that the copy kernel between them keeps its place among the code
// object's kernels: pixel.hpp.)
#define GS_PIXEL_FIRST_HALF
#include "pixel.hpp"
#undef GS_PIXEL_FIRST_HALF

// Progressive views: the per-view records of a pass, at most GS_VSTATE_BATCH per call, by value
// like gs_views_kernel's.
__global__ void gs_view_state_kernel(ViewStateBatch vb, GsViewState* __restrict__ dst) {
    const uint64_t* src = reinterpret_cast<const uint64_t*>(vb.s);
    uint64_t* out = reinterpret_cast<uint64_t*>(dst + vb.first);
    for (uint32_t k = threadIdx.x; k < vb.n; k += blockDim.x) out[k] = src[k];
}

#include "pixel.hpp"
#if !defined(GS_PIXEL_HPP_PASSES) || !defined(GS_PIXEL_HPP_VIEWS_ROUNDS)
#error "pixel.hpp: the second include must follow the first, so that both halves are there"
#endif

// =============================================================== the kernel table and launchers
// (kernels.hpp; everything else on the host side lives in csrc/host/scene.cpp and launch.cpp)
void (*kernel_for(int feat))(KArgs) {
#ifdef GS_ONLY_FEAT  // register-pressure experiments (tools/resource_usage.sh): one instantiation
    (void)feat;
    return gs_render_kernel<GS_ONLY_FEAT>;
#else
    // The product instantiations, each also in its fixed-spp form (| GS_FEAT_FIXED) and in the
    // views form of that (| GS_FEAT_FIXED | GS_FEAT_VIEWS; has_views); those without media or BVHs
    // under instances also in the split batch-round form (| GS_FEAT_FIXED | GS_FEAT_RSPLIT;
    // has_rsplit).  The catch-all kernel (GS_K0) has no views form.
#define GS_K0(F)                                             \
    case (F): return gs_render_kernel<(F)>;                  \
    case (F) | GS_FEAT_FIXED: return gs_render_kernel<(F) | GS_FEAT_FIXED>;
#define GS_K(F) \
    GS_K0(F)    \
    case (F) | GS_FEAT_FIXED | GS_FEAT_VIEWS: return gs_render_kernel<(F) | GS_FEAT_FIXED | GS_FEAT_VIEWS>;
#define GS_KR(F) \
    GS_K(F)      \
    case (F) | GS_FEAT_FIXED | GS_FEAT_RSPLIT: return gs_render_kernel<(F) | GS_FEAT_FIXED | GS_FEAT_RSPLIT>;
    switch (feat) {
        GS_K(GS_FEAT_MEDIA)
        GS_K(GS_FEAT_NESTED)
        GS_K(GS_FEAT_MEDIA | GS_FEAT_NESTED)
        GS_KR(GS_FEAT_LEAFRUN)
        GS_K(GS_FEAT_LEAFRUN | GS_FEAT_MEDIA)
        GS_K(GS_FEAT_LEAFRUN | GS_FEAT_NESTED)
        GS_K(GS_FEAT_LEAFRUN | GS_FEAT_MEDIA | GS_FEAT_NESTED)
        GS_KR(GS_FEAT_LDSTREE)
        GS_KR(GS_FEAT_LDSTREE | GS_FEAT_LEAFRUN)
        GS_KR(GS_FEAT_MIXED)
        GS_KR(GS_FEAT_MIXED | GS_FEAT_LEAFRUN)
        GS_KR(GS_FEAT_MIXED | GS_FEAT_LDSTREE)
        GS_KR(GS_FEAT_MIXED | GS_FEAT_LDSTREE | GS_FEAT_LEAFRUN)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_LDSTREE)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_LDSTREE)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_PLAIN)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_PLAIN | GS_FEAT_LDSTREE)
        GS_K0(GS_FEAT_GENERAL_KERNEL)
        GS_KR(GS_FEAT_SPHLEAF)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_LDSTREE)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED | GS_FEAT_LDSTREE)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED | GS_FEAT_PLAIN)
        GS_KR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED | GS_FEAT_PLAIN | GS_FEAT_LDSTREE)
        case GS_FEAT_FIXED: return gs_render_kernel<GS_FEAT_FIXED>;
        case GS_FEAT_FIXED | GS_FEAT_VIEWS: return gs_render_kernel<GS_FEAT_FIXED | GS_FEAT_VIEWS>;
        case GS_FEAT_FIXED | GS_FEAT_RSPLIT: return gs_render_kernel<GS_FEAT_FIXED | GS_FEAT_RSPLIT>;
        case GS_FEAT_PILOT: return gs_render_kernel<GS_FEAT_PILOT>;
        // (a views launch never falls back to a kernel that ignores KParams.views)
        default: return (feat & GS_FEAT_VIEWS) ? nullptr : gs_render_kernel<0>;
    }
#undef GS_K0
#undef GS_KR
#undef GS_K
#endif
}
// The feature word of the instantiation kernel_for(feat) returns: every line of its table maps a
// word to that word's own instantiation, and every other word to the fallback (or to none).
int kernel_feat(int feat) {
#ifdef GS_ONLY_FEAT
    (void)feat;
    return GS_ONLY_FEAT;
#else
    return kernel_for(feat) == kernel_for(0) ? 0 : feat;
#endif
}
// A split batch round may take the (F | FIXED | RSPLIT) instantiation (kernel_for's GS_KR list).
bool has_rsplit(int feat) {
#ifdef GS_ONLY_FEAT
    (void)feat;
    return false;
#else
    return (feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED | GS_FEAT_GENERAL | GS_FEAT_VISITS)) == 0;
#endif
}

// A views launch has its (F | FIXED | VIEWS) instantiation (kernel_for's GS_K list): every
// product kernel but the catch-all one and the pilot's.
bool has_views(int feat) {
#ifdef GS_ONLY_FEAT
    (void)feat;
    return false;
#else
    return (feat & (GS_FEAT_GENERAL | GS_FEAT_VISITS)) == 0 && kernel_for(feat | GS_FEAT_FIXED | GS_FEAT_VIEWS) != nullptr;
#endif
}
// The split batch round of a views adaptation (gs_render_tiles_views_rounds_async), a table of its
// own: one instantiation per product feature set that has a views form.  GS_VR: the sets of
// kernel_for's GS_KR lines (and the empty set), in the fixed kernel's sample loop over the round's
// items (F | FIXED | RSPLIT | VIEWS).  GS_VL: the six media / nested-BVH sets of its GS_K lines, in
// the loop's kernel with per-sample split items (F | VIEWS), as a plain round pass runs them.
// Null for every other word: a views launch has no fallback.
void (*views_round_kernel_for(int feat))(KArgs) {
#ifdef GS_ONLY_FEAT
    (void)feat;
    return nullptr;
#else
#define GS_VR(F) \
    case (F) | GS_FEAT_FIXED | GS_FEAT_RSPLIT | GS_FEAT_VIEWS: return gs_render_kernel<(F) | GS_FEAT_FIXED | GS_FEAT_RSPLIT | GS_FEAT_VIEWS>;
#define GS_VL(F) \
    case (F) | GS_FEAT_VIEWS: return gs_render_kernel<(F) | GS_FEAT_VIEWS>;
    switch (feat) {
        GS_VL(GS_FEAT_MEDIA)
        GS_VL(GS_FEAT_NESTED)
        GS_VL(GS_FEAT_MEDIA | GS_FEAT_NESTED)
        GS_VR(GS_FEAT_LEAFRUN)
        GS_VL(GS_FEAT_LEAFRUN | GS_FEAT_MEDIA)
        GS_VL(GS_FEAT_LEAFRUN | GS_FEAT_NESTED)
        GS_VL(GS_FEAT_LEAFRUN | GS_FEAT_MEDIA | GS_FEAT_NESTED)
        GS_VR(GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_LDSTREE | GS_FEAT_LEAFRUN)
        GS_VR(GS_FEAT_MIXED)
        GS_VR(GS_FEAT_MIXED | GS_FEAT_LEAFRUN)
        GS_VR(GS_FEAT_MIXED | GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_MIXED | GS_FEAT_LDSTREE | GS_FEAT_LEAFRUN)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_PLAIN)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LEAFRUN | GS_FEAT_MIXED | GS_FEAT_PLAIN | GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_SPHLEAF)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED | GS_FEAT_LDSTREE)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED | GS_FEAT_PLAIN)
        GS_VR(GS_FEAT_SPHLEAF | GS_FEAT_MIXED | GS_FEAT_PLAIN | GS_FEAT_LDSTREE)
        GS_VR(0)
        default: return nullptr;
    }
#undef GS_VR
#undef GS_VL
#endif
}
// A views adaptation's rounds have an instantiation for the scene's feature set, in either form.
bool has_views_rounds(int feat) {
    return views_round_kernel_for(feat | GS_FEAT_FIXED | GS_FEAT_RSPLIT | GS_FEAT_VIEWS) != nullptr ||
           views_round_kernel_for(feat | GS_FEAT_VIEWS) != nullptr;
}

// The views of a views launch, at most GS_VIEW_BATCH per call: by value, like gs_params_kernel's
// block, so the caller's array is read before the call returns.
hipError_t launch_views_kernel(hipStream_t st, const ViewBatch& vb, gs_view* dst) {
    hipLaunchKernelGGL(gs_views_kernel, dim3(1), dim3(64), 0, st, vb, dst);
    return hipGetLastError();
}

// Each launcher enqueues one kernel on the stream and returns that launch's error.
hipError_t launch_params_kernel(hipStream_t st, const KParams& kp, KParams* dst) {
    hipLaunchKernelGGL(gs_params_kernel, dim3(1), dim3(64), 0, st, kp, dst);
    return hipGetLastError();
}
hipError_t launch_combine_kernel(hipStream_t st, unsigned grid, const KParams* P) {
    hipLaunchKernelGGL(gs_combine_kernel, dim3(grid), dim3(256), 0, st, P);
    return hipGetLastError();
}
hipError_t launch_accumulate_kernel(hipStream_t st, const KParams* P, uint32_t capacity) {
    hipLaunchKernelGGL(gs_accumulate_kernel, dim3(gs_accum_blocks(capacity)), dim3(256), 0, st, P);
    return hipGetLastError();
}
hipError_t launch_view_state_kernel(hipStream_t st, const ViewStateBatch& vb, GsViewState* dst) {
    hipLaunchKernelGGL(gs_view_state_kernel, dim3(1), dim3(64), 0, st, vb, dst);
    return hipGetLastError();
}
hipError_t launch_views_order_kernel(hipStream_t st, const KParams* P, int32_t* dst, uint32_t n_pos, uint32_t view_h) {
    hipLaunchKernelGGL(gs_views_order_kernel, dim3(gs_views_order_blocks(n_pos)), dim3(256), 0, st, P, dst, n_pos, view_h);
    return hipGetLastError();
}
hipError_t launch_views_accumulate_kernel(hipStream_t st, const KParams* P, uint32_t slots) {
    hipLaunchKernelGGL(gs_views_accumulate_kernel, dim3(slots), dim3(256), 0, st, P);
    return hipGetLastError();
}
hipError_t launch_round_init_kernel(hipStream_t st, unsigned grid, const KParams* P) {
    hipLaunchKernelGGL(gs_round_init_kernel, dim3(grid), dim3(256), 0, st, P);
    return hipGetLastError();
}
hipError_t launch_round_params_kernel(hipStream_t st, KParams* P, uint32_t round, uint32_t seg, uint32_t seg_px,
                                      int32_t chunk_req, int32_t whole_mode) {
    hipLaunchKernelGGL(gs_round_params_kernel, dim3(1), dim3(64), 0, st, P, round, seg, seg_px, chunk_req, whole_mode);
    return hipGetLastError();
}
hipError_t launch_round_combine_kernel(hipStream_t st, unsigned grid, const KParams* P, uint32_t round) {
    hipLaunchKernelGGL(gs_round_combine_kernel, dim3(grid), dim3(256), 0, st, P, round);
    return hipGetLastError();
}
hipError_t launch_round_fold_kernel(hipStream_t st, unsigned grid, const KParams* P, uint32_t round) {
    hipLaunchKernelGGL(gs_round_fold_kernel, dim3(grid), dim3(256), 0, st, P, round);
    return hipGetLastError();
}
hipError_t launch_round_resolve_kernel(hipStream_t st, const KParams* P, uint32_t capacity) {
    hipLaunchKernelGGL(gs_round_resolve_kernel, dim3(gs_accum_blocks(capacity)), dim3(256), 0, st, P);
    return hipGetLastError();
}
hipError_t launch_render_kernel(hipStream_t st, void (*kernel)(KArgs), unsigned blocks, size_t lds, const KArgs& a) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(GS_BLOCK), lds, st, a);
    return hipGetLastError();
}
