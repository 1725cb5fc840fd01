// bvh_build.hip — BVHNode::from_list (BVH.rs:15-65) built on the device, bit for bit.
//
// The reference draws no random axis: a node's box is the left fold of its members' boxes in
// their current order, the axis is bbox.longest_axis(), the members are stably sorted on
// bbox[axis].min and split at len / 2.  The tree's shape is therefore a function of n alone
// (bvh_shape.hpp) and only the members' order and the boxes depend on the data, so the host
// enqueues a fixed sequence of launches with no read-back, level by level from the root:
//
//   per level with segments of more than BVH_T members (global passes)
//     fold    one workgroup per segment: box fold, axis, the node, the two child segments
//     keys    one record (segment, key, position) per member
//     sort    a bitonic sort of all records (LDS steps for strides inside a 2048 chunk)
//     apply   order'[i] = order[record[i].position]
//   a segment of at most BVH_T members is finished by one workgroup, whole subtree in LDS
//
// Exactness.  The fold's only order dependence is the sign of a zero bound (-0.0 <= +0.0 and
// +0.0 <= -0.0 both hold, the earlier value stays), so a parallel fold takes the minimum of
// (value with -0.0 = +0.0, position) and writes that member's own bits; AABB::EMPTY is the
// candidate before position 0.  The sort's equal keys keep the order the parent level left
// them in: the position is the key's last word, which makes keys unique.  NaN bounds (the
// host throws) raise a flag that gs_bvh_build_status reports; the kernels complete normally.
//
// No kernel waits on another block.  Every kernel runs without scratch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdio>
#include <string>

#include "../../../include/grayshift_gpu.h"
#include "../host/bvh_shape.hpp"

extern "C" void gs_set_last_error(const char* msg);

namespace {

// Members one workgroup finishes in LDS.  A workgroup may declare all 160 KiB of a CU's LDS;
// a member costs 26 B there (16 record, 4 order, and 12 of fold slots per two members), so
// 6301 fit: the largest power of two below is 4096 (106 KiB in all).
constexpr uint32_t BVH_T = 4096;
constexpr int SUB_THREADS = 1024;
constexpr int SUB_PER = BVH_T / SUB_THREADS;
constexpr int FOLD_THREADS = 256;
constexpr int SORT_THREADS = 256;
constexpr uint32_t SORT_CHUNK = 2048;  // records a sort block holds in LDS (32 KiB)
constexpr int ELEM_THREADS = 256;
constexpr uint32_t NOPOS = 0xFFFFFFFFu;
constexpr uint32_t PAD_SEG = 0xFFFFFFFFu;
constexpr size_t HEADER_BYTES = 256;  // word 0: the NaN flag

struct Rec {  // 16 B: ordered by (seg, key, pos)
    unsigned long long key;
    uint32_t seg, pos;
};
struct Seg {  // a segment of the current level: members [start, start + size), its node
    uint32_t start, size, node, axis;
};

// f64 -> u64 of the same order, -0.0 and +0.0 equal (partial_cmp; NaN is flagged elsewhere).
__device__ __forceinline__ unsigned long long ord_key(double v) {
    v = (v == 0.0) ? 0.0 : v;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ bool rec_less(const Rec& a, const Rec& b) {
    if (a.seg != b.seg) return a.seg < b.seg;
    if (a.key != b.key) return a.key < b.key;
    return a.pos < b.pos;
}
__device__ __forceinline__ int longest_axis(double sx, double sy, double sz) {  // AABB.rs:115-121
    if (sx > sy) return sx > sz ? 0 : 2;
    return sy > sz ? 1 : 2;
}
__device__ __forceinline__ uint32_t leaf_ref(const uint32_t* refs, uint32_t member) {
    return refs ? refs[member] : GS_MAKE_REF(GS_REF_BUILD_MEMBER, member);
}

__global__ __launch_bounds__(ELEM_THREADS) void gs_bvh_init_kernel(uint32_t n, uint32_t* order, Seg* segs,
                                                                   uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * ELEM_THREADS + threadIdx.x;
    if (i < n) order[i] = (uint32_t)i;
    if (i == 0) {
        flag[0] = 0;
        segs[0] = Seg{0u, n, 0u, 0u};
    }
}

// One workgroup per segment of the level: segments of more than BVH_T members get their node
// here; every segment gets its two entries of the next level (size 0: nothing left to do).
__global__ __launch_bounds__(FOLD_THREADS) void gs_bvh_fold_kernel(const double* __restrict__ boxes,
                                                                   const uint32_t* __restrict__ order, Seg* segs,
                                                                   Seg* next, gs_node* nodes, uint32_t node_base,
                                                                   uint32_t* flag) {
    __shared__ unsigned long long s_ext[6];
    __shared__ uint32_t s_pos[6];
    __shared__ double s_val[6];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const Seg sg = segs[s];
    if (sg.size <= BVH_T) {
        if (next && tid == 0) {
            next[2 * (size_t)s] = Seg{0u, 0u, 0u, 0u};
            next[2 * (size_t)s + 1] = Seg{0u, 0u, 0u, 0u};
        }
        return;
    }
    // each thread folds its members in position order; position 0 is AABB::EMPTY
    double v[6];
    uint32_t p[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        v[c] = c < 3 ? DBL_MAX : -DBL_MAX;
        p[c] = 0;
    }
    bool nan = false;
#pragma unroll 4
    for (uint32_t j = tid; j < sg.size; j += FOLD_THREADS) {
        const double* b = boxes + (size_t)order[(size_t)sg.start + j] * 6;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double x = b[c];
            nan |= x != x;
            if (c < 3 ? x < v[c] : x > v[c]) {
                v[c] = x;
                p[c] = j + 1;
            }
        }
    }
    if (nan) atomicOr(flag, 1u);
    if (tid < 6) {
        s_ext[tid] = tid < 3 ? ~0ull : 0ull;
        s_pos[tid] = NOPOS;
    }
    __syncthreads();
    unsigned long long k[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        k[c] = ord_key(v[c]);
        if (c < 3) atomicMin(&s_ext[c], k[c]);
        else atomicMax(&s_ext[c], k[c]);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 6; c++)
        if (k[c] == s_ext[c]) atomicMin(&s_pos[c], p[c]);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 6; c++)
        if (k[c] == s_ext[c] && p[c] == s_pos[c]) s_val[c] = v[c];  // (several only for EMPTY: same bits)
    __syncthreads();
    if (tid == 0) {
        gs_node nd;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            nd.min[c] = s_val[c];
            nd.max[c] = s_val[3 + c];
        }
        const uint32_t h = sg.size / 2;
        const uint32_t lnode = sg.node + 1, rnode = sg.node + 1 + (uint32_t)gs_shape_nodes(h);
        nd.left = GS_MAKE_REF(GS_REF_NODE, node_base + lnode);
        nd.right = GS_MAKE_REF(GS_REF_NODE, node_base + rnode);
        nd.pad[0] = nd.pad[1] = 0;
        nodes[sg.node] = nd;
        segs[s].axis = (uint32_t)longest_axis(nd.max[0] - nd.min[0], nd.max[1] - nd.min[1], nd.max[2] - nd.min[2]);
        if (next) {
            next[2 * (size_t)s] = Seg{sg.start, h, lnode, 0u};
            next[2 * (size_t)s + 1] = Seg{sg.start + h, sg.size - h, rnode, 0u};
        }
    }
}

// The sort record of every position of the padded array at level `level`.  A position finds its
// segment by walking the splits from n (the shape is a function of n); positions of segments
// that are finished, and the padding, get key 0 and so stay where they are.
__global__ __launch_bounds__(ELEM_THREADS) void gs_bvh_keys_kernel(const double* __restrict__ boxes,
                                                                   const uint32_t* __restrict__ order,
                                                                   const Seg* __restrict__ segs, uint32_t n,
                                                                   uint32_t padded, int level, Rec* rec) {
    const size_t i = (size_t)blockIdx.x * ELEM_THREADS + threadIdx.x;
    if (i >= padded) return;
    Rec r{0ull, PAD_SEG, (uint32_t)i};
    if (i < n) {
        uint32_t start = 0, size = n, s = 0;
        for (int l = 0; l < level; l++) {
            const uint32_t h = size / 2;
            if (i < (size_t)start + h) {
                size = h;
                s = 2 * s;
            } else {
                start += h;
                size -= h;
                s = 2 * s + 1;
            }
        }
        const Seg sg = segs[s];
        r.seg = s;
        if (sg.size > BVH_T) r.key = ord_key(boxes[(size_t)order[i] * 6 + sg.axis]);
    }
    rec[i] = r;
}

__device__ __forceinline__ void bitonic_step(Rec* s, uint32_t half, uint32_t base, uint32_t k, uint32_t j,
                                             uint32_t tid, uint32_t threads) {
    for (uint32_t t = tid; t < half; t += threads) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
        const bool asc = ((base + i) & k) == 0;
        const Rec a = s[i], b = s[l];
        if (rec_less(b, a) == asc) {
            s[i] = b;
            s[l] = a;
        }
    }
    __syncthreads();
}

// A block's chunk of SORT_CHUNK records in LDS: k_outer == 0 sorts the chunk (every step up to
// k = SORT_CHUNK), else the steps j < SORT_CHUNK of the merge k_outer.
__global__ __launch_bounds__(SORT_THREADS) void gs_bvh_sort_local_kernel(Rec* rec, uint32_t k_outer) {
    __shared__ Rec s[SORT_CHUNK];
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SORT_CHUNK;
    for (uint32_t t = tid; t < SORT_CHUNK; t += SORT_THREADS) s[t] = rec[base + t];
    __syncthreads();
    if (k_outer == 0) {
        for (uint32_t k = 2; k <= SORT_CHUNK; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_step(s, SORT_CHUNK / 2, (uint32_t)base, k, j, tid, SORT_THREADS);
    } else {
        for (uint32_t j = SORT_CHUNK >> 1; j > 0; j >>= 1)
            bitonic_step(s, SORT_CHUNK / 2, (uint32_t)base, k_outer, j, tid, SORT_THREADS);
    }
    for (uint32_t t = tid; t < SORT_CHUNK; t += SORT_THREADS) rec[base + t] = s[t];
}

// One step (k, j >= SORT_CHUNK) over the whole padded array; a thread owns one pair.
__global__ __launch_bounds__(ELEM_THREADS) void gs_bvh_sort_global_kernel(Rec* rec, uint32_t padded, uint32_t k,
                                                                          uint32_t j) {
    const size_t t = (size_t)blockIdx.x * ELEM_THREADS + threadIdx.x;
    if (t >= padded / 2) return;
    const size_t i = ((t & ~(size_t)(j - 1)) << 1) | (t & (j - 1)), l = i + j;
    const bool asc = (i & k) == 0;
    const Rec a = rec[i], b = rec[l];
    if (rec_less(b, a) == asc) {
        rec[i] = b;
        rec[l] = a;
    }
}

__global__ __launch_bounds__(ELEM_THREADS) void gs_bvh_apply_kernel(const Rec* __restrict__ rec,
                                                                    const uint32_t* __restrict__ order, uint32_t n,
                                                                    uint32_t* order_next) {
    const size_t i = (size_t)blockIdx.x * ELEM_THREADS + threadIdx.x;
    if (i < n) {
        const uint32_t p = rec[i].pos;  // (the padding sorts behind every member: p < n)
        order_next[i] = order[p < n ? p : 0u];
    }
}

// One workgroup per segment of at most BVH_T members: its whole subtree, level by level in LDS.
__global__ __launch_bounds__(SUB_THREADS) void gs_bvh_subtree_kernel(const double* __restrict__ boxes,
                                                                     const uint32_t* __restrict__ refs,
                                                                     const uint32_t* __restrict__ order,
                                                                     const Seg* __restrict__ segs, gs_node* nodes,
                                                                     uint32_t node_base, uint32_t* order_out,
                                                                     uint32_t* flag) {
    __shared__ Rec s_rec[BVH_T];
    __shared__ uint32_t s_ord[BVH_T];
    __shared__ unsigned long long s_ext[BVH_T / 2];  // per segment of 3 or more: the fold's extreme
    __shared__ uint32_t s_pos[BVH_T / 2];            // ... and the earliest position holding it
    __shared__ uint8_t s_axis[BVH_T / 2];
    const uint32_t tid = threadIdx.x;
    const Seg sg = segs[blockIdx.x];
    const uint32_t m = sg.size;
    if (m == 0 || m > BVH_T) return;
    uint32_t pm = 2;  // the sort's padded length
    while (pm < m) pm <<= 1;
    {
        bool nan = false;
        for (uint32_t j = tid; j < m; j += SUB_THREADS) {
            const uint32_t mem = order[(size_t)sg.start + j];
            s_ord[j] = mem;
            const double* b = boxes + (size_t)mem * 6;
#pragma unroll
            for (int c = 0; c < 6; c++) nan |= b[c] != b[c];
        }
        if (nan) atomicOr(flag, 1u);
    }
    __syncthreads();
    for (uint32_t l = 0;; l++) {
        const uint32_t ne = 1u << l;                    // segments of this level (some inactive)
        const uint32_t hi = (m + ne - 1) >> l;          // the largest of them
        // -- this thread's members: segment, and whether it is one of 3 or more
        uint32_t ee[SUB_PER];
        bool big[SUB_PER];
#pragma unroll
        for (int q = 0; q < SUB_PER; q++) {
            const uint32_t j = tid + q * SUB_THREADS;
            uint32_t st = 0, sz = m, e = 0;
            bool fin = false;
            for (uint32_t t = 0; t < l; t++) {
                if (sz <= 2) {  // finished at level t: keep the walk's order
                    e <<= (l - t);
                    fin = true;
                    break;
                }
                const uint32_t h = sz / 2;
                if (j < st + h) {
                    sz = h;
                    e = 2 * e;
                } else {
                    st += h;
                    sz -= h;
                    e = 2 * e + 1;
                }
            }
            ee[q] = e;
            big[q] = j < m && !fin && sz >= 3;
        }
        // -- this thread's segments (two at most while any has 3 or more; leaves: up to SUB_PER)
        uint32_t g_sz[SUB_PER], g_nd[SUB_PER];
#pragma unroll
        for (int q = 0; q < SUB_PER; q++) {
            const uint32_t e = tid + q * SUB_THREADS;
            uint32_t st = 0, sz = m, nd = sg.node;
            bool act = e < ne;
            if (act)
                for (int t = (int)l - 1; t >= 0; t--) {
                    if (sz <= 2) {
                        act = false;
                        break;
                    }
                    const uint32_t h = sz / 2;
                    if ((e >> t) & 1u) {
                        nd += 1 + (uint32_t)gs_shape_nodes(h);
                        st += h;
                        sz -= h;
                    } else {
                        nd += 1;
                        sz = h;
                    }
                }
            g_sz[q] = act ? sz : 0;
            g_nd[q] = nd;
            if (act && sz <= 2) {  // BVH.rs:20-42: one member, or two in list order
                const uint32_t m0 = s_ord[st];
                const double* a = boxes + (size_t)m0 * 6;
                gs_node out;
                if (sz == 1) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        out.min[c] = a[c];
                        out.max[c] = a[3 + c];
                    }
                    out.left = leaf_ref(refs, m0);
                    out.right = GS_MAKE_REF(GS_REF_NONE, 0);
                } else {
                    const uint32_t m1 = s_ord[st + 1];
                    const double* b = boxes + (size_t)m1 * 6;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        out.min[c] = a[c] <= b[c] ? a[c] : b[c];
                        out.max[c] = a[3 + c] >= b[3 + c] ? a[3 + c] : b[3 + c];
                    }
                    out.left = leaf_ref(refs, m0);
                    out.right = leaf_ref(refs, m1);
                }
                out.pad[0] = out.pad[1] = 0;
                nodes[nd] = out;
            }
        }
        if (hi <= 2) break;
        // -- the boxes of the segments of 3 or more, one bound at a time: min x, max x, min y, ...
        double size3[2][3];
        double cur_min[2];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const bool is_min = (c & 1) == 0;
            const int comp = (c >> 1) + (is_min ? 0 : 3);
            for (uint32_t e = tid; e < ne; e += SUB_THREADS) {
                s_ext[e] = ord_key(is_min ? DBL_MAX : -DBL_MAX);  // AABB::EMPTY, before position 0
                s_pos[e] = NOPOS;
            }
            __syncthreads();
            double x[SUB_PER];
            unsigned long long k[SUB_PER];
#pragma unroll
            for (int q = 0; q < SUB_PER; q++)
                if (big[q]) {
                    x[q] = boxes[(size_t)s_ord[tid + q * SUB_THREADS] * 6 + comp];
                    k[q] = ord_key(x[q]);
                    if (x[q] == x[q]) {
                        if (is_min) atomicMin(&s_ext[ee[q]], k[q]);
                        else atomicMax(&s_ext[ee[q]], k[q]);
                    }
                }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < SUB_PER; q++)
                if (big[q] && x[q] == x[q] && k[q] == s_ext[ee[q]]) atomicMin(&s_pos[ee[q]], tid + q * SUB_THREADS);
            __syncthreads();
            bool win[SUB_PER];
#pragma unroll
            for (int q = 0; q < SUB_PER; q++)
                win[q] = big[q] && x[q] == x[q] && k[q] == s_ext[ee[q]] && s_pos[ee[q]] == tid + q * SUB_THREADS;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < SUB_PER; q++)
                if (win[q]) s_ext[ee[q]] = (unsigned long long)__double_as_longlong(x[q]);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; q++)
                if (g_sz[q] >= 3) {
                    const uint32_t e = tid + q * SUB_THREADS;
                    const double val = s_pos[e] == NOPOS ? (is_min ? DBL_MAX : -DBL_MAX)
                                                         : __longlong_as_double((long long)s_ext[e]);
                    if (is_min) {
                        nodes[g_nd[q]].min[c >> 1] = val;
                        cur_min[q] = val;
                    } else {
                        nodes[g_nd[q]].max[c >> 1] = val;
                        size3[q][c >> 1] = val - cur_min[q];
                    }
                }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < 2; q++)
            if (g_sz[q] >= 3) {
                const uint32_t e = tid + q * SUB_THREADS;
                const uint32_t h = g_sz[q] / 2;
                gs_node* nd = nodes + g_nd[q];
                nd->left = GS_MAKE_REF(GS_REF_NODE, node_base + g_nd[q] + 1);
                nd->right = GS_MAKE_REF(GS_REF_NODE, node_base + g_nd[q] + 1 + (uint32_t)gs_shape_nodes(h));
                nd->pad[0] = nd->pad[1] = 0;
                s_axis[e] = (uint8_t)longest_axis(size3[q][0], size3[q][1], size3[q][2]);
            }
        __syncthreads();
        // -- records, sort, new order
#pragma unroll
        for (int q = 0; q < SUB_PER; q++) {
            const uint32_t j = tid + q * SUB_THREADS;
            if (j < pm) {
                Rec r{0ull, PAD_SEG, j};
                if (j < m) {
                    r.seg = ee[q];
                    if (big[q]) r.key = ord_key(boxes[(size_t)s_ord[j] * 6 + s_axis[ee[q]]]);
                }
                s_rec[j] = r;
            }
        }
        __syncthreads();
        for (uint32_t k = 2; k <= pm; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) bitonic_step(s_rec, pm / 2, 0u, k, j, tid, SUB_THREADS);
        uint32_t moved[SUB_PER];
#pragma unroll
        for (int q = 0; q < SUB_PER; q++) {
            const uint32_t j = tid + q * SUB_THREADS;
            const uint32_t p = j < m ? s_rec[j].pos : 0u;  // (the padding sorts behind every member: p < m)
            moved[q] = s_ord[p < m ? p : 0u];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SUB_PER; q++) {
            const uint32_t j = tid + q * SUB_THREADS;
            if (j < m) s_ord[j] = moved[q];
        }
        __syncthreads();
    }
    __syncthreads();
    for (uint32_t j = tid; j < m; j += SUB_THREADS) order_out[(size_t)sg.start + j] = s_ord[j];
}

struct WorkLayout {
    size_t rec, order[2], segs[2], bytes;
    uint32_t padded, max_segs;
};

uint32_t level_max(uint32_t n, int level) { return (uint32_t)(((uint64_t)n + (1ull << level) - 1) >> level); }
uint32_t level_min(uint32_t n, int level) { return n >> level; }

WorkLayout work_layout(uint32_t n) {
    WorkLayout w{};
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    w.padded = 0;
    if (n > BVH_T) {
        w.padded = 1;
        while (w.padded < n) w.padded <<= 1;
    }
    int last = 0;  // the last level any segment is worked on
    while (level_max(n, last) > BVH_T) last++;
    w.max_segs = 1u << last;
    size_t off = HEADER_BYTES;
    w.rec = off;
    off = up(off + (size_t)w.padded * sizeof(Rec));
    for (int k = 0; k < 2; k++) {
        w.order[k] = off;
        off = up(off + (size_t)n * 4);
    }
    for (int k = 0; k < 2; k++) {
        w.segs[k] = off;
        off = up(off + (size_t)w.max_segs * sizeof(Seg));
    }
    w.bytes = off;
    return w;
}

gs_status fail(gs_status code, const std::string& msg) {
    gs_set_last_error(msg.c_str());
    return code;
}
gs_status hip_fail(const char* what, hipError_t e) {
    return fail(GS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define BVH_LAUNCHED(what)                         \
    do {                                           \
        const hipError_t e_ = hipGetLastError();   \
        if (e_ != hipSuccess) return hip_fail(what, e_); \
    } while (0)

inline uint32_t blocks_for(size_t items, int threads) { return (uint32_t)((items + threads - 1) / threads); }

}  // namespace

extern "C" {

int64_t gs_bvh_node_count(uint32_t n) { return n == 0 ? -1 : (int64_t)gs_shape_nodes(n); }
int32_t gs_bvh_depth(uint32_t n) { return gs_shape_depth(n); }
uint32_t gs_bvh_build_lds_members(void) { return BVH_T; }
int64_t gs_bvh_build_work_bytes(uint32_t n) { return n == 0 ? -1 : (int64_t)work_layout(n).bytes; }

gs_status gs_bvh_build_async(const double* d_boxes, const uint32_t* d_refs, uint32_t n, uint32_t node_base,
                             gs_node* d_nodes, uint32_t* d_order, void* d_work, int64_t work_bytes, void* stream) {
    if (!d_boxes || !d_nodes || !d_order || !d_work) return fail(GS_ERR_ARG, "gs_bvh_build_async: null pointer");
    if (n == 0) return fail(GS_ERR_ARG, "gs_bvh_build_async: BVHNode::from_list of an empty list");
    if (n >= GS_REF_MASK) return fail(GS_ERR_ARG, "gs_bvh_build_async: too many members for a 28-bit reference");
    if ((uint64_t)node_base + gs_shape_nodes(n) > (uint64_t)GS_REF_MASK)
        return fail(GS_ERR_ARG, "gs_bvh_build_async: node_base + nodes(n) exceeds a 28-bit reference");
    const WorkLayout w = work_layout(n);
    if (work_bytes < (int64_t)w.bytes)
        return fail(GS_ERR_ARG, "gs_bvh_build_async: work buffer of " + std::to_string(work_bytes) + " B, " +
                                    std::to_string(w.bytes) + " needed (gs_bvh_build_work_bytes)");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)d_work;
    uint32_t* flag = (uint32_t*)base;
    Rec* rec = (Rec*)(base + w.rec);
    uint32_t* order[2] = {(uint32_t*)(base + w.order[0]), (uint32_t*)(base + w.order[1])};
    Seg* segs[2] = {(Seg*)(base + w.segs[0]), (Seg*)(base + w.segs[1])};

    hipLaunchKernelGGL(gs_bvh_init_kernel, dim3(blocks_for(n, ELEM_THREADS)), dim3(ELEM_THREADS), 0, st, n, order[0],
                       segs[0], flag);
    BVH_LAUNCHED("gs_bvh_init_kernel");
    int cur = 0;
    for (int level = 0;; level++) {
        const uint32_t nseg = 1u << level;
        const bool any_big = level_max(n, level) > BVH_T;      // segments the global passes split
        const bool any_small = level_min(n, level) <= BVH_T;   // segments a workgroup finishes
        if (any_small) {
            hipLaunchKernelGGL(gs_bvh_subtree_kernel, dim3(nseg), dim3(SUB_THREADS), 0, st, d_boxes, d_refs,
                               (const uint32_t*)order[cur], (const Seg*)segs[level & 1], d_nodes, node_base, d_order, flag);
            BVH_LAUNCHED("gs_bvh_subtree_kernel");
        }
        if (!any_big) break;
        hipLaunchKernelGGL(gs_bvh_fold_kernel, dim3(nseg), dim3(FOLD_THREADS), 0, st, d_boxes,
                           (const uint32_t*)order[cur], segs[level & 1], segs[(level + 1) & 1], d_nodes, node_base, flag);
        BVH_LAUNCHED("gs_bvh_fold_kernel");
        hipLaunchKernelGGL(gs_bvh_keys_kernel, dim3(blocks_for(w.padded, ELEM_THREADS)), dim3(ELEM_THREADS), 0, st,
                           d_boxes, (const uint32_t*)order[cur], (const Seg*)segs[level & 1], n, w.padded, level, rec);
        BVH_LAUNCHED("gs_bvh_keys_kernel");
        const uint32_t chunks = w.padded / SORT_CHUNK;
        hipLaunchKernelGGL(gs_bvh_sort_local_kernel, dim3(chunks), dim3(SORT_THREADS), 0, st, rec, 0u);
        for (uint32_t k = SORT_CHUNK * 2; k <= w.padded && k != 0; k <<= 1) {
            for (uint32_t j = k >> 1; j >= SORT_CHUNK; j >>= 1)
                hipLaunchKernelGGL(gs_bvh_sort_global_kernel, dim3(blocks_for(w.padded / 2, ELEM_THREADS)),
                                   dim3(ELEM_THREADS), 0, st, rec, w.padded, k, j);
            hipLaunchKernelGGL(gs_bvh_sort_local_kernel, dim3(chunks), dim3(SORT_THREADS), 0, st, rec, k);
        }
        BVH_LAUNCHED("gs_bvh_sort kernels");
        hipLaunchKernelGGL(gs_bvh_apply_kernel, dim3(blocks_for(n, ELEM_THREADS)), dim3(ELEM_THREADS), 0, st,
                           (const Rec*)rec, (const uint32_t*)order[cur], n, order[cur ^ 1]);
        BVH_LAUNCHED("gs_bvh_apply_kernel");
        cur ^= 1;
    }
    return GS_OK;
}

gs_status gs_bvh_build_status(void* d_work, void* stream) {
    if (!d_work) return fail(GS_ERR_ARG, "gs_bvh_build_status: null pointer");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("gs_bvh_build_status: hipStreamSynchronize", e);
    uint32_t flag = 0;
    e = hipMemcpy(&flag, d_work, sizeof(flag), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("gs_bvh_build_status: hipMemcpy", e);
    if (flag) return fail(GS_ERR_ARG, "BVH sort: NaN bounding box");
    return GS_OK;
}

}  // extern "C"
