// bvh_shape.hpp — the shape of BVHNode::from_list's tree, which is a function of the member
// count alone (BVH.rs:18-65: one node for n <= 2, else a split at n / 2), shared by the host
// (world.cpp, from_order) and the device builder (bvh_build.hip).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GS_SHAPE_FN __host__ __device__ inline
#else
#define GS_SHAPE_FN inline
#endif

// nodes(n) = 1 if n <= 2 else 1 + nodes(n / 2) + nodes(n - n / 2), without recursion: at every
// depth the sizes are a = n >> d and a + 1, so the pair (nodes(a), nodes(a + 1)) is carried
// from the top bit of n down.  n == 0 gives 0.
GS_SHAPE_FN uint64_t gs_shape_nodes(uint32_t n) {
    if (n == 0) return 0;
    int top = 31;
    while (!((n >> top) & 1u)) top--;
    uint64_t f0 = 1, f1 = 1;  // a = 1: nodes(1), nodes(2)
    for (int d = top - 1; d >= 0; d--) {
        const uint32_t a = n >> d;  // = 2 a' + b
        uint64_t g0, g1;
        if (a & 1u) {
            g0 = 1 + f0 + f1;
            g1 = 1 + 2 * f1;
        } else {
            g0 = 1 + 2 * f0;
            g1 = 1 + f0 + f1;
        }
        f0 = a <= 2 ? 1 : g0;
        f1 = a <= 1 ? 1 : g1;
    }
    return f0;
}

// Levels of the tree: 1 for n <= 2, else 1 + depth(n - n / 2) (the larger half is the deeper).
GS_SHAPE_FN int32_t gs_shape_depth(uint32_t n) {
    if (n == 0) return 0;
    int32_t d = 1;
    while (n > 2) {
        n = n - n / 2;
        d++;
    }
    return d;
}
