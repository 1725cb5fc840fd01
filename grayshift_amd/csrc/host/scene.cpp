// scene.cpp — a flat scene (include/grayshift_scene.h) becomes a device scene: validation of
// everything the kernels index, the threaded tree and its static visit estimate, the placement
// of its records for the LDS mirror, the device materials, the choice of kernel instantiation
// (GS_FEAT_*) and the upload.  Plain C++ over the HIP runtime API: no kernels here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <unordered_map>

#include "render_host.hpp"

using namespace gsd;

namespace {

// Bytes of threaded records mirrored in LDS per block (the most-tested ones): what is
// left of the block's share of the CU's 160 KiB (4 waves/SIMD = 1024 lanes per CU) after
// the lane state of the scene's fixed-spp kernel (none when that kernel keeps it in registers,
// lane_state_in_regs).  -1 = that budget; >= 0 explicit (A/B).
#ifndef GS_LDS_MIRROR
#define GS_LDS_MIRROR -1
#endif
const int64_t g_lds_mirror = GS_LDS_MIRROR;  // (compile-time A/B only)
int64_t lds_mirror_budget(bool lane_regs) {
    const int64_t share = (int64_t)160 * 1024 * GS_BLOCK / (GS_MIN_WAVES * 4 * 64);  // the block's share of the CU
    // (sized for fixed-spp launches; an adaptive launch's larger lane state shrinks the
    // mirror's prefixes to fit at launch)
    const int64_t lane = lane_regs ? 0 : (int64_t)GS_BLOCK * (L_ND_CHUNKED * 8 + L_NI * 4);
    const int64_t left = share - lane - 1024;  // 1 KiB: the block's counters + slack
    return left > 0 ? left : 0;
}
#ifndef GS_KIND_SHADE_BATCH
#define GS_KIND_SHADE_BATCH 44
#endif
#ifndef GS_KIND_LEAF_BATCH
#define GS_KIND_LEAF_BATCH 24
#endif
#ifndef GS_KIND_NODE_STEPS
#define GS_KIND_NODE_STEPS 8
#endif

struct Layout {
    std::vector<uint8_t> blob;
    size_t add(const void* p, size_t n) {
        size_t off = (blob.size() + 255) & ~(size_t)255;
        blob.resize(off + n + 1, 0);  // +1 keeps empty arrays at distinct, valid addresses
        if (n && p) std::memcpy(blob.data() + off, p, n);
        return off;
    }
};

// The aligned form of a quad (cube_record) when its normal is
// exactly +-e_a, w is zero off axis a, and u, v are each non-zero on one other axis.
static bool aligned_tquad(const gs_quad& q, TQuad& out) {
    int ax = -1;
    for (int k = 0; k < 3; k++) {
        if (q.normal[k] == 0.0) continue;
        if (std::fabs(q.normal[k]) != 1.0 || ax >= 0) return false;
        ax = k;
    }
    if (ax < 0) return false;
    auto one_axis = [&](const double* v) {
        int at = -1;
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(v[k])) return -2;
            if (v[k] != 0.0) {
                if (at >= 0) return -2;
                at = k;
            }
        }
        return at;
    };
    const int iu = one_axis(q.u), iv = one_axis(q.v);
    if (iu < 0 || iv < 0 || iu == ax || iv == ax || iu == iv) return false;
    for (int k = 0; k < 3; k++)
        if (k != ax && q.w[k] != 0.0) return false;
    if (!std::isfinite(q.w[ax]) || !std::isfinite(q.d) || !std::isfinite(q.q[iu]) || !std::isfinite(q.q[iv])) return false;
    const int o = iu == (ax + 1) % 3 ? 0 : 1;  // (then iv == (ax + 2) % 3 for o == 0)
    const double sgn = o == 0 ? 1.0 : -1.0;
    TQuad r{};
    const uint64_t tag = ((uint64_t)(GS_AQ_TAG | (uint32_t)(2 * ax + o))) << 32;
    std::memcpy(&r.nx, &tag, 8);
    r.ny = q.normal[ax] * q.d;  // D' (exact: a sign)
    r.nz = q.q[iu];
    r.d = q.q[iv];
    r.qx = q.u[iu];
    r.qy = q.v[iv];
    r.qz = sgn * q.w[ax];  // W'
    out = r;
    return true;
}

#ifndef GS_PLAIN_KERNELS
#define GS_PLAIN_KERNELS 1  // (A/B: 0 keeps C4 on the generic staged shading)
#endif
static const bool g_plain_kernels = GS_PLAIN_KERNELS;
// A Quad::cube list's device record (cube_test): six consecutive quads whose aligned forms
// carry cube_code(k) in order and equal, field by field, what cube_src derives from the 12
// numbers taken from them.  Returns false (the list keeps the loop) otherwise.
static bool cube_record(const gs_flat_scene& s, const gs_list& l, uint32_t& q0, double* out) {
    if (l.count != 6 || (uint64_t)l.first + 6 > s.n_list_refs) return false;
    q0 = s.list_refs[l.first] & GS_REF_MASK;
    if (q0 >= GS_CUBE_FLAG) return false;
    double f[6][6];  // face k: D', Q_iu, Q_iv, U_iu, V_iv, W'
    for (uint32_t k = 0; k < 6; k++) {
        const uint32_t ref = s.list_refs[l.first + k];
        if ((ref >> GS_REF_SHIFT) != GS_REF_QUAD || (ref & GS_REF_MASK) != q0 + k || q0 + k >= s.n_quads) return false;
        TQuad a;
        if (!aligned_tquad(s.quads[q0 + k], a)) return false;
        uint64_t tag;
        std::memcpy(&tag, &a.nx, 8);
        if ((uint32_t)(tag >> 32) != (GS_AQ_TAG | (uint32_t)cube_code((int)k))) return false;
        const double v[6] = {a.ny, a.nz, a.d, a.qx, a.qy, a.qz};
        for (int j = 0; j < 6; j++) f[k][j] = v[j];
    }
    // x0 y0 z0 x1 y1 z1 dx dy dz w_xy w_zy w_xz, read off faces 3, 5, 2, 1, 4, 0 (cube_src)
    const double c[GS_CUBE_DOUBLES] = {f[3][0], f[5][0], f[2][0], f[1][0], f[4][0], f[0][0],
                                       f[0][3], f[0][4], f[3][3], f[0][5], f[3][5], f[5][5]};
    for (int k = 0; k < 6; k++)
        for (int j = 0; j < 6; j++) {
            const int v = cube_src(k, j);
            if (!(f[k][j] == (v < 0 ? -c[-v] : c[v]))) return false;
        }
    for (int j = 0; j < GS_CUBE_DOUBLES; j++) out[j] = c[j];
    return true;
}

// Raw links of ThreadedTree records: a record index, or the end of the top-level walk, or
// the end of a nested tree's walk (THR_END / THR_RET once placed).
#define RAW_END 0xFFFFFFFFu
#define RAW_RET 0xFFFFFFFEu

}  // namespace

// Order the records by how likely a ray tests them and fill the block's LDS byte budget in
// that order (32-B node records, 48-B leaf records; quads take the rest).  `visits` (one
// count per record, nullable): measured by a pilot launch (GS_FEAT_VISITS), ranked by
// visits per byte, which maximises the visits the mirror serves; the static estimate
// orders the unvisited and serves when there is no pilot.  Records outside the mirror
// stay in pre-order.
Placed place_records(const gs_device_scene* ds, const std::vector<uint64_t>* visits) {
    const ThreadedTree& t = ds->tree;
    const int64_t budget = ds->mirror_budget;
    const uint32_t n = (uint32_t)t.rec.size();
    Placed out;
    std::vector<uint32_t> order(n), pos(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    auto rec_bytes = [&](uint32_t i) { return t.leaf[i] ? (int64_t)sizeof(TLeaf) : (int64_t)sizeof(TNode); };
    auto static_first = [&](uint32_t a, uint32_t b) {
        return t.score[a] > t.score[b] || (t.score[a] == t.score[b] && t.depth[a] < t.depth[b]);
    };
    if (visits) {
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            // compare visits_a / bytes_a with visits_b / bytes_b exactly (integers)
            const unsigned __int128 va = (unsigned __int128)(*visits)[a] * (uint64_t)rec_bytes(b);
            const unsigned __int128 vb = (unsigned __int128)(*visits)[b] * (uint64_t)rec_bytes(a);
            if (va != vb) return va > vb;
            return static_first(a, b);
        });
    } else {
        std::stable_sort(order.begin(), order.end(), static_first);
    }
    std::vector<uint8_t> top(n, 0);
    int64_t used = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t r = order[i];
        const int64_t sz = rec_bytes(r);
        if (used + sz > budget) {
            if (used + (int64_t)sizeof(TNode) > budget) break;
            continue;
        }
        used += sz;
        top[r] = 1;
        (t.leaf[r] ? out.mirror.leaves : out.mirror.nodes)++;
    }
    // (the nested trees' records are ranked with the top level's: one node / leaf array)
    // a prefix of the quads up to the last quad tested by the quad test that fits (cube-list
    // quads are read from the cube records)
    const int64_t fit = std::max<int64_t>(0, budget - used) / (int64_t)sizeof(TQuad);
    out.mirror.quads = 0;
    for (uint32_t q : ds->single_quads)
        if ((int64_t)q < fit) out.mirror.quads = q + 1;
    used += (int64_t)out.mirror.quads * (int64_t)sizeof(TQuad);
    // then the Quad::cube records (cube order)
    out.mirror.cubes = (uint32_t)std::min<int64_t>(ds->n_cubes, std::max<int64_t>(0, budget - used) / (GS_CUBE_DOUBLES * 8));
    // The mirrored records take their positions in rank order, so a launch that must
    // shrink the prefixes (a larger lane state, gs_render_tiles_timed_async) drops the
    // least-tested ones; the rest keep pre-order.
    uint32_t nt = 0, nl = 0, nt_rest = out.mirror.nodes, nl_rest = out.mirror.leaves;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = order[k];
        if (top[i]) pos[i] = t.leaf[i] ? nl++ : nt++;
    }
    for (uint32_t i = 0; i < n; i++)
        if (!top[i]) pos[i] = t.leaf[i] ? nl_rest++ : nt_rest++;
    out.tnodes.resize(nt_rest);
    out.tboxes.resize(nt_rest);
    out.tleaves.resize(nl_rest);
    auto tag = [&](uint32_t l) {
        if (l == RAW_RET) return THR_RET;
        return l >= n ? THR_END : (t.leaf[l] ? (THR_LEAF | pos[l]) : node_link(pos[l]));
    };
    for (uint32_t i = 0; i < n; i++) {
        const DNode& r = t.rec[i];
        if (t.leaf[i]) {
            out.tleaves[pos[i]] = TLeaf{r.mnx, r.mny, r.mnz, r.mxx * r.mxx, tag(r.left), r.right, 0u, 0u};
        } else {
            // f32 box coordinates rounded to nearest (the certified test's error model)
            out.tnodes[pos[i]] = TNode{(float)r.mnx, (float)r.mny, (float)r.mxx, (float)r.mxy, (float)r.mnz,
                                       (float)r.mxz, tag(r.left), tag(r.right)};
            out.tboxes[pos[i]] = TBox{r.mnx, r.mny, r.mnz, r.mxx, r.mxy, r.mxz};
        }
    }
    out.root = n == 0 ? THR_END : tag(0);
    for (uint32_t r : ds->nroot_rec) out.nroots.push_back(tag(r));
    out.pos = std::move(pos);
    return out;
}

void adopt_placement(gs_device_scene* ds, Placed& pl) {
    ds->thr_root = pl.root;
    ds->mirror = pl.mirror;
    ds->pos = std::move(pl.pos);
    ds->lcfg.clear();  // mirror prefixes changed
}

namespace {

// Host-side validation of everything the kernel indexes, so a malformed scene is an
// error code, never a GPU fault.
// inst_reached (out): per instance, whether a leaf reachable from the root walks it (the scene
// upload threads the BVHs under reached instances only).
gs_status validate(const gs_flat_scene& s, uint32_t* depth_out, bool* nested_out, std::vector<uint8_t>* inst_reached,
                   bool* general_out, std::vector<uint8_t>* media_reached) {
    media_reached->assign(s.n_media, 0);
    bool general = false;  // a composition only GS_FEAT_GENERAL kernels walk (round 6)
    auto bad = [](const std::string& m) { return fail(GS_ERR_ARG, "invalid flat scene: " + m); };
    auto unsup = [](const std::string& m) { return fail(GS_ERR_UNSUPPORTED, m); };
    if (!s.nodes && s.n_nodes) return bad("nodes");
    if (!s.media && s.n_media) return bad("media");
    // the kernel forms node / sphere byte offsets as u32 (ref << 6, ref << 5)
    if (s.n_nodes >= (1u << 26) || s.n_spheres >= (1u << 27)) return unsup("more than 2^26 BVH nodes or 2^27 spheres");
    if (s.n_materials == 0 || !s.materials) return bad("no materials");
    if (!s.instances && s.n_instances) return bad("instances");
    inst_reached->assign(s.n_instances, 0);
    auto prim_ok = [&](uint32_t r) {
        uint32_t k = r >> GS_REF_SHIFT, i = r & GS_REF_MASK;
        switch (k) {
            case GS_REF_SPHERE: return i < s.n_spheres;
            case GS_REF_MSPHERE: return i < s.n_mspheres;
            case GS_REF_QUAD: return i < s.n_quads;
            case GS_REF_TRIANGLE: return i < s.n_triangles;
            default: return false;
        }
    };
    // Walks a Translate/RotateY chain: 0 ok, 1 bad, 2 unsupported (deeper than GS_MAX_CHAIN).
    // mark: 1 a leaf's chain, 2 a medium boundary's (kept: a chain reached both ways is 2)
    auto chain_ok = [&](uint32_t& cur, uint8_t mark = 1) -> int {
        int chain = 0;
        while ((cur >> GS_REF_SHIFT) == GS_REF_INSTANCE) {
            uint32_t i = cur & GS_REF_MASK;
            if (i >= s.n_instances) return 1;
            if (++chain > GS_MAX_CHAIN) return 2;
            if (chain > 4) general = true;  // (the other kernels' hit record keeps 4)
            (*inst_reached)[i] = std::max((*inst_reached)[i], mark);
            const gs_instance& in = s.instances[i];
            if (in.kind != GS_INST_TRANSLATE && in.kind != GS_INST_ROTATE_Y) return 1;
            cur = in.child;
        }
        return 0;
    };
    // A list of primitives or one primitive (what walk_chain may end in).
    auto shape_ok = [&](uint32_t cur) -> int {
        const uint32_t k = cur >> GS_REF_SHIFT;
        if (k == GS_REF_LIST) {
            uint32_t i = cur & GS_REF_MASK;
            if (i >= s.n_lists) return 1;
            const gs_list& l = s.lists[i];
            if ((uint64_t)l.first + l.count > s.n_list_refs) return 1;
            for (uint32_t q = 0; q < l.count; q++)
                if (!prim_ok(s.list_refs[l.first + q])) return 2;
            return 0;
        }
        if (k == GS_REF_NODE || k == GS_REF_MEDIUM || k == GS_REF_INSTANCE) return 2;
        return prim_ok(cur) ? 0 : 1;
    };
    // A BVH under an instance chain: nodes in range, leaves lists or primitives, depth at
    // most GS_NESTED_STACK (the device walk is threaded and needs no stack; the bound keeps
    // the host's threading finite).  Subtrees may be shared between chains (instancing);
    // the depth bound ends cycles and a visit budget ends blow-ups.
    // A BVH as a medium boundary (GS_FEAT_GENERAL, tree_test): nodes in range, leaves lists or
    // primitives, depth bounded (threaded with the BVHs under instances).
    uint64_t boundary_budget = 64ull << 20;
    auto boundary_tree_ok = [&](uint32_t root) -> int {
        std::vector<std::pair<uint32_t, uint32_t>> st{{root, 1u}};
        while (!st.empty()) {
            auto [r, d] = st.back();
            st.pop_back();
            if (boundary_budget-- == 0) return 1;
            if ((r >> GS_REF_SHIFT) == GS_REF_NODE) {
                const uint32_t i = r & GS_REF_MASK;
                if (i >= s.n_nodes) return 1;
                if (d > GS_NESTED_STACK) return 2;
                if (s.nodes[i].left == GS_REF_NONE) return 1;
                st.push_back({s.nodes[i].left, d + 1});
                if (s.nodes[i].right != GS_REF_NONE) st.push_back({s.nodes[i].right, d + 1});
            } else {
                const int e = shape_ok(r);
                if (e) return e;
            }
        }
        return 0;
    };
    // A ConstantMedium: its boundary a primitive or list behind an optional chain; round 6
    // (GS_FEAT_GENERAL): also a BVH, or one level of another medium.
    std::function<int(uint32_t, int)> medium_ok_l = [&](uint32_t cur, int level) -> int {
        uint32_t i = cur & GS_REF_MASK;
        if (i >= s.n_media || !s.media) return 1;
        if (s.media[i].material >= s.n_materials) return 1;
        uint32_t b = s.media[i].boundary;
        const int e = chain_ok(b, 2);
        (*media_reached)[i] = 1;
        if (e) return e;
        if ((b >> GS_REF_SHIFT) == GS_REF_NODE) {
            general = true;
            return boundary_tree_ok(b);
        }
        if ((b >> GS_REF_SHIFT) == GS_REF_MEDIUM) {
            if (level > 0) return 2;  // media two deep inside media
            general = true;
            return medium_ok_l(b, level + 1);
        }
        return shape_ok(b);
    };
    auto medium_ok = [&](uint32_t cur) -> int { return medium_ok_l(cur, 0); };
    bool nested = false;
    uint64_t nested_budget = 64ull << 20;
    auto nested_ok = [&](uint32_t root) -> int {
        std::vector<std::pair<uint32_t, uint32_t>> st{{root, 1u}};
        while (!st.empty()) {
            auto [r, d] = st.back();
            st.pop_back();
            if (nested_budget-- == 0) return 1;
            if ((r >> GS_REF_SHIFT) == GS_REF_NODE) {
                const uint32_t i = r & GS_REF_MASK;
                if (i >= s.n_nodes) return 1;
                if (d > GS_NESTED_STACK) return 2;
                if (s.nodes[i].left == GS_REF_NONE) return 1;
                st.push_back({s.nodes[i].left, d + 1});
                if (s.nodes[i].right != GS_REF_NONE) st.push_back({s.nodes[i].right, d + 1});
            } else {
                // (since round 5 the tree is walked by the main passes, whose leaf test takes
                // media like the top level's: the hit's instance is the tree's chain; round 6: a
                // chain inside the tree, ending in a primitive, list or medium -- not another BVH)
                uint32_t c = r;
                int e = chain_ok(c);
                if (!e) {
                    if (c != r) general = true;  // a chain inside the tree: two-chain hit records
                    if ((c >> GS_REF_SHIFT) == GS_REF_NODE) e = 2;
                    else e = (c >> GS_REF_SHIFT) == GS_REF_MEDIUM ? medium_ok(c) : shape_ok(c);
                }
                if (e) return e;
            }
        }
        nested = true;
        return 0;
    };
    auto leaf_ok = [&](uint32_t r) -> int {  // 0 ok, 1 bad, 2 unsupported
        uint32_t cur = r;
        int e = chain_ok(cur);
        if (e) return e;
        if ((cur >> GS_REF_SHIFT) == GS_REF_NODE && cur != r) return nested_ok(cur);
        if ((cur >> GS_REF_SHIFT) == GS_REF_MEDIUM) return medium_ok(cur);
        if ((cur >> GS_REF_SHIFT) == GS_REF_NODE) return cur != r ? 2 : 1;
        return shape_ok(cur);
    };
    // Walk the tree from the root: indices in range, no node reached twice, depth bound.
    std::vector<uint8_t> seen(s.n_nodes, 0);
    std::vector<std::pair<uint32_t, uint32_t>> stk;
    stk.push_back({s.root, 0});
    uint32_t maxd = 0;
    while (!stk.empty()) {
        auto [r, d] = stk.back();
        stk.pop_back();
        if ((r >> GS_REF_SHIFT) == GS_REF_NODE) {
            uint32_t i = r & GS_REF_MASK;
            if (i >= s.n_nodes) return bad("node index");
            if (seen[i]) return bad("node reached twice (not a tree)");
            seen[i] = 1;
            if (d + 1 > maxd) maxd = d + 1;
            if (s.nodes[i].left == GS_REF_NONE) return bad("node without left child");
            stk.push_back({s.nodes[i].left, d + 1});
            if (s.nodes[i].right != GS_REF_NONE) stk.push_back({s.nodes[i].right, d + 1});
        } else {
            int e = leaf_ok(r);
            if (e == 1) return bad("leaf reference");
            if (e == 2) return unsup("instance chain deeper than " + std::to_string(GS_MAX_CHAIN) +
                                     ", a BVH under an instance deeper than " + std::to_string(GS_NESTED_STACK) +
                                     " or holding another BVH under an instance, a BVH inside a medium boundary, "
                                     "nested media, or a list member that is not a primitive");
        }
    }
    *depth_out = maxd;
    *nested_out = nested;
    *general_out = general;
    auto mat_ok = [&](uint32_t m) { return m < s.n_materials; };
    for (uint32_t i = 0; i < s.n_spheres; i++) if (!mat_ok(s.spheres[i].material)) return bad("sphere material");
    for (uint32_t i = 0; i < s.n_mspheres; i++) if (!mat_ok(s.mspheres[i].material)) return bad("msphere material");
    for (uint32_t i = 0; i < s.n_quads; i++) if (!mat_ok(s.quads[i].material)) return bad("quad material");
    for (uint32_t i = 0; i < s.n_triangles; i++) if (!mat_ok(s.triangles[i].material)) return bad("triangle material");
    for (uint32_t i = 0; i < s.n_materials; i++) {
        const gs_material& m = s.materials[i];
        if (m.kind == GS_MAT_LAMBERTIAN || m.kind == GS_MAT_DIFFUSE_LIGHT || m.kind == GS_MAT_ISOTROPIC) {
            if (m.texture >= s.n_textures) return bad("material texture");
        } else if (m.kind != GS_MAT_METAL && m.kind != GS_MAT_DIELECTRIC) {
            return bad("material kind");
        }
    }
    for (uint32_t i = 0; i < s.n_textures; i++) {
        const gs_texture& t = s.textures[i];
        if (t.kind == GS_TEX_CHECKERED) {
            if (t.even >= s.n_textures || t.odd >= s.n_textures) return bad("checkered child");
        } else if (t.kind == GS_TEX_IMAGE) {
            if (t.image >= s.n_images) return bad("image index");
            const gs_image& im = s.images[t.image];
            if (!im.width || !im.height) return bad("empty image");
            if (im.offset + (uint64_t)im.width * im.height * 3 > s.n_texels8) return bad("image texels out of range");
        } else if (t.kind == GS_TEX_NOISE) {
            if (s.n_noise_perm != 256 || !s.noise_perm) return bad("noise texture without its 256-byte permutation");
        } else if (t.kind != GS_TEX_SOLID) {
            return bad("texture kind");
        }
    }
    if (s.background.kind == GS_BG_HDRI) {
        if (!s.background.width || !s.background.height) return bad("empty HDRI");
        if ((uint64_t)s.background.width * s.background.height * 3 > s.n_hdri_floats || !s.hdri_rgb)
            return bad("HDRI texels");
    } else if (s.background.kind != GS_BG_SOLID) {
        return bad("background kind");
    }
    return GS_OK;
}

// f32 RGB -> RGBE8 (shared exponent), accepted only if m * 2^(e-136) reproduces all
// three floats exactly (true for texels that came from an RGBE file, as airport.hdr's).
bool encode_rgbe(const float* c, uint32_t* out) {
    const float r = c[0], g = c[1], b = c[2];
    if (!(r >= 0.0f && g >= 0.0f && b >= 0.0f)) return false;
    if (std::signbit(r) || std::signbit(g) || std::signbit(b)) return false;
    const float mx = std::fmax(r, std::fmax(g, b));
    if (mx == 0.0f) {
        *out = 0;
        return true;
    }
    int ex = 0;
    std::frexp((double)mx, &ex);
    for (int e = ex + 128; e >= 1 && e >= ex + 120; e--) {  // try the canonical exponent first
        if (e > 255) continue;
        const double scale = std::ldexp(1.0, e - 136);
        uint32_t m[3];
        bool ok = true;
        for (int k = 0; k < 3 && ok; k++) {
            const double q = (double)c[k] / scale;
            ok = q >= 0.0 && q <= 255.0 && q == std::floor(q) && (float)(q * scale) == c[k];
            m[k] = ok ? (uint32_t)q : 0;
        }
        if (ok) {
            *out = m[0] | (m[1] << 8) | (m[2] << 16) | ((uint32_t)e << 24);
            return true;
        }
    }
    return false;
}

// Does the texture tree under `t` contain an image (=> sphere uv must be computed)?
bool tex_needs_uv(const gs_flat_scene& s, uint32_t t, int depth = 0) {
    if (t >= s.n_textures || depth > 16) return false;
    const gs_texture& x = s.textures[t];
    if (x.kind == GS_TEX_IMAGE) return true;
    if (x.kind == GS_TEX_CHECKERED) return tex_needs_uv(s, x.even, depth + 1) || tex_needs_uv(s, x.odd, depth + 1);
    return false;
}

// What the upload copies besides the flat scene's own arrays and the placed records.
struct DeviceArrays {
    std::vector<gs_list> lists;      // the scene's lists, a Quad::cube list as {cube index, GS_CUBE_FLAG | first quad}
    std::vector<double> cubes;       // GS_CUBE_DOUBLES per Quad::cube list
    std::vector<gs_instance> insts;  // a BVH child as GS_REF_NODE | tree index
    std::vector<gs_medium> media;    // (GS_FEAT_GENERAL) a BVH boundary likewise
    std::vector<DMaterial> mats;
    std::vector<TQuad> tquads;
    std::vector<DSphere> sph;
    std::vector<uint32_t> sph_mat;
    std::vector<uint32_t> rgbe;  // the HDRI as RGBE8 texels, or empty
};

// Quad::cube lists (cube_test): their device list records and cube records.  Their quads
// are never read through the quad mirror, so the mirror holds a prefix of the quads only
// as far as the last other quad in it (single_quads).
void find_cube_lists(const gs_flat_scene& s, bool on, DeviceArrays& a, std::vector<uint32_t>& single_quads) {
    a.lists.assign(s.lists, s.lists + s.n_lists);
    std::vector<uint8_t> in_cube(s.n_quads, 0);
    // (the LDS mirror holds a prefix of the cube records in list order: largest boxes
    // first measured neutral, profiles/r04/ab_cube_order.txt)
    for (uint32_t i = 0; on && i < s.n_lists; i++) {
        uint32_t q0;
        double rec[GS_CUBE_DOUBLES];
        if (!cube_record(s, s.lists[i], q0, rec)) continue;
        a.lists[i] = gs_list{(uint32_t)(a.cubes.size() / GS_CUBE_DOUBLES), GS_CUBE_FLAG | q0};
        a.cubes.insert(a.cubes.end(), rec, rec + GS_CUBE_DOUBLES);
        for (uint32_t k = 0; k < 6; k++) in_cube[q0 + k] = 1;
    }
    // (a quad may also be referenced directly elsewhere: any ref outside a cube list keeps
    // it a mirror candidate -- conservatively, every quad not in a cube list)
    for (uint32_t i = 0; i < s.n_quads; i++)
        if (!in_cube[i]) single_quads.push_back(i);
}

// Appends the subtree at `ref` to the threaded records (see THR_END) in pre-order: a node
// {box, hit = next record, miss = after its subtree}, a leaf occurrence {a stationary sphere
// inline, next, ABI ref}.  The links that leave the subtree become `end_link`: RAW_END for the
// top-level tree, RAW_RET for a tree under an instance chain or a medium.
void thread_subtree(const gs_flat_scene& s, uint32_t ref, uint32_t end_link, ThreadedTree& t) {
    const uint32_t first = (uint32_t)t.rec.size();
    // Iterative pre-order: a node pushes a "close" marker below its children, which
    // sets its miss link once its subtree is emitted.
    std::vector<std::pair<uint32_t, bool>> work{{ref, false}};
    while (!work.empty()) {
        auto [x, close] = work.back();
        work.pop_back();
        if (close) {  // x = record index of a node whose subtree is now complete
            t.rec[x].right = (uint32_t)t.rec.size();
            continue;
        }
        const uint32_t idx = (uint32_t)t.rec.size();
        DNode rec{};
        if ((x >> GS_REF_SHIFT) == GS_REF_NODE) {
            const gs_node& n = s.nodes[x & GS_REF_MASK];
            rec = DNode{n.min[0], n.min[1], n.min[2], n.max[0], n.max[1], n.max[2], idx + 1u, 0u, 0u, 0u};
            t.rec.push_back(rec);
            t.leaf.push_back(0);
            work.push_back({idx, true});
            if (n.right != GS_REF_NONE) work.push_back({n.right, false});
            work.push_back({n.left, false});
        } else {
            if ((x >> GS_REF_SHIFT) == GS_REF_SPHERE) {
                const gs_sphere& q = s.spheres[x & GS_REF_MASK];
                rec.mnx = q.center[0];
                rec.mny = q.center[1];
                rec.mnz = q.center[2];
                rec.mxx = q.radius;
            }
            rec.left = idx + 1u;  // next
            rec.right = x;        // the primitive's ref
            t.rec.push_back(rec);
            t.leaf.push_back(1);
        }
    }
    // (an explicit end link, so records appended later keep their indices)
    const uint32_t end = (uint32_t)t.rec.size();
    for (uint32_t k = first; k < end; k++) {
        if (t.rec[k].left == end) t.rec[k].left = end_link;
        if (!t.leaf[k] && t.rec[k].right == end) t.rec[k].right = end_link;
    }
}

double box_area(const DNode& b) {
    const double dx = b.mxx - b.mnx, dy = b.mxy - b.mny, dz = b.mxz - b.mnz;
    return dx * dy + dy * dz + dz * dx;
}
// f(c) for each child record c of node record i, within the records [.., end).
template <class F>
void for_children(const ThreadedTree& t, uint32_t i, uint32_t end, F f) {
    for (uint32_t c = t.rec[i].left; c < t.rec[i].right && c < end;) {
        f(c);
        c = t.leaf[c] ? c + 1 : t.rec[c].right;  // next child of node i
    }
}
bool sphere_leaf(const ThreadedTree& t, uint32_t i) {
    return t.leaf[i] && (t.rec[i].right >> GS_REF_SHIFT) == GS_REF_SPHERE;
}

// Placement: the records a ray is most likely to test first, so a block can mirror
// them in LDS; the rest in pre-order.  Static estimate (until a launch's pilot
// measures the real visits, place_records): the smallest surface area of a box on
// the record's path from the root (a ray tests a record only if it hit all of
// them), ties broken by depth.  Links are explicit, so placement does not change
// the walk.
// Scores the top-level tree (all of t so far) and derives the expected node tests per leaf
// test and the share of leaf tests that are not stationary spheres.
void score_top_level(ThreadedTree& t, double& nodes_per_leaf, double& other_leaf_frac) {
    const uint32_t n = (uint32_t)t.rec.size();
    t.depth.assign(n, 0);
    t.score.assign(n, 0.0);
    // records are pre-order: a node's descendants follow it, so depths and scores
    // propagate in one forward pass
    // score = surface area of the parent's box (the chance a ray tests the record)
    if (n) t.score[0] = 1e308;
    for (uint32_t i = 0; i < n; i++)
        if (!t.leaf[i]) {
            const double sa = box_area(t.rec[i]);
            for_children(t, i, n, [&](uint32_t c) {
                t.depth[c] = t.depth[i] + 1;
                t.score[c] = std::min(t.score[i], sa);
            });
        }
    // Expected node tests per leaf test (the score over the root box's area is the
    // chance a ray entering the root tests the record).
    nodes_per_leaf = other_leaf_frac = 0.0;
    if (n && !t.leaf[0]) {
        const double sa_root = box_area(t.rec[0]);
        double pn = 0.0, pl = 0.0, po = 0.0;
        for (uint32_t i = 0; i < n; i++) {
            const double p = i == 0 ? 1.0 : (sa_root > 0.0 ? std::min(1.0, t.score[i] / sa_root) : 1.0);
            (t.leaf[i] ? pl : pn) += p;
            if (t.leaf[i] && !sphere_leaf(t, i)) po += p;
        }
        nodes_per_leaf = pl > 0.0 ? pn / pl : 0.0;
        other_leaf_frac = pl > 0.0 ? po / pl : 0.0;
    } else if (n) {
        other_leaf_frac = !sphere_leaf(t, 0) ? 1.0 : 0.0;
    }
}

// BVHs under instance chains (GS_FEAT_NESTED: final_scene's box of balls, main.rs:
// 741-755): each distinct tree under a reached instance is threaded once, in pre-order,
// into the same records after the top-level tree -- node {box, hit = next record, miss
// = after its subtree}, leaf {a stationary sphere inline, next, ABI ref} -- its last
// links RAW_RET (THR_RET: back to the top-level ray); the instance's device child
// becomes GS_REF_NODE | tree index, and nroot_rec[tree] its root record.  The lane
// walks it in the main loop's node and leaf passes (render kernel, leaf pass), so its
// records are placed and mirrored with the top level's by measured visits.
gs_status thread_nested_trees(const gs_flat_scene& s, bool general, const std::vector<uint8_t>& inst_reached,
                              const std::vector<uint8_t>& media_reached, ThreadedTree& t, DeviceArrays& a,
                              std::vector<uint32_t>& nroot_rec) {
    std::unordered_map<uint32_t, uint32_t> tree_of;  // gs node index -> tree
    // thread the tree at BVH node ref `node_ref` once; returns its tree index
    auto tree_index = [&](uint32_t node_ref) -> uint32_t {
        const uint32_t root = node_ref & GS_REF_MASK;
        auto it = tree_of.find(root);
        if (it != tree_of.end()) return it->second;
        const uint32_t tr = (uint32_t)nroot_rec.size();
        tree_of.emplace(root, tr);
        nroot_rec.push_back((uint32_t)t.rec.size());
        thread_subtree(s, node_ref, RAW_RET, t);
        return tr;
    };
    for (size_t ii = 0; ii < a.insts.size(); ii++) {
        gs_instance& in = a.insts[ii];
        if ((in.child >> GS_REF_SHIFT) != GS_REF_NODE) continue;
        // Only instances a reachable leaf walks: validate() checked their trees (indices,
        // depth, leaves); an unreachable one is never read by the kernel and may be
        // malformed, so its node child is dropped, not walked.
        if (!inst_reached[ii]) {
            in.child = GS_REF_NONE;
            continue;
        }
        in.child = GS_MAKE_REF(GS_REF_NODE, tree_index(in.child));
    }
    // (GS_FEAT_GENERAL) a BVH that is a medium's boundary with no chain: threaded alike,
    // the medium's device boundary the tree's ref (tree_test)
    if (general)
        for (size_t mi = 0; mi < a.media.size(); mi++)
            if (media_reached[mi] && (a.media[mi].boundary >> GS_REF_SHIFT) == GS_REF_NODE)
                a.media[mi].boundary = GS_MAKE_REF(GS_REF_NODE, tree_index(a.media[mi].boundary));
    if (nroot_rec.size() > GS_REF_MASK) return fail(GS_ERR_UNSUPPORTED, "too many BVHs under instances");
    return GS_OK;
}

// Static estimate for the nested records (those from n_top on): a top-level leaf whose chain
// ends in a tree gives it its score and depth; inside, the smallest surface area on the path
// relative to the tree's root box (rigid transforms keep areas).
void score_nested_trees(ThreadedTree& t, uint32_t n_top, const std::vector<gs_instance>& insts,
                        const std::vector<uint32_t>& nroot_rec) {
    std::vector<double> tree_score(nroot_rec.size(), 0.0);  // a tree's best entry (its leaves' score)
    std::vector<uint32_t> tree_depth(nroot_rec.size(), 0);
    for (uint32_t i = 0; i < n_top; i++) {
        if (!t.leaf[i]) continue;
        uint32_t r = t.rec[i].right;
        for (int k = 0; k < GS_MAX_CHAIN && (r >> GS_REF_SHIFT) == GS_REF_INSTANCE; k++) r = insts[r & GS_REF_MASK].child;
        if ((r >> GS_REF_SHIFT) != GS_REF_NODE) continue;
        const uint32_t tr = r & GS_REF_MASK;
        if (t.score[i] > tree_score[tr]) {
            tree_score[tr] = t.score[i];
            tree_depth[tr] = t.depth[i] + 1;
        }
    }
    const uint32_t total = (uint32_t)t.rec.size();
    t.depth.resize(total, 0);
    t.score.resize(total, 0.0);
    for (size_t tr = 0; tr < nroot_rec.size(); tr++) {
        const uint32_t first = nroot_rec[tr];
        const uint32_t end = tr + 1 < nroot_rec.size() ? nroot_rec[tr + 1] : total;
        const double sa_root = box_area(t.rec[first]);
        t.depth[first] = tree_depth[tr];
        t.score[first] = tree_score[tr];
        std::vector<double> local(end - first, sa_root);
        for (uint32_t i = first; i < end; i++)
            if (!t.leaf[i]) {
                const double sa = std::min(local[i - first], box_area(t.rec[i]));
                for_children(t, i, end, [&](uint32_t c) {
                    t.depth[c] = t.depth[i] + 1;
                    local[c - first] = sa;
                    t.score[c] = sa_root > 0.0 ? tree_score[tr] * std::min(1.0, sa / sa_root) : tree_score[tr];
                });
            }
    }
}

// Leaf runs pay when at least a quarter of the leaf records are the first of two
// adjacent sphere leaves (C4's two-sphere leaves of BVH.rs:44-55: ~half).
bool has_leaf_runs(const ThreadedTree& t) {
    // (over every record: a nested tree's leaf pairs run in the same leaf passes)
    const uint32_t na = (uint32_t)t.rec.size();
    uint64_t leaves = 0, pairs = 0;
    for (uint32_t i = 0; i < na; i++) {
        leaves += t.leaf[i];
        pairs += i + 1 < na && sphere_leaf(t, i) && sphere_leaf(t, i + 1) && t.rec[i].left == i + 1;
    }
    return leaves && pairs * 4 >= leaves;
}
// Every top-level leaf (the records before n_top) is a stationary sphere, and there is one.
bool sphere_leaves_only(const ThreadedTree& t, uint32_t n_top) {
    bool any = false;
    for (uint8_t l : t.leaf) any |= l != 0;
    for (uint32_t i = 0; i < n_top && any; i++) any = !t.leaf[i] || sphere_leaf(t, i);
    return any;
}
// Node steps per node pass (MI355X, Msamples/s).  Sphere-only trees take long
// node runs (C4: 3 -> 6101, 8 -> 6347).  Trees whose leaf tests are mostly other
// kinds keep their lanes in step, one node per pass, so that a leaf pass finds
// them at one leaf and takes the scalar-load path (C3: 1 -> 10336, 3 -> 9194,
// 8 -> 6818).  Mixed trees in between (C5: 3 -> 5629, 8 -> 5088).
int32_t scene_node_steps(double other_leaf_frac) {
    return other_leaf_frac == 0.0 ? GS_NODE_STEPS : (other_leaf_frac >= 0.5 ? 1 : 3);
}

std::vector<DMaterial> device_materials(const gs_flat_scene& s) {
    std::vector<DMaterial> mats(s.n_materials);
    for (uint32_t i = 0; i < s.n_materials; i++) {
        const gs_material& m = s.materials[i];
        DMaterial d{};
        d.texture = m.texture;
        const bool textured = m.kind == GS_MAT_LAMBERTIAN || m.kind == GS_MAT_DIFFUSE_LIGHT || m.kind == GS_MAT_ISOTROPIC;
        d.needs_uv = textured ? tex_needs_uv(s, m.texture) : 0;
        if (textured) {
            const gs_texture& t = s.textures[m.texture];
            const bool solid = t.kind == GS_TEX_SOLID;
            const bool checker2 = t.kind == GS_TEX_CHECKERED && s.textures[t.even].kind == GS_TEX_SOLID &&
                                  s.textures[t.odd].kind == GS_TEX_SOLID;
            if (m.kind == GS_MAT_LAMBERTIAN) {
                d.kind = solid ? DM_LAMB_SOLID : (checker2 ? DM_LAMB_CHECKER : DM_LAMB_TEX);
            } else if (m.kind == GS_MAT_ISOTROPIC) {
                d.kind = solid ? DM_ISO_SOLID : DM_ISO_TEX;
            } else {
                d.kind = solid ? DM_LIGHT_SOLID : DM_LIGHT_TEX;
            }
            if (solid) {
                for (int k = 0; k < 3; k++) d.a[k] = t.color[k];
            } else if (checker2 && m.kind == GS_MAT_LAMBERTIAN) {
                for (int k = 0; k < 3; k++) {
                    d.a[k] = s.textures[t.even].color[k];
                    d.b[k] = s.textures[t.odd].color[k];
                }
                d.param = t.scale_inv;
            }
        } else if (m.kind == GS_MAT_METAL) {
            d.kind = DM_METAL;
            for (int k = 0; k < 3; k++) d.a[k] = m.albedo[k];
            d.param = m.param;
        } else {
            d.kind = DM_DIELECTRIC;
            d.param = m.param;
        }
        mats[i] = d;
    }
    return mats;
}

// The kernel instantiation (GS_FEAT_*) for a scene, from the facts it depends on.
struct FeatFacts {
    bool media;         // the scene has ConstantMedium records
    bool nested;        // BVHs under instance chains (validate)
    bool general;       // a composition only the catch-all kernel walks (validate)
    bool leaf_runs;     // has_leaf_runs
    bool sph_leaves;    // sphere_leaves_only
    bool all_mirrored;  // the static placement mirrors every node and leaf record
    bool sky;           // the background is not a solid colour
    const std::vector<DMaterial>* mats;
};
int choose_feat(const FeatFacts& f) {
    // compositions only the catch-all instantiation walks (round 6; validate)
    if (f.general) return GS_FEAT_GENERAL_KERNEL;
    int feat = (f.media ? GS_FEAT_MEDIA : 0) | (f.nested ? GS_FEAT_NESTED : 0) | (f.leaf_runs ? GS_FEAT_LEAFRUN : 0);
    const bool flat = !(feat & (GS_FEAT_MEDIA | GS_FEAT_NESTED));
    if (flat && f.all_mirrored) feat |= GS_FEAT_LDSTREE;  // (cleared at launch if the device's LDS cannot hold it all)
    // staged shading when three or more of its sharing cases can meet in one wave
    bool lamb = false, metal = false, diel = false, iso = false;
    for (const DMaterial& m : *f.mats) {
        lamb |= m.kind >= DM_LAMB_SOLID && m.kind <= DM_LAMB_TEX;
        metal |= m.kind == DM_METAL;
        diel |= m.kind == DM_DIELECTRIC;
        iso |= m.kind == DM_ISO_SOLID || m.kind == DM_ISO_TEX;
    }
    const int cases = (int)lamb + (int)metal + (int)diel + (int)iso + (int)f.sky;
    if (cases >= 3 && flat) feat |= GS_FEAT_MIXED;
    // (round 6: also without leaf runs -- C1, C2, A1's lone sphere -- for the sphere-only hit record)
    if (f.sph_leaves && flat) feat |= GS_FEAT_SPHLEAF;
    if ((feat & (GS_FEAT_SPHLEAF | GS_FEAT_MIXED)) == (GS_FEAT_SPHLEAF | GS_FEAT_MIXED) && g_plain_kernels) {
        // every hit a stationary sphere (SPHLEAF): plain materials, no uv -> GS_FEAT_PLAIN
        bool plain = true;
        for (const DMaterial& m : *f.mats)
            plain &= (m.kind == DM_LAMB_SOLID || m.kind == DM_LAMB_CHECKER || m.kind == DM_METAL ||
                      m.kind == DM_DIELECTRIC) && !m.needs_uv;
        if (plain) feat |= GS_FEAT_PLAIN;
    }
    return feat;
}

// The quads' and spheres' traversal records, the device materials, and the HDRI as 4-byte
// RGBE texels when every f32 texel round-trips exactly.
void convert_primitives(const gs_flat_scene& s, DeviceArrays& a) {
    a.tquads.resize(s.n_quads);
    for (uint32_t i = 0; i < s.n_quads; i++) {
        const gs_quad& q = s.quads[i];
        a.tquads[i] = TQuad{q.normal[0], q.normal[1], q.normal[2], q.d, q.q[0], q.q[1], q.q[2], q.u[0],
                            q.u[1],      q.u[2],      q.v[0],      q.v[1], q.v[2], q.w[0], q.w[1], q.w[2]};
    }
    a.sph.resize(s.n_spheres);
    a.sph_mat.resize(s.n_spheres);
    for (uint32_t i = 0; i < s.n_spheres; i++) {
        const gs_sphere& x = s.spheres[i];
        a.sph[i] = DSphere{x.center[0], x.center[1], x.center[2], x.radius};
        a.sph_mat[i] = x.material;
    }
    a.mats = device_materials(s);
    if (s.background.kind == GS_BG_HDRI) {
        const uint64_t n = (uint64_t)s.background.width * s.background.height;
        a.rgbe.resize(n);
        for (uint64_t k = 0; k < n && !a.rgbe.empty(); k++)
            if (!encode_rgbe(s.hdri_rgb + 3 * k, &a.rgbe[k])) a.rgbe.clear();
    }
}

// One device allocation for every array and the launch slots' parameter blocks; fills
// ds->dev, ds->tquads, ds->nroots and the slots.  On failure the caller destroys the scene.
gs_status upload_scene(const gs_flat_scene& s, const DeviceArrays& a, const Placed& pl, gs_device_scene* ds) {
    Layout L;
    const size_t o_nroots = L.add(pl.nroots.data(), pl.nroots.size() * 4);
    const size_t o_tnodes = L.add(pl.tnodes.data(), pl.tnodes.size() * sizeof(TNode));
    const size_t o_tboxes = L.add(pl.tboxes.data(), pl.tboxes.size() * sizeof(TBox));
    const size_t o_tleaves = L.add(pl.tleaves.data(), pl.tleaves.size() * sizeof(TLeaf));
    const size_t o_tquads = L.add(a.tquads.data(), a.tquads.size() * sizeof(TQuad));
    const size_t o_sph = L.add(a.sph.data(), a.sph.size() * sizeof(DSphere));
    const size_t o_sphm = L.add(a.sph_mat.data(), a.sph_mat.size() * 4);
    const size_t o_msph = L.add(s.mspheres, s.n_mspheres * sizeof(gs_msphere));
    const size_t o_quad = L.add(s.quads, s.n_quads * sizeof(gs_quad));
    const size_t o_tri = L.add(s.triangles, s.n_triangles * sizeof(gs_triangle));
    const size_t o_list = L.add(a.lists.data(), a.lists.size() * sizeof(gs_list));
    const size_t o_cubes = L.add(a.cubes.data(), a.cubes.size() * sizeof(double));
    const size_t o_lref = L.add(s.list_refs, s.n_list_refs * 4);
    const size_t o_inst = L.add(a.insts.data(), a.insts.size() * sizeof(gs_instance));
    const size_t o_media = L.add(a.media.data(), a.media.size() * sizeof(gs_medium));
    const size_t o_perm = L.add(s.noise_perm, s.noise_perm ? s.n_noise_perm : 0);
    const size_t o_mat = L.add(a.mats.data(), a.mats.size() * sizeof(DMaterial));
    const size_t o_tex = L.add(s.textures, s.n_textures * sizeof(gs_texture));
    const size_t o_img = L.add(s.images, s.n_images * sizeof(gs_image));
    const size_t o_texel = L.add(s.texels8, s.n_texels8);
    const size_t o_hdri = L.add(s.hdri_rgb, (s.background.kind == GS_BG_HDRI && a.rgbe.empty()) ? s.n_hdri_floats * 4 : 0);
    const size_t o_rgbe = L.add(a.rgbe.data(), a.rgbe.size() * 4);
    size_t o_slot[kLaunchSlots];
    for (int k = 0; k < kLaunchSlots; k++) o_slot[k] = L.add(nullptr, 256 + sizeof(KParams));  // queue, params

    (void)hipGetDevice(&ds->device);
    ds->bytes = L.blob.size();
    if (hipMalloc(&ds->mem, ds->bytes) != hipSuccess) {
        ds->mem = nullptr;
        return fail(GS_ERR_OOM, "hipMalloc of " + std::to_string(L.blob.size()) + " bytes failed");
    }
    hipError_t e = hipMemcpy(ds->mem, L.blob.data(), ds->bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    uint8_t* b = (uint8_t*)ds->mem;
    DevScene& d = ds->dev;
    d.nroots = (const uint32_t*)(b + o_nroots);
    d.spheres = (const DSphere*)(b + o_sph);
    d.sphere_mat = (const uint32_t*)(b + o_sphm);
    d.mspheres = (const gs_msphere*)(b + o_msph);
    d.quads = (const gs_quad*)(b + o_quad);
    d.tris = (const gs_triangle*)(b + o_tri);
    d.lists = (const gs_list*)(b + o_list);
    d.list_refs = (const uint32_t*)(b + o_lref);
    d.cubes = (const double*)(b + o_cubes);
    d.inst = (const gs_instance*)(b + o_inst);
    d.media = (const gs_medium*)(b + o_media);
    d.noise_perm = (const uint8_t*)(b + o_perm);
    d.mats = (const DMaterial*)(b + o_mat);
    d.texs = (const gs_texture*)(b + o_tex);
    d.images = (const gs_image*)(b + o_img);
    d.texels = (const uint8_t*)(b + o_texel);
    d.hdri = (const float*)(b + o_hdri);
    d.hdri_rgbe = a.rgbe.empty() ? nullptr : (const uint32_t*)(b + o_rgbe);
    d.bg = s.background;
    d.root = device_ref(s.root);
    d.tnodes = (const TNode*)(b + o_tnodes);
    d.tboxes = (const TBox*)(b + o_tboxes);
    d.tleaves = (const TLeaf*)(b + o_tleaves);
    ds->tquads = (const TQuad*)(b + o_tquads);
    ds->nroots = (uint32_t*)(b + o_nroots);
    for (int k = 0; k < kLaunchSlots; k++) {
        ds->slots[k].queue = (uint32_t*)(b + o_slot[k]);
        ds->slots[k].params = (KParams*)(b + o_slot[k] + 256);
        if (hipEventCreateWithFlags(&ds->slots[k].done, hipEventDisableTiming) != hipSuccess)
            return fail(GS_ERR_HIP, "hipEventCreateWithFlags failed");
    }
    return GS_OK;
}

struct DestroyScene {
    void operator()(gs_device_scene* ds) const { (void)gs_device_scene_destroy(ds); }
};

}  // namespace

extern "C" {

gs_status gs_device_scene_create(const gs_flat_scene* s, gs_device_scene** out) {
    if (!s || !out) return fail(GS_ERR_ARG, "null argument");
    *out = nullptr;
    uint32_t depth = 1;
    bool nested = false, general = false;
    std::vector<uint8_t> inst_reached, media_reached;
    gs_status st = validate(*s, &depth, &nested, &inst_reached, &general, &media_reached);
    if (st != GS_OK) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GS_ERR_NO_DEVICE, "no HIP device visible");

    std::unique_ptr<gs_device_scene, DestroyScene> ds(new gs_device_scene());
    DeviceArrays a;
    const Knobs knobs = read_knobs();  // one snapshot of the upload's test hooks
    find_cube_lists(*s, knobs.cube_lists != 0, a, ds->single_quads);
    ds->n_cubes = (uint32_t)(a.cubes.size() / GS_CUBE_DOUBLES);
    a.insts.assign(s->instances, s->instances + s->n_instances);
    a.media.assign(s->media, s->media + s->n_media);

    // The threaded tree, kept by the scene: re-placed after a launch's pilot (place_records).
    ThreadedTree& t = ds->tree;
    thread_subtree(*s, s->root, RAW_END, t);
    const uint32_t n_top = (uint32_t)t.rec.size();
    score_top_level(t, ds->nodes_per_leaf, ds->other_leaf_frac);
    st = thread_nested_trees(*s, general, inst_reached, media_reached, t, a, ds->nroot_rec);
    if (st != GS_OK) return st;
    score_nested_trees(t, n_top, a.insts, ds->nroot_rec);

    // (the placement's prefix is cut for the scene's fixed-spp kernel, whose lane-state layout
    // follows from these facts alone -- choose_feat; the shading flags do not enter it)
    const bool flat = !general && !nested && s->n_media == 0;
    const int64_t own_budget = lds_mirror_budget(lane_state_in_regs(
        GS_FEAT_FIXED | (flat ? 0 : GS_FEAT_GENERAL_KERNEL) | (flat && sphere_leaves_only(t, n_top) ? GS_FEAT_SPHLEAF : 0)));
    ds->mirror_budget = g_lds_mirror < 0 ? own_budget : g_lds_mirror;
    if (knobs.mirror_budget >= 0) ds->mirror_budget = std::min(knobs.mirror_budget, own_budget);  // (test hook)
    Placed pl = place_records(ds.get(), nullptr);
    if (pl.tnodes.size() >= (1u << 26) || pl.tleaves.size() >= (1u << 26))
        return fail(GS_ERR_UNSUPPORTED, "more than 2^26 top-level BVH records");
    ds->cert_boxes = knobs.cert_boxes != 0;  // (0, a test hook: every node step takes the f64 test)
    for (const TBox& b : pl.tboxes)
        for (double v : {b.mnx, b.mny, b.mnz, b.mxx, b.mxy, b.mxz})
            if (!(std::fabs(v) <= 1e15)) ds->cert_boxes = false;
    ds->node_records = (uint32_t)pl.tnodes.size();
    ds->leaf_records = (uint32_t)pl.tleaves.size();

    convert_primitives(*s, a);
    st = upload_scene(*s, a, pl, ds.get());
    if (st != GS_OK) return st;
    adopt_placement(ds.get(), pl);

    ds->n_nodes = s->n_nodes;
    ds->n_quads = s->n_quads;
    ds->bvh_depth = depth < 1 ? 1 : depth;
    FeatFacts f{};
    f.media = s->n_media != 0;
    f.nested = nested;
    f.general = general;
    f.leaf_runs = has_leaf_runs(t);
    f.sph_leaves = sphere_leaves_only(t, n_top);
    f.all_mirrored = ds->mirror.nodes == ds->node_records && ds->mirror.leaves == ds->leaf_records;
    f.sky = s->background.kind != GS_BG_SOLID;
    f.mats = &a.mats;
    ds->feat = choose_feat(f);
    ds->node_steps = scene_node_steps(ds->other_leaf_frac);
    // Scenes with BVHs under instances (kind-batched leaf passes over many leaf kinds) gather
    // more lanes per leaf pass, each pass serving one kind, and step nodes in full passes:
    // final_scene 1440^2 x 64 spp, (leaf batch, node steps): (12, 1) 1206, (32, 3) 1540,
    // (48, 3) 1594, (48, 8) 1679, (64, 8) 1662 Msamples/s (profiles/r03/sweep_final_scene_
    // leaf_batch*.txt).  Not for staged shading alone: C5 leaf batch 12 6178, 24 5989, 48 5236.
    // ... and shade smaller batches (round 4, after the nested-leaf changes; shade batch x leaf
    // batch at 8 node steps, twice: 44 / 48: 2 396, 2 462; 44 / 56: 2 449, 2 453; 52 / 48:
    // 2 365, 2 398 Msamples/s, profiles/r04/sweep_final_scene_shade_leaf_batch.txt).
    // Round 5 walks the nested BVHs in the main node passes, so a leaf pass holds fewer
    // leaf kinds and smaller batches pay: leaf batch 48 -> 2 577, 24 -> 2 644-2 660
    // Msamples/s (profiles/r05).
    if (ds->feat & GS_FEAT_NESTED) {
        ds->leaf_batch = GS_KIND_LEAF_BATCH;
        ds->shade_batch = GS_KIND_SHADE_BATCH;
        ds->node_steps = std::max<int32_t>(ds->node_steps, GS_KIND_NODE_STEPS);
    }
    *out = ds.release();
    return GS_OK;
}

gs_status gs_device_scene_info(const gs_device_scene* ds, gs_scene_info* out) {
    if (!ds || !out) return fail(GS_ERR_ARG, "null argument");
    gs_scene_info i{};
    i.node_records = ds->node_records;
    i.leaf_records = ds->leaf_records;
    i.lds_nodes = ds->mirror.nodes;
    i.lds_leaves = ds->mirror.leaves;
    i.lds_quads = ds->mirror.quads;
    i.feat = ds->feat;
    i.node_steps = launch_node_steps(ds, read_knobs());
    i.cert_boxes = ds->cert_boxes ? 1 : 0;
    i.nodes_per_leaf = ds->nodes_per_leaf;
    i.other_leaf_frac = ds->other_leaf_frac;
    i.placement = ds->placement.load(std::memory_order_acquire);
    i.long_samples = ds->long_samples.load(std::memory_order_relaxed) ? 1 : 0;
    i.pilot_ms = ds->pilot_ms;
    *out = i;
    return GS_OK;
}

gs_status gs_device_scene_destroy(gs_device_scene* ds) {
    if (!ds) return GS_OK;
    for (auto& sl : ds->slots) {
        if (sl.done) {
            if (sl.used) (void)hipEventSynchronize(sl.done);
            (void)hipEventDestroy(sl.done);
        }
        if (sl.partial) (void)hipFree(sl.partial);
        if (sl.rbuf) (void)hipFree(sl.rbuf);
        if (sl.nest_save) (void)hipFree(sl.nest_save);
        if (sl.views) (void)hipFree(sl.views);
        if (sl.vstate) (void)hipFree(sl.vstate);
        if (sl.vorder) (void)hipFree(sl.vorder);
    }
    if (ds->query_done) {
        if (ds->query_used) (void)hipEventSynchronize(ds->query_done);
        (void)hipEventDestroy(ds->query_done);
    }
    if (ds->mem) (void)hipFree(ds->mem);
    delete ds;
    return GS_OK;
}

}  // extern "C"
