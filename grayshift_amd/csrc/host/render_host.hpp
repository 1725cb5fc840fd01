// render_host.hpp — the host side of the renderer, shared by scene.cpp (flat scene -> device
// scene) and launch.cpp (device scene -> launches): the device scene itself, its launch slots,
// the threaded tree and its placement, the process knobs and the error helpers.
#pragma once
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../device/kernel_abi.hpp"
#include "internal.hpp"

// Sets the thread's gs_last_error text and returns `code`.
gs_status fail(gs_status code, const std::string& msg);
#define HIPCHK(x)                                                                               \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return fail(GS_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Process-wide tuning (the gs_set_* / gs_debug_set_* setters, launch.cpp), as one snapshot:
// a setter may run while another thread launches; each launch takes one snapshot, so one
// launch never mixes two settings of the same knob.
struct Knobs {
    int32_t shade_batch;     // 0: the scene's own
    int32_t blocks_per_cu;   // 0 = occupancy query
    int32_t node_steps;      // 0: the scene's own (gs_device_scene.node_steps)
    int32_t leaf_batch;      // 0: the scene's own
    int32_t cam_batch;       // 0: the scene's own (gs_set_camera_batch)
    int32_t tail_pct;        // guided tail (gs_debug_set_guided_tail): 0 = default
    int32_t sample_chunk;    // -1 auto, 0 never split a pixel's samples
    int32_t placement;       // 1: placement pilot at a scene's first launch; 0: the static estimate only
    uint64_t partial_budget; // auto chunks: at most this many bytes of chunk sums (per launch slot)
    int32_t adaptive_rounds; // 1 auto (GS_ROUND_MIN_CAP), 2 always rounds, 0 never
    int32_t round_whole;     // work items of a round: 0 split, 1 whole-batch, -1 whole while the lanes fill twice
    int32_t cube_lists;      // gs_debug_set_cube_lists
    int32_t cert_boxes;      // gs_debug_set_cert_boxes: 1 the 1e15 rule decides, 0 no scene has certified boxes
    int64_t mirror_budget;   // gs_debug_set_mirror_budget: -1 the block's own budget, >= 0 at most this many bytes
    int32_t max_blocks;      // gs_debug_set_max_blocks: 0 no limit, >= 1 at most this many blocks per launch
};
Knobs read_knobs();

// The prefixes of the node, leaf, quad and Quad::cube record arrays that each block mirrors
// in LDS (KArgs::lds_*), in that order.
struct MirrorPrefix {
    uint32_t nodes = 0, leaves = 0, quads = 0, cubes = 0;
    int64_t bytes() const {
        return (int64_t)nodes * (int64_t)sizeof(TNode) + (int64_t)leaves * (int64_t)sizeof(TLeaf) +
               (int64_t)quads * (int64_t)sizeof(TQuad) + (int64_t)cubes * (GS_CUBE_DOUBLES * 8);
    }
};

// One in-flight launch's device state: its parameter block, its work-queue counter and
// its chunk sums.  A scene keeps a small ring of them, so launches of one scene on
// different streams (or host threads) never share state; a slot is reused only after
// the stream of the new launch has waited for the slot's previous launch (its event).
struct LaunchSlot {
    KParams* params = nullptr;  // device
    uint32_t* queue = nullptr;  // device
    double* partial = nullptr;  // chunk partial sums, grown on demand
    size_t partial_bytes = 0;
    hipEvent_t done = nullptr;  // recorded after the slot's last launch
    hipStream_t stream = nullptr;  // the stream of the slot's last launch
    bool used = false;
    // batch rounds (adaptive settings): round counts, the two active lists, the running sums
    void* rbuf = nullptr;
    size_t rbuf_bytes = 0;
    // GS_FEAT_NESTED: each lane's save slots (KParams::nest_save), 8 slot-major arrays of 8 B per lane of the grid
    double* nest_save = nullptr;
    size_t nest_save_bytes = 0;
    // a views launch's records (KParams::views)
    gs_view* views = nullptr;
    size_t views_bytes = 0;
    // a progressive views pass's per-view records (KParams::vstate) and its tile order (KParams::order)
    GsViewState* vstate = nullptr;
    size_t vstate_bytes = 0;
    int32_t* vorder = nullptr;
    size_t vorder_bytes = 0;
};
static const int kLaunchSlots = 4;

// The threaded top-level tree before placement: pre-order records (DNode: a node's f64
// box, hit link = the next record, miss link; a leaf's sphere inline, next link, ABI ref),
// with each record's depth and static visit estimate.
struct ThreadedTree {
    std::vector<gsd::DNode> rec;
    std::vector<uint8_t> leaf;
    std::vector<uint32_t> depth;
    std::vector<double> score;
};

// The device arrays of one placement: node records, their f64 boxes, leaf records, with
// the mirrored prefixes first, and the root's link.
struct Placed {
    std::vector<TNode> tnodes;
    std::vector<TBox> tboxes;
    std::vector<TLeaf> tleaves;
    std::vector<uint32_t> pos;  // tree record -> its position in tnodes / tleaves
    std::vector<uint32_t> nroots;  // the links of the nested trees' roots (DevScene::nroots)
    MirrorPrefix mirror;
    uint32_t root = THR_END;
};

struct gs_device_scene {
    int device = 0;
    void* mem = nullptr;  // one allocation for every array
    size_t bytes = 0;
    // The device arrays (the threaded tree's node records, their f64 boxes and leaf records
    // among them: dev.tnodes, dev.tboxes, dev.tleaves).
    DevScene dev{};
    uint32_t n_nodes = 0;
    uint32_t bvh_depth = 1;  // top-level BVH depth (informational: the walk keeps no stack)
    bool cert_boxes = false;  // every top-level node coordinate |x| <= 1e15 (box_cert applies)
    int feat = 0;             // GS_FEAT_* of the kernel instantiation to launch
    // Test hook (gs_debug_last_launch_feat): the feature word the most recent render-kernel
    // launch of this scene passed to kernel_for (-1: no launch yet).  Host only.
    mutable std::atomic<int32_t> last_launch_feat{-1};
    const TQuad* tquads = nullptr;  // every quad's traversal record, gs_quad order
    uint32_t thr_root = THR_END;    // the threaded tree's first link (THR_*)
    MirrorPrefix mirror;            // mirrored prefixes (per block) of the current placement
    // BVHs under instance chains, threaded into the node / leaf arrays with the top-level
    // tree: each tree's root record (tree index -> record of ThreadedTree), and the device
    // array of their links (DevScene::nroots), rewritten with the records at re-placement
    std::vector<uint32_t> nroot_rec;
    uint32_t* nroots = nullptr;
    uint32_t n_cubes = 0;  // Quad::cube records (cube_test)
    int32_t node_steps = GS_NODE_STEPS;      // node steps per node pass (from the tree's shape)
    int32_t leaf_batch = 12;                 // lanes at a leaf before a leaf pass (scene's choice)
    int32_t shade_batch = 52;                // finished lanes a wave shades together (scene's choice)
    int32_t cam_batch = 1;                   // lanes waiting for camera rays before a wave runs get_ray
    // A sample's cost on this device, lane-microseconds (kernel time x lanes / samples), from
    // the frame context's last frame (gs_device_scene_note_frame); 0 = not measured yet.  Once
    // a frame measured long samples, the guided tail's small-frame rule stays off for the
    // scene (long_samples: sticky, so a scene near the threshold does not alternate layouts
    // from frame to frame).
    std::atomic<double> lane_us_per_sample{0.0};
    std::atomic<bool> long_samples{false};
    uint32_t node_records = 0, leaf_records = 0;
    double nodes_per_leaf = 0.0, other_leaf_frac = 0.0;
    // Launch state, mutated by launches of a const scene: guarded by `mu`.
    std::mutex mu;
    // launch geometry, computed at the first launch (host API queries cost ~0.5 ms each)
    // Launch shape per launched instantiation (`want`: the word the launch asks kernel_for or
    // views_round_kernel_for for, e.g. feat | GS_FEAT_FIXED) and lane-state size (chunked: a
    // fixed-spp launch, which keeps no Σlum / Σlum² / count): the mirror prefixes that fit next
    // to that kernel's lane state, the dynamic LDS, the kernel's f64 lane fields (KArgs::lane_nd),
    // the word to launch (`want` minus GS_FEAT_LDSTREE when the mirror is a strict prefix) and
    // blocks/CU.  A few entries per scene at most; emptied when the placement changes.
    struct LaunchCfg {
        int want = 0;
        bool views_round = false, chunked = false;
        MirrorPrefix mirror;
        uint32_t nest_lds = 0, lane_nd = 0;
        size_t lds = 0;
        int feat = 0, per_cu = 0;
    };
    std::vector<LaunchCfg> lcfg;
    int cus = 0;
    LaunchSlot slots[kLaunchSlots];
    uint32_t next_slot = 0;
    // Ray queries (query.cpp) take no slot: the event after the last one, for the pilot's end and
    // the scene's destruction to wait for, and that query's stream
    hipEvent_t query_done = nullptr;
    hipStream_t query_stream = nullptr;
    bool query_used = false;
    // Placement of the threaded records (place_records): the static estimate until the
    // first launch, whose pilot (run_pilot) measures the visits and re-places them.
    ThreadedTree tree;
    std::vector<uint32_t> pos;  // tree record -> position (current placement)
    uint32_t n_quads = 0;
    std::vector<uint32_t> single_quads;  // the quads outside cube lists (place_records)
    int64_t mirror_budget = 0;
    std::atomic<int> placement{0};  // 0 static, pilot pending; 1 static (final); 2 measured
    double pilot_ms = 0.0;
    std::mutex place_mu;  // held while a pilot runs and the records are re-placed
};

// scene.cpp
// Order the scene's threaded records by how likely a ray tests them (measured `visits` per
// record when given, else the static estimate) and cut the mirror prefixes for its budget.
Placed place_records(const gs_device_scene* ds, const std::vector<uint64_t>* visits);
// Makes `pl`, whose records the device arrays already hold, the scene's current placement:
// the root link, the mirror prefixes, the record positions; the launch shapes are derived
// again at the next launch.  (The caller holds `mu` once the scene is shared.)
void adopt_placement(gs_device_scene* ds, Placed& pl);

// launch.cpp
// Node steps per node pass of a launch: the knob or the scene's own, within the unroll.
int32_t launch_node_steps(const gs_device_scene* ds, const Knobs& k);
