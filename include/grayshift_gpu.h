/*
 * grayshift_gpu.h — the C-ABI drop-in boundary of the MI355X path tracer.
 *
 * This is what the reference's `Camera::render` (src/camera.rs:100) calls in place
 * of its pixel loop (camera.rs:105-114: pixel list + rayon `par_iter` + `sample`).
 * The host (the reference's Rust crate, or the C++ mirror in grayshift_amd/csrc/host)
 * builds the world, builds the BVH with the reference's own median split
 * (hittable/BVH.rs:18-65) and flattens it into the plain arrays below; the library
 * copies them into HBM and runs the persistent HIP megakernel.  The output stage
 * (PPM header + write_color, camera.rs:101-103,116-118) stays on the host.
 *
 * Plain pointers and sizes only; no torch, no HIP types in the signatures (a stream
 * is passed as `void*`).  No exceptions cross the ABI: every entry point returns a
 * gs_status and leaves a message for gs_last_error().  Launches of one gs_device_scene
 * may be issued from several host threads and on several streams: each launch takes
 * its own parameter / work-queue / chunk-sum slot from a small ring (a slot is reused
 * only after its previous launch has finished, by a stream wait on that launch's event).
 */
#ifndef GRAYSHIFT_GPU_H
#define GRAYSHIFT_GPU_H

#include <stddef.h>
#include <stdint.h>
#include "grayshift_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 11

typedef int32_t gs_status;
enum {
    GS_OK = 0,
    GS_ERR_ARG = -1,         /* bad argument / malformed scene */
    GS_ERR_HIP = -2,         /* HIP runtime error */
    GS_ERR_OOM = -3,         /* device allocation failed */
    GS_ERR_UNSUPPORTED = -4, /* scene feature the device path does not implement */
    GS_ERR_NO_DEVICE = -5    /* no gfx950 device visible */
};

/* ---- tagged child references (32 bit: kind << 28 | index) ---- */
#define GS_REF_SHIFT 28u
#define GS_REF_MASK 0x0FFFFFFFu
enum gs_ref_kind {
    GS_REF_NONE = 0,     /* absent right child (BVH.rs:20-28 n == 1 wrapper) */
    GS_REF_NODE = 1,     /* BVHNode                       -> nodes[]     */
    GS_REF_SPHERE = 2,   /* stationary Sphere             -> spheres[]   */
    GS_REF_MSPHERE = 3,  /* moving Sphere                 -> mspheres[]  */
    GS_REF_QUAD = 4,     /* Quad                          -> quads[]     */
    GS_REF_TRIANGLE = 5, /* Triangle                      -> triangles[] */
    GS_REF_LIST = 6,     /* HittableList of primitives    -> lists[]     */
    GS_REF_INSTANCE = 7, /* Translate / RotateY           -> instances[] */
    GS_REF_MEDIUM = 8,   /* ConstantMedium                -> media[]     */
    GS_REF_BUILD_MEMBER = 15 /* build-only: member index of a gs_bvh_build_async without refs; no
                              * scene may hold it (gs_device_scene_create rejects it) */
};
#define GS_MAKE_REF(kind, idx) (((uint32_t)(kind) << GS_REF_SHIFT) | ((uint32_t)(idx) & GS_REF_MASK))

/* BVH node: the reference AABB in f64 (AABB.rs:7-11) and the two children.
 * 64 B = one cache line, array-of-structs: a lane reads its whole node at once. */
typedef struct gs_node {
    double min[3];
    double max[3];
    uint32_t left, right; /* tagged refs; right may be GS_REF_NONE */
    uint32_t pad[2];
} gs_node;

/* Stationary sphere (sphere.rs:11-18): 40 B. */
typedef struct gs_sphere {
    double center[3];
    double radius;
    uint32_t material;
    uint32_t pad;
} gs_sphere;

/* Moving sphere: center(time) = center_start + time * center_path (sphere.rs:51-53). 64 B. */
typedef struct gs_msphere {
    double center_start[3];
    double center_path[3];
    double radius;
    uint32_t material;
    uint32_t pad;
} gs_msphere;

/* Quad with its plane (quad.rs:12-38, plane.rs:10-18): 136 B. */
typedef struct gs_quad {
    double q[3], u[3], v[3], w[3];
    double normal[3];
    double d;
    uint32_t material;
    uint32_t pad;
} gs_quad;

/* Triangle (triangle.rs:10-28): normal = (b-a)x(c-a), unnormalised. 104 B. */
typedef struct gs_triangle {
    double a[3], b[3], c[3];
    double normal[3];
    uint32_t material;
    uint32_t pad;
} gs_triangle;

/* HittableList (hittable.rs:45-91): list_refs[first .. first+count), each a primitive ref. */
typedef struct gs_list {
    uint32_t first, count;
} gs_list;

/* Instance transform, one per Translate / RotateY (hittable.rs:93-215). 32 B.
 * child: the wrapped object (another instance, a list, a primitive, a medium, or a BVH node:
 * a BVH under an instance chain, whose leaves are lists, primitives or media -- not
 * instances; at most 4 instances in a chain).  Other compositions: GS_ERR_UNSUPPORTED. */
enum { GS_INST_TRANSLATE = 1, GS_INST_ROTATE_Y = 2 };
typedef struct gs_instance {
    uint32_t kind;
    uint32_t child;
    double p[3]; /* TRANSLATE: offset; ROTATE_Y: sin_theta, cos_theta, 0 */
} gs_instance;

/* ConstantMedium (hittable/volume.rs:10-29): 16 B.  boundary: an instance chain, a list
 * or a primitive (no BVH, no medium); material: the phase function (any material). */
typedef struct gs_medium {
    uint32_t boundary;
    uint32_t material;
    double density_neg_inv; /* -1 / density (volume.rs:18) */
} gs_medium;

/* Material record (material.rs): 40 B. */
typedef struct gs_material {
    uint32_t kind;    /* gs_mat_kind */
    uint32_t texture; /* LAMBERTIAN / DIFFUSE_LIGHT / ISOTROPIC */
    double albedo[3]; /* METAL */
    double param;     /* METAL: fuzz; DIELECTRIC: refraction_index */
} gs_material;

/* Texture record (texture.rs): 48 B. */
typedef struct gs_texture {
    uint32_t kind;      /* gs_tex_kind */
    uint32_t even, odd; /* CHECKERED: texture indices */
    uint32_t image;     /* IMAGE: index into images[] */
    double color[3];    /* SOLID; NOISE: color[0] = scale (texture.rs:103) */
    double scale_inv;   /* CHECKERED: 1/scale (texture.rs:42) */
} gs_texture;

typedef struct gs_image {
    uint32_t width, height;
    uint64_t offset; /* byte offset into texels8 (RGB8, row-major, top row first) */
} gs_image;

/* Background (camera.rs:246-270).  For HDRI the rotation's matrix entries are
 * precomputed by the host with the exact expressions of rotate_vector (util.rs:67-86). */
typedef struct gs_background {
    uint32_t kind; /* gs_bg_kind */
    uint32_t width, height;
    uint32_t pad;
    double color[3];
    double rot[9]; /* row-major: x' = v.x*rot[0] + v.y*rot[1] + v.z*rot[2], ... */
} gs_background;

/* Flattened scene as handed over by the host. */
typedef struct gs_flat_scene {
    uint32_t root; /* tagged ref of the world BVH root */
    uint32_t max_bvh_depth;
    const gs_node* nodes;         uint32_t n_nodes;
    const gs_sphere* spheres;     uint32_t n_spheres;
    const gs_msphere* mspheres;   uint32_t n_mspheres;
    const gs_quad* quads;         uint32_t n_quads;
    const gs_triangle* triangles; uint32_t n_triangles;
    const gs_list* lists;         uint32_t n_lists;
    const uint32_t* list_refs;    uint32_t n_list_refs;
    const gs_instance* instances; uint32_t n_instances;
    const gs_material* materials; uint32_t n_materials;
    const gs_texture* textures;   uint32_t n_textures;
    const gs_image* images;       uint32_t n_images;
    const uint8_t* texels8;       uint64_t n_texels8;  /* bytes */
    gs_background background;
    const float* hdri_rgb;        uint64_t n_hdri_floats; /* width*height*3 */
    const gs_medium* media;       uint32_t n_media;       /* (ABI 2) */
    /* Perlin::default()'s permutation table (noise 0.9 PermutationTable::new(0)): 256
     * bytes when any texture is NOISE, else NULL / 0 (ABI 3). */
    const uint8_t* noise_perm;    uint32_t n_noise_perm;
} gs_flat_scene;

/* The fields `Camera::new` derives (camera.rs:17-98), computed by the host. */
typedef struct gs_camera {
    int32_t image_width, image_height;
    uint32_t max_depth;
    uint32_t pad;
    double center[3];
    double starting_pixel_pos[3];
    double pixel_delta_u[3];
    double pixel_delta_v[3];
    double defocus_angle;
    double defocus_disk_u[3];
    double defocus_disk_v[3];
} gs_camera;

/* Image-space partition: the frame is cut into tile_w x tile_h tiles.  Position
 * k = slot * world_size + r belongs to rank r; by default position k holds tile k
 * (round-robin, for load balance under adaptive sampling).  A rank's pixels are packed
 * slot after slot, each tile row-major inside, padded to full tiles: packed index =
 * slot*tile_w*tile_h + ty*tile_w + tx.
 * (ABI 3) d_tile_order, when set, is a DEVICE array of slots_per_rank * world_size tile
 * ids, position k -> tile (-1: an empty slot), e.g. the cost-balanced plan of
 * gs_plan_tiles; every tile must appear exactly once. */
typedef struct gs_partition {
    int32_t rank, world_size;
    int32_t tile_w, tile_h;
    const int32_t* d_tile_order; /* nullable */
    int32_t slots_per_rank;      /* with d_tile_order */
    int32_t pad;
} gs_partition;

/* Device-resident scene (opaque): uploaded once, rendered many times. */
typedef struct gs_device_scene gs_device_scene;

const char* gs_last_error(void);
int32_t gs_version(void);

/* Launch tuning, process-wide: shade_batch in [0, 64] = finished lanes a wave
 * collects before it shades them together (0 = the scene's own choice: 52, or 44 for
 * scenes with BVHs under instances; ABI 8); blocks_per_cu in [0, 8], 0 = from the
 * occupancy query; leaf_batch in [0, 64] = lanes waiting at a leaf before the wave
 * runs a leaf-test pass (0 = the scene's own choice: 12, or 48 for scenes with BVHs
 * under instances, whose leaf passes serve one leaf kind each);
 * sample_chunk = samples per work item when the settings run a single batch
 * (max_samples < batch_size, as every fixed-spp render): -1 auto (16, or batch/64 for
 * big batches: at most 64 chunks per pixel, and at most 4 GiB of chunk sums; ABI 7: the
 * launch's last tiles in queue order in the finest chunks, batch/64 or 1, so a frame
 * does not end waiting on a few long items), 0 never split a pixel, n > 0 explicit.
 * Chunks keep every sample's RNG stream; a pixel's chunk sums are added in sample order,
 * so only the association of the f64 colour sum differs from the sequential loop. */
gs_status gs_set_tuning(int32_t shade_batch, int32_t blocks_per_cu, int32_t leaf_batch, int32_t sample_chunk);

/* Node steps per traversal node pass, 1 .. 8 (ABI 4): a node pass lets every lane take
 * up to this many BVH node steps before the wave re-checks which lanes sit at leaves.
 * 0 (default) = the scene's own choice, from its tree's shape at gs_device_scene_create. */
gs_status gs_set_node_steps(int32_t node_steps);

/* Camera-ray batch, process-wide (ABI 9): lanes of a wave that want a camera ray (a new
 * sample's Camera::get_ray, camera.rs:204-221) before the wave generates them together,
 * in [0, 64]; 0 (default) = the scene's own choice.  Waiting lanes idle like finished
 * ones; a wave never waits when none of its lanes has a ray to trace or the work queue
 * is empty.  Every sample's draws and ray are unchanged: only when a lane starts its next
 * sample moves, so frames and counters do not depend on it. */
gs_status gs_set_camera_batch(int32_t cam_batch);

/* Placement of the threaded BVH records (ABI 7).  1 (default): before a scene's first
 * launch, when its records do not all fit the per-block LDS mirror, a pilot renders the
 * launch's camera at 1 spp on a coarse pixel grid counting the tests of every record,
 * and the records are re-placed so the mirror holds the most-tested bytes (the pilot's
 * cost is reported as gs_scene_info.pilot_ms; results never depend on placement).
 * 0: keep the static estimate placed by gs_device_scene_create.  Applies to scenes
 * whose first launch comes after the call.
 * Blocking (ABI 8 note): the launch that runs the pilot waits for it on the host (a
 * stream synchronisation and a copy of the counts) before it issues its own kernels, so
 * that one call of gs_render_tiles*_async is not asynchronous.  A launch of fewer than 16x
 * the pilot's pixel samples (W*H*batch_size < 16 x ~64 k) leaves the pilot to a later,
 * larger launch.  The frame context (gs_multi_render) runs the pilots of all its devices
 * concurrently before its timed render. */
gs_status gs_set_placement(int32_t mode);

/* Diagnostic (ABI 7): one launch like gs_render_tiles_async that also counts, into the
 * device array d_visits (node_records + leaf_records u32, zeroed by the call), the tests
 * of every threaded record by its current position: node records first, then leaf
 * records.  Runs the scene's placement first, like any launch. */
gs_status gs_debug_record_visits(const gs_device_scene* scene, const gs_camera* cam,
                                 const gs_sample_settings* ss, uint64_t seed, const gs_partition* part,
                                 float* d_packed_rgb, uint32_t* d_visits, void* stream);

/* Adaptive settings (ABI 8) -- SampleSettings that run more than one batch
 * (max_samples >= batch_size, camera.rs:135-165).  Batch rounds: round r renders batch r of
 * every pixel still active, its samples spread over the lanes like the fixed-spp chunks,
 * each sample's colour kept; a combine pass then adds each pixel's batch into its running
 * sums in sample order and takes the reference's stop test, so the result is
 * bit-identical to the per-lane loop.  A launch then issues a few small kernels per round
 * on its stream (no host synchronisation).  The per-lane loop: one work item per pixel
 * running all of its batches.  mode 1 (default): rounds when a pixel can take 512 samples
 * or more ((max_samples / batch + 1) x batch: the per-lane loop's tail), else the loop;
 * 2: always rounds; 0: always the loop.  The loop also serves more than 65536 possible
 * batches, a sample chunk of 0 and the diagnostic per-pixel visit output. */
gs_status gs_set_adaptive_mode(int32_t mode);

/* Test hook (ABI 8): the work items of batch rounds.  0 (default): each batch split into
 * sample chunks whose colours a combine pass folds in order.  1: each pixel's batch as one
 * item (from its running sums, the stop test in the lane: no per-sample colours; batches up
 * to 256).  -1: whole-batch items while a round's active pixels are at least twice the
 * device's lanes, split after.  Every choice renders the same bits. */
gs_status gs_debug_set_round_items(int32_t mode);

/* Test hook: scenes uploaded after this call test each Quad::cube list (six consecutive
 * axis-aligned quads in cube order) as straight-line code with the faces' axes fixed at
 * compile time (1, default) or with the generic list loop (0).  Both render the same bits. */
gs_status gs_debug_set_cube_lists(int32_t on);

/* Test hook (additive: the ABI stays 11): scenes uploaded after this call take the certified f32
 * box test where gs_scene_info.cert_boxes allows it (1, default: every node coordinate
 * |x| <= 1e15 decides) or never (0: cert_boxes is 0 whatever the coordinates, so every node
 * step of every launch of the scene takes the reference's f64 box test).  Both render the same
 * bits and counters.  Other values: GS_ERR_ARG.  Host only; callable without a device. */
gs_status gs_debug_set_cert_boxes(int32_t on);

/* Test hook (additive: the ABI stays 11): the byte budget of the per-block LDS mirror for scenes
 * uploaded after this call.  -1 (default): the block's own budget.  bytes >= 0: that many bytes
 * at most, and never more than the block's own budget; the upload's placement and the pilot's
 * re-placement fill it, and gs_scene_info reports the prefixes.  A tree the budget cuts loses
 * feature bit 8 (whole tree in LDS).  Placement never changes a result: every budget renders
 * the same bits and counters.  Values below -1: GS_ERR_ARG.  Host only; callable without a
 * device. */
gs_status gs_debug_set_mirror_budget(int64_t bytes);

/* Test hook (additive: the ABI stays 11): at most this many blocks in a render-kernel launch
 * (0, default: the device's CUs x blocks per CU, and no more lanes than work items).  With
 * fewer lanes than items every lane runs many items in turn.  Scheduling only: every value
 * renders the same bits and counters.  Negative values: GS_ERR_ARG.  Host only; callable
 * without a device. */
gs_status gs_debug_set_max_blocks(int32_t blocks);

/* Test hook: the auto sample-chunk rule's budget for chunk sums (default 4 GiB; 0
 * restores it).  A smaller budget makes renders take the chunk-doubling branch. */
gs_status gs_debug_set_partial_budget(uint64_t bytes);

/* Test hook (ABI 10; ABI 11: fine_chunk 0 or 1 only): the auto sample-chunk rule's guided
 * tail -- how much of the frame runs in 1-sample items, as tail_pct percent of the device's
 * lanes x the coarse chunk in samples (0: the default, 200).  tail_pct > 0 also gives an
 * explicit gs_set_tuning sample_chunk (the coarse chunk) a tail.  The tail is scheduling
 * only: its items' sums are regrouped into the coarse chunks, so every choice renders the
 * same bits.  fine_chunk > 1 is rejected (GS_ERR_ARG). */
gs_status gs_debug_set_guided_tail(int32_t fine_chunk, int32_t tail_pct);

/* Test hook: the kernel feature word (gs_scene_info.feat's bits, plus 128 fixed-spp, 1024 split
 * batch round, 2048 views) that the scene's most recent render-kernel launch selected its
 * instantiation with -- the scene's own choice after the launch's changes (8 cleared when the
 * LDS mirror is a strict prefix; the fixed, round and views forms added).  -1 before any launch.
 * Host only: read after the call that enqueued the launch returned. */
gs_status gs_debug_last_launch_feat(const gs_device_scene* scene, int32_t* feat);

/* Test hook: the scene's device record -- the struct of device pointers (the folded materials,
 * the quads, textures, texels, the HDRI in the form chosen at upload, ...) and the background
 * that every kernel launch of the scene passes by value -- copied into out.  Its layout is
 * internal (csrc/device/kernel_abi.hpp, DevScene): for test kernels compiled from this tree,
 * which run the product's device functions on the records the product built.  out_bytes must
 * equal the record's size (GS_ERR_ARG else; the message states it).  The pointers stay valid
 * until gs_device_scene_destroy.  Host only. */
gs_status gs_debug_device_scene_record(const gs_device_scene* scene, void* out, int64_t out_bytes);

/* Test hook: what the leaf tests read beside the device record -- the device array of the quads'
 * traversal records (n_quads records of 128 bytes, gs_quad order; layout internal: csrc/device/
 * geometry.hpp, TQuad), the number of Quad::cube records (gs_debug_set_cube_lists) and the
 * prefixes of both that the scene's current placement mirrors in LDS.  out_bytes must equal
 * sizeof(gs_debug_leaf_stage) (GS_ERR_ARG else).  The pointer stays valid until
 * gs_device_scene_destroy.  Host only; sets nothing. */
typedef struct gs_debug_leaf_stage {
    const void* tquads;
    uint32_t n_quads, n_cubes;
    uint32_t lds_quads, lds_cubes;
} gs_debug_leaf_stage;
gs_status gs_debug_leaf_stage_record(const gs_device_scene* scene, gs_debug_leaf_stage* out, int64_t out_bytes);

/* Upload a flattened scene to the current HIP device. */
gs_status gs_device_scene_create(const gs_flat_scene* scene, gs_device_scene** out);
gs_status gs_device_scene_destroy(gs_device_scene* scene);

/* What gs_device_scene_create built (ABI 5): the threaded top-level tree, the per-block
 * LDS mirror prefixes (before any launch-time shrinking) and the kernel choices taken
 * from the tree's shape.  nodes_per_leaf: expected node tests per leaf test of a ray
 * that enters the root box (surface-area estimate: a record is tested with probability
 * min over its ancestors' box areas / the root box's area); other_leaf_frac: the share of
 * those leaf tests that are not stationary spheres (quads, triangles, lists, instances,
 * media, moving spheres). */
typedef struct gs_scene_info {
    uint32_t node_records, leaf_records;
    uint32_t lds_nodes, lds_leaves, lds_quads;
    int32_t feat;       /* kernel features: 1 media, 2 nested BVHs, 4 sphere leaf runs, 8 whole tree in LDS,
                           64 every top-level leaf a stationary sphere (ABI 7),
                           16 staged shading (three or more shading cases share its stages) */
    int32_t node_steps; /* node steps per node pass the scene's launches use (see gs_set_node_steps) */
    int32_t cert_boxes; /* every node coordinate |x| <= 1e15: the certified f32 box test applies */
    double nodes_per_leaf;
    double other_leaf_frac;
    int32_t placement;  /* (ABI 7) 0 static estimate, first launch pending; 1 static estimate (final);
                           2 measured by the first launch's pilot (gs_set_placement) */
    int32_t long_samples; /* (ABI 11) 1 once a frame of the frame context measured more than 50 lane-us a
                             sample (gs_multi_render's frame notes; sticky): small frames then take the
                             guided tail's 1-sample items too -- scheduling only, the bits are unchanged */
    double pilot_ms;    /* (ABI 7) host time of that pilot and re-placement */
} gs_scene_info;
gs_status gs_device_scene_info(const gs_device_scene* scene, gs_scene_info* out);

/* What one frame did (SURVEY.md §5 metrics row): filled by gs_render, gs_render_ppm,
 * gs_render_multi and gs_multi_render (ABI 6; before ABI 6 only gs_render_multi, and
 * gs_render / gs_render_ppm took a gs_counters*).  Times are HIP events on the launch
 * streams (device) or the host clock (host). */
typedef struct gs_stats {
    gs_counters counters;       /* work done, summed over devices (exact, = the oracle's) */
    double setup_ms;            /* host: scene uploads, communicator and tile plan of this call (one-shot
                                   calls); gs_multi_render: the tile plan when it was (re)computed, plus
                                   the placement pilots of a scene's first frame (ABI 8), else 0 */
    double total_ms;            /* host: the whole call */
    double render_ms_max;       /* slowest device's render: parameter + megakernel + chunk-combine launches */
    double render_ms_min;       /* fastest device's */
    double gather_ms;           /* first device: RCCL gather (N > 1) + unpack (+ PPM text when asked);
                                   one device without a collective renders into the frame itself:
                                   the PPM text's time, else 0 (ABI 10) */
    uint64_t algorithmic_bytes; /* SURVEY.md §8d bytes of every launch (cache-served, not HBM) */
    uint64_t gathered_bytes;    /* bytes the gather delivered to the first device (0 for one device) */
    int32_t num_gpus;
    int32_t pad;
    double kernel_ms_max;       /* (ABI 6) the megakernel alone, slowest device */
    double kernel_ms_min;       /* (ABI 6) the megakernel alone, fastest device */
} gs_stats;

/* Number of packed pixels (tiles * tile_w * tile_h) this rank renders. */
int64_t gs_partition_capacity(const gs_camera* cam, const gs_partition* part);

/* Render this rank's tiles asynchronously on `stream` (hipStream_t as void*, NULL =
 * default stream).  d_packed_rgb: device buffer of capacity*3 f32, linear colour
 * (pixel_color / sample_count, camera.rs:167) for each packed pixel; padding pixels
 * are written as 0.  d_counters: device gs_counters (nullable), accumulated into. */
gs_status gs_render_tiles_async(const gs_device_scene* scene, const gs_camera* cam,
                                const gs_sample_settings* ss, uint64_t seed,
                                const gs_partition* part, float* d_packed_rgb,
                                gs_counters* d_counters, void* stream);

/* Outputs of one launch, per packed pixel (capacity entries; padding pixels get 0).
 * At least one of rgb / rgb8 must be set. */
typedef struct gs_render_outputs {
    float* rgb;            /* capacity*3 f32, linear colour (camera.rs:167), nullable */
    uint8_t* rgb8;         /* capacity*3 u8, write_color's bytes (color.rs:8-18) of the f64
                              colour (not of the f32 one), nullable */
    uint32_t* item_visits; /* capacity u32, BVH node visits per pixel (diagnostic), nullable */
} gs_render_outputs;

/* gs_render_tiles_async with a choice of outputs (ABI 3). */
gs_status gs_render_tiles_ex_async(const gs_device_scene* scene, const gs_camera* cam,
                                   const gs_sample_settings* ss, uint64_t seed,
                                   const gs_partition* part, const gs_render_outputs* out,
                                   gs_counters* d_counters, void* stream);

/* Diagnostic variant: also writes, per packed pixel, the number of BVH node visits
 * its samples made (d_item_visits: capacity u32, nullable; zeroed by the call). */
gs_status gs_render_tiles_debug_async(const gs_device_scene* scene, const gs_camera* cam,
                                      const gs_sample_settings* ss, uint64_t seed,
                                      const gs_partition* part, float* d_packed_rgb,
                                      gs_counters* d_counters, uint32_t* d_item_visits, void* stream);

/* Scatter the packed buffers of all ranks (world_size * capacity * 3 f32, rank-major,
 * as a gather leaves them) into a W*H*3 frame.  Runs on the current device. */
gs_status gs_unpack_tiles_async(const gs_camera* cam, int32_t world_size, int32_t tile_w,
                                int32_t tile_h, int64_t capacity, const float* d_gathered,
                                float* d_frame, void* stream);

/* As gs_unpack_tiles_async, for the 3-byte rgb8 output (ABI 3). */
gs_status gs_unpack_tiles_u8_async(const gs_camera* cam, int32_t world_size, int32_t tile_w,
                                   int32_t tile_h, int64_t capacity, const uint8_t* d_gathered,
                                   uint8_t* d_frame, void* stream);

/* ---- Output stage on the device (camera.rs:101-103,116-118; color.rs:8-18) (ABI 3) ----
 * The reference writes an ASCII PPM: "P3\n{W} {H}\n255\n", then one "{r} {g} {b}\n"
 * line per pixel in row-major order.  gs_ppm_encode_async formats that text on the
 * device from a W*H*3 byte frame (rgb8 output, unpacked): per-block text lengths, one
 * scan into offsets, then each block formats 2048 pixels in LDS and streams them out.
 * The host writes the result with one write call. */
int64_t gs_ppm_max_bytes(int32_t width, int32_t height);     /* text capacity bound */
int64_t gs_ppm_scratch_bytes(int32_t width, int32_t height); /* device scratch size */
/* d_rgb8: device, W*H*3 bytes, 4-byte aligned; d_text: device, >= gs_ppm_max_bytes,
 * 16-byte aligned (hipMalloc'd buffers are); d_len: device
 * int64, receives the text length; d_scratch: device, >= gs_ppm_scratch_bytes, 8-byte
 * aligned (overwritten; reusable once the stream has passed this call). */
gs_status gs_ppm_encode_async(const uint8_t* d_rgb8, int32_t width, int32_t height, char* d_text,
                              int64_t text_capacity, int64_t* d_len, void* d_scratch,
                              int64_t scratch_bytes, void* stream);

/* Synchronous full render to PPM text on the current device: the whole of
 * Camera::render (camera.rs:100-121) past the world build.  out_text: host buffer of
 * text_capacity >= gs_ppm_max_bytes(W, H) bytes; *out_len receives the length. */
gs_status gs_render_ppm(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss,
                        uint64_t seed, char* out_text, int64_t text_capacity, int64_t* out_len,
                        gs_stats* stats /* nullable (ABI 6: was gs_counters*) */);

/* Cost-balanced partition (ABI 3): a 1-spp pilot render of the whole frame on this
 * device (per-pixel BVH node visits, deterministic, so every rank computes the same
 * plan), then longest-processing-time assignment of tiles to world_size ranks (at
 * most ceil(tiles / world_size) each), each rank's tiles in frame order.  Writes
 * order_out (host, world_size * slots entries, see gs_partition.d_tile_order) and
 * *slots_per_rank; order_cap = entries available (query: order_out NULL, returns the
 * entries needed in *slots_per_rank * world_size via *slots_per_rank).  Synchronous. */
gs_status gs_plan_tiles(const gs_device_scene* scene, const gs_camera* cam, uint64_t seed, int32_t world_size,
                        int32_t tile_w, int32_t tile_h, int32_t* order_out, int64_t order_cap,
                        int32_t* slots_per_rank);

/* Unpack for any partition (incl. d_tile_order): elem_bytes 12 (f32 rgb) or 3 (rgb8). */
gs_status gs_unpack_tiles_part_async(const gs_camera* cam, const gs_partition* part, int64_t capacity,
                                     const void* d_gathered, void* d_frame, int32_t elem_bytes, void* stream);

/* ---- The N-GPU render behind one call (ABI 4) ----
 * The whole pixel loop of camera.rs:105-114 on the GPUs of one node, from one host
 * thread: the scene is uploaded to every device, the frame is cut into tile_w x tile_h
 * tiles (plan = 1: cost-balanced, gs_plan_tiles on the first device; 0: round-robin),
 * each device renders its tiles on its own stream, ONE grouped RCCL gather (ncclGather
 * over xGMI, communicator from ncclCommInitAll, one rank per device) brings the packed
 * tiles to the first device, which unpacks them (and formats the PPM text when asked).
 * The frame equals gs_render's for every device count (per-pixel RNG streams).
 * Synchronous; RCCL is loaded at the first call (GS_ERR_UNSUPPORTED without it). */
typedef struct gs_launch {
    int32_t num_gpus;       /* devices used; 0 = every visible device (devices must then be NULL) */
    int32_t tile_w, tile_h; /* 0 = 64 (tile_h 0 = tile_w) */
    int32_t plan;           /* 1: cost-balanced tiles, 0: round-robin */
    const int32_t* devices; /* nullable: num_gpus distinct HIP device ids (default 0..num_gpus-1) */
} gs_launch;

/* Host outputs of gs_render_multi; any subset, at least one. */
typedef struct gs_multi_outputs {
    float* rgb;           /* W*H*3 f32, linear colour (camera.rs:167), nullable */
    uint8_t* rgb8;        /* W*H*3 write_color bytes of the f64 colour, nullable */
    char* ppm_text;       /* the PPM file Camera::render writes (camera.rs:101-118), nullable */
    int64_t ppm_capacity; /* >= gs_ppm_max_bytes(W, H) when ppm_text is set */
    int64_t* ppm_len;     /* receives the text length when ppm_text is set */
} gs_multi_outputs;

gs_status gs_render_multi(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss,
                          uint64_t seed, const gs_launch* launch, const gs_multi_outputs* out, gs_stats* stats);

/* ---- Persistent N-GPU frame context (ABI 6) ----
 * gs_render_multi is gs_multi_create + one gs_multi_render + gs_multi_destroy.  A caller
 * rendering many frames of one world (an animation, a benchmark) creates the context once:
 * the scene upload to every device, the per-device streams and events and the RCCL
 * communicator (ncclCommInitAll, N > 1 only) happen there, outside every frame.  The tile
 * plan is computed at the first frame of a camera and kept while the camera is unchanged.
 * launch->num_gpus <= 0 means every visible device and then requires devices == NULL.
 * num_gpus == 1 uses no collective: the device unpacks its own tiles.
 * A context is not reentrant: one gs_multi_render at a time (calls are serialised). */
typedef struct gs_multi gs_multi;
gs_status gs_multi_create(const gs_flat_scene* scene, const gs_launch* launch, gs_multi** out);
/* One synchronous frame.  out: host outputs (any subset, at least one), or NULL: the linear
 * f32 frame then stays on the first device (gs_multi_frame), nothing crosses PCIe. */
gs_status gs_multi_render(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                          const gs_multi_outputs* out, gs_stats* stats);
/* The last frame's device buffers on the first device (W*H*3 f32 / u8; NULL if that output
 * was not produced), valid until the next gs_multi_render or gs_multi_destroy. */
gs_status gs_multi_frame(const gs_multi* m, const float** d_rgb, const uint8_t** d_rgb8, int32_t* device);
/* Devices of the context in rank order (devices: num_gpus entries, nullable). */
gs_status gs_multi_devices(const gs_multi* m, int32_t* num_gpus, int32_t* devices, int32_t capacity);
/* The device-resident scene of rank `rank` (e.g. for gs_device_scene_info); owned by the context. */
gs_status gs_multi_scene(const gs_multi* m, int32_t rank, const gs_device_scene** scene);
gs_status gs_multi_destroy(gs_multi* m);
/* Test hook: 1 = contexts created from now on use the RCCL communicator and gather even for
 * one device (so a one-GPU machine runs that code); 0 (default) = no collective for one. */
gs_status gs_debug_set_multi_collective(int32_t always);
/* Test hook (ABI 11): 1 = contexts created from now on accept a device list that repeats a
 * device (launch->devices) and, for N > 1, gather the ranks' packed tiles by device copies on
 * the ranks' streams instead of RCCL -- so a one-GPU machine runs the N-rank frame loop (one
 * scene, stream and event set per rank, the plan, the concurrent launches, the rank-major
 * unpack, the summed counters, per-rank frame notes) with N scenes on one device; 0 (default). */
gs_status gs_debug_set_multi_same_device(int32_t on);

/* ---- Progressive rendering (additive: the ABI stays 11, no existing call changes) ----
 * A fixed-spp frame as a sequence of passes over device-resident f64 sums: render n samples,
 * look at the frame, render n more, checkpoint, resume.
 *
 * The contract: sample s of a pixel draws from stream_seed(seed, pixel, s) whichever launch
 * runs it, and a pixel's sum is ((0 + C_0) + C_1) + ... over chunk sums of `chunk` samples
 * taken in sample order.  A pass continues that sum where the last one stopped, so passes of
 * n_1, n_2, ... samples (each a multiple of `chunk`) leave the sums, the linear f32 frame, the
 * rgb8 frame and the cumulative counters of ONE render of n_1 + n_2 + ... samples with the same
 * seed and chunk, bit for bit -- for any split into passes, any device count or tile plan, and
 * across a checkpoint.  That one render is gs_multi_render / gs_render at a fixed spp whose
 * coarse chunk is `chunk` (e.g. gs_set_tuning(.., sample_chunk = chunk) with spp / chunk <= 64).
 * Here a pass is a sample count; adaptive settings have a pass form of their own, in batch
 * rounds ("Progressive adaptive passes" below).
 *
 * The tile-level primitive, stateless: renders samples [sample_base, sample_base + samples) of
 * this rank's packed pixels, adds them to d_sums (device, capacity*3 f64 in packed order, owned
 * by the caller and zeroed before the first pass) and writes d_sums / (sample_base + samples) to
 * out->rgb / out->rgb8 (padding pixels get 0).  chunk: the coarse chunk c, 0 = 16, taken as
 * given (none of the one-shot render's frame- and size-dependent rules apply); the launch is
 * always chunked.  GS_ERR_ARG, before any device work, when: an argument is NULL (d_counters
 * may be), samples == 0, samples or sample_base is not a multiple of c, samples / c > 64, the
 * pass's chunk sums (capacity * samples / c * 24 bytes) exceed the partial budget (4 GiB), or
 * sample_base + samples overflows 32 bits.  d_counters is accumulated into; the kernel counts
 * `pixels` in every pass, so a caller summing passes takes `pixels` from the first alone. */
gs_status gs_render_tiles_pass_async(const gs_device_scene* scene, const gs_camera* cam, uint32_t samples,
                                     uint64_t seed, const gs_partition* part, uint32_t sample_base,
                                     uint32_t chunk, double* d_sums, const gs_render_outputs* out,
                                     gs_counters* d_counters, void* stream);

/* The frame context's accumulation.  gs_multi_accum_begin fixes the camera, the seed and the
 * chunk (0 = 16), computes the tile plan once and allocates zeroed sums on every rank.  Each
 * gs_multi_accum_pass then renders the next `samples` samples (1 to 64 whole chunks) of every
 * pixel on every rank and delivers the resolved frame like gs_multi_render: `out` as there, NULL
 * leaves the frame on the first device (gs_multi_frame); `stats` describes this pass alone.
 * While an accumulation is open gs_multi_render returns GS_ERR_ARG (its re-plan would
 * invalidate the packed sums); gs_multi_accum_end frees the sums and closes it.  Calls on a
 * context without an open accumulation return GS_ERR_ARG. */
typedef struct gs_accum_info {
    int32_t width, height;
    uint32_t chunk;       /* the coarse chunk c (resolved: never 0) */
    uint32_t passes;      /* passes run since gs_multi_accum_begin / _upload */
    uint64_t seed;
    uint64_t samples;     /* samples per pixel in the sums */
    double last_delta;    /* the last pass's change: the mean over W*H*3 values of |colour after - colour
                             before| (f64 colours; before = 0 for the first pass).  Deterministic: per-block
                             partial sums on a grid set by the rank's capacity alone, added in index and
                             rank order -- the same bits run to run; the last bits depend on the device
                             count (the order of the additions), nothing else does */
    gs_counters counters; /* cumulative; equal to a one-shot render's (`pixels` counted once) */
} gs_accum_info;
gs_status gs_multi_accum_begin(gs_multi* m, const gs_camera* cam, uint64_t seed, uint32_t chunk);
gs_status gs_multi_accum_pass(gs_multi* m, uint32_t samples, const gs_multi_outputs* out, gs_stats* stats);
gs_status gs_multi_accum_info(const gs_multi* m, gs_accum_info* info);
/* Checkpoints: the sums in image order, [H][W][3] f64 (host), so sums saved on N devices resume
 * on M.  gs_multi_accum_upload opens an accumulation like _begin and fills it: `samples` (whole
 * chunks) are in `sums`, `counters` are the cumulative counters saved with them.  Not hot: the
 * tile permutation runs on the host. */
gs_status gs_multi_accum_download(gs_multi* m, double* sums);
gs_status gs_multi_accum_upload(gs_multi* m, const gs_camera* cam, uint64_t seed, uint32_t chunk, uint64_t samples,
                                const double* sums, const gs_counters* counters);
gs_status gs_multi_accum_end(gs_multi* m);

/* ---- Progressive adaptive passes (additive: the ABI stays 11, no existing call changes) ----
 * Adaptive settings (max_samples >= batch_size) in passes of batch rounds.  Write bs =
 * batch_size and R = max_samples / bs + 1, the most batches a pixel can run.  Round r renders
 * batch r (samples [r bs, r bs + bs)) of every pixel still active and folds it into the pixel's
 * Σr, Σg, Σb, Σlum, Σlum² in sample order, then takes the reference's stop test.
 *
 * The contract:
 *  1. Rounds rendered in passes of r_1, r_2, ... rounds until no pixel is active (at the latest
 *     after R rounds) leave the linear f32 frame, the rgb8 bytes and the counters of gs_multi_render
 *     / gs_render with the same settings and seed, bit for bit -- for any split into passes, any
 *     rank count or tile plan, any gs_set_tuning sample chunk or partial budget, and across a
 *     checkpoint.
 *  2. After k rounds (1 <= k < R) a stopped pixel shows its final colour and an active one
 *     Σrgb / (double)(k bs): bit for bit the one-shot frame with max_samples = k bs - 1.  The
 *     cumulative counters equal that render's except `pixels`, which counts the stopped pixels.
 *  3. The maps, per pixel: `samples` (u32) the samples taken so far, a multiple of bs;
 *     `rel_error` (f32) what the stop test compares with `tolerance`, computed in f64, in this
 *     order and without contraction, from the pixel's stored sums and n = its samples:
 *       mean = lsum / n;  var = 1.0 / (n - 1.0) * (lsq - lsum * lsum / n);
 *       rel_error = sqrt(confidence * confidence * var / n / (mean * mean))
 *     A stopped pixel keeps its final sums.  NaN and inf are legal values (batch size 1 gives
 *     0/0 after the first round; a black pixel has mean 0).
 *  4. The state crosses to the host in image order: `sums` [H][W][5] f64 (Σr, Σg, Σb, Σlum, Σlum²)
 *     and `state` [H][W] u32 (batches taken; the top bit once the pixel has stopped), and an
 *     upload of these continues to the same bits on any rank count.
 *
 * The tile-level primitive, stateless: renders rounds [first_round, first_round + rounds) of this
 * rank's packed pixels on the state in d_state, a caller-owned device blob of at least
 * gs_round_state_bytes(cam, part, ss) bytes (-1: bad arguments, or settings with no round form)
 * whose layout is private; first_round == 0 initialises it.  Then every packed pixel's colour is
 * resolved into out->rgb / out->rgb8 (at least one non-NULL; padding pixels get 0) -- stopped
 * pixels too, so a buffer never seen before is filled whole -- and the maps into out->samples /
 * out->rel_error when non-NULL, all indexed per packed pixel.  Round items are always split
 * (gs_debug_set_round_items is ignored).  GS_ERR_ARG, before any device work, when: an
 * argument is NULL (d_counters may be), the partition is bad, rounds == 0, batch_size == 0, the
 * settings run one batch (max_samples < batch_size: see gs_render_tiles_pass_async), R > 65536,
 * first_round + rounds > R, state_bytes is too small, or one pixel's batch (batch_size * 24
 * bytes) exceeds the partial budget.  d_counters is accumulated into; `pixels` counts stops. */
#define GS_ADAPT_STOPPED 0x80000000u /* a `state` word's top bit: the pixel has stopped */
typedef struct gs_round_outputs {
    float* rgb;        /* capacity*3 f32, linear (nullable when rgb8 is set) */
    uint8_t* rgb8;     /* capacity*3 u8, write_color bytes (nullable) */
    uint32_t* samples; /* capacity u32 (nullable) */
    float* rel_error;  /* capacity f32 (nullable) */
} gs_round_outputs;
int64_t gs_round_state_bytes(const gs_camera* cam, const gs_partition* part, const gs_sample_settings* ss);
gs_status gs_render_tiles_rounds_async(const gs_device_scene* scene, const gs_camera* cam,
                                       const gs_sample_settings* ss, uint64_t seed, const gs_partition* part,
                                       uint32_t first_round, uint32_t rounds, void* d_state, int64_t state_bytes,
                                       const gs_round_outputs* out, gs_counters* d_counters, void* stream);

/* The frame context's adaptation.  gs_multi_adapt_begin fixes the camera, the settings and the
 * seed, computes the tile plan once and allocates the round state on every rank.  Each
 * gs_multi_adapt_pass renders the next `rounds` rounds (clipped to what remains) on every rank
 * and delivers the resolved frame like gs_multi_accum_pass; once the adaptation is finished (no
 * pixel active) a pass renders nothing and delivers the same frame again.  While an adaptation
 * is open gs_multi_render and gs_multi_accum_begin return GS_ERR_ARG, and gs_multi_adapt_begin
 * does while an accumulation is open; calls without an open adaptation return GS_ERR_ARG.
 * gs_multi_adapt_end closes it and frees the state (gs_multi_destroy does too). */
typedef struct gs_adapt_info {
    int32_t width, height;
    uint32_t batch;          /* batch_size */
    uint32_t rounds;         /* rounds run so far */
    uint32_t max_rounds;     /* R */
    uint32_t finished;       /* 1: no pixel is active */
    uint64_t seed;
    uint64_t active_pixels;
    uint64_t samples_total;  /* Σ over pixels of the samples taken: equals counters.paths */
    uint64_t samples_max;    /* the most samples any pixel has taken */
    gs_counters counters;    /* cumulative; `pixels` counts the stopped pixels */
} gs_adapt_info;
gs_status gs_multi_adapt_begin(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed);
gs_status gs_multi_adapt_pass(gs_multi* m, uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats);
gs_status gs_multi_adapt_info(const gs_multi* m, gs_adapt_info* info);
/* The maps of contract item 3 as host arrays in image order, [H][W] each; either may be NULL.
 * Before the first pass every value is 0.  Not hot: the tile permutation runs on the host. */
gs_status gs_multi_adapt_maps(gs_multi* m, uint32_t* samples, float* rel_error);
/* Checkpoints (contract item 4).  gs_multi_adapt_upload opens an adaptation like _begin and fills
 * it: `rounds_done` rounds are in `sums` / `state`, `counters` are the cumulative counters saved
 * with them.  GS_ERR_ARG when a pixel's state disagrees with rounds_done. */
gs_status gs_multi_adapt_download(gs_multi* m, double* sums, uint32_t* state);
gs_status gs_multi_adapt_upload(gs_multi* m, const gs_camera* cam, const gs_sample_settings* ss, uint64_t seed,
                                uint32_t rounds_done, const double* sums, const uint32_t* state,
                                const gs_counters* counters);
gs_status gs_multi_adapt_end(gs_multi* m);

/* ---- Views: a batch of cameras in one launch (additive: the ABI stays 11, no existing call changes) ----
 * V cameras of one device-resident scene at a fixed number of samples per pixel, all of the same
 * width W and height H: turntables, camera paths, stereo pairs, the faces of an environment probe.
 * The batch runs as one tall frame of W x (V H) pixels, view v in rows [v H, (v + 1) H): one
 * parameter upload, one megakernel launch, one queue drain and one resolve for all of them.
 *
 * The contract: view v's linear f32 frame and rgb8 frame are, bit for bit, what a one-shot
 * fixed-spp render of views[v].cam gives with seed views[v].seed and the same coarse chunk
 * (gs_render / gs_multi_render; gs_render_tiles_pass_async at sample_base 0), and the call's
 * counters are the exact sums of those V renders' counters.  The number of views in the call,
 * their order, the other cameras in the batch, the rank count, the tile size and the guided tail
 * move no bit: sample s of pixel p of a view draws from stream_seed(seed, p, s) with p the pixel's
 * index in its own W x H frame, and a pixel's sum is ((0 + C_0) + C_1) + ... over chunk sums of
 * `chunk` samples -- everything else is scheduling.  Views may differ in every camera field but
 * the size: lanes of one wave may hold different views, with and without defocus, of different
 * max_depth.
 *
 * These calls are fixed spp, without PPM text (progressive passes over views, view by view, are
 * "Progressive views" below; a batch under adaptive settings is "Adaptive views").  A scene that
 * needs the catch-all kernel (compositions beyond the reference scenes': gs_scene_info.feat & 512)
 * returns GS_ERR_UNSUPPORTED: that kernel has no views form.
 *
 * Argument checks, all before any device work, each GS_ERR_ARG with a gs_last_error message: a
 * NULL pointer (d_counters / stats may be), n_views == 0, views that differ in width or height,
 * any max_depth == 0, samples == 0 or not a multiple of c, samples / c > 64, V W H or the item
 * count not fitting 32 bits, chunk sums (capacity * samples / c * 24 bytes) over the partial
 * budget (4 GiB).  Where the scene's placement pilot has not run yet it runs with view 0's camera;
 * it never changes a result. */
typedef struct gs_view {
    gs_camera cam;
    uint64_t seed;
} gs_view;

/* The tile-level primitive, stateless, the sibling of gs_render_tiles_pass_async: renders this
 * rank's tiles of the tall frame into packed device buffers (out->rgb / out->rgb8, at least one;
 * padding pixels get 0; out->item_visits must be NULL).  `part` cuts the tall frame:
 * gs_partition_capacity on a camera with image_height = V H gives the capacity, and
 * gs_unpack_tiles_part_async with that camera scatters the ranks' buffers into [V][H][W][3].
 * views: host array, read before the call returns.  chunk: the coarse chunk c, 0 = 16, taken as
 * given (gs_views_chunk gives a one-shot render's); the launch is always chunked.  d_counters is
 * accumulated into. */
gs_status gs_render_tiles_views_async(const gs_device_scene* scene, const gs_view* views, uint32_t n_views,
                                      uint32_t samples, uint32_t chunk, const gs_partition* part,
                                      const gs_render_outputs* out, gs_counters* d_counters, void* stream);

/* One synchronous batch on the frame context, like gs_multi_render: out->rgb / out->rgb8 are
 * [V][H][W][3] (ppm_text must be NULL), NULL `out` leaves the frames on the first device
 * (gs_multi_frame: a W x (V H) frame).  Tiles are assigned round-robin whatever the context's
 * `plan` setting: the cost pilot behind a plan is a one-camera notion.  GS_ERR_ARG while an
 * accumulation or adaptation is open, as gs_multi_render. */
gs_status gs_multi_render_views(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t samples,
                                uint32_t chunk, const gs_multi_outputs* out, gs_stats* stats);

/* The coarse chunk a one-shot fixed-spp render (gs_render / gs_multi_render at `samples` spp,
 * under the process's knobs as they stand) of one view's W x H frame takes -- of that frame, not
 * of the tall one: the small-frame rule makes c depend on the frame size.  A views call with
 * this chunk equals plain renders of each camera (a render that does not split its pixels sums
 * them as one chunk of `samples`).  scene NULL: the rule for a scene whose samples are alike (no
 * media, no BVHs under instances, no staged shading: feat & 19 == 0).  0: bad arguments.  A chunk that does not divide `samples` is
 * the one-shot render's all the same, but a views call refuses it. */
uint32_t gs_views_chunk(const gs_device_scene* scene, const gs_camera* cam, uint32_t samples);

/* ---- Progressive views (additive: the ABI stays 11, no existing call changes) ----
 * A batch of views accumulated in passes, view by view: V views (all W x H) of one device-resident
 * scene, the coarse chunk c taken as given (0 = 16).  A pass renders n samples (1 to 64 whole
 * chunks) of a SUBSET of the views.  After any sequence of passes in which view v received n_v
 * samples in total:
 *  1. Frames.  View v's f64 sums, f32 frame and rgb8 frame are, bit for bit, those of a one-shot
 *     fixed-spp render of views[v].cam with seed views[v].seed, n_v samples and chunk c
 *     (gs_multi_render_views with that one view; gs_multi_accum_* on that camera) -- for any split
 *     into passes, any subset history, any other cameras in the batch, any rank count, any tile
 *     size, and across a checkpoint.  Why: sample s of pixel p of a view draws from
 *     stream_seed(seed, p, s) whichever launch runs it, and the pixel's sum is ((0 + C_0) + C_1)
 *     + ... over chunk sums of c samples in sample order; a pass continues that sum at chunk n_v / c.
 *  2. Counters.  The cumulative counters are the exact sums of those V renders' counters, `pixels`
 *     counted once per view: no sample of an unselected view is ever traced, and a view with
 *     n_v = 0 contributes nothing and resolves to 0.
 *  3. Outputs.  A pass writes all V frames ([V][H][W][3]); an unselected view is resolved again
 *     from its stored sums as sum / (double)n_v, so a fresh output buffer may be handed in at any
 *     pass.
 *  4. Per-view change.  delta[v] is the mean over the view's W H 3 values of |colour after -
 *     colour before| in f64 (before = 0 at n_v = 0) of the last pass that selected v; an unselected
 *     view keeps its value.  Deterministic run to run: each tile slot of a rank gives one partial
 *     (each thread adds its pixels' terms in pixel order, the block folds them in a fixed tree),
 *     and the host adds a view's partials rank after rank, each rank's in slot order -- no float
 *     atomics.  Its last bits may depend on the rank count and the tile size; nothing else of a
 *     pass does.
 *
 * Tiles never straddle a view: the tile height must divide H.  gs_views_tile_h(H, tile_h) is the
 * largest divisor of H that is <= tile_h (225, 64 -> 45; 1080, 64 -> 60; 24, 16 -> 12; 64, 64 -> 64;
 * 719, 64 -> 1: a prime H gives W x 1 tiles, which is allowed, if not fast); 0 for bad arguments.
 * By the views contract the tile size moves no bit of a frame.
 *
 * The tile-level primitive, stateless, the sibling of gs_render_tiles_pass_async and
 * gs_render_tiles_views_async: renders samples [b, b + samples) of the selected views' pixels
 * among this rank's tiles of the tall frame, b being the selected views' common view_samples
 * value (the launch's one sample base), adds them to d_sums (device, capacity * 3 f64 in packed
 * order, owned by the caller, zeroed before the first pass), and resolves EVERY packed pixel into
 * out->rgb / out->rgb8.  view_samples: host, V counts, the samples each view's sums hold before
 * the pass.  selected: host, V bytes (non-zero: render the view), NULL = every view.  The
 * megakernel runs on a tile order of its own in which the unselected views' tiles are empty
 * slots (their pixels retire without a camera ray) and every selected tile keeps the slot it has
 * in `part`, so the packed sums never move; part->d_tile_order may therefore be any order of the
 * tall frame's tiles.  d_delta_partials (device, nullable): capacity / (tile_w tile_h) doubles,
 * one per tile slot, the sum of |colour after - colour before| over the slot's real pixels and
 * channels (0 for a slot that is empty or of an unselected view).  d_counters is accumulated
 * into; the kernel counts `pixels` for the selected views in every pass, so a caller summing
 * passes takes `pixels` from a view's first pass alone.
 * GS_ERR_ARG, before any device work and with a gs_last_error message: the views call's rules
 * (NULL pointers, 0 views, views that differ in size, max_depth 0, samples not whole chunks or more
 * than 64 chunks, the 32-bit limits, the partial budget), a NULL d_sums or view_samples, a
 * view_samples value that is not whole chunks, an empty selection, selected views that hold
 * different counts, a count that would pass 2^32, a tile_h that does not divide H.  A scene that
 * needs the catch-all kernel: GS_ERR_UNSUPPORTED. */
int32_t gs_views_tile_h(int32_t height, int32_t tile_h);
gs_status gs_render_tiles_views_pass_async(const gs_device_scene* scene, const gs_view* views, uint32_t n_views,
                                           const uint32_t* view_samples, const uint8_t* selected, uint32_t samples,
                                           uint32_t chunk, const gs_partition* part, double* d_sums,
                                           const gs_render_outputs* out, double* d_delta_partials,
                                           gs_counters* d_counters, void* stream);

/* The frame context's views accumulation.  gs_multi_views_accum_begin fixes the views and the
 * chunk, cuts the tall frame round-robin into tile_w x gs_views_tile_h(H, tile_h) tiles and
 * allocates zeroed sums on every rank.  Each gs_multi_views_accum_pass renders the next `samples`
 * samples of the selected views (selected: V bytes, NULL = all; they must all hold the same count,
 * else GS_ERR_ARG -- a caller with uneven counts runs one pass per count) and delivers all V
 * frames like gs_multi_render_views: out->rgb / out->rgb8 are [V][H][W][3] (ppm_text must be NULL),
 * NULL `out` leaves them on the first device (gs_multi_frame); `stats` describes this pass alone.
 * While it is open gs_multi_render, gs_multi_render_views, gs_multi_accum_begin and
 * gs_multi_adapt_begin return GS_ERR_ARG, and gs_multi_views_accum_begin does while an
 * accumulation or adaptation is open; calls without an open views accumulation return GS_ERR_ARG.
 * gs_multi_views_accum_end closes it and frees the sums (gs_multi_destroy does too). */
typedef struct gs_views_accum_info {
    int32_t width, height;  /* of one view */
    uint32_t n_views;
    uint32_t chunk;         /* the coarse chunk c (resolved: never 0) */
    uint32_t passes;        /* passes run since _begin / _upload */
    int32_t tile_h;         /* gs_views_tile_h(height, the context's tile height) */
    gs_counters counters;   /* cumulative; the sum of the V one-shot renders' (`pixels` once per view) */
} gs_views_accum_info;
gs_status gs_multi_views_accum_begin(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t chunk);
gs_status gs_multi_views_accum_pass(gs_multi* m, uint32_t samples, const uint8_t* selected,
                                    const gs_multi_outputs* out, gs_stats* stats);
/* view_samples_out (V u32) and delta_out (V f64) may be NULL. */
gs_status gs_multi_views_accum_info(const gs_multi* m, gs_views_accum_info* info, uint32_t* view_samples_out,
                                    double* delta_out);
/* Checkpoints: the sums in image order, [V][H][W][3] f64 (host), so sums saved on N ranks resume on
 * M.  gs_multi_views_accum_upload opens a views accumulation like _begin and fills it: view v's
 * sums hold view_samples[v] samples (whole chunks), `counters` are the cumulative counters saved
 * with them.  The deltas start at 0.  Not hot: the tile permutation runs on the host. */
gs_status gs_multi_views_accum_download(gs_multi* m, double* sums);
gs_status gs_multi_views_accum_upload(gs_multi* m, const gs_view* views, uint32_t n_views, uint32_t chunk,
                                      const uint32_t* view_samples, const double* sums, const gs_counters* counters);
gs_status gs_multi_views_accum_end(gs_multi* m);

/* ---- Adaptive views (additive: the ABI stays 11, no existing call changes) ----
 * A batch of views under adaptive settings: V views (all W x H) of one device-resident scene and
 * ONE gs_sample_settings (max_samples >= batch_size) for the batch, run in batch rounds ("Progressive
 * adaptive passes" above: bs, R, the round state) on the tall frame W x (V H), view v in rows
 * [v H, (v + 1) H).  A round's active list holds the surviving pixels of every view, so a round is
 * one parameter kernel, one megakernel and one fold for the whole batch, and a wave of a late round
 * may hold pixels of several views.
 *
 * The contract:
 *  1. Rounds rendered in passes of r_1, r_2, ... rounds until no pixel of any view is active (at
 *     the latest after R rounds) leave, for every view v, the linear f32 frame, the rgb8 bytes, the
 *     `samples` map and the `rel_error` map of a one-shot adaptive render of views[v].cam with seed
 *     views[v].seed and the same settings (gs_render / gs_multi_adapt_* run to the end), bit for
 *     bit, and cumulative counters that are the exact sums of those V renders' counters.  The number
 *     of views, their order, the other cameras in the batch, the split into passes, the rank count,
 *     the tile size, gs_set_tuning's sample chunk, the partial budget (the segment count) and a
 *     checkpoint move no bit: sample s of pixel p of a view draws from stream_seed(seed, p, s) with p
 *     the pixel's index in its own W x H frame, the fold adds a pixel's samples in sample order, and
 *     the stop test reads that pixel's sums alone -- everything else is scheduling.
 *  2. After k rounds every view shows what gs_multi_adapt_* shows for it after k rounds (item 2 of
 *     that contract), `pixels` counting the stopped pixels of all views.
 *  3. Maps and state cross to the host in image order, view after view: `samples` and `rel_error`
 *     [V][H][W], `sums` [V][H][W][5] f64 and `state` [V][H][W] u32 (GS_ADAPT_STOPPED), and an upload
 *     of these continues to the same bits on any rank count.
 *
 * Tiles never straddle a view (the tile height is gs_views_tile_h(H, tile_h)) and are assigned
 * round-robin, as in gs_multi_render_views.  A scene that needs the catch-all kernel
 * (gs_scene_info.feat & 512) returns GS_ERR_UNSUPPORTED: that kernel has no views form.  The
 * rounds run on instantiations of their own: the fixed kernel's sample loop over the round's split
 * items where the scene has neither media nor BVHs under instances, else the loop's kernel with
 * per-sample items.  A library built with GS_USE_RSPLIT 0 (an A/B switch) has only the second
 * kind, and returns GS_ERR_UNSUPPORTED for scenes of the first.
 *
 * Out of scope: per-view settings (one gs_sample_settings per batch: the rounds share one batch
 * size and one R); per-pass view selection (every active pixel of every view takes every round);
 * a views form of the catch-all kernel; cost-planned tiles for batches (the cost pilot is a
 * one-camera notion); PPM text over views.
 *
 * The tile-level primitive, stateless, the sibling of gs_render_tiles_rounds_async: renders rounds
 * [first_round, first_round + rounds) of this rank's packed pixels of the tall frame on the state
 * in d_state, at least gs_round_state_bytes(tall camera, part, ss) bytes (the tall camera: view 0's
 * with image_height = V H); first_round == 0 initialises it.  Outputs as there, per packed pixel.
 * views: host array, read before the call returns.  GS_ERR_ARG, before any device work and with a
 * gs_last_error message: the views rules (a NULL pointer -- d_counters may be --, n_views == 0,
 * views that differ in width or height, any max_depth == 0, V W H not fitting 32 bits, a tile_h that
 * does not divide H) and the adaptation rules (rounds == 0, batch_size == 0, max_samples <
 * batch_size, R > 65536, first_round + rounds > R, state_bytes too small, one pixel's batch over
 * the partial budget).  Where the scene's placement pilot has not run yet it runs with view 0's
 * camera; it never changes a result. */
gs_status gs_render_tiles_views_rounds_async(const gs_device_scene* scene, const gs_view* views, uint32_t n_views,
                                             const gs_sample_settings* ss, const gs_partition* part,
                                             uint32_t first_round, uint32_t rounds, void* d_state, int64_t state_bytes,
                                             const gs_round_outputs* out, gs_counters* d_counters, void* stream);

/* The frame context's views adaptation: gs_multi_adapt_* on the tall frame.  _begin fixes the views
 * and the settings, cuts the tall frame round-robin into tile_w x gs_views_tile_h(H, tile_h) tiles
 * and allocates the round state on every rank.  Each _pass renders the next `rounds` rounds (clipped
 * to what remains; none once no pixel is active) and delivers all V frames like
 * gs_multi_render_views: out->rgb / out->rgb8 are [V][H][W][3] (ppm_text must be NULL), NULL `out`
 * leaves them on the first device (gs_multi_frame).  While it is open gs_multi_render,
 * gs_multi_render_views and the three other _begin calls return GS_ERR_ARG, and
 * gs_multi_views_adapt_begin does while an accumulation, an adaptation or a views accumulation is
 * open; the gs_multi_adapt_* calls do not see it, and calls without an open views adaptation return
 * GS_ERR_ARG.  _end closes it and frees the state (gs_multi_destroy does too). */
typedef struct gs_views_adapt_info {
    int32_t width, height;   /* of one view */
    uint32_t n_views;
    int32_t tile_h;          /* gs_views_tile_h(height, the context's tile height) */
    uint32_t batch;          /* batch_size */
    uint32_t rounds;         /* rounds run so far */
    uint32_t max_rounds;     /* R */
    uint32_t finished;       /* 1: no pixel of any view is active */
    uint64_t active_pixels;  /* over all views */
    uint64_t samples_total;  /* Σ over all pixels of the samples taken: equals counters.paths */
    uint64_t samples_max;    /* the most samples any pixel has taken */
    gs_counters counters;    /* cumulative; `pixels` counts the stopped pixels */
} gs_views_adapt_info;
gs_status gs_multi_views_adapt_begin(gs_multi* m, const gs_view* views, uint32_t n_views,
                                     const gs_sample_settings* ss);
gs_status gs_multi_views_adapt_pass(gs_multi* m, uint32_t rounds, const gs_multi_outputs* out, gs_stats* stats);
/* view_active_out (V u64, nullable): the active pixels of each view, counted on the host from the
 * downloaded state words -- not hot. */
gs_status gs_multi_views_adapt_info(gs_multi* m, gs_views_adapt_info* info, uint64_t* view_active_out);
/* The maps as [V][H][W] host arrays; either may be NULL.  Before the first pass every value is 0. */
gs_status gs_multi_views_adapt_maps(gs_multi* m, uint32_t* samples, float* rel_error);
/* Checkpoints: `sums` [V][H][W][5] f64, `state` [V][H][W] u32.  _upload opens a views adaptation
 * like _begin and fills it; GS_ERR_ARG when a pixel's state disagrees with rounds_done. */
gs_status gs_multi_views_adapt_download(gs_multi* m, double* sums, uint32_t* state);
gs_status gs_multi_views_adapt_upload(gs_multi* m, const gs_view* views, uint32_t n_views,
                                      const gs_sample_settings* ss, uint32_t rounds_done, const double* sums,
                                      const uint32_t* state, const gs_counters* counters);
gs_status gs_multi_views_adapt_end(gs_multi* m);

/* Path of the RCCL library gs_render_multi uses (loaded on this call), or NULL. */
const char* gs_rccl_library(void);

/* Device memory helpers for callers without their own allocator (ctypes, FFI). */
gs_status gs_device_alloc(int64_t bytes, void** d_out);
gs_status gs_device_free(void* d_ptr);
gs_status gs_device_upload(void* d_dst, const void* host_src, int64_t bytes);
gs_status gs_device_download(void* host_dst, const void* d_src, int64_t bytes); /* (ABI 6) synchronous */

/* ---- BVHNode::from_list on the device (additive, ABI 11) ----
 * The reference's tree (BVH.rs:15-65) draws no random axis: the box is the left fold of the
 * members' boxes in their current order, the axis is longest_axis(), the sort is stable on
 * bbox[axis].min and the split is at len / 2.  The shape is therefore a function of n alone --
 * nodes(n) = 1 if n <= 2 else 1 + nodes(n / 2) + nodes(n - n / 2) -- and the device builds the
 * host's tree bit for bit (gs_host_bvh_build is the yardstick).
 *
 * d_boxes: n member boxes, double[n][6] (min xyz, max xyz) in list order.  d_refs (nullable):
 * the tagged ref written where member i becomes a leaf; NULL writes GS_REF_BUILD_MEMBER | i.
 * d_nodes: gs_bvh_node_count(n) nodes in the host flattener's pre-order (the left subtree
 * follows its parent, the right child of a node of m members sits at idx + 1 + nodes(m / 2));
 * child refs are GS_REF_NODE | (node_base + idx); pads are zero.  d_order: the member at each
 * leaf position, left to right.  d_work: gs_bvh_build_work_bytes(n) bytes, 256-byte aligned.
 *
 * The call enqueues a fixed sequence of launches (a function of n) on the stream and returns;
 * nothing is read back between levels and no kernel waits on another block.  A segment of at
 * most gs_bvh_build_lds_members() members is finished by one workgroup in LDS.  GS_ERR_ARG,
 * before any device work: a NULL pointer (d_refs may be), n == 0, n or node_base + nodes(n) past
 * 28 bits, work_bytes too small.  A NaN bound (the host throws) is found on the device:
 * gs_bvh_build_status waits for the stream and returns GS_ERR_ARG with a message; the outputs
 * of such a build must not be used. */
int64_t gs_bvh_node_count(uint32_t n); /* nodes(n); -1 for n == 0 */
int32_t gs_bvh_depth(uint32_t n);      /* levels of that tree (0 for n == 0) */
int64_t gs_bvh_build_work_bytes(uint32_t n); /* a function of n alone; -1 for n == 0 */
uint32_t gs_bvh_build_lds_members(void);
gs_status gs_bvh_build_async(const double* d_boxes, const uint32_t* d_refs /* nullable */, uint32_t n,
                             uint32_t node_base, gs_node* d_nodes, uint32_t* d_order, void* d_work,
                             int64_t work_bytes, void* stream);
gs_status gs_bvh_build_status(void* d_work, void* stream); /* synchronises; GS_ERR_ARG on NaN */

/* ---- Ray queries: world.hit(ray, Interval, rec) for caller rays (additive, ABI 11) ----
 * What the reference answers with `world.hit(&ray, Interval::new(tmin, tmax), &mut rec)`
 * (hittable.rs; BVH.rs:69-90 for the scene's tree), for a batch of rays in one launch of a kernel
 * of its own: the same records in the same left-first order with the same open intervals, the
 * triangle that ignores ray_t, and a ConstantMedium's draw taken inside the traversal.  Ray i's
 * stream starts at stream_seed(seed, i, 0) and `state` is the stream after the walk,
 * hit or miss.  GS_QUERY_CLOSEST walks to the end; GS_QUERY_ANY leaves at the first accepted hit
 * (the same walk, draws and all, up to there), so its `hit` equals the closest query's.
 *
 * A hit: t, and HitRecord's fields at t -- p, n (against the ray), front, material (the flat
 * scene's index), u, v -- with ref (the primitive or medium) and inst (the Translate / RotateY
 * chain it was reached through, or GS_REF_NONE).  A miss: hit = 0, t = the tmax given, material =
 * ref = inst = GS_REF_NONE, p, n, u, v all +0.0.  counts (nullable): the ray's own tests, uint32
 * [n][8]: node visits, then sphere, moving-sphere, quad, triangle, instance, list and medium tests.
 *
 * Any ray bits are accepted (NaN, infinities, a zero direction, tmin > tmax): the answer is what
 * the reference's arithmetic makes of them, and the walk ends after at most one visit per record.
 * GS_ERR_ARG, before anything touches the device: a NULL scene, rays or hits; n < 0 or n >= 2^31;
 * a mode other than the two.  n == 0 is GS_OK with no launch.  The async form takes device
 * pointers and enqueues one launch on `stream`; it shares no buffer with the scene's renders and
 * may overlap them on other streams.  The synchronous form takes host arrays. */
typedef struct gs_ray {
    double o[3], d[3];
    double time, tmin, tmax;
} gs_ray; /* 72 B */
typedef struct gs_ray_hit {
    double t, p[3], n[3], u, v;
    uint32_t hit, front, material, ref, inst, pad;
    uint64_t state;
} gs_ray_hit; /* 104 B */
#define GS_QUERY_CLOSEST 0
#define GS_QUERY_ANY 1
gs_status gs_query_rays_async(const gs_device_scene* scene, const gs_ray* d_rays, int64_t n, int32_t mode,
                              uint64_t seed, gs_ray_hit* d_hits, uint32_t* d_counts /* nullable */, void* stream);
gs_status gs_query_rays(const gs_device_scene* scene, const gs_ray* rays, int64_t n, int32_t mode, uint64_t seed,
                        gs_ray_hit* hits, uint32_t* counts /* nullable */);

/* ---- Radiance queries: ray_color(ray, depth, world) for caller rays (additive, ABI 11) ----
 * What the reference answers with `Camera::ray_color(&ray, max_depth, world)` (camera.rs:174-202),
 * for a batch of rays and `samples` samples of each, in a kernel of its own: the other half of the
 * per-pixel path, for any camera (panoramas, fisheye, orthographic, a measured lens), for baking
 * and probes, and for replaying one pixel's path.  Sample s of ray i is ray_color(Ray(o, d, time),
 * max_depth, world) with its stream started at stream_seed(seed, i, s) or, when
 * d_states is given, at d_states[i * samples + s] -- a stream carried over from a closest query's
 * `state`, or from the caller's own ray generator.  Every segment is tested over Interval(0.001,
 * f64::MAX), as camera.rs:177 does: gs_ray.tmin and gs_ray.tmax are NOT read, so one ray buffer
 * serves both kinds of query.  max_depth == 0 traces no ray: rgb = +0.0, rays = 0, state = the last
 * sample's start state.
 *
 * A sample's colour takes the forward form: T = (1 a1) a2 ..., and a path
 * that ends does so with T c -- c the sky's colour, the emitted colour, or 0 for an absorbed ray; a
 * path that runs out of depth is black.  A ray's samples are cut into chunks of `chunk` consecutive
 * samples (0: 16; the last may be short) and rgb = ((0 + C_0) + C_1) + ... with each C_k = ((0 + s)
 * + s) + ... in sample order: the render's association, so the bits are a function of (ray, seed or
 * states, samples, chunk, max_depth, scene) alone -- not of the batch's size, the ray's place in it
 * or the scheduling.
 *
 * d_counters (nullable, accumulated into): the batch's totals in a render's meaning -- rays, the
 * seven test counters, medium_tests, hits, image_texels, hdri_texels, noise_evals; paths receives
 * n * samples; pixels is left alone.
 *
 * GS_ERR_ARG, before anything touches the device: a NULL scene, rays or out; n < 0; samples == 0;
 * n * ceil(samples / chunk) >= 2^31; with more than one chunk per ray, a d_scratch that is NULL or
 * smaller than gs_query_radiance_scratch_bytes (which is 0 for one chunk per ray: d_scratch may
 * then be NULL); then a scene on another device.  n == 0 is GS_OK with no launch.  Any ray bits are
 * accepted, as in gs_query_rays: the depth bound and the forward-only links end every path.  The
 * async form takes device pointers and enqueues its launches on `stream`; d_scratch (256-byte
 * alignment is not needed, 8 is) belongs to the call until they have run.  The synchronous form
 * takes host arrays, allocates its own scratch and adds the totals to a host gs_counters. */
typedef struct gs_ray_radiance {
    double rgb[3];  /* the SUM over the ray's samples of ray_color, f64 (divide by samples for the mean) */
    uint64_t rays;  /* world.hit calls of all its samples (camera.rs:177) */
    uint64_t state; /* the stream after the last sample's path */
} gs_ray_radiance; /* 40 B */
int64_t gs_query_radiance_scratch_bytes(int64_t n, uint32_t samples, uint32_t chunk); /* -1: bad arguments */
/* Test hook: the lanes of a wave that wait at the end of their walk before the wave shades them together,
 * 1 .. 64 (0: the default, 24; others GS_ERR_ARG).  Process-wide.  Scheduling only: every choice returns
 * the same bits. */
gs_status gs_debug_set_radiance_batch(int32_t shade_batch);
gs_status gs_query_radiance_async(const gs_device_scene* scene, const gs_ray* d_rays, int64_t n, uint32_t samples,
                                  uint32_t chunk, uint32_t max_depth, uint64_t seed,
                                  const uint64_t* d_states /* nullable */, gs_ray_radiance* d_out,
                                  gs_counters* d_counters /* nullable */, void* d_scratch, int64_t scratch_bytes,
                                  void* stream);
gs_status gs_query_radiance(const gs_device_scene* scene, const gs_ray* rays, int64_t n, uint32_t samples,
                            uint32_t chunk, uint32_t max_depth, uint64_t seed, const uint64_t* states /* nullable */,
                            gs_ray_radiance* out, gs_counters* counters /* nullable */);

/* ---- Radiance queries with device ray generators (additive, ABI 11) ----
 * gs_query_radiance traces the same ray for every sample of an item.  The reference's Camera::sample
 * (camera.rs:138-141) draws the ray of every sample from the sample's own stream before it calls
 * ray_color, and so do these entries: jitter inside the pixel, a point on the defocus disk, a time,
 * a cosine-weighted direction over a texel's hemisphere -- made on the device at the start of each
 * sample, with nothing uploaded per sample.
 *
 * Items: n = width * height, row-major -- item q is row j = q / width, column i = q % width.
 * GS_GEN_CAMERA takes both dimensions from gen->cam (gen->width and gen->height are not read);
 * GS_GEN_HEMISPHERE has height = 1 and width = n points.  Sample s of item q draws from
 * stream_seed(seed, q, first_sample + s), the render's (pixel, sample) stream, in this order (wy =
 * one f64 draw; every sum and product as written, left to right):
 *   GS_GEN_CAMERA      Camera::get_ray (camera.rs:204-221): offx = wy - 0.5, offy = wy - 0.5; si =
 *                      (double)i + offx, sj = (double)j + offy; ps = (starting_pixel_pos +
 *                      pixel_delta_u * si) + pixel_delta_v * sj; the origin is `center`, or with
 *                      defocus_angle > 0: draw dx = wy * 2 - 1, dy = wy * 2 - 1 until dx dx + dy dy
 *                      < 1, origin = (center + defocus_disk_u * dx) + defocus_disk_v * dy; d = ps -
 *                      origin; time = wy, the last draw.
 *   GS_GEN_PANORAMA    offx, offy, si, sj as above; theta = ((si + 0.5) / width - 0.5) * (2 pi),
 *                      phi = (0.5 - (sj + 0.5) / height) * pi, dl = unit((cos phi cos theta, cos phi
 *                      sin theta, sin phi)); d = (axis[0] * dl.x + axis[1] * dl.y) + axis[2] * dl.z,
 *                      o = origin; time = wy.  Identity axes, no jitter: query.panorama_rays.
 *   GS_GEN_ORTHO       offx, offy, si, sj as above; o = (origin + axis[0] * ((si + 0.5) / width)) +
 *                      axis[1] * ((sj + 0.5) / height) (axis[0], axis[1]: the rectangle's edges), d =
 *                      axis[2] as given; time = wy.  No jitter: query.ortho_rays.
 *   GS_GEN_HEMISPHERE  p = d_points[q].o, nrm = d_points[q].d, time = d_points[q].time (tmin, tmax:
 *                      not read); OrthonormalBasis::new(nrm) (ONB.rs:10-23); r1 = wy, r2 = wy and
 *                      random_cosine_direction (util.rs:48-60, its r2^(1/4) kept) as (x, y, z); o =
 *                      p, d = unit(u * x + v * y + w * z): Lambertian::scatter's direction
 *                      (material.rs:52-53).  No time draw.
 * Then ray_color(Ray(o, d, time), max_depth, world) goes on from the stream the generator left.
 * Any bits are accepted in gen and the points, as everywhere in the queries.
 *
 * d_out[q]: the gs_ray_radiance of gs_query_radiance -- the f64 sum in chunks of `chunk` (0: 16) in
 * sample order, the world.hit calls, the stream after the last sample.  max_depth == 0 draws nothing
 * and traces nothing: rgb = +0.0, rays = 0, state = the last sample's start state, and nothing is
 * written to d_rays_out / d_states_out.  Otherwise d_rays_out[q * samples + s] (nullable) receives
 * the generated ray, with tmin = 0.001 and tmax = f64::MAX, and d_states_out[q * samples + s]
 * (nullable) the stream right after the generation: gs_query_radiance's d_states indexing, so at
 * samples = 1 over n * samples rays the pair gives the same paths.  d_counters: as gs_query_radiance.
 * A progressive caller adds calls over [first_sample, first_sample + samples) ranges.
 *
 * GS_ERR_ARG, before anything touches the device: a NULL scene, gen or out; a kind outside the
 * four; a dimension below 1; GS_GEN_HEMISPHERE without points (points given with another kind are
 * ignored); samples == 0; first_sample + samples > 2^32; n * ceil(samples / chunk) >= 2^31; a
 * scratch that is NULL or smaller than gs_query_radiance_scratch_bytes(n, samples, chunk) where that
 * is not 0; then a scene on another device.  Concurrency is the radiance queries'.  The synchronous
 * form takes host arrays (rays_out, states_out: n * samples each; GS_ERR_ARG when that many gs_ray
 * exceed half the address space) and allocates its own scratch. */
#define GS_GEN_CAMERA 0
#define GS_GEN_PANORAMA 1
#define GS_GEN_ORTHO 2
#define GS_GEN_HEMISPHERE 3
typedef struct gs_raygen {
    int32_t kind, width, height, pad;
    gs_camera cam;     /* GS_GEN_CAMERA */
    double origin[3];  /* PANORAMA: the eye; ORTHO: the rectangle's corner */
    double axis[3][3]; /* PANORAMA: the frame's x, y, z (z up); ORTHO: edge_u, edge_v, the direction */
} gs_raygen; /* 280 B */
gs_status gs_query_radiance_gen_async(const gs_device_scene* scene, const gs_raygen* gen /* host */,
                                      const gs_ray* d_points /* GS_GEN_HEMISPHERE only */, uint32_t samples,
                                      uint32_t first_sample, uint32_t chunk, uint32_t max_depth, uint64_t seed,
                                      gs_ray_radiance* d_out, gs_counters* d_counters /* nullable */,
                                      gs_ray* d_rays_out /* nullable */, uint64_t* d_states_out /* nullable */,
                                      void* d_scratch, int64_t scratch_bytes, void* stream);
gs_status gs_query_radiance_gen(const gs_device_scene* scene, const gs_raygen* gen,
                                const gs_ray* points /* GS_GEN_HEMISPHERE only */, uint32_t samples,
                                uint32_t first_sample, uint32_t chunk, uint32_t max_depth, uint64_t seed,
                                gs_ray_radiance* out, gs_counters* counters /* nullable */,
                                gs_ray* rays_out /* nullable */, uint64_t* states_out /* nullable */);

/* Synchronous full-frame render on the current device: upload, render, copy back.
 * out_rgb: host buffer W*H*3 f32 (linear).  stats: host, nullable (counters, kernel and
 * render times, algorithmic bytes).  This is the one-call replacement for camera.rs:105-114:
 * gs_multi_create + gs_multi_render + gs_multi_destroy on the current device. */
gs_status gs_render(const gs_flat_scene* scene, const gs_camera* cam, const gs_sample_settings* ss,
                    uint64_t seed, float* out_rgb, gs_stats* stats /* nullable (ABI 6: was gs_counters*) */);

#ifdef __cplusplus
}
#endif
#endif /* GRAYSHIFT_GPU_H */
