"""Shared by the BVH build tests: the box lists the device builder is compared on, the
scenes the rebuilt host path is compared on, and helpers over the C entry points."""
import ctypes as C

import numpy as np

from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import SceneBuilder, fixed_spp

NODE = np.dtype([("min", "<f8", 3), ("max", "<f8", 3), ("left", "<u4"), ("right", "<u4"), ("pad", "<u4", 2)])
assert NODE.itemsize == 64
REF_NODE, REF_BUILD_MEMBER = 1, 15


def nodes_of(n):
    """The reference tree's node count: one node for n <= 2, else a split at n // 2."""
    return 1 if n <= 2 else 1 + nodes_of(n // 2) + nodes_of(n - n // 2)


def depth_of(n):
    return 1 if n <= 2 else 1 + max(depth_of(n // 2), depth_of(n - n // 2))


def _spheres(n, rng):
    c = rng.random((n, 3)) * 20.0 - 10.0
    r = rng.random((n, 1)) * 0.5 + 0.05
    return np.concatenate([c - r, c + r], axis=1)


def box_cases(n, seed=11):
    """{name: float64 [n, 6] (min xyz, max xyz)}: the issue's eight kinds of box lists."""
    rng = np.random.default_rng(seed + n)
    out = {}
    out["random"] = _spheres(n, rng)
    # an integer grid, one radius: long runs of equal keys on every axis at every level
    g = max(1, int(round(n ** (1.0 / 3.0))))
    idx = rng.permutation(n)
    c = np.stack([idx % g, (idx // g) % g, idx // (g * g)], axis=1).astype(np.float64)
    out["grid"] = np.concatenate([c - 0.25, c + 0.25], axis=1)
    out["identical"] = np.tile(np.array([[-1.0, -2.0, -3.0, 1.5, 2.5, 3.5]]), (n, 1))
    s = _spheres(n, rng) * 0.01
    s[:, 0] += np.arange(n)
    s[:, 3] += np.arange(n)
    out["sorted"] = s
    out["reversed"] = s[::-1].copy()
    # -0.0 and +0.0 in alternation on the sort axis (x: the longest) and in the fold (x and y)
    z = np.zeros((n, 6))
    i = np.arange(n)
    z[:, 0] = np.where(i % 2 == 0, -0.0, 0.0)
    z[i % 5 == 3, 0] = 1.0
    z[i % 7 == 4, 0] = -1.0
    z[:, 1] = np.where(i % 2 == 0, 0.0, -0.0)
    z[:, 2] = np.where(i % 3 == 0, -0.0, 0.0)
    z[:, 3] = 5.0
    z[:, 4] = np.where(i % 2 == 0, 1.0, 0.5)
    z[:, 5] = np.where(i % 4 == 0, 0.0, -0.0) + (i % 3 == 1) * 0.25
    out["signed_zeros"] = z
    # axis ties: x.size == y.size > z.size, and x.size == y.size == z.size
    for name, zdiv in (("tie_xy", 2), ("tie_xyz", 1)):
        gg = max(2, int(round(n ** 0.5)))
        c = rng.integers(0, gg, (n, 3)).astype(np.float64)
        c[:, 2] = np.floor(c[:, 2] / zdiv)
        c[0] = 0.0
        if n > 1:
            c[1] = (gg - 1, gg - 1, (gg - 1) // zdiv)
        out[name] = np.concatenate([c - 0.5, c + 0.5], axis=1)
    # thin slabs: the longest axis of a segment changes from level to level
    c = rng.random((n, 3))
    half = np.full((n, 3), 0.001)
    half[np.arange(n), rng.integers(0, 3, n)] = 0.3
    out["slabs"] = np.concatenate([c - half, c + half], axis=1)
    inf = _spheres(n, rng)
    inf[0, 3] = np.inf
    inf[n - 1, 1] = -np.inf
    out["infinite"] = inf
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in out.items()}


def host_build(boxes, node_base=0):
    """gs_host_bvh_build: (nodes as NODE records, order)."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    n = boxes.shape[0]
    nodes = np.zeros(N.lib.gs_bvh_node_count(n), dtype=NODE)
    order = np.zeros(n, dtype=np.uint32)
    N.check(N.lib.gs_host_bvh_build(boxes.ctypes.data, n, node_base, nodes.ctypes.data, order.ctypes.data))
    return nodes, order


def device_build(boxes, refs=None, node_base=0):
    """gs_bvh_build_async + gs_bvh_build_status on the current device: (status, nodes, order)."""
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    n = boxes.shape[0]
    n_nodes = N.lib.gs_bvh_node_count(n)
    work = N.lib.gs_bvh_build_work_bytes(n)
    sizes = [boxes.nbytes, n_nodes * NODE.itemsize, n * 4, work, n * 4]
    d = [C.c_void_p() for _ in sizes]
    try:
        for p, size in zip(d, sizes):
            N.check(N.lib.gs_device_alloc(size, C.byref(p)))
        N.check(N.lib.gs_device_upload(d[0], boxes.ctypes.data, boxes.nbytes))
        d_refs = None
        if refs is not None:
            refs = np.ascontiguousarray(refs, dtype=np.uint32)
            N.check(N.lib.gs_device_upload(d[4], refs.ctypes.data, refs.nbytes))
            d_refs = d[4]
        N.check(N.lib.gs_bvh_build_async(d[0], d_refs, n, node_base, d[1], d[2], d[3], work, None))
        status = N.lib.gs_bvh_build_status(d[3], None)
        nodes = np.zeros(n_nodes, dtype=NODE)
        order = np.zeros(n, dtype=np.uint32)
        N.check(N.lib.gs_device_download(nodes.ctypes.data, d[1], nodes.nbytes))
        N.check(N.lib.gs_device_download(order.ctypes.data, d[2], order.nbytes))
        return status, nodes, order
    finally:
        for p in d:
            if p:
                N.lib.gs_device_free(p)


def triangle_grid(nx=23, ny=46):
    """2 * nx * ny triangles on the integer grid (2 116 by default): grid-aligned ties."""
    b = SceneBuilder()
    m = b.lambertian((0.6, 0.7, 0.5))
    for j in range(ny):
        for i in range(nx):
            p00, p10, p01, p11 = (i, j, 0.0), (i + 1.0, j, 0.0), (i, j + 1.0, 0.0), (i + 1.0, j + 1.0, 0.0)
            b.add(b.triangle(p00, p10, p11, m))
            b.add(b.triangle(p00, p11, p01, m))
    b.background_solid((0.7, 0.8, 1.0))
    return b.build()


def scene_specs():
    """{name: gs_scene_spec holder}: the five scenes the rebuilt path is compared on."""
    return {
        "bouncing_spheres": scenes.bouncing_spheres(width=64, settings=fixed_spp(1)).spec,
        "cornell_box": scenes.cornell_box(width=64, settings=fixed_spp(1)).spec,
        "final_scene": scenes.final_scene(width=64, settings=fixed_spp(1)).spec,
        "triangle_grid": triangle_grid(),
        "C4": scenes.config("C4", width=64, spp=1).spec,
    }


FLAT_ARRAYS = [("nodes", "n_nodes", "gs_node"), ("spheres", "n_spheres", "gs_sphere"),
               ("mspheres", "n_mspheres", "gs_msphere"), ("quads", "n_quads", "gs_quad"),
               ("triangles", "n_triangles", "gs_triangle"), ("lists", "n_lists", "gs_list"),
               ("list_refs", "n_list_refs", 4), ("instances", "n_instances", "gs_instance"),
               ("media", "n_media", "gs_medium"), ("noise_perm", "n_noise_perm", 1),
               ("materials", "n_materials", "gs_material"), ("textures", "n_textures", "gs_texture"),
               ("images", "n_images", "gs_image"), ("texels8", "n_texels8", 1), ("hdri_rgb", "n_hdri_floats", 4)]


def flat_bytes(flat):
    """{array name: its bytes} of a gs_flat_scene, plus the scalar fields."""
    out = {"root": flat.root, "max_bvh_depth": flat.max_bvh_depth}
    for name, count, rec in FLAT_ARRAYS:
        k = int(getattr(flat, count))
        size = rec if isinstance(rec, int) else int(N.lib.gs_host_struct_size(rec.encode()))
        assert size > 0, rec
        p = getattr(flat, name)
        addr = p if isinstance(p, int) or p is None else C.cast(p, C.c_void_p).value
        out[count] = k
        out[name] = C.string_at(addr, k * size) if k and addr else b""
    bg = flat.background
    out["background"] = C.string_at(C.addressof(bg), C.sizeof(bg))
    return out
