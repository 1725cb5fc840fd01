"""Ray queries: what does this ray hit?

``RayQuery`` answers the reference's ``world.hit(ray, Interval(tmin, tmax), rec)`` (hittable.rs,
BVH.rs:69-90) for batches of caller rays on the device, through gs_query_rays (a kernel of its
own, csrc/device/query.hip): the closest hit with HitRecord's fields, or whether anything is hit
at all.  Picking, visibility tests, depth / normal / material probes, baking, and "why does this
pixel differ from the oracle" all start here.
"""
import ctypes as C

import numpy as np

from . import _native as N

HIT_COUNTERS = ("node_visits", "sphere_tests", "msphere_tests", "quad_tests", "tri_tests", "instance_tests",
                "list_tests", "medium_tests")

RAY_DTYPE = np.dtype([("o", "<f8", 3), ("d", "<f8", 3), ("time", "<f8"), ("tmin", "<f8"), ("tmax", "<f8")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", 3), ("n", "<f8", 3), ("u", "<f8"), ("v", "<f8"), ("hit", "<u4"),
                      ("front", "<u4"), ("material", "<u4"), ("ref", "<u4"), ("inst", "<u4"), ("pad", "<u4"),
                      ("state", "<u8")])
assert RAY_DTYPE.itemsize == C.sizeof(N.gs_ray) == 72 and HIT_DTYPE.itemsize == C.sizeof(N.gs_ray_hit) == 104


def pack_rays(rays):
    """An [n, 9] f64 array (o, d, time, tmin, tmax per row), or a dict with the keys o [n, 3],
    d [n, 3], time, tmin, tmax ([n] or scalars), as a contiguous [n, 9] f64 array: n gs_ray."""
    if isinstance(rays, dict):
        o = np.asarray(rays["o"], dtype=np.float64).reshape(-1, 3)
        n = len(o)
        a = np.empty((n, 9), dtype=np.float64)
        a[:, 0:3] = o
        a[:, 3:6] = np.asarray(rays["d"], dtype=np.float64).reshape(-1, 3)
        for k, key in ((6, "time"), (7, "tmin"), (8, "tmax")):
            a[:, k] = np.broadcast_to(np.asarray(rays[key], dtype=np.float64), (n,))
        return a
    a = np.ascontiguousarray(rays, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 9:
        raise ValueError("rays must be an [n, 9] f64 array (o, d, time, tmin, tmax) or a dict of them")
    return a


def camera_rays(cam, time=0.0, tmin=0.001, tmax=np.finfo(np.float64).max):
    """The pixel-centre rays of a gs_camera, row by row, as an [H * W, 9] array: get_ray
    (camera.rs:203-221) with a zero pixel offset and the origin at the camera's centre -- no
    jitter and no defocus -- over (tmin, tmax) at `time`."""
    W, H = cam.image_width, cam.image_height
    p0, du, dv = (np.array(v[:], dtype=np.float64) for v in (cam.starting_pixel_pos, cam.pixel_delta_u,
                                                             cam.pixel_delta_v))
    c = np.array(cam.center[:], dtype=np.float64)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ps = (p0[None, :] + du[None, :] * i.reshape(-1, 1)) + dv[None, :] * j.reshape(-1, 1)
    a = np.empty((W * H, 9), dtype=np.float64)
    a[:, 0:3] = c
    a[:, 3:6] = ps - c
    a[:, 6], a[:, 7], a[:, 8] = time, tmin, tmax
    return a


class RayQuery:
    """Closest-hit and any-hit queries against one scene on the current device.

    scene_or_spec: a scene of grayshift_amd.scenes (anything with a ``.spec``) or a spec itself;
    bvh: who builds its BVHs, as HostScene.  MultiRenderer.query() makes one over a frame context's
    scene without a second upload."""

    def __init__(self, scene_or_spec, bvh="host", _shared=None):
        self._own = _shared is None
        self.host = None
        if _shared is not None:
            self.dev = _shared
            return
        from .renderer import HostScene
        spec = scene_or_spec if hasattr(scene_or_spec, "ptr") else scene_or_spec.spec
        self.host = HostScene(spec, bvh=bvh)
        d = C.c_void_p()
        try:
            N.check(N.lib.gs_device_scene_create(self.host.flat_ptr, C.byref(d)))
        except Exception:
            self.host.close()
            raise
        self.dev = d

    def close(self):
        if self._own and self.dev:
            N.lib.gs_device_scene_destroy(self.dev)
        self.dev = None
        if self.host is not None:
            self.host.close()
            self.host = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: the binding may be gone)
            pass

    def _run(self, rays, mode, seed, counts):
        a = pack_rays(rays)
        n = len(a)
        hits = np.zeros(n, dtype=HIT_DTYPE)
        cnt = np.zeros((n, 8), dtype=np.uint32) if counts else None
        N.check(N.lib.gs_query_rays(self.dev, a.ctypes.data, n, mode, seed, hits.ctypes.data,
                                    cnt.ctypes.data if counts else None))
        res = {k: hits[k].copy() for k in ("t", "p", "n", "u", "v", "material", "ref", "inst", "state")}
        res["hit"] = hits["hit"] != 0
        res["front"] = hits["front"] != 0
        if counts:
            for j, name in enumerate(HIT_COUNTERS):
                res[name] = cnt[:, j].copy()
        return res

    def closest(self, rays, seed=1, counts=False):
        """The closest hit of each ray in (tmin, tmax).  A dict of arrays: hit, front (bool), t, p,
        n, u, v, material, ref, inst (GS_REF_NONE = 0 on a miss, t = tmax), state (the ray's stream
        after the walk); with counts=True also the ray's own test counters (HIT_COUNTERS)."""
        return self._run(rays, N.GS_QUERY_CLOSEST, seed, counts)

    def any(self, rays, seed=1, counts=False):
        """The first accepted hit of each ray's walk: `hit` equals closest()'s; the record is that
        hit's, not the nearest one's."""
        return self._run(rays, N.GS_QUERY_ANY, seed, counts)
