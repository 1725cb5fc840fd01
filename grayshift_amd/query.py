"""Ray queries: what does this ray hit?

``RayQuery`` answers the reference's ``world.hit(ray, Interval(tmin, tmax), rec)`` (hittable.rs,
BVH.rs:69-90) for batches of caller rays on the device, through gs_query_rays (a kernel of its
own, csrc/device/query.hip): the closest hit with HitRecord's fields, or whether anything is hit
at all.  Picking, visibility tests, depth / normal / material probes, baking, and "why does this
pixel differ from the oracle" all start here.

``RayQuery.radiance`` answers the other half of the per-pixel path, ``Camera::ray_color(ray, depth,
world)`` (camera.rs:174-202), through gs_query_radiance (csrc/device/radiance.hip): the light that
comes back along each caller ray, for cameras the reference does not have (``panorama_rays``,
``ortho_rays``), light-map baking, probes, and replaying one pixel's path.

``RayQuery.radiance_gen`` is that query with a ray drawn on the device for every sample, from the
sample's own stream (gs_query_radiance_gen, csrc/device/raygen.hip): a ``RayGen`` names the
generator -- the reference's thin-lens camera, a jittered panorama or orthographic camera, or
cosine-weighted directions about caller points for baking -- and nothing is uploaded per sample.
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
RADIANCE_DTYPE = np.dtype([("rgb", "<f8", 3), ("rays", "<u8"), ("state", "<u8")])
assert RAY_DTYPE.itemsize == C.sizeof(N.gs_ray) == 72 and HIT_DTYPE.itemsize == C.sizeof(N.gs_ray_hit) == 104
assert RADIANCE_DTYPE.itemsize == C.sizeof(N.gs_ray_radiance) == 40


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


def panorama_rays(center, width, height, time=0.0):
    """An equirectangular camera at `center`: [height * width, 9] rays, row by row, with unit
    directions over the full sphere through the texel centres of a width x height sky map.

    The convention is HDRI::sample's (camera.rs:257-270) run backwards, in the sky map's own frame
    (the background's rotation applied to nothing): pixel (row j, column i) looks along
    (cos phi cos theta, cos phi sin theta, sin phi) with theta = ((i + 0.5) / width - 0.5) 2 pi and
    phi = (0.5 - (j + 0.5) / height) pi -- z is up, row 0 is next to the +z pole, column 0 starts at
    theta = -pi -- so that u = 0.5 + atan2(y, x) / 2 pi and v = 0.5 - asin(z) / pi name texel (i, j):
    in an empty world under an unrotated width x height HDRI the radiance is the sky map itself."""
    W, H = int(width), int(height)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    theta = ((i.reshape(-1) + 0.5) / W - 0.5) * (2.0 * np.pi)
    phi = (0.5 - (j.reshape(-1) + 0.5) / H) * np.pi
    a = np.empty((W * H, 9), dtype=np.float64)
    a[:, 0:3] = np.asarray(center, dtype=np.float64)
    a[:, 3], a[:, 4], a[:, 5] = np.cos(phi) * np.cos(theta), np.cos(phi) * np.sin(theta), np.sin(phi)
    a[:, 3:6] /= np.linalg.norm(a[:, 3:6], axis=1, keepdims=True)
    a[:, 6], a[:, 7], a[:, 8] = time, 0.001, np.finfo(np.float64).max
    return a


def ortho_rays(corner, edge_u, edge_v, direction, width, height, time=0.0):
    """An orthographic camera: [height * width, 9] parallel rays along `direction` (as given, not
    normalised), row by row, from the cell centres corner + (i + 0.5) / width edge_u + (j + 0.5) /
    height edge_v of a rectangle cut into width x height cells."""
    W, H = int(width), int(height)
    c, eu, ev = (np.asarray(v, dtype=np.float64) for v in (corner, edge_u, edge_v))
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a = np.empty((W * H, 9), dtype=np.float64)
    a[:, 0:3] = (c[None, :] + eu[None, :] * ((i.reshape(-1, 1) + 0.5) / W)) + ev[None, :] * ((j.reshape(-1, 1) + 0.5) / H)
    a[:, 3:6] = np.asarray(direction, dtype=np.float64)
    a[:, 6], a[:, 7], a[:, 8] = time, 0.001, np.finfo(np.float64).max
    return a


class RayGen:
    """A device ray generator of RayQuery.radiance_gen (a gs_raygen and, for a hemisphere, its
    points): item q = row q // width, column q % width of a width x height image, sample s drawn from
    stream_seed(seed, q, first_sample + s).  The draws of each kind: include/grayshift_gpu.h."""

    def __init__(self, raw, points=None):
        self.raw = raw
        self.points = points  # [n, 9] f64 (o = the point, d = the normal, time), GS_GEN_HEMISPHERE only

    @property
    def shape(self):
        """(height, width) of the generator's image."""
        if self.raw.kind == N.GS_GEN_CAMERA:
            return self.raw.cam.image_height, self.raw.cam.image_width
        return self.raw.height, self.raw.width

    @staticmethod
    def camera(cam):
        """Camera::get_ray (camera.rs:204-221) of a gs_camera: the pixel's jitter, the defocus disk
        when defocus_angle > 0, and the time draw -- the render's own camera rays."""
        g = N.gs_raygen()
        g.kind, g.width, g.height = N.GS_GEN_CAMERA, cam.image_width, cam.image_height
        C.memmove(C.addressof(g.cam), C.addressof(cam), C.sizeof(N.gs_camera))
        return RayGen(g)

    @staticmethod
    def panorama(center, w, h, axes=None):
        """panorama_rays' equirectangular camera at `center`, jittered inside each texel, with a time
        draw; axes: the rows x, y, z of the camera's frame in the world ([3, 3]; None: the world's)."""
        g = N.gs_raygen()
        g.kind, g.width, g.height = N.GS_GEN_PANORAMA, int(w), int(h)
        g.origin[:] = [float(x) for x in center]
        ax = np.eye(3) if axes is None else np.asarray(axes, dtype=np.float64).reshape(3, 3)
        for k in range(3):
            g.axis[k][:] = [float(x) for x in ax[k]]
        return RayGen(g)

    @staticmethod
    def ortho(corner, edge_u, edge_v, direction, w, h):
        """ortho_rays' orthographic camera, jittered inside each cell, with a time draw."""
        g = N.gs_raygen()
        g.kind, g.width, g.height = N.GS_GEN_ORTHO, int(w), int(h)
        g.origin[:] = [float(x) for x in corner]
        for k, v in enumerate((edge_u, edge_v, direction)):
            g.axis[k][:] = [float(x) for x in v]
        return RayGen(g)

    @staticmethod
    def hemisphere(points, normals, time=0.0):
        """Cosine-weighted directions about `normals` from `points` ([n, 3] each), at `time` (a
        scalar or [n]): Lambertian::scatter's direction (material.rs:52-53).  A 1 x n image."""
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        a = np.zeros((len(p), 9), dtype=np.float64)
        a[:, 0:3] = p
        a[:, 3:6] = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        a[:, 6] = np.broadcast_to(np.asarray(time, dtype=np.float64), (len(p),))
        a[:, 7], a[:, 8] = 0.001, np.finfo(np.float64).max
        g = N.gs_raygen()
        g.kind, g.width, g.height = N.GS_GEN_HEMISPHERE, len(p), 1
        return RayGen(g, a)


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

    def radiance(self, rays, samples=1, max_depth=50, seed=1, chunk=0, states=None, counters=False):
        """Camera::ray_color(ray, max_depth, world) of each ray, `samples` samples each (the rays'
        tmin / tmax are not read: every segment is tested over (0.001, f64::MAX)).  Sample s of ray i
        draws from stream_seed(seed, i, s), or from states[i * samples + s] when `states` ([n *
        samples] u64) is given.  A dict of arrays: sum [n, 3] f64 (the samples' colours added in
        chunks of `chunk`, 0 = 16: the render's association), rgb = sum / samples, rays (world.hit
        calls), state (the stream after the last sample); with counters=True also "counters", the
        batch's totals as a dict (a render's counters; pixels stays 0)."""
        a = pack_rays(rays)
        n = len(a)
        st = None
        if states is not None:
            st = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1)
            if len(st) != n * int(samples):
                raise ValueError("states must hold n * samples stream states")
        out = np.zeros(n, dtype=RADIANCE_DTYPE)
        cnt = N.gs_counters() if counters else None
        N.check(N.lib.gs_query_radiance(self.dev, a.ctypes.data, n, samples, chunk, max_depth, seed,
                                        st.ctypes.data if st is not None and len(st) else None, out.ctypes.data,
                                        C.addressof(cnt) if counters else None))
        res = {"sum": out["rgb"].copy(), "rgb": out["rgb"] / float(samples), "rays": out["rays"].copy(),
               "state": out["state"].copy()}
        if counters:
            res["counters"] = cnt.as_dict()
        return res

    def radiance_gen(self, gen, samples, max_depth=50, seed=1, chunk=0, first_sample=0, counters=False, emit=False):
        """Camera::ray_color along a ray the device draws for every sample of every item of `gen` (a
        RayGen), samples [first_sample, first_sample + samples) of the (item, sample) streams of
        `seed`.  A dict of arrays: sum [H, W, 3] f64 (the samples' colours added in chunks of `chunk`,
        0 = 16), rgb = sum / samples, rays [H, W] (world.hit calls), state [H, W] (the stream after the
        last sample); with counters=True also "counters"; with emit=True also "gen_rays" [H * W *
        samples, 9] and "gen_states" [H * W * samples]: each sample's generated ray and the stream
        right after its generation, which radiance(gen_rays, samples=1, states=gen_states) retraces."""
        h, w = gen.shape
        n = max(h, 0) * max(w, 0)
        samples = int(samples)
        out = np.zeros(n, dtype=RADIANCE_DTYPE)
        cnt = N.gs_counters() if counters else None
        rays = np.zeros((n * samples, 9), dtype=np.float64) if emit else None
        states = np.zeros(n * samples, dtype=np.uint64) if emit else None
        pts = gen.points
        N.check(N.lib.gs_query_radiance_gen(self.dev, C.addressof(gen.raw), pts.ctypes.data if pts is not None else None,
                                            samples, first_sample, chunk, max_depth, seed, out.ctypes.data,
                                            C.addressof(cnt) if counters else None,
                                            rays.ctypes.data if emit and rays.size else None,
                                            states.ctypes.data if emit and states.size else None))
        res = {"sum": out["rgb"].reshape(h, w, 3).copy(), "rgb": out["rgb"].reshape(h, w, 3) / float(samples),
               "rays": out["rays"].reshape(h, w).copy(), "state": out["state"].reshape(h, w).copy()}
        if counters:
            res["counters"] = cnt.as_dict()
        if emit:
            res["gen_rays"], res["gen_states"] = rays, states
        return res
