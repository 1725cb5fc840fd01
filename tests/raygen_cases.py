"""Generators, shapes and the numpy restatement of the generated radiance queries' tests
(tests/test_raygen_host.py, tests/test_gpu_raygen.py).

restate() spells out the four device ray generators of gs_query_radiance_gen (include/grayshift_gpu.h,
csrc/device/raygen.hip) from the oracle's pieces alone -- oracle.stream_seed and oracle.wyrand for the
draws, oracle.onb and oracle.random_cosine_direction for the hemisphere -- in the header's order and
association: every (item, sample)'s ray and the stream right after its generation.  It extends what
tests/test_gpu_radiance.py's _camera_rays_and_states does, with the defocus disk's rejection loop, the
panorama, the orthographic camera and the hemisphere.  CAMERA and ORTHO use no libm; PANORAMA's sines
and cosines and HEMISPHERE's are the host's (numpy, glibc), as query.panorama_rays' are.

The scenes are tests/radiance_cases.py's.  Everything is generated from fixed seeds and cached.
"""
import functools
import math

import numpy as np

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import query as GQ
from grayshift_amd.scene import camera_spec

import oracle

from tests import query_cases as Q

WY_C0 = 0x2d358dccaa6c78a5
M64 = (1 << 64) - 1
SEED = 23
IMAGES = ((5, 3), (17, 16))                    # 272 items: two blocks, the second partial
SAMPLES = ((1, 1), (5, 2), (33, 16))           # (samples, chunk): one chunk, three (the last short), three (the last of 1)
SCENES = ("spheres_sky", "media_sky", "general_all_sky", "textured_hdri")
KINDS = ("camera", "camera_defocus", "panorama", "ortho", "hemisphere")
LIBM_FREE_KINDS = ("camera", "camera_defocus", "ortho")
DEFOCUS = 0.6
# where a scene is looked at from (tests/test_gpu_radiance.py's frames): (look_from, fov, depth)
VIEW = {"spheres_sky": ((0.0, 2.0, 26.0), 40.0), "media_sky": ((0.0, 2.0, 26.0), 40.0),
        "mixed_sky": ((0.0, 2.0, 26.0), 40.0), "general_all_sky": ((0.5, 2.0, 9.0), 40.0),
        "textured_hdri": ((2.0, 3.0, 24.0), 45.0)}
ASPECT = {(5, 3): 1.6, (17, 16): 1.0625, (32, 32): 1.0}  # Camera::new: height = int(width / aspect)
# a frame that is no rotation of the world's (x, y, z rows; z, the panorama's up, along the world's y)
AXES = ((0.8, 0.0, 0.6), (-0.6, 0.0, 0.8), (0.0, 1.0, 0.0))


def camera(scene, w, h, defocus=0.0, max_depth=50):
    look_from, fov = VIEW[scene]
    cs = camera_spec(ASPECT[(w, h)], w, max_depth, fov, look_from, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), defocus,
                     math.sqrt(sum(x * x for x in look_from)))
    cam = g.camera(cs)
    assert (cam.image_width, cam.image_height) == (w, h)
    return cs, cam


def hemisphere_points(scene, n):
    """n points above the scene with normals roughly toward it, every sixth along +-x (the basis's
    other helper axis, |w.x| > 0.9), at times in [0, 1)."""
    rng = np.random.default_rng(500 + n)
    small = scene.startswith("general")
    p = rng.uniform(-3.0, 3.0, (n, 3)) if small else rng.uniform(-8.0, 8.0, (n, 3))
    p[:, 1] = rng.uniform(3.0, 5.0, n) if small else rng.uniform(9.0, 12.0, n)
    nrm = -p + rng.normal(size=(n, 3))  # (not unit: the basis normalises)
    nrm[::6] = np.column_stack([np.where(np.arange(len(nrm[::6])) % 2 == 0, 5.0, -5.0), rng.normal(size=(len(nrm[::6]), 2))])
    return p, nrm, rng.uniform(0.0, 1.0, n)


@functools.lru_cache(maxsize=None)
def gen(kind, scene, w, h):
    """The RayGen of one kind aimed at a scene, w x h items."""
    look_from, _ = VIEW[scene]
    small = scene.startswith("general")
    if kind in ("camera", "camera_defocus"):
        return GQ.RayGen.camera(camera(scene, w, h, DEFOCUS if kind == "camera_defocus" else 0.0)[1])
    if kind == "panorama":
        return GQ.RayGen.panorama((look_from[0], look_from[1], 0.5 * look_from[2]), w, h, AXES)
    if kind == "ortho":
        if small:
            return GQ.RayGen.ortho((-3.0, 0.2, 9.0), (6.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, -1.0), w, h)
        return GQ.RayGen.ortho((-9.0, 7.0, 22.0), (18.0, 0.0, 1.0), (0.0, -14.0, 0.5), (0.1, 0.0, -1.5), w, h)
    assert kind == "hemisphere"
    return GQ.RayGen.hemisphere(*hemisphere_points(scene, w * h))


class _Stream:
    """One sample's stream: draws taken one by one from a block of the oracle's."""

    def __init__(self, state):
        self.s0, self.k = state, 0
        self.f, _ = oracle.wyrand(state, 64)

    def f64(self):
        assert self.k < 64  # (a rejection loop of 30 rounds: never)
        self.k += 1
        return float(self.f[self.k - 1])

    @property
    def state(self):
        return (self.s0 + self.k * WY_C0) & M64


def _v(a):
    return np.array(a[:], dtype=np.float64)


def restate(rg, samples, seed, first_sample=0, jitter=True):
    """The rays ([n * samples, 9], tmin = 0.001 and tmax = f64::MAX) and post-generation streams
    ([n * samples] u64) of RayGen `rg`, sample s of item q at q * samples + s, and "retries": the
    defocus loop's rejected rounds.  jitter=False puts 0 in place of the two offsets after drawing
    them (the unjittered cameras of grayshift_amd.query, for the reach tests)."""
    raw = rg.raw
    kind = raw.kind
    H, W = rg.shape
    n = W * H
    rays = np.empty((n * samples, 9))
    states = np.empty(n * samples, dtype=np.uint64)
    si, sj = np.empty(n * samples), np.empty(n * samples)
    retries = 0
    cam = raw.cam
    p0, du, dv, c, ku, kv = (_v(x) for x in (cam.starting_pixel_pos, cam.pixel_delta_u, cam.pixel_delta_v, cam.center,
                                              cam.defocus_disk_u, cam.defocus_disk_v))
    origin, ax = _v(raw.origin), [_v(raw.axis[k]) for k in range(3)]
    k = 0
    for q in range(n):
        pj, pi = divmod(q, W)
        for s in range(samples):
            st = _Stream(oracle.stream_seed(seed, q, first_sample + s))
            if kind == N.GS_GEN_HEMISPHERE:
                pt = rg.points[q]
                b = oracle.onb(pt[3:6])  # rows u, v, w
                r1 = st.f64()
                r2 = st.f64()
                cd = oracle.random_cosine_direction(r1, r2)
                d = (b[0] * cd[0] + b[1] * cd[1]) + b[2] * cd[2]
                with np.errstate(invalid="ignore"):
                    d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                rays[k, 0:3], rays[k, 3:6], rays[k, 6] = pt[0:3], d, pt[6]
            else:
                offx = st.f64() - 0.5
                offy = st.f64() - 0.5
                if not jitter:
                    offx = offy = 0.0
                si[k], sj[k] = float(pi) + offx, float(pj) + offy
                if kind == N.GS_GEN_CAMERA:
                    ps = (p0 + du * si[k]) + dv * sj[k]
                    org = c
                    if cam.defocus_angle > 0.0:
                        while True:
                            dx = st.f64() * 2.0 + -1.0
                            dy = st.f64() * 2.0 + -1.0
                            if dx * dx + dy * dy + 0.0 * 0.0 < 1.0:
                                break
                            retries += 1
                        org = (c + ku * dx) + kv * dy
                    rays[k, 0:3], rays[k, 3:6] = org, ps - org
                rays[k, 6] = st.f64()  # (PANORAMA and ORTHO: o and d below, for all samples at once)
            states[k] = st.state
            k += 1
    if kind == N.GS_GEN_PANORAMA:  # query.panorama_rays' expressions, then the axes
        theta = ((si + 0.5) / W - 0.5) * (2.0 * np.pi)
        phi = (0.5 - (sj + 0.5) / H) * np.pi
        dl = np.empty((n * samples, 3))
        dl[:, 0], dl[:, 1], dl[:, 2] = np.cos(phi) * np.cos(theta), np.cos(phi) * np.sin(theta), np.sin(phi)
        dl /= np.linalg.norm(dl, axis=1, keepdims=True)
        rays[:, 0:3] = origin
        rays[:, 3:6] = (ax[0][None, :] * dl[:, 0:1] + ax[1][None, :] * dl[:, 1:2]) + ax[2][None, :] * dl[:, 2:3]
    elif kind == N.GS_GEN_ORTHO:  # query.ortho_rays' association
        rays[:, 0:3] = (origin[None, :] + ax[0][None, :] * ((si.reshape(-1, 1) + 0.5) / W)) + \
            ax[1][None, :] * ((sj.reshape(-1, 1) + 0.5) / H)
        rays[:, 3:6] = ax[2]
    rays[:, 7], rays[:, 8] = 0.001, Q.DMAX
    return {"rays": rays, "states": states, "retries": retries}


@functools.lru_cache(maxsize=None)
def restated(kind, scene, w, h, samples, seed=SEED, first_sample=0):
    r = restate(gen(kind, scene, w, h), samples, seed, first_sample)
    r["rays"].setflags(write=False)
    r["states"].setflags(write=False)
    return r


def fold_chunks(col, samples, chunk):
    """[n * samples, ...] per-sample values -> [n, ...]: ((0 + C_0) + C_1) + ... with each C_k = ((0 +
    s) + s) + ... over `chunk` consecutive samples; a single chunk is its C_0 itself, as the kernel
    writes it."""
    col = col.reshape((-1, samples) + col.shape[1:])
    chunk = chunk or 16
    parts = []
    for k0 in range(0, samples, chunk):
        c = np.zeros_like(col[:, 0])
        for s in range(k0, min(samples, k0 + chunk)):
            c = c + col[:, s]
        parts.append(c)
    if len(parts) == 1:
        return parts[0]
    total = np.zeros_like(parts[0])
    for c in parts:
        total = total + c
    return total


def _fold_chunks_self_check():
    """The helper against the association written out: (5 samples, chunk 2) and one chunk."""
    col = np.random.default_rng(1).uniform(0.0, 1.0, (3 * 5, 3))
    c = col.reshape(3, 5, 3)
    want = ((0.0 + ((0.0 + c[:, 0]) + c[:, 1])) + ((0.0 + c[:, 2]) + c[:, 3])) + (0.0 + c[:, 4])
    assert np.array_equal(fold_chunks(col, 5, 2), want)
    assert np.array_equal(fold_chunks(col, 5, 0), (((((0.0 + c[:, 0]) + c[:, 1]) + c[:, 2]) + c[:, 3]) + c[:, 4]))


_fold_chunks_self_check()
