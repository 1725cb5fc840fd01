"""Scenes, rays and the reference fold of the radiance-query tests (tests/test_radiance_host.py,
tests/test_gpu_radiance.py).

The scenes are tests/query_cases.py's, lit: their own background is black and none outside the
composition set has a light, so every colour on them is zero and a colour comparison shows nothing.
A lit variant is QScene(name, build) whose builder first sets a background and then calls the query
scene's builder: a solid sky (the libm-free cases), or a 64 x 32 HDRI whose texels are all distinct
and survive RGBE8 exactly, so the colour tells which direction left the scene.  `textured` adds a
checker, an image texture, a noise texture and a light quad under that HDRI; `mirrors` is metal and
dielectric spheres only, the scene with no libm call on its colour path; `outer_light` puts a light
and a fuzzy metal behind two instance chains, for the catch-all set's two-chain hit record.

The reference: ray_color_fold composes the oracle's batch entries on the scene's *twin* (one BVH of
the world's members: the world's own tree).  World(twin).bounce(0, ray, state) is exactly one level
of Camera::ray_color (camera.rs:174-202): the hit over (0.001, f64::MAX), then emitted, then scatter;
World.background(d) is the miss; the next ray is (p, dir, same time) and the stream carries on from
`state`.  The colour is taken in the project's forward form, T = (1 a1) a2 ..., ended by T c;
ray_color_recursive folds the same trail right to left, emitted + colour * attenuation, as the
reference's recursion does (camera.rs:193-195).

Everything is generated from fixed seeds; answers are computed once per (scene, depth) and shared.
"""
import functools

import numpy as np

import oracle

from tests import query_cases as Q

SEED = 11      # the radiance queries' seed: sample s of ray i starts at stream_seed(SEED, i, s)
N_RAYS = 4096
DEPTHS = (50, 4)
SKY, LIGHT, ABSORBED, DEPTH = 1, 2, 3, 4  # how a path ended
SOLID_SKY = (0.7, 0.8, 1.0)
HDRI_W, HDRI_H = 64, 32
HDRI_ROTATION = (0.3, -0.5, 1.1)
TEST_COUNTERS = ("node_visits", "sphere_tests", "msphere_tests", "quad_tests", "tri_tests", "instance_tests",
                 "list_tests", "medium_tests")


def hdri_map():
    """64 x 32 x 3 f32, every texel distinct and a multiple of 2^-8 with its largest channel in
    [0.5, 1): RGBE8 (8-bit mantissas under one exponent, here 2^0) holds each exactly."""
    k = np.arange(HDRI_W * HDRI_H)
    a = np.empty((HDRI_W * HDRI_H, 3), dtype=np.float32)
    a[:, 0] = (128 + k % 128) / 256.0
    a[:, 1] = (16 * (k // 128) + 3) / 256.0
    a[:, 2] = ((k * 7) % 128) / 256.0
    return a.reshape(HDRI_H, HDRI_W, 3)


def _image():
    j, i = np.meshgrid(np.arange(8), np.arange(16), indexing="ij")
    return np.stack([(i * 16 + 7) % 256, (j * 32 + 9) % 256, (i * 5 + j * 11 + 40) % 256], axis=2).astype(np.uint8)


def _mirrors(b):  # metal and dielectric spheres only: no libm call between a ray and its colour under a solid sky
    rng = np.random.default_rng(21)
    m = [b.metal((0.8, 0.7, 0.6), 0.0), b.metal((0.6, 0.8, 0.7), 0.25), b.dielectric(1.5), b.metal((0.9, 0.9, 0.9), 0.6)]
    return [(b.sphere(tuple(rng.uniform(-8.0, 8.0, 3)), float(rng.uniform(0.6, 1.6)), m[k % 4]), "sphere")
            for k in range(48)]


def _textured(b):
    out = []
    chk = b.lambertian_texture(b.checkered_from_colors(0.8, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    deep = b.lambertian_texture(b.checkered(1.7, b.checkered_from_colors(0.4, (0.9, 0.2, 0.2), (0.2, 0.2, 0.9)),
                                            b.solid((0.8, 0.8, 0.3))))
    img = b.lambertian_texture(b.image_texture(b.image(_image())))
    noi = b.lambertian_texture(b.noise(2.0))
    out.append((b.sphere((0.0, -114.0, 0.0), 100.0, chk), "ground"))  # (below every ray origin)
    out.append((b.sphere((-3.0, 0.0, 2.0), 2.0, img), "image_sphere"))
    out.append((b.quad((1.0, -3.0, -5.0), (5.0, 0.0, 1.0), (0.0, 4.0, 0.5), img), "image_quad"))
    out.append((b.sphere((3.5, -1.0, 3.0), 1.8, noi), "noise_sphere"))
    out.append((b.sphere((-5.0, 3.0, -4.0), 2.2, deep), "checker_sphere"))
    out.append((b.sphere((1.0, 2.5, 0.0), 1.2, b.dielectric(1.5)), "glass"))
    out.append((b.sphere((6.0, 3.0, -2.0), 1.5, b.metal((0.8, 0.8, 0.8), 0.05)), "metal"))
    out.append((b.quad((-2.0, 6.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), b.diffuse_light((4.0, 3.0, 2.0))), "light"))
    out.append((b.sphere((-6.0, -2.0, 5.0), 1.0, b.diffuse_light(
        (0.0, 0.0, 0.0))), "dark_light"))  # (emits nothing: an absorbed-looking end on a light)
    return out


def _outer_light(b):
    """A catch-all scene whose light and whose fuzzy metal sit behind a chain inside a BVH that is
    itself under a chain: their hits carry two chains (hit_outer), so the emitter's and the
    absorbing metal's ends of a path pass through the two-chain HitRecord."""
    rng = np.random.default_rng(22)
    white, blue = b.lambertian((0.7, 0.7, 0.7)), b.lambertian((0.2, 0.3, 0.8))
    members = [b.sphere(tuple(rng.uniform(-6.0, 6.0, 3)), float(rng.uniform(0.6, 1.4)), (white, blue)[k % 2])
               for k in range(10)]
    light = b.quad((-2.5, 0.0, -2.5), (5.0, 0.0, 0.0), (0.0, 0.0, 5.0), b.diffuse_light((5.0, 4.0, 3.0)))
    members.append(b.translate(b.rotate_y(light, 20.0), (0.5, 7.0, 0.0)))
    members.append(b.translate(b.rotate_y(b.sphere((0.0, 0.0, 0.0), 2.0, b.metal((0.9, 0.8, 0.7), 0.5)), 35.0),
                               (3.0, -3.0, 2.0)))
    return [(b.translate(b.rotate_y(b.bvh(members), 25.0), (0.4, 0.0, -0.3)), "nested"),
            (b.sphere((0.0, -114.0, 0.0), 100.0, white), "ground")]


OWN = {"mirrors": _mirrors, "textured": _textured, "outer_light": _outer_light}
# lit scene -> (the builder's name, the sky)
LIT = {
    "mixed_sky": ("mixed", "solid"), "media_sky": ("media", "solid"), "spheres_sky": ("spheres", "solid"),
    "fog_sky": ("fog", "solid"), "general_all_sky": ("general_all", "solid"), "nested_media_sky": ("nested_media", "solid"),
    "mirrors_sky": ("mirrors", "solid"), "outer_light_sky": ("outer_light", "solid"),
    "mixed_hdri": ("mixed", "hdri"), "media_hdri": ("media", "hdri"), "general_all_hdri": ("general_all", "hdri"),
    "textured_hdri": ("textured", "hdri"),
}
HDRI_SCENES = tuple(sorted(k for k, (_, sky) in LIT.items() if sky == "hdri"))
LIBM_FREE = ("mirrors_sky",)
NOISE_SCENES = ("textured_hdri",)
# the kernel set each lit scene must launch (MEDIA = 1 / NESTED = 2 / GENERAL = 512 of its feat)
FEAT_BITS = {"mixed_sky": 2, "media_sky": 3, "spheres_sky": 0, "fog_sky": 1, "mirrors_sky": 0, "mixed_hdri": 2,
             "media_hdri": 3, "textured_hdri": 0, "general_all_sky": 512, "nested_media_sky": 512,
             "general_all_hdri": 512, "outer_light_sky": 512}

# The ends a scene's geometry can give, asked of it at both depths (tests/test_radiance_host.py): the
# sky and the depth limit everywhere; a light where the scene holds one; an absorbed ray where it
# holds a fuzzy metal (or, `textured`, a light that emits nothing).  What is left out cannot occur:
# `fog` and `nested_media` hold no metal, and only `nested_media`, `textured` and `outer_light` a light.
ENDS = {name: {SKY, DEPTH} for name in LIT}
for _name in ("nested_media_sky", "textured_hdri", "outer_light_sky"):
    ENDS[_name] = ENDS[_name] | {LIGHT}
for _name in LIT:
    if LIT[_name][0] not in ("fog", "nested_media"):
        ENDS[_name] = ENDS[_name] | {ABSORBED}


def _grazing(centre, radius, n, seed, lo=0.995):
    """n rays from 20 units away that meet the sphere at an impact parameter in [lo, 1) radius: a
    fuzzy metal absorbs a ray whose fuzzed reflection points into the surface, which takes a
    grazing one (fuzz 0.1: the last half percent of the radius)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, dtype=np.float64)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)          # from the sphere toward the origin of the ray
    p = np.cross(v, rng.normal(size=(n, 3)))
    p /= np.linalg.norm(p, axis=1, keepdims=True)          # across it
    o = c + 20.0 * v
    tgt = c + p * (radius * rng.uniform(lo, 1.0, n))[:, None]
    a = np.empty((n, 9))
    a[:, 0:3], a[:, 3:6] = o, tgt - o
    a[:, 6], a[:, 7], a[:, 8] = rng.uniform(0.0, 1.0, n), 0.001, Q.DMAX
    return a


def _inside_ground(centre, radius, n, seed):
    """n rays that start inside the Lambertian ground sphere: every bounce stays inside, so the path
    runs to the depth limit whatever the depth."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, dtype=np.float64)
    a = np.empty((n, 9))
    a[:, 0:3] = c + rng.uniform(-0.4, 0.4, (n, 3)) * radius
    a[:, 3:6] = rng.normal(size=(n, 3))
    a[:, 6], a[:, 7], a[:, 8] = rng.uniform(0.0, 1.0, n), 0.001, Q.DMAX
    return a


def aimed(name):
    """The rays that take the place of a scene's last random rays, where the random ones fall short
    of an end the scene can give ([m, 9], m possibly 0)."""
    base = LIT[name][0]
    if base == "mixed":  # its metals' fuzz is 0.1: the dyadic metal sphere, grazed
        return _grazing((3.0, -2.0, 4.0), 0.5, 256, 41)
    if base == "nested_media":  # no specular material: its only long paths are inside the ground
        return _inside_ground((0.0, -101.0, 0.0), 100.0, 16, 42)
    if base == "outer_light":
        return _inside_ground((0.0, -114.0, 0.0), 100.0, 16, 44)
    return np.zeros((0, 9))


def _builder(base):
    return OWN[base] if base in OWN else (Q.SCENES[base] if base in Q.SCENES else Q.GENERAL[base])


@functools.lru_cache(maxsize=None)
def scene(name):
    base, sky = LIT[name]

    def build(b):
        if sky == "solid":
            b.background_solid(SOLID_SKY)
        else:
            b.background_hdri(hdri_map(), HDRI_ROTATION)
        return _builder(base)(b)
    return Q.QScene(name, build)


@functools.lru_cache(maxsize=None)
def rays(name):
    """4 096 rays of the scene ([n, 9]; tmin / tmax as the ray queries', unread here): random ones,
    the last of them replaced by the scene's aimed rays."""
    base = LIT[name][0]
    r = Q.random_rays(base, N_RAYS, 300 + sorted(LIT).index(name))
    extra = aimed(name)
    if len(extra):
        r[N_RAYS - len(extra):] = extra
    r.setflags(write=False)
    return r


def seeds(n, samples=1, first=0, seed=SEED):
    """[n * samples] start states: stream_seed(seed, first + i, s) at i * samples + s."""
    return np.array([oracle.stream_seed(seed, first + i, s) for i in range(n) for s in range(samples)], dtype=np.uint64)


# ----------------------------------------------------------------------------- the reference fold
def ray_color_fold(twin, rays_, s0, max_depth, trail=False, totals=False):
    """ray_color(Ray(o, d, time), max_depth, world) of each ray in the forward form, vectorised over
    the rays still alive.  A dict: rgb [n, 3], rays (world.hit calls), state (the stream after),
    end (SKY / LIGHT / ABSORBED / DEPTH; 0 with max_depth 0), noise (bool: a noise texture lies on
    the path); with trail=True also the per-level records ray_color_recursive folds; with
    totals=True also "counters": the batch's totals in a render's meaning."""
    n = len(rays_)
    w = oracle.World(twin)
    T = np.ones((n, 3))
    rgb = np.zeros((n, 3))
    nrays = np.zeros(n, dtype=np.uint64)
    state = np.array(s0, dtype=np.uint64).copy()
    end = np.zeros(n, dtype=np.int32)
    noise = np.zeros(n, dtype=bool)
    o, d, time = rays_[:, 0:3].copy(), rays_[:, 3:6].copy(), rays_[:, 6].copy()
    alive = np.arange(n)
    levels = []
    tot = {k: 0 for k in ("rays", "hits", "image_texels", "hdri_texels", "noise_evals") + TEST_COUNTERS}
    try:
        for level in range(max_depth):
            if len(alive) == 0:
                break
            ray = np.column_stack([o[alive], d[alive], time[alive]])
            zeros = np.zeros(len(alive), dtype=np.int32)
            b = w.bounce(zeros, ray, state[alive])
            if totals:
                h = w.hit(zeros, ray, 0.001, Q.DMAX, state[alive])
                for k in TEST_COUNTERS:
                    tot[k] += int(h[k].sum())
            nrays[alive] += np.uint64(1)
            state[alive] = b["state"]
            noise[alive] |= b["noise_evals"] > 0
            hit, sc = b["hit"], b["scatter"]
            miss = ~hit
            bg, hd = w.background(d[alive][miss])
            tot["rays"] += len(alive)
            tot["hits"] += int(hit.sum())
            tot["image_texels"] += int(b["image_texels"].sum())
            tot["noise_evals"] += int(b["noise_evals"].sum())
            tot["hdri_texels"] += int(hd.sum()) + int(b["hdri_texels"].sum())
            term = np.zeros((len(alive), 3))  # a path that ends here ends with T * term
            term[miss] = bg
            stop = hit & ~sc
            term[stop] = b["emitted"][stop]
            ends = miss | stop
            rgb[alive[ends]] = T[alive[ends]] * term[ends]
            end[alive[miss]] = SKY
            end[alive[stop]] = np.where((b["emitted"][stop] != 0.0).any(axis=1), LIGHT, ABSORBED)
            if trail:
                levels.append({"idx": alive.copy(), "ends": ends.copy(), "term": term.copy(),
                               "emitted": b["emitted"].copy(), "attenuation": b["attenuation"].copy()})
            T[alive[sc]] = T[alive[sc]] * b["attenuation"][sc]
            o[alive[sc]] = b["p"][sc]
            d[alive[sc]] = b["dir"][sc]
            alive = alive[sc]
        end[alive] = DEPTH if max_depth > 0 else 0  # out of depth: black (camera.rs:175)
    finally:
        w.close()
    res = {"rgb": rgb, "rays": nrays, "state": state, "end": end, "noise": noise}
    if trail:
        res["trail"] = levels
    if totals:
        tot["paths"] = n
        res["counters"] = tot
    return res


def ray_color_recursive(n, levels):
    """The reference's own association over a fold's trail: from the last level back to the first,
    colour = emitted + colour * attenuation for a scattered ray (camera.rs:193-195), the sky or the
    emitted colour where the path ends, 0 below the depth limit."""
    c = np.zeros((n, 3))
    for lv in reversed(levels):
        idx, ends = lv["idx"], lv["ends"]
        below = c[idx]  # (0 where nothing was traced below: the depth limit)
        c[idx] = np.where(ends[:, None], lv["term"], lv["emitted"] + below * lv["attenuation"])
    return c


@functools.lru_cache(maxsize=None)
def answers(name, max_depth):
    """The fold of the scene's rays at one sample each, with the batch's totals."""
    r = rays(name)
    return ray_color_fold(scene(name).twin, r, seeds(len(r)), max_depth, totals=True)
