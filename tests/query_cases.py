"""Scenes, twins and rays of the ray-query tests (tests/test_query_host.py, tests/test_gpu_query.py).

A scene is a world of top-level objects, as the product takes it.  Its *twin* is the same spec with
one world object, SceneBuilder.bvh(members) of the same members in the same order:
BVHNode::construct_tree of that list is the world's own tree, so oracle.World(twin).hit(0, ray,
tmin, tmax, s0) is the reference's world.hit -- the answer, the stream after and the eight test
counters.  (A fold of World(spec).hit(k, ...) over the top-level objects in list order is not: the
reference's Triangle::hit ignores ray_t, so the last triangle tested wins, and media draw in visit
order.  fold() below is kept for the host test's reach assertion only.)

Everything is generated from fixed seeds; answers are computed once per scene and shared.
"""
import ctypes as C
import functools

import numpy as np

import grayshift_amd as g
from grayshift_amd import _native as N

import oracle

DMAX = np.finfo(np.float64).max
SEED = 7  # the queries' seed: ray i's stream starts at stream_seed(SEED, i, 0)
BATCHES = (0, 1, 63, 64, 65, 255, 256, 257)


class QScene:
    """spec: the product's scene; twin: the same objects, world = [bvh(members)]; b: the builder
    (its object list is read for the material map); tags: top-level member -> a label."""

    def __init__(self, name, build):
        self.name = name
        b = g.SceneBuilder()
        self.tags = build(b)  # [(object handle, label)] in world order
        self.members = [h for h, _ in self.tags]
        self.labels = [t for _, t in self.tags]
        self.objects = [(o.kind, o.material, o.first, o.count, tuple(o.p)) for o in b._objects]
        self.children = list(b._children)
        for h in self.members:
            b.add(h)
        self.spec = b.build()
        b._world = [b.bvh(self.members)]
        self.twin = b.build()


# ----------------------------------------------------------------------------- scenes
def _mixed(b, media=False):
    rng = np.random.default_rng(11)
    lam, met, die = b.lambertian((0.7, 0.3, 0.2)), b.metal((0.8, 0.8, 0.9), 0.1), b.dielectric(1.5)
    out = []
    # four spheres on small dyadic coordinates (rays that start exactly on a box face), 36 random ones
    dy = [((-4.0, 2.0, 1.0), 1.0), ((3.0, -2.0, 4.0), 0.5), ((0.0, 5.0, -3.0), 2.0), ((6.0, 1.0, -6.0), 0.25)]
    for k in range(40):
        if k < 4:
            c, r = dy[k]
        else:
            c, r = tuple(rng.uniform(-8.0, 8.0, 3)), float(rng.uniform(0.4, 1.3))
        out.append((b.sphere(c, r, (lam, met, die)[k % 3]), "sphere"))
    out.append((b.moving_sphere((-6.0, -5.0, 2.0), (-6.0, -3.0, 3.5), 0.9, b.lambertian((0.2, 0.6, 0.3))), "msphere"))
    out.append((b.quad((2.0, -7.0, -2.0), (3.0, 0.0, 0.5), (0.0, 2.5, 1.0), b.lambertian((0.4, 0.4, 0.8))), "quad"))
    out.append((b.triangle((-7.0, 3.0, -6.0), (-3.0, 4.0, -5.0), (-5.0, 7.0, -7.0), b.metal((0.9, 0.6, 0.2), 0.0)),
                "triangle"))
    cube = b.cube((0.0, 0.0, 0.0), (2.0, 1.5, 1.0), b.lambertian((0.9, 0.9, 0.1)))
    out.append((b.translate(b.rotate_y(cube, 18.0), (4.0, 3.0, 5.0)), "cube"))
    balls = [b.sphere((0.9 * (k % 3), 0.9 * (k // 3), 0.3 * k), 0.4, b.lambertian((0.1 + 0.1 * k, 0.5, 0.5)))
             for k in range(9)]
    out.append((b.translate(b.rotate_y(b.bvh(balls), 15.0), (-5.0, -7.0, -5.0)), "nested"))
    if media:
        out.append((b.medium_isotropic(b.sphere((1.0, -3.0, 6.0), 2.0, die), 0.6, (0.9, 0.9, 0.9)), "medium_sphere"))
        box = b.cube((0.0, 0.0, 0.0), (3.0, 2.0, 2.0), lam)
        out.append((b.medium_isotropic(b.translate(box, (-8.0, 4.0, 3.0)), 0.3, (0.2, 0.2, 0.2)), "medium_cube"))
    return out


def _spheres(b):
    rng = np.random.default_rng(12)
    m = [b.lambertian((0.5, 0.5, 0.5)), b.metal((0.7, 0.7, 0.7), 0.3)]
    return [(b.sphere(tuple(rng.uniform(-8.0, 8.0, 3)), float(rng.uniform(0.5, 1.5)), m[k % 2]), "sphere")
            for k in range(64)]


def _tiny(n):
    def build(b):
        cs = [((0.0, 0.0, 0.0), 1.0), ((3.0, 1.0, -2.0), 2.0), ((-4.0, -2.0, 3.0), 0.5)]
        return [(b.sphere(c, r, b.lambertian((0.3 * (k + 1), 0.5, 0.5))), "tiny%d" % k) for k, (c, r) in enumerate(cs[:n])]
    return build


def _fog(b):  # media without a nested tree: the GS_FEAT_MEDIA-only kernel
    out = [(b.sphere((2.0 * k - 7.0, 0.5 * k - 2.0, 1.0 - k), 0.8, b.lambertian((0.1 * k, 0.4, 0.6))), "sphere")
           for k in range(8)]
    out.append((b.medium_isotropic(b.sphere((0.0, 2.0, 3.0), 3.0, b.dielectric(1.5)), 0.4, (0.8, 0.8, 0.8)),
                "medium_sphere"))
    return out


# The compositions of tests/test_gpu_composition.py (GS_FEAT_GENERAL scenes), restated as worlds.
def _deep_chain(b, obj, depth):
    for k in range(depth):
        obj = b.rotate_y(obj, 7.0 + 11.0 * k) if k % 2 == 0 else b.translate(obj, (0.1 * k, 0.05, -0.07 * k))
    return obj


def _g_deep(depth):
    def build(b):
        red, white = b.lambertian((0.8, 0.2, 0.2)), b.lambertian((0.7, 0.7, 0.7))
        return [(_deep_chain(b, b.cube((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), red), depth), "deep_cube"),
                (_deep_chain(b, b.sphere((1.5, 0.5, 0.0), 0.5, b.metal((0.8, 0.8, 0.9), 0.1)), depth), "deep_sphere"),
                (b.sphere((0.0, -100.0, 0.0), 100.0, white), "ground")]
    return build


def _g_nested(what):
    def build(b):
        white, blue, m = b.lambertian((0.7, 0.7, 0.7)), b.lambertian((0.2, 0.3, 0.8)), b.lambertian((0.9, 0.5, 0.1))
        members = [b.sphere((-1.5 + 0.6 * k, 0.3, 0.2 * k), 0.25, blue) for k in range(6)]
        if what == "sphere":
            members += [b.translate(b.rotate_y(b.sphere((0.8, 0.6, 0.0), 0.5, b.metal((0.9, 0.9, 0.9), 0.0)), 30.0),
                                    (0.0, 0.2, 0.5))]
        elif what == "cube":
            members += [b.translate(b.rotate_y(b.cube((0.0, 0.0, 0.0), (0.8, 1.2, 0.8), m), -20.0), (0.5, 0.0, 0.3)),
                        b.rotate_y(b.cube((-1.2, 0.0, -0.4), (-0.6, 0.6, 0.2), b.dielectric(1.5)), 45.0)]
        elif what == "quad":
            members += [b.translate(b.quad((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.3), m), (0.3, 0.1, 0.6))]
        elif what == "medium":
            med = b.medium(b.cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m), 1.2, b.isotropic((0.8, 0.8, 0.8)))
            members += [b.translate(b.rotate_y(med, 15.0), (0.4, 0.0, 0.2))]
        else:
            members += [_deep_chain(b, b.sphere((0.5, 0.5, 0.5), 0.4, m), 7)]
        return [(b.translate(b.rotate_y(b.bvh(members), 25.0), (0.2, 0.0, -0.3)), "nested"),
                (b.sphere((0.0, -100.0, 0.0), 100.0, white), "ground"),
                (b.quad((-3.0, 4.0, -3.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), b.diffuse_light((3.0, 3.0, 3.0))), "light")]
    return build


def _g_bvh_boundary(chain):
    def build(b):
        glass, white = b.dielectric(1.5), b.lambertian((0.7, 0.7, 0.7))
        blobs = b.bvh([b.sphere((0.6 * k - 1.2, 0.2 * (k % 2), 0.1 * k), 0.5, glass) for k in range(5)] +
                      [b.cube((-0.5, -0.6, -0.5), (0.5, -0.2, 0.5), white)])
        boundary = b.translate(b.rotate_y(blobs, 20.0), (0.1, 0.2, 0.0)) if chain else blobs
        return [(b.medium(boundary, 0.8, b.isotropic((0.9, 0.6, 0.3))), "medium_bvh"),
                (b.sphere((0.0, -101.0, 0.0), 100.0, white), "ground"),
                (b.quad((-2.0, 3.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), b.diffuse_light((4.0, 4.0, 4.0))), "light")]
    return build


def _g_nested_media(b):
    glass, white = b.dielectric(1.5), b.lambertian((0.7, 0.7, 0.7))
    inner = b.medium(b.sphere((0.0, 0.0, 0.0), 1.2, glass), 1.5, b.isotropic((0.3, 0.8, 0.4)))
    return [(b.medium(inner, 0.7, b.lambertian((0.8, 0.3, 0.3))), "medium_medium"),
            (b.medium(b.translate(b.medium(b.cube((0, 0, 0), (1, 1, 1), white), 2.0, b.isotropic((0.9, 0.9, 0.9))),
                                  (1.4, -0.9, -0.8)), 0.9, b.isotropic((0.5, 0.5, 0.9))), "medium_medium2"),
            (b.sphere((0.0, -101.0, 0.0), 100.0, white), "ground"),
            (b.quad((-2.0, 3.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), b.diffuse_light((4.0, 4.0, 4.0))), "light")]


def _g_all(b):
    m, white = b.lambertian((0.9, 0.5, 0.1)), b.lambertian((0.7, 0.7, 0.7))
    inner = [b.translate(b.rotate_y(b.cube((0, 0, 0), (0.6, 0.9, 0.6), m), 30.0), (0.4, 0.0, 0.2))]
    return [(b.translate(b.rotate_y(b.bvh([b.sphere((-1.0 + 0.5 * k, 0.3, 0.0), 0.2, white) for k in range(4)] + inner),
                                    15.0), (-0.5, 0.0, 0.0)), "nested"),
            (b.medium(b.bvh([b.sphere((1.2, 0.4, 0.3 * k), 0.35, white) for k in range(3)]), 1.0,
                      b.isotropic((0.4, 0.7, 0.9))), "medium_bvh"),
            (_deep_chain(b, b.sphere((0.0, 1.4, -1.0), 0.4, b.metal((0.9, 0.9, 0.9), 0.2)), 6), "deep_sphere"),
            (b.sphere((0.0, -101.0, 0.0), 100.0, white), "ground")]


SCENES = {
    "mixed": lambda b: _mixed(b), "media": lambda b: _mixed(b, media=True), "spheres": _spheres,
    "tiny1": _tiny(1), "tiny2": _tiny(2), "tiny3": _tiny(3), "fog": _fog,
}
GENERAL = {
    "deep5": _g_deep(5), "deep9": _g_deep(9), "deep16": _g_deep(16),
    "nested_sphere": _g_nested("sphere"), "nested_cube": _g_nested("cube"), "nested_quad": _g_nested("quad"),
    "nested_medium": _g_nested("medium"), "nested_deep": _g_nested("deep"),
    "bvh_boundary": _g_bvh_boundary(False), "bvh_boundary_chain": _g_bvh_boundary(True),
    "nested_media": _g_nested_media, "general_all": _g_all,
}
# the kernel set each scene must launch (the MEDIA = 1 / NESTED = 2 / GENERAL = 512 bits of its feat)
FEAT_BITS = {"mixed": 2, "media": 3, "spheres": 0, "tiny1": 0, "tiny2": 0, "tiny3": 0, "fog": 1}


@functools.lru_cache(maxsize=None)
def scene(name):
    return QScene(name, SCENES[name] if name in SCENES else GENERAL[name])


# ----------------------------------------------------------------------------- rays
def _unit_rows(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def random_rays(name, n, seed):
    """n rays from a 24-unit box toward the scene, over (0.001, f64::MAX), times in [0, 1)."""
    rng = np.random.default_rng(seed)
    general = name in GENERAL
    half_o, half_t = (6.0, 2.5) if general else (12.0, {"tiny1": 1.2, "tiny2": 3.0, "tiny3": 4.0, "fog": 6.0}.get(name, 8.0))
    o = rng.uniform(-half_o, half_o, (n, 3))
    tgt = rng.uniform(-half_t, half_t, (n, 3))
    if general:
        o[:, 1] = np.abs(o[:, 1]) + 0.2  # (above the ground sphere)
        tgt[:, 1] = rng.uniform(-0.5, 2.0, n)
    a = np.empty((n, 9))
    a[:, 0:3], a[:, 3:6] = o, tgt - o
    a[:, 6], a[:, 7], a[:, 8] = rng.uniform(0.0, 1.0, n), 0.001, DMAX
    return a


def _ray(o, d, time=0.0, tmin=0.001, tmax=DMAX):
    return [*o, *d, time, tmin, tmax]


def special_rays(name):
    """The edge cases that need no answer to build: (rays [m, 9], tags [m])."""
    rows, tags = [], []

    def add(tag, *a, **k):
        rows.append(_ray(*a, **k))
        tags.append(tag)
    axes = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    inside = {"mixed": [(-4.0, 2.0, 1.0), (0.0, 5.0, -3.0), (3.0, -2.0, 4.0)], "tiny1": [(0.0, 0.0, 0.0)],
              "tiny2": [(0.0, 0.0, 0.0), (3.0, 1.0, -2.0)], "tiny3": [(0.0, 0.0, 0.0), (-4.0, -2.0, 3.0)],
              "fog": [(0.0, 2.0, 3.0), (-7.0, -2.0, 1.0)], "spheres": [(0.0, 0.0, 0.0)]}
    inside["media"] = inside["mixed"] + [(1.0, -3.0, 6.0), (1.5, -2.5, 6.5), (-6.5, 5.0, 4.0), (-7.0, 4.5, 3.5)]
    if name in ("mixed", "media"):  # inside the cube: Translate(RotateY(cube)) -- its centre taken back to the world
        s, c = np.sin(np.radians(18.0)), np.cos(np.radians(18.0))
        lx, ly, lz = 1.0, 0.75, 0.5
        inside[name] = inside[name] + [(c * lx + s * lz + 4.0, ly + 3.0, -s * lx + c * lz + 5.0)]
    rng = np.random.default_rng(5)
    for p in inside.get(name, []):
        for d in rng.normal(size=(6, 3)):
            add("inside", p, d, time=0.5)
        # axis-parallel directions, both signs of every zero component
        for ax in range(3):
            for sgn in (1.0, -1.0):
                for z1 in (0.0, -0.0):
                    for z2 in (0.0, -0.0):
                        d = [z1, z2]
                        d.insert(ax, sgn)
                        add("axis", p, d)
    # origins exactly on a box face of a dyadic sphere, directions along the face (0 * inf = NaN slabs)
    faces = {"mixed": ((-4.0, 2.0, 1.0), 1.0), "media": ((-4.0, 2.0, 1.0), 1.0), "tiny1": ((0.0, 0.0, 0.0), 1.0),
             "tiny2": ((0.0, 0.0, 0.0), 1.0), "tiny3": ((0.0, 0.0, 0.0), 1.0)}
    if name in faces:
        (cx, cy, cz), r = faces[name]
        for ax in range(3):
            for side in (-1.0, 1.0):
                o = [cx + 0.25 * r, cy - 0.5 * r, cz + 0.125 * r]
                o[ax] = (cx, cy, cz)[ax] + side * r
                for ax2 in range(3):
                    for sgn in (1.0, -1.0):
                        d = [0.0, 0.0, 0.0]
                        d[ax2] = sgn
                        add("face", o, d)
                        d2 = list(d)
                        d2[(ax2 + 1) % 3] = -0.0
                        add("face", o, d2)
                add("face", o, [-side if k == ax else 0.25 for k in range(3)])  # from the face into the box
    # malformed rays: accepted by contract, answered as the reference's arithmetic answers them
    nan, inf = float("nan"), float("inf")
    o0, d0 = (10.0, 9.0, 11.0), (-1.0, -0.9, -1.1)
    add("empty", o0, d0, tmin=5.0, tmax=1.0)
    add("empty", o0, d0, tmin=2.0, tmax=2.0)
    add("zero_dir", o0, (0.0, 0.0, 0.0))
    add("zero_dir", (0.0, 0.0, 0.0), (0.0, -0.0, 0.0))
    for bad in (nan, inf, -inf):
        for k in range(3):
            o, d = list(o0), list(d0)
            o[k] = bad
            add("bad_o", o, d0)
            d[k] = bad
            add("bad_d", o0, d)
        add("bad_iv", o0, d0, tmin=bad)
        add("bad_iv", o0, d0, tmax=bad)
        add("bad_iv", o0, d0, tmin=bad, tmax=bad)
    add("bad_all", (nan,) * 3, (nan,) * 3, time=nan, tmin=nan, tmax=nan)
    if name in ("mixed", "media"):  # the moving sphere at times 0, 1 and in between
        for time in (0.0, 0.25, 0.5, 1.0):
            c = np.array((-6.0, -5.0, 2.0)) + time * (np.array((-6.0, -3.0, 3.5)) - np.array((-6.0, -5.0, 2.0)))
            for off in ((0.0, 0.0, 0.0), (0.5, 0.3, 0.0), (0.0, 0.85, 0.0), (0.0, -0.85, 0.2)):
                o = np.array((-6.0, -4.0, 14.0))
                add("moving", o, c + np.array(off) - o, time=time)
    return np.array(rows, dtype=np.float64).reshape(-1, 9), tags


def seeds(n, first=0, seed=SEED):
    """s0 of rays first .. first + n - 1 of a batch."""
    return np.array([oracle.stream_seed(seed, first + i, 0) for i in range(n)], dtype=np.uint64)


def twin_hit(name, rays, s0):
    """The reference's world.hit of each ray: oracle.World(twin).hit(0, ...)."""
    w = oracle.World(scene(name).twin)
    try:
        return w.hit(np.zeros(len(rays), dtype=np.int32), rays[:, :7], rays[:, 7], rays[:, 8], s0)
    finally:
        w.close()


N_RANDOM = {"tiny1": 600, "tiny2": 600, "tiny3": 600, "fog": 1500}


@functools.lru_cache(maxsize=None)
def rays(name):
    """(rays [n, 9], tags [n]) of a scene: the random set first, the special rays, then -- for up to
    256 of the random set's hits -- tmax and tmin set to the twin's own t and to one ulp below and
    above it.  A ray's stream depends on its index, so the variants are built from the answers the
    random set gives at its own indices; their own answers (answers()) are computed at theirs."""
    n_rand = N_RANDOM.get(name, 400 if name in GENERAL else 4000)
    rnd = random_rays(name, n_rand, 100 + sorted(list(SCENES) + list(GENERAL)).index(name))
    sp, sp_tags = special_rays(name) if name in SCENES else (np.zeros((0, 9)), [])
    first = twin_hit(name, rnd, seeds(n_rand))
    idx = np.flatnonzero(first["hit"])[:256]
    rows, tags = [], []
    for i in idx:
        t = first["t"][i]
        for key, col in (("tmax", 8), ("tmin", 7)):
            for v in (t, np.nextafter(t, -np.inf), np.nextafter(t, np.inf)):
                r = rnd[i].copy()
                r[col] = v
                rows.append(r)
                tags.append(key)
    var = np.array(rows, dtype=np.float64).reshape(-1, 9)
    allr = np.ascontiguousarray(np.vstack([rnd, sp, var]))
    return allr, ["random"] * n_rand + list(sp_tags) + tags


@functools.lru_cache(maxsize=None)
def answers(name):
    r, _ = rays(name)
    return twin_hit(name, r, seeds(len(r)))


def fold(name, rays_, s0):
    """Brute force: World(spec).hit(k, ...) folded over the top-level objects in list order with a
    shrinking closest and one running stream.  NOT the reference's answer (module docstring): the
    host test shows that the two differ on some rays of `mixed` and `media`."""
    sc = scene(name)
    w = oracle.World(sc.spec)
    n = len(rays_)
    hit = np.zeros(n, dtype=bool)
    t = rays_[:, 8].copy()
    obj = np.full(n, -1)
    state = s0.copy()
    try:
        for k in range(len(sc.members)):
            h = w.hit(np.full(n, k, dtype=np.int32), rays_[:, :7], rays_[:, 7], t, state)
            state = h["state"]
            hit |= h["hit"]
            t = np.where(h["hit"], h["t"], t)
            obj = np.where(h["hit"], k, obj)
    finally:
        w.close()
    return {"hit": hit, "t": t, "obj": obj, "state": state}


# ----------------------------------------------------------------------------- which object was hit
def _prims(sc, h, level=0):
    """(kind, anchor, spec material) of every primitive under spec object h; a medium adds its own
    entry, keyed by the smallest anchor under its boundary."""
    kind, mat, first, count, p = sc.objects[h]
    if kind == N.GS_OBJ_SPHERE:
        return [("s", p[0:3], mat)]
    if kind == N.GS_OBJ_MOVING_SPHERE:
        return [("m", p[0:3], mat)]
    if kind == N.GS_OBJ_QUAD:
        return [("q", p[0:3], mat)]
    if kind == N.GS_OBJ_TRIANGLE:
        return [("t", p[0:3], mat)]
    if kind == N.GS_OBJ_CUBE:  # quad.rs:54-80
        mn = tuple(min(p[k], p[k + 3]) for k in range(3))
        mx = tuple(max(p[k], p[k + 3]) for k in range(3))
        qs = [(mn[0], mn[1], mx[2]), (mx[0], mn[1], mx[2]), (mx[0], mn[1], mn[2]), mn, (mn[0], mx[1], mx[2]), mn]
        return [("q", q, mat) for q in qs]
    if kind in (N.GS_OBJ_LIST, N.GS_OBJ_BVH):
        return [x for c in sc.children[first:first + count] for x in _prims(sc, c, level)]
    if kind in (N.GS_OBJ_TRANSLATE, N.GS_OBJ_ROTATE_Y):
        return _prims(sc, first, level)
    if kind == N.GS_OBJ_MEDIUM:
        inner = _prims(sc, first, level)
        return inner + [("v", min(a for k, a, _ in inner if k != "v"), mat)]
    raise ValueError(kind)


def material_map(sc, flat):
    """{flat material: spec material} through the primitives' anchors (a sphere's centre, a quad's q,
    a triangle's a, a medium's smallest boundary anchor), as the shading KAT matches leaves: the flat
    scene numbers materials as it meets them.  Anchors that two primitives of different materials
    share (the composition scenes reuse unit cubes) are left out."""
    from tests.shade_cases import Flat, REF_LIST, REF_MASK, REF_MEDIUM, REF_MSPHERE, REF_NODE, REF_QUAD, REF_SHIFT, \
        REF_SPHERE, REF_TRI
    F = Flat(flat, index=False)
    spec = {}
    for h in sc.members:
        for kind, a, m in _prims(sc, h):
            spec.setdefault((kind, tuple(a)), set()).add(m)
    fl = {}
    for i in range(flat.n_spheres):
        fl.setdefault(("s", tuple(F.sph[i].center)), set()).add(F.sph[i].material)
    for i in range(flat.n_mspheres):
        fl.setdefault(("m", tuple(F.msph[i].center_start)), set()).add(F.msph[i].material)
    for i in range(flat.n_quads):
        fl.setdefault(("q", tuple(F.quads[i].q)), set()).add(F.quads[i].material)
    for i in range(flat.n_triangles):
        fl.setdefault(("t", tuple(F.tris[i].a)), set()).add(F.tris[i].material)

    def anchors(ref):
        _, end = F.chain(ref)
        kind, i = end >> REF_SHIFT, end & REF_MASK
        if kind == REF_LIST:
            return [a for x in F.members(end) for a in anchors(x)]
        if kind == REF_NODE:
            return [a for x in F.tree_leaves(end) for a in anchors(x)]
        if kind == REF_MEDIUM:
            return anchors(F.media[i].boundary)
        return [tuple({REF_SPHERE: lambda: F.sph[i].center, REF_MSPHERE: lambda: F.msph[i].center_start,
                       REF_QUAD: lambda: F.quads[i].q, REF_TRI: lambda: F.tris[i].a}[kind]())]
    for i in range(flat.n_media):
        fl.setdefault(("v", min(anchors(F.media[i].boundary))), set()).add(F.media[i].material)
    out = {}
    for key, fm in fl.items():
        sm = spec.get(key, set())
        if len(sm) == 1 and len(fm) == 1:
            f, s = next(iter(fm)), next(iter(sm))
            assert out.get(f, s) == s, "one flat material, two spec materials"
            out[f] = s
    return out


def hit_label(sc, ans):
    """Per ray of `ans` (a twin answer): the label of the top-level member whose material was hit, or
    None -- by spec material (each label's own materials; shared sphere materials count as 'sphere')."""
    by_mat = {}
    for h, label in sc.tags:
        if sc.objects[h][0] == N.GS_OBJ_MEDIUM:  # (its boundary's material is never a hit's)
            by_mat.setdefault(sc.objects[h][1], set()).add(label)
            continue
        for _, _, m in _prims(sc, h):
            by_mat.setdefault(m, set()).add(label)
    return [sorted(by_mat.get(int(m), {"?"}))[0] if hit else None for hit, m in zip(ans["hit"], ans["mat"])]
