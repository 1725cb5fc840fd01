"""Scenes and cases of the shading known-answer tests (tests/test_shade_cases_host.py on the
CPU, tests/test_gpu_shading_kat.py on the device): what runs after a hit is accepted -- the
HitRecord, the textures, Material::emitted / scatter -- and the miss path.

Every scene gives each object a material of its own and keeps its objects far apart; a case is
one ray aimed at one object (or a miss lane, k = -1), a ray time and a stream state.  The
oracle answers each case with that object's own `hit`, then `emitted` and `scatter`
(oracle.World.bounce); the device is handed the oracle's t and the leaf the flat scene holds
for that object.  Everything is drawn from one fixed seed.
"""
import ctypes as C
import functools
import math

import numpy as np

import grayshift_amd as g
from grayshift_amd import _native as N

import oracle

SEED = 0x5EED5AD3
PI = math.pi
LAUNCH = 4096  # cases per harness launch, at most

REF_SHIFT, REF_MASK = 28, 0x0FFFFFFF
REF_NONE, REF_NODE, REF_SPHERE, REF_MSPHERE, REF_QUAD, REF_TRI, REF_LIST, REF_INST, REF_MEDIUM = range(9)


def _records(ptr, T):
    return C.cast(ptr, C.POINTER(T))


class gs_list(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32)]


class Flat:
    """The flat scene's records and (index) its top-level leaves by key = (media levels, anchor).
    anchor: a primitive's first point (a sphere's centre, a quad's q, a triangle's a); a HittableList's
    is its first member's, a BVH's the smallest of its leaves', a medium's its boundary's, one level
    more.  It matches a leaf to its spec object; the material index cannot, alone: the flat scene
    numbers materials as it meets them (a medium's boundary has one too), not as the spec does."""

    def __init__(self, flat, index=True):
        self.flat = flat
        self.nodes, self.inst = _records(flat.nodes, N.gs_node), _records(flat.instances, N.gs_instance)
        self.sph, self.msph = _records(flat.spheres, N.gs_sphere), _records(flat.mspheres, N.gs_msphere)
        self.quads, self.tris = _records(flat.quads, N.gs_quad), _records(flat.triangles, N.gs_triangle)
        self.media = _records(flat.media, N.gs_medium_rec)
        self.lists, self.list_refs = _records(flat.lists, gs_list), _records(flat.list_refs, C.c_uint32)
        self.leaves = {}
        if index:
            self._walk(flat.root)

    def _walk(self, ref):
        if ref == REF_NONE:
            return
        if (ref >> REF_SHIFT) == REF_NODE:
            n = self.nodes[ref & REF_MASK]
            self._walk(n.left)
            self._walk(n.right)
            return
        key = self.key(ref)
        assert key not in self.leaves, "two leaves share the key %r" % (key,)
        self.leaves[key] = ref

    def chain(self, ref):
        """The instance records of a chain, outermost first, and the ref it ends in."""
        recs = []
        while (ref >> REF_SHIFT) == REF_INST:
            recs.append(self.inst[ref & REF_MASK])
            ref = recs[-1].child
        return recs, ref

    def members(self, ref):
        l = self.lists[ref & REF_MASK]
        return [self.list_refs[l.first + j] for j in range(l.count)]

    def tree_leaves(self, ref):
        if (ref >> REF_SHIFT) != REF_NODE:
            return [ref]
        n = self.nodes[ref & REF_MASK]
        return self.tree_leaves(n.left) + (self.tree_leaves(n.right) if n.right != REF_NONE else [])

    def key(self, ref):
        _, end = self.chain(ref)
        kind, i = end >> REF_SHIFT, end & REF_MASK
        if kind == REF_SPHERE:
            return 0, tuple(self.sph[i].center)
        if kind == REF_MSPHERE:
            return 0, tuple(self.msph[i].center_start)
        if kind == REF_QUAD:
            return 0, tuple(self.quads[i].q)
        if kind == REF_TRI:
            return 0, tuple(self.tris[i].a)
        if kind == REF_LIST:
            return self.key(self.members(end)[0])
        if kind == REF_NODE:
            return 0, min(self.key(x)[1] for x in self.tree_leaves(end))
        if kind == REF_MEDIUM:
            lv, a = self.key(self.media[i].boundary)
            return lv + 1, a
        raise ValueError("leaf kind %d is not part of these scenes" % kind)

    def materials(self, ref):
        """The flat materials a hit of this leaf can carry, in member order."""
        _, end = self.chain(ref)
        kind, i = end >> REF_SHIFT, end & REF_MASK
        if kind == REF_LIST:
            return [m for x in self.members(end) for m in self.materials(x)]
        if kind == REF_NODE:
            return []
        return [{REF_SPHERE: self.sph, REF_MSPHERE: self.msph, REF_QUAD: self.quads, REF_TRI: self.tris,
                 REF_MEDIUM: self.media}[kind][i].material]

    def forward(self, ref, o, d):
        """A ray through the leaf's chain as Translate::hit / RotateY::hit transform it
        (hittable.rs:107-113, 179-193), in their operations' order; o, d: [n, 3].  (o, d, end ref)."""
        recs, end = self.chain(ref)
        o, d = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)
        for rec in recs:
            if rec.kind == 1:  # GS_INST_TRANSLATE
                o = o - np.array(rec.p[:])
            else:
                s, c = rec.p[0], rec.p[1]
                o = np.stack([(c * o[:, 0]) - (s * o[:, 2]), o[:, 1], (s * o[:, 0]) + (c * o[:, 2])], -1)
                d = np.stack([(c * d[:, 0]) - (s * d[:, 2]), d[:, 1], (s * d[:, 0]) + (c * d[:, 2])], -1)
        return o, d, end


def flat_leaves(flat):
    """The flat tree's leaves as {anchor: (hit_ref, hit_inst, hit_outer, material)}: the
    primitive (or medium) at the end of the leaf's chain and the refs a hit on it carries --
    its own chain, and for a chain inside a BVH under a chain that BVH's chain too (a plain
    member of such a BVH carries the BVH's chain as its own).  anchor: Flat's."""
    F = Flat(flat, index=False)
    out = {}

    def walk(ref, outer):
        if ref == REF_NONE:
            return
        if (ref >> REF_SHIFT) == REF_NODE:
            n = F.nodes[ref & REF_MASK]
            walk(n.left, outer)
            walk(n.right, outer)
            return
        _, end = F.chain(ref)
        chain = ref if (ref >> REF_SHIFT) == REF_INST else REF_NONE
        if (end >> REF_SHIFT) == REF_NODE:
            assert outer == REF_NONE
            walk(end, ref)
            return
        a, m = F.key(end)[1], F.materials(end)[0]
        assert a not in out, "two leaves share an anchor"
        if outer != REF_NONE and chain != REF_NONE:
            out[a] = (end, chain, outer, m)
        elif outer != REF_NONE:
            out[a] = (end, outer, REF_NONE, m)
        else:
            out[a] = (end, chain, REF_NONE, m)

    walk(flat.root, REF_NONE)
    return out


def flat_textures(spec, flat, spec_mat, flat_mat):
    """{spec texture index: flat texture index} of the texture tree under a material."""
    ft, fm = _records(flat.textures, N.gs_texture), _records(flat.materials, N.gs_material)
    out = {}

    def walk(s, f):
        out[s] = f
        t = spec.textures[s]
        assert t.kind == ft[f].kind
        if t.kind == N.GS_TEX_CHECKERED:
            walk(t.a, ft[f].even)
            walk(t.b, ft[f].odd)

    walk(spec.materials[spec_mat].texture, fm[flat_mat].texture)
    return out


# ------------------------------------------------------------------------------ geometry
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _perp(rng, nrm):
    a = rng.normal(size=nrm.shape)
    a -= (a * nrm).sum(-1, keepdims=True) * nrm
    return _unit(a)


def _roty(p, deg):  # RotateY's back-transform of a point (hittable.rs:196-209)
    rad = deg / 180.0 * PI
    s, c = math.sin(rad), math.cos(rad)
    return np.stack([c * p[..., 0] + s * p[..., 2], p[..., 1], -s * p[..., 0] + c * p[..., 2]], -1)


def to_world(chain, p):
    """A local point through a chain of ("t", offset) / ("r", degrees), innermost first."""
    p = np.asarray(p, dtype=np.float64)
    for kind, a in chain:
        p = p + np.asarray(a) if kind == "t" else _roty(p, a)
    return p


class Obj:
    """One top-level object: kind 'sphere' | 'msphere' | 'quad' | 'tri' | 'medium', its spec
    material, what it is for (a label), its anchor (flat_leaves) and its geometry in world
    space (c, r; q, u, v; a, b, c): the instance chains are applied, approximately -- it only
    aims the rays."""

    def __init__(self, kind, mat, label, anchor, **geo):
        self.kind, self.mat, self.label, self.anchor = kind, mat, label, tuple(float(x) for x in anchor)
        self.__dict__.update(geo)


class ShadeScene:
    def __init__(self, name, builder, objs, extra=None):
        self.name = name
        self.spec = builder.build()
        self.objs = objs
        self.extra = extra or {}
        assert self.spec.n_world >= len(objs)
        mats = [o.mat for o in objs]
        assert len(set(mats)) == len(mats), "every object has a material of its own"


def _image_5x3():
    k = np.arange(15, dtype=np.uint32).reshape(3, 5)
    return np.stack([10 + 16 * k, 255 - 13 * k, (k * 37) % 256], -1).astype(np.uint8)  # every texel its own colour


def _wrap(b, obj, steps):
    """steps: ("t", offset) / ("r", degrees), innermost first."""
    for kind, a in steps:
        obj = b.translate(obj, a) if kind == "t" else b.rotate_y(obj, a)
    return obj


def _add_sphere(b, objs, k, mat, label, r=1.0, c=None):
    c = (100.0 * k, 0.0, 0.0) if c is None else c
    b.add(b.sphere(c, r, mat))
    objs.append(Obj("sphere", mat, label, c, c=np.array(c, dtype=np.float64), r=r))


def scene_mixed():
    b = g.SceneBuilder()
    objs = []
    img = b.image(_image_5x3())
    t_img = b.image_texture(img)
    t_tree = b.checkered(0.37, b.checkered(0.11, t_img, b.solid((0.9, 0.1, 0.2))), b.solid((0.1, 0.8, 0.3)))
    mats = [
        (b.lambertian((0.8, 0.3, 0.2)), "lamb_solid"),
        (b.lambertian_texture(b.checkered_from_colors(0.32, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), "lamb_checker"),
        (b.lambertian_texture(t_tree), "lamb_tree"),
        (b.lambertian_texture(b.noise(4.0)), "lamb_noise"),
        (b.lambertian_texture(t_img), "lamb_image"),
        (b.metal((0.8, 0.8, 0.9), 0.0), "metal_0"),
        (b.metal((0.7, 0.6, 0.5), 0.3), "metal_03"),
        (b.metal((0.9, 0.5, 0.4), 1.0), "metal_1"),
        (b.dielectric(1.5), "diel_15"),
        (b.dielectric(1.0 / 1.5), "diel_inv"),
        (b.dielectric(2.4), "diel_24"),
        (b.diffuse_light((4.0, 3.0, 2.0)), "light_solid"),
        (b._mat(N.GS_MAT_DIFFUSE_LIGHT, t_img), "light_image"),
    ]
    for k, (m, label) in enumerate(mats):
        _add_sphere(b, objs, k, m, label)
    k = len(objs)
    c1, c2 = (100.0 * k, 0.0, 0.0), (100.0 * k + 0.5, 0.7, -0.3)
    m = b.lambertian((0.3, 0.4, 0.5))
    b.add(b.moving_sphere(c1, c2, 1.0, m))
    objs.append(Obj("msphere", m, "moving", c1, c=np.array(c1), c2=np.array(c2), r=1.0))
    k += 1
    q, u, v = (100.0 * k - 1.0, -1.0, 0.0), (2.0, 0.0, 0.3), (0.0, 2.0, 0.2)
    m = b.lambertian_texture(t_img)
    b.add(b.quad(q, u, v, m))
    objs.append(Obj("quad", m, "quad", q, q=np.array(q), u=np.array(u), v=np.array(v)))
    k += 1
    ta, tb, tc = (100.0 * k - 1.0, -1.0, 0.1), (100.0 * k + 1.0, -0.8, 0.0), (100.0 * k, 1.2, -0.2)
    m = b.lambertian_texture(t_img)
    b.add(b.triangle(ta, tb, tc, m))
    objs.append(Obj("tri", m, "tri", ta, a=np.array(ta), b=np.array(tb), c=np.array(tc)))
    k += 1
    q, u, v = (-1.0, -1.0, 0.25), (2.0, 0.1, 0.0), (0.0, 2.0, 0.4)
    chain = [("r", 30.0), ("t", (100.0 * k, 0.5, -0.25))]
    m = b.metal((0.6, 0.7, 0.8), 0.1)
    b.add(_wrap(b, b.quad(q, u, v, m), chain))
    objs.append(Obj("quad", m, "quad_chain", q, q=to_world(chain, q), u=_roty(np.array(u), 30.0),
                    v=_roty(np.array(v), 30.0)))
    for label, phase in (("medium_solid", b.isotropic((0.7, 0.8, 0.9))),
                         ("medium_tex", b.isotropic_texture(b.checkered_from_colors(0.41, (0.9, 0.2, 0.2),
                                                                                      (0.2, 0.2, 0.9))))):
        k += 1
        c = (100.0 * k, 0.0, 0.0)
        b.add(b.medium(b.sphere(c, 2.0, b.lambertian((0.5, 0.5, 0.5))), 1.5, phase))
        objs.append(Obj("medium", phase, label, c, c=np.array(c), r=2.0))
    b.background_solid((0.25, 0.5, 0.75))
    return ShadeScene("mixed", b, objs)


def scene_spheres(uv):
    b = g.SceneBuilder()
    objs = []
    mats = [(b.lambertian((0.8, 0.3, 0.2)), "lamb_solid"),
            (b.lambertian_texture(b.checkered_from_colors(0.32, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), "lamb_checker"),
            (b.metal((0.8, 0.8, 0.9), 0.0), "metal_0"), (b.metal((0.9, 0.5, 0.4), 1.0), "metal_1"),
            (b.dielectric(1.5), "diel_15"), (b.dielectric(2.4), "diel_24")]
    if uv:
        mats += [(b.lambertian_texture(b.image_texture(b.image(_image_5x3()))), "lamb_image"),
                 (b.lambertian_texture(b.noise(2.5)), "lamb_noise"), (b.diffuse_light((4.0, 3.0, 2.0)), "light_solid")]
    for k, (m, label) in enumerate(mats):
        _add_sphere(b, objs, k, m, label, r=1.0 if k == 0 else 0.5 + 0.25 * (k % 3))
    b.background_solid((0.7, 0.8, 1.0))
    return ShadeScene("spheres_uv" if uv else "spheres_plain", b, objs)


def _alternating(depth, k0=0):
    return [("r", 7.0 + 11.0 * (k + k0)) if (k + k0) % 2 == 0 else ("t", (0.1 * (k + 1), 0.05, -0.07 * (k + 1)))
            for k in range(depth)]


def scene_deep():
    b = g.SceneBuilder()
    objs = []
    img_mat = lambda: b.lambertian_texture(b.image_texture(b.image(_image_5x3())))  # noqa: E731
    k = 0
    for depth in (1, 4, 5, 6):  # 4: the last chain reconstruct keeps in registers; 5: the first it re-walks
        chain = _alternating(depth - 1) + [("t", (100.0 * k, 0.0, 0.0))]  # depth instances in all
        m = img_mat() if depth != 4 else b.metal((0.8, 0.8, 0.9), 0.2)
        c = (1.0 + k, 0.25, -0.5)  # (an anchor of its own)
        b.add(_wrap(b, b.sphere(c, 1.0, m), chain))
        objs.append(Obj("sphere", m, "chain%d" % depth, c, c=to_world(chain, c), r=1.0))
        k += 1
    # a sphere under a chain of 3, in a BVH (with a member no ray reaches) under a chain of 2
    inner, outer = _alternating(3, 1), [("r", 25.0), ("t", (100.0 * k, 0.0, -0.3))]
    c, m = (0.5, 0.5, 0.75), img_mat()
    far = b.sphere((0.0, 5000.0, 0.0), 1.0, b.lambertian((0.1, 0.1, 0.1)))
    b.add(_wrap(b, b.bvh([_wrap(b, b.sphere(c, 1.0, m), inner), far]), outer))
    objs.append(Obj("sphere", m, "chain3_in_bvh_chain2", c, c=to_world(inner + outer, c), r=1.0))
    k += 1
    # a plain member of a BVH under a chain of 2 (the hit carries the BVH's chain)
    outer = [("t", (0.25, 0.0, 0.5)), ("r", -40.0), ("t", (100.0 * k, 0.0, 0.0))]
    c, m = (-0.5, 0.25, 0.0), b.dielectric(1.5)
    far = b.sphere((0.0, 6000.0, 0.0), 1.0, b.lambertian((0.2, 0.1, 0.1)))
    b.add(_wrap(b, b.bvh([b.sphere(c, 1.0, m), far]), outer))
    objs.append(Obj("sphere", m, "plain_in_bvh_chain3", c, c=to_world(outer, c), r=1.0))
    k += 1
    _add_sphere(b, objs, k, b.lambertian((0.6, 0.6, 0.6)), "lamb_solid")
    b.background_solid((0.4, 0.5, 0.6))
    return ShadeScene("deep", b, objs)


SKY_W, SKY_H = 16, 8
SKY_ROT = (0.3, -0.7, 1.1)


def sky_texels(f32):
    """16 x 8 texels m * 2^(e - 136) with byte mantissas (the largest >= 128): each one
    round-trips through RGBE8; every 17th is black (RGBE's e == 0).  f32: one texel that
    does not round-trip."""
    k = np.arange(SKY_W * SKY_H)
    m = np.stack([128 + (5 * k) % 128, (37 * k) % 256, (91 * k) % 256], -1).astype(np.float64)
    exact = m * np.exp2((118 + k % 24) - 136.0)[:, None]
    exact[k % 17 == 3] = 0.0
    a = exact.astype(np.float32).reshape(SKY_H, SKY_W, 3)
    assert np.array_equal(a.astype(np.float64).reshape(-1, 3), exact)
    if f32:
        a[3, 5] = (0.1, 0.2, 0.3)
    return a


def scene_sky(f32):
    b = g.SceneBuilder()
    objs = []
    for k, (m, label) in enumerate([(b.lambertian((0.8, 0.3, 0.2)), "lamb_solid"), (b.metal((0.8, 0.8, 0.9), 0.3), "metal_03"),
                                    (b.dielectric(1.5), "diel_15")]):
        _add_sphere(b, objs, k, m, label)
    tex = sky_texels(f32)
    b.background_hdri(tex, SKY_ROT)
    return ShadeScene("sky_f32" if f32 else "sky_rgbe", b, objs, {"hdri": tex})


SCENES = {"mixed": scene_mixed, "spheres_uv": lambda: scene_spheres(True), "spheres_plain": lambda: scene_spheres(False),
          "deep": scene_deep, "sky_rgbe": lambda: scene_sky(False), "sky_f32": lambda: scene_sky(True)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


# --------------------------------------------------------------------------------- cases
class _Cases:
    def __init__(self):
        self.k, self.o, self.d, self.tag, self.time = [], [], [], [], []

    def add(self, k, o, d, tag, time=None):
        """time: the rays' times (default: drawn later, uniform in [0, 1))."""
        o, d = np.atleast_2d(np.asarray(o, dtype=np.float64)), np.atleast_2d(np.asarray(d, dtype=np.float64))
        assert o.shape == d.shape
        self.time.append(np.full(len(o), np.nan) if time is None else np.asarray(time, dtype=np.float64))
        self.k.append(np.full(len(o), k, dtype=np.int32))
        self.o.append(o)
        self.d.append(d)
        self.tag += [tag] * len(o)


def _scaled(rng, d):
    """The reference's rays are not unit: a random length per ray."""
    return d * rng.uniform(0.25, 4.0, (len(d), 1))


def _aim_sphere(rng, c, r, n):
    o = c + r * rng.uniform(1.5, 4.0, (n, 1)) * _dirs(rng, n)
    t = c + 0.97 * r * rng.random((n, 1)) ** (1.0 / 3.0) * _dirs(rng, n)
    return o, _scaled(rng, t - o)


def _inside_sphere(rng, c, r, n):
    o = c + 0.6 * r * rng.random((n, 1)) ** (1.0 / 3.0) * _dirs(rng, n)
    return o, _scaled(rng, _dirs(rng, n))


def _at_angle(rng, c, r, nrm, theta, leaving, scale=True):
    """Rays that meet the sphere at c + r nrm under angle theta to the normal: from outside, or
    (leaving) from inside, the origin halfway along the chord."""
    tan = _perp(rng, nrm)
    ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
    d = (ct * nrm if leaving else -ct * nrm) + st * tan
    p = c + r * nrm
    length = r * np.maximum(ct, 0.02) if leaving else r * rng.uniform(0.5, 3.0, (len(nrm), 1))
    o = p - length * d
    return o, (_scaled(rng, d) if scale else d)


def _sphere_cases(cs, rng, k, ob, n_rand=96, n_in=32):
    """Rays from outside at points all over the sphere, and rays from inside it."""
    for n, aim, tag in ((n_rand, _aim_sphere, "rand"), (n_in, _inside_sphere, "inside")):
        time = rng.random(n)
        # (a moving sphere: its centre at the ray's time, sphere.rs:51-53)
        c = ob.c + time[:, None] * (ob.c2 - ob.c) if ob.kind == "msphere" else ob.c
        o, d = aim(rng, c, ob.r, n)
        cs.add(k, o, d, tag, time)


def _uv_cases(cs, rng, k, ob, exact):
    """sphere_uv's edges.  Points 1e-8 .. 1e-3 rad off the seam and off the poles; and (exact)
    both poles themselves, the seam atan2(-0.0, -1) against atan2(+0.0, -1) (u = 0 and u = 1),
    and points down to 1e-15 rad off them: texel choices on or within 1e-9 of a texel boundary,
    few enough to stay under 1% of the scene's image texels.  (The sphere's centre has z = +0.0.)"""
    c, r = ob.c, ob.r
    assert c[2] == 0.0 and not np.signbit(c[2])
    for lo, hi, n, tag in ((-8, -3, 24, "near"), (-15, -10, 4, "tiny")):
        if tag == "tiny" and not exact:
            continue
        eps = 10.0 ** rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)
        nrm = _unit(np.stack([-np.ones(n), rng.normal(size=n) * 1e-3, eps], -1))   # next to the seam
        o, d = _at_angle(rng, c, r, nrm, np.zeros(n), False)
        cs.add(k, o, d, tag + "_seam")
        nrm = _unit(np.stack([eps, rng.choice([-1.0, 1.0], n), rng.normal(size=n) * 1e-6], -1))  # next to a pole
        o, d = _at_angle(rng, c, r, nrm, np.zeros(n), False)
        cs.add(k, o, d, tag + "_pole")
    if not exact:
        return
    for s in (1.0, -1.0):  # the poles, from outside and from inside
        cs.add(k, c + (0.0, 3.0 * s * r, 0.0), (0.0, -s, 0.0), "pole")
        cs.add(k, c + (0.0, 0.5 * s * r, 0.0), (0.0, s * 2.0, 0.0), "pole")
    for z in (0.0, -0.0):  # the seam: the hit point's z is the origin's and the direction's zero
        for x, dx in ((-3.0 * r, 1.0), (-0.5 * r, -0.5)):
            o = c + (x, 0.0, 0.0)
            o[2] = z  # (c.z + -0.0 would be +0.0)
            cs.add(k, o, (dx, 0.0, z), "seam")


def dielectric_terms(d, n, front, ri):
    """Dielectric::scatter's ri, unit direction, cos(theta), sin(theta) and the unclamped
    cosine (material.rs:123-131), in its operations' order."""
    ri_eff = np.where(front, 1.0 / ri, ri)
    ud = unit3(d)
    raw = dot3(-ud, n)
    cos = np.minimum(raw, 1.0)
    return ri_eff, ud, cos, np.sqrt(1.0 - cos * cos), raw


def _dielectric_cases(cs, rng, k, ob, ri, wd, n_tir=600):
    """Incidence at total internal reflection, entering and leaving: rays at the critical
    angle, kept where the reference's own ri sin(theta) -- from the normal its hit computes --
    lands within 8 ulps of 1 (either side), and some of the others; normal incidence (the
    cos(theta) min clamp); grazing incidence (Schlick's (1 - cos)^5 near 1)."""
    for leaving in (False, True):
        ri_eff = ri if leaving else 1.0 / ri
        tag = "leave" if leaving else "enter"
        if ri_eff > 1.0:
            m = 24 * n_tir
            theta = np.full(m, math.asin(1.0 / ri_eff))
            o, d = _at_angle(rng, ob.c, ob.r, _dirs(rng, m), theta, leaving)
            a = wd.bounce(np.full(m, k), np.column_stack([o, d, np.zeros(m)]), np.zeros(m, dtype=np.uint64))
            r, _, _, sin, _ = dielectric_terms(d, a["n"], a["front"], ri)
            val = r * sin
            near = a["hit"] & (np.abs(val - 1.0) <= 8 * 2.0 ** -52)
            keep = np.concatenate([np.flatnonzero(near & (val > 1.0))[:n_tir // 3],
                                   np.flatnonzero(near & ~(val > 1.0))[:n_tir // 3], np.flatnonzero(~near)[:n_tir // 3]])
            cs.add(k, o[keep], d[keep], "tir_" + tag)
        n = 24
        nrm = np.vstack([np.eye(3), -np.eye(3), _dirs(rng, n - 6)])
        o, d = _at_angle(rng, ob.c, ob.r, nrm, np.zeros(n), leaving, scale=False)
        cs.add(k, o, d, "normal_" + tag)
        o, d = _at_angle(rng, ob.c, ob.r, nrm, np.zeros(n), leaving)
        cs.add(k, o, d, "normal_" + tag)
        n = 48
        theta = PI / 2 - 10.0 ** rng.uniform(-9 if not leaving else -1.5, -0.5, n)
        o, d = _at_angle(rng, ob.c, ob.r, _dirs(rng, n), theta, leaving)
        cs.add(k, o, d, "graze_" + tag)


def _metal_cases(cs, rng, k, ob, n):
    """Grazing reflections: with fuzz the reflected ray ends on either side of the surface."""
    theta = PI / 2 - 10.0 ** rng.uniform(-4, -0.3, n)
    o, d = _at_angle(rng, ob.c, ob.r, _dirs(rng, n), theta, False)
    cs.add(k, o, d, "graze")


def _onb_cases(cs, rng, k, ob, n=420):
    """Normals with |w.x| at 0.9 and an ulp or two either side (the ONB's axis switch) and at
    +-1, front faces and back faces.  (The sphere is the unit sphere at the origin.)"""
    assert np.all(ob.c == 0.0) and ob.r == 1.0
    for sign in (1.0, -1.0):
        for leaving in (False, True):
            x = sign * (0.9 + rng.integers(-4, 5, n) * 2.0 ** -53)
            phi = rng.uniform(0, 2 * PI, n)
            rad = np.sqrt(1.0 - x * x)
            nrm = np.stack([x, rad * np.cos(phi), rad * np.sin(phi)], -1)
            theta = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0, 1.2, n))
            o, d = _at_angle(rng, ob.c, ob.r, nrm, theta, leaving, scale=False)
            cs.add(k, o, d, "onb")
        cs.add(k, (3.0 * sign, 0.0, 0.0), (-sign, 0.0, 0.0), "axis")      # n = (+-1, 0, 0) exactly
        cs.add(k, (0.5 * sign, 0.0, 0.0), (0.5 * sign, 0.0, 0.0), "axis")  # ... and a back face
        cs.add(k, (3.0 * sign, 0.0, -0.0), (-2.0 * sign, -0.0, 0.0), "axis")


def _quad_cases(cs, rng, k, ob, n=160):
    ab = rng.uniform(-0.01, 1.01, (n, 2))
    t = ob.q + ab[:, :1] * ob.u + ab[:, 1:] * ob.v
    nrm = _unit(np.cross(ob.u, ob.v))
    o = t + nrm * rng.uniform(0.5, 3.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1)) + rng.normal(size=(n, 3))
    cs.add(k, o, _scaled(rng, t - o), "rand")


def _tri_cases(cs, rng, k, ob, n=160):
    w = rng.dirichlet((1.0, 1.0, 1.0), n) * 1.06 - 0.02
    t = w[:, :1] * ob.a + w[:, 1:2] * ob.b + w[:, 2:] * ob.c
    nrm = _unit(np.cross(ob.b - ob.a, ob.c - ob.a))
    side = np.where(rng.random((n, 1)) < 0.96, -1.0, 1.0)  # (Triangle::hit culls rays against its normal)
    o = t + nrm * rng.uniform(0.5, 3.0, (n, 1)) * side + 0.5 * rng.normal(size=(n, 3))
    cs.add(k, o, _scaled(rng, t - o), "rand")


def _medium_cases(cs, rng, k, ob, n=160):
    o = ob.c + ob.r * rng.uniform(1.5, 3.0, (n, 1)) * _dirs(rng, n)
    t = ob.c + 0.6 * ob.r * rng.random((n, 1)) ** (1.0 / 3.0) * _dirs(rng, n)
    cs.add(k, o, _scaled(rng, t - o), "rand")
    o = ob.c + 0.5 * ob.r * _dirs(rng, n // 4)  # from inside the boundary
    cs.add(k, o, _scaled(rng, _dirs(rng, n // 4)), "inside")


def _sky_dirs(rng):
    """Directions whose rotated form falls into every texel, next to column and row boundaries
    (1e-8 .. 1e-4 rad off), at the poles and at the seam theta = +-pi."""
    sx, sy, sz = (math.sin(a) for a in SKY_ROT)
    cx, cy, cz = (math.cos(a) for a in SKY_ROT)
    R = np.array([[cy * cz, cx * sz + sx * sy * cz, sx * sz - cx * sy * cz],
                  [-cy * sz, cx * cz - sx * sy * sz, sx * cz + cx * sy * sz],
                  [sy, -sx * cy, cx * cy]])  # rotate_vector (util.rs:67-86)
    xs, ys = np.meshgrid(np.arange(SKY_W), np.arange(SKY_H))
    xs, ys = np.tile(xs.ravel(), 8), np.tile(ys.ravel(), 8)
    n = len(xs)
    u, v = (xs + rng.uniform(0.02, 0.98, n)) / SKY_W, (ys + rng.uniform(0.02, 0.98, n)) / SKY_H
    m = 384
    delta = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-8, -4, m)
    u[:m // 2] = rng.integers(0, SKY_W + 1, m // 2) / SKY_W + delta[:m // 2] / (2 * PI)
    v[m // 2:m] = rng.integers(1, SKY_H, m // 2) / SKY_H + delta[m // 2:] / PI
    theta, phi = 2 * PI * (u - 0.5), PI * (0.5 - v)
    rot = np.stack([np.cos(phi) * np.cos(theta), np.cos(phi) * np.sin(theta), np.sin(phi)], -1)
    rot = np.vstack([rot, [(0, 0, 1), (0, 0, -1), (-1, 0.0, 0), (-1, -0.0, 0), (-1, 1e-12, 0), (-1, -1e-12, 0), (1, 0, 0),
                           (0, 1, 0), (0, -1, 0)]])
    return _scaled(rng, rot @ R)  # (R is orthogonal: rot = R d  <=>  d = R^T rot)


def _interleave(k):
    """An order in which every object's cases are spread evenly over the whole list, so each
    run of 64 holds every kind of lane."""
    pos = np.zeros(len(k))
    for v in np.unique(k):
        idx = np.flatnonzero(k == v)
        pos[idx] = (np.arange(len(idx)) + 0.5) / len(idx)
    return np.argsort(pos, kind="stable")


MORE_RAYS = {("mixed", "lamb_image"): 650, ("mixed", "light_image"): 500, ("mixed", "moving"): 32,
              ("spheres_uv", "lamb_image"): 1500}


@functools.lru_cache(maxsize=None)
def cases(name):
    """{"k", "ray" [n,7], "s0", "tag"}: the scene's cases, interleaved.  k = -1: a miss lane."""
    sc = scene(name)
    rng = np.random.default_rng([SEED, sorted(SCENES).index(name)])
    cs = _Cases()
    for k, ob in enumerate(sc.objs):
        if ob.kind in ("sphere", "msphere"):
            # (more ordinary rays at the image spheres: the texels an ulp can move stay under 1%;
            # at the moving sphere: one in every wave)
            _sphere_cases(cs, rng, k, ob, n_rand=96 + MORE_RAYS.get((name, ob.label), 0))
        if ob.kind == "quad":
            _quad_cases(cs, rng, k, ob)
        if ob.kind == "tri":
            _tri_cases(cs, rng, k, ob)
        if ob.kind == "medium":
            _medium_cases(cs, rng, k, ob)
        if name in ("mixed", "spheres_uv") and ob.label in ("lamb_image", "light_image", "lamb_tree"):
            _uv_cases(cs, rng, k, ob, exact=ob.label == "lamb_image")
        if ob.label.startswith("diel"):
            ri = {"diel_15": 1.5, "diel_inv": 1.0 / 1.5, "diel_24": 2.4}[ob.label]
            _dielectric_cases(cs, rng, k, ob, ri, world(name), n_tir=420 if name == "mixed" else 60)
        if ob.label.startswith("metal"):
            _metal_cases(cs, rng, k, ob, {"metal_0": 64, "metal_03": 256, "metal_1": 320}[ob.label] if name == "mixed" else 64)
        if ob.label == "lamb_solid" and name in ("mixed", "spheres_plain"):
            _onb_cases(cs, rng, k, ob, n=320 if name == "mixed" else 48)
    n_aimed = sum(len(x) for x in cs.k)
    if name.startswith("sky"):
        d = _sky_dirs(rng)
    else:
        d = _scaled(rng, _dirs(rng, max(64, n_aimed // 16)))
    cs.add(-1, rng.uniform(-50, 50, d.shape), d, "miss")
    k, o, d = np.concatenate(cs.k), np.vstack(cs.o), np.vstack(cs.d)
    tag = np.array(cs.tag)
    time = np.concatenate(cs.time)
    time = np.where(np.isnan(time), rng.random(len(k)), time)
    s0 = rng.integers(0, 2 ** 64, len(k), dtype=np.uint64)
    order = _interleave(k)
    ray = np.ascontiguousarray(np.column_stack([o, d, time])[order])
    return {"k": k[order], "ray": ray, "s0": s0[order], "tag": tag[order], "label": np.array(
        [sc.objs[i].label if i >= 0 else "miss" for i in k[order]])}


@functools.lru_cache(maxsize=None)
def world(name):
    return oracle.World(scene(name).spec)


@functools.lru_cache(maxsize=None)
def answers(name):
    """The oracle's answer to every case (oracle.World.bounce; a miss lane: background), once."""
    c = cases(name)
    w = world(name)
    aimed = c["k"] >= 0
    a = w.bounce(np.where(aimed, c["k"], 0), c["ray"], c["s0"])
    for key in ("hit", "scatter", "front"):
        a[key] = a[key] & aimed
    for key in ("t", "p", "n", "u", "v", "emitted", "attenuation", "dir"):  # (a miss lane has no answer)
        a[key] = np.where(aimed if a[key].ndim == 1 else aimed[:, None], a[key], 0.0)
    a["mat"] = np.where(aimed, a["mat"], -1)
    a["state_hit"] = np.where(aimed, a["state_hit"], c["s0"])
    a["state"] = np.where(aimed, a["state"], c["s0"])
    for key in ("image_texels", "noise_evals", "hdri_texels"):
        a[key] = np.where(a["hit"], a[key], 0)
    miss = ~a["hit"]
    bg, texels = w.background(c["ray"][miss, 3:6])
    a["bg"] = np.zeros((len(aimed), 3))
    a["bg"][miss] = bg
    a["hdri_texels"][miss] = texels
    for v in a.values():
        v.setflags(write=False)
    return a


# ------------------------------------------------------- what the reference computes, in numpy
def dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # Vec3::dot's order


def unit3(a):
    return a / np.sqrt(dot3(a, a))[:, None]


def draws(state_from, state_to, most=400):
    """How many numbers a stream drew between two states (wyrand adds one constant per draw)."""
    c0 = np.uint64(0x2d358dccaa6c78a5)
    n = np.full(len(state_from), -1, dtype=np.int64)
    s = state_from.copy()
    with np.errstate(over="ignore"):
        for j in range(most + 1):
            n[(n < 0) & (s == state_to)] = j
            s = s + c0
    assert (n >= 0).all()
    return n


def uv_texel_group(c, a):
    """The cases whose colour is an image texel chosen through a sphere's u, v (a quad's and a
    triangle's u, v are exact)."""
    return a["hit"] & (a["image_texels"] > 0) & ~np.isin(c["label"], ("quad", "tri"))


def image_far(u, v, W, H, eps=1e-9):
    """ImageTexture::value_at's texel choice is farther than eps from a texel boundary in u W and
    (1 - v) H (closer, an ulp of acos / atan2 in the sphere's u, v decides)."""
    uw, vh = np.clip(u, 0.0, 1.0) * W, (1.0 - np.clip(v, 0.0, 1.0)) * H
    return (np.abs(uw - np.round(uw)) > eps) & (np.abs(vh - np.round(vh)) > eps)


def sky_angles(d):
    """HDRI::sample's u W and v H of a direction (camera.rs:257-270), the rotation by the oracle."""
    rot = np.array([oracle.rotate_vector(x, SKY_ROT) for x in d])
    rot = unit3(rot)
    theta, phi = np.arctan2(rot[:, 1], rot[:, 0]), np.arcsin(rot[:, 2])
    return (0.5 + theta / (2.0 * PI)) * SKY_W, (0.5 - phi / PI) * SKY_H


def sky_far(uW, vH, eps=1e-9):
    """Farther than eps rad from a texel boundary: the threshold, and the reason, of
    test_sky_index_f64_matches_the_formula (a column is 2 pi / W wide, a row pi / H)."""
    return (np.abs(uW - np.round(uW)) * (2 * PI / SKY_W) > eps) & (np.abs(vH - np.round(vH)) * (PI / SKY_H) > eps)


# ----------------------------------------------------------- texture cases (kat_texture)
@functools.lru_cache(maxsize=None)
def texture_cases():
    """(spec texture [n], u, v, p [n,3], what [n]) over the mixed scene's textures: the image
    lookup's clamp, flip and texel edges on the 5 x 3 image; the checkers' saturating casts and
    wrapping sum; noise on ordinary points."""
    sc = scene("mixed")
    rng = np.random.default_rng([SEED, 99])
    spec = sc.spec.spec
    by_label = {o.label: spec.materials[o.mat].texture for o in sc.objs if spec.materials[o.mat].texture >= 0}
    t_img, t_tree, t_ck, t_noise = (by_label[x] for x in ("lamb_image", "lamb_tree", "lamb_checker", "lamb_noise"))
    t_tree_inner = spec.textures[t_tree].a
    W, H = 5, 3
    tex, U, V, P, what = [], [], [], [], []

    def add(t, u, v, p, w):
        u, v = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64))
        n = u.size
        tex.append(np.full(n, t, dtype=np.int32))
        U.append(u.ravel())
        V.append(v.ravel())
        P.append(np.broadcast_to(np.asarray(p, dtype=np.float64), (n, 3)))
        what.extend([w] * n)

    edge = np.array([-1.0, -0.0, 0.0, 1.0 - 2.0 ** -53, 1.0, 2.0, np.nan])
    uu, vv = np.meshgrid(edge, edge)
    add(t_img, uu, vv, (0.0, 0.0, 0.0), "image_edge")

    def around(n):  # x with x * n on, and an ulp or two either side of, every integer 0 .. n
        x = np.arange(n + 1) / n
        out = [x]
        for _ in range(3):
            out.append(np.nextafter(out[-1], np.inf))
        lo = x
        for _ in range(3):
            lo = np.nextafter(lo, -np.inf)
            out.append(lo)
        return np.concatenate(out)
    au, av = around(W), 1.0 - around(H)
    add(t_img, au, rng.random(len(au)), (0.0, 0.0, 0.0), "image_u")
    add(t_img, rng.random(len(av)), av, (0.0, 0.0, 0.0), "image_v")
    av2 = np.concatenate([np.arange(H + 1) / H] + [np.nextafter(np.arange(H + 1) / H, s) for s in (np.inf, -np.inf)])
    add(t_img, rng.random(len(av2)), av2, (0.0, 0.0, 0.0), "image_v")
    n = 400
    add(t_img, rng.uniform(-0.1, 1.1, n), rng.uniform(-0.1, 1.1, n), (0.0, 0.0, 0.0), "image_rand")
    for t, scale, w in ((t_ck, 0.32, "checker"), (t_tree, 0.37, "tree"), (t_tree_inner, 0.11, "tree_inner")):
        big = 2.0 ** 31 * scale
        comp = np.array([0.0, -0.0, -0.5 * scale, -1.5 * scale, -2.0 * scale, 0.999999 * scale, scale, big, -big,
                         np.nextafter(big, 0.0), np.nextafter(-big, 0.0), 1.001 * big, -1.001 * big, 3.0 * big,
                         -3.0 * big, 1e300, -1e300, np.inf, -np.inf, np.nan])
        px, py, pz = np.meshgrid(comp, comp, comp)
        p = np.stack([px.ravel(), py.ravel(), pz.ravel()], -1)
        p = p[rng.permutation(len(p))[:700]]
        add(t, rng.random(len(p)), rng.random(len(p)), p, w + "_edge")
        p = rng.uniform(-3, 3, (200, 3))
        add(t, rng.random(len(p)), rng.random(len(p)), p, w + "_rand")
    p = rng.uniform(-3, 3, (300, 3))
    p[:8] = [(0, 0, 0), (-0.0, 0, 0), (0, -0.0, -0.0), (-0.5, -1.25, -2.75), (1, 2, 3), (-1, -2, -3), (0.5, 0, 0), (0, 0, -0.5)]
    add(t_noise, rng.random(len(p)), rng.random(len(p)), p, "noise")
    out = (np.concatenate(tex), np.concatenate(U), np.concatenate(V), np.ascontiguousarray(np.vstack(P)), np.array(what))
    assert len(out[0]) <= LAUNCH
    return out
