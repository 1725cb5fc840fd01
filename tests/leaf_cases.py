"""Scenes and cases of the leaf stage's known-answer tests (tests/test_leaf_cases_host.py on the
CPU, tests/test_gpu_leaf_kat.py on the device): what the megakernel's leaf pass runs for a
non-node child -- leaf_other<FEAT, UNI> of csrc/device/leaf.hpp -- against the oracle's
Hittable::hit of the same object over the same interval (oracle.World.hit).

Every scene keeps its objects 128 apart (a dyadic step: translations stay exact) and gives every
primitive a material of its own, so the material of a hit names the accepted list member.  A
case is one top-level object k, a ray, an interval (tmin, tmax) and a stream state.  The oracle
tests its top-level objects one by one and the device one leaf, so objects may overlap: a
medium's boundary stands in the scene a second time as an object of its own (its twin), at the
same place -- the oracle's hits of the twin are the medium's t1 and t2, which is how
test_leaf_cases_host.py recognises the clips.  Rays come from one fixed seed; the exact cases
are built from small dyadic numbers.  An interval is (0.001, f64::MAX), or is drawn around the
oracle's own t of the same ray (closest an ulp below, equal, an ulp above; tmin equal, an ulp
above): equal is then a true equality in f64 for every kind, chains and cube faces included.

A leaf is matched to its object by key = (media levels, anchor), shade_cases.Flat's: the anchor
of the shading cases -- a primitive's first point -- extended to a HittableList (its first
member's), a BVH (the smallest of its leaves') and a medium (its boundary's, one level more)."""
import functools

import numpy as np

import grayshift_amd as g

import oracle

from tests import shade_cases as S
from tests.shade_cases import Flat, _dirs, _scaled, _wrap, to_world  # noqa: F401  (Flat: for the tests)

SEED = 0x1EAF5EED
DMAX = 1.7976931348623157e308  # f64::MAX
TMIN = 0.001
STEP = 128.0
EPS = 2.0 ** -20   # "just outside": representable next to every coordinate of these scenes
DEN = 1e-8         # plane.rs:22's threshold, as the double both sides compare with

# the feature sets of leaf_other's instantiations (kat_device.hip, k_leaf: which = 2 f + uni)
# (0, MEDIA, NESTED, MEDIA | NESTED, MEDIA | NESTED | GENERAL)
F_NONE, F_MEDIA, F_NESTED, F_MEDIA_NESTED, F_GENERAL = range(5)


# ------------------------------------------------------------------------------- objects
class Obj:
    """One top-level object.  kind: sphere, msphere, quad, tri, list, cube, medium or bvh (a chain
    that ends in a BVH); mats: the spec materials a hit can carry, in member order; key: its
    leaf's (Flat.key); c, r: a ball around it in world space (it only aims the rays); twin: the
    object that is this medium's boundary; need: the least feature set that tests it; depth: its
    chain's."""

    def __init__(self, kind, label, mats, key, c, r, need=F_NONE, twin=None, depth=0, **geo):
        self.kind, self.label, self.mats, self.key = kind, label, list(mats), key
        self.c, self.r, self.need, self.twin, self.depth = np.array(c, dtype=np.float64), float(r), need, twin, depth
        self.__dict__.update(geo)


class Builder:
    def __init__(self, name):
        self.name, self.b, self.objs = name, g.SceneBuilder(), []

    def x(self):
        return STEP * len(self.objs)

    def mat(self):
        return self.b.lambertian((0.1 + 0.001 * len(self.objs), 0.5, 0.5))

    def add(self, handle, obj):
        self.b.add(handle)
        self.objs.append(obj)
        return len(self.objs) - 1


def _chain(depth, x, k0=0):
    """depth instances, Translate and RotateY mixed, innermost first; the last moves to x."""
    return S._alternating(depth - 1, k0) + [("t", (x, 0.0, 0.0))]


def _need_of_depth(depth, need=F_NONE):
    return F_GENERAL if depth > 4 else need  # (the other kernels' hit record keeps a chain of 4)


def add_sphere(B, label, depth=0, moving=False):
    x, m = B.x(), B.mat()
    c = (x, 0.0, 0.0) if depth == 0 else (2.0 ** -6 * len(B.objs), 0.25, -0.5)
    chain = _chain(depth, x) if depth else []
    if moving:
        c2 = (c[0] + 0.5, c[1] + 0.75, c[2] - 0.25)
        h = B.b.moving_sphere(c, c2, 1.0, m)
    else:
        h = B.b.sphere(c, 1.0, m)
    return B.add(_wrap(B.b, h, chain), Obj("msphere" if moving else "sphere", label, [m], (0, tuple(map(float, c))),
                                           to_world(chain, c), 2.0 if moving else 1.0, _need_of_depth(depth), depth=depth,
                                           exact=depth == 0 and not moving))


def add_quad(B, label, depth=0, oblique=False):
    x, m = B.x(), B.mat()
    x0 = x if depth == 0 else 2.0 ** -6 * len(B.objs)
    if oblique:
        q, u, v = (x0 - 1.0, -1.0, 0.25), (2.0, 0.25, 0.5), (-0.25, 2.0, 0.75)
    else:
        q, u, v = (x0 - 1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
    chain = _chain(depth, x) if depth else []
    mid = np.array(q) + 0.5 * np.array(u) + 0.5 * np.array(v)
    return B.add(_wrap(B.b, B.b.quad(q, u, v, m), chain),
                 Obj("quad", label, [m], (0, tuple(map(float, q))), to_world(chain, mid), 1.6, _need_of_depth(depth),
                     depth=depth, exact=depth == 0 and not oblique, x0=x0))


def add_tri(B, label, depth=0):
    x, m = B.x(), B.mat()
    x0 = x if depth == 0 else 2.0 ** -6 * len(B.objs)
    a, b, c = (x0 - 1.0, -1.0, 0.125), (x0 + 1.0, -0.75, 0.0), (x0, 1.25, -0.25)
    chain = _chain(depth, x) if depth else []
    mid = (np.array(a) + np.array(b) + np.array(c)) / 3.0
    return B.add(_wrap(B.b, B.b.triangle(a, b, c, m), chain),
                 Obj("tri", label, [m], (0, tuple(map(float, a))), to_world(chain, mid), 1.5, _need_of_depth(depth),
                     depth=depth))


def _cube(B, lo, hi):
    m = B.mat()
    return B.b.cube(lo, hi, m), [m] * 6, (0, (float(min(lo[0], hi[0])), float(min(lo[1], hi[1])), float(max(lo[2], hi[2]))))


def add_cube(B, label, depth=0, flat=False):
    """Quad::cube: its first quad's q is (min.x, min.y, max.z) (quad.rs:54-80)."""
    x = B.x()
    x0 = x if depth == 0 else 2.0 ** -6 * len(B.objs)
    lo, hi = (x0 - 1.0, -1.0 if not flat else 0.5, -1.0), (x0 + 1.0, 1.0 if not flat else 0.5, 1.0)
    h, mats, key = _cube(B, lo, hi)
    chain = _chain(depth, x) if depth else []
    return B.add(_wrap(B.b, h, chain), Obj("cube", label, mats, key, to_world(chain, (x0, lo[1] * 0.5 + hi[1] * 0.5, 0.0)),
                                           1.75, _need_of_depth(depth), depth=depth, exact=depth == 0 and not flat, x0=x0,
                                           flat=flat))


def add_loose_cube(B, label):
    """The six quads of a cube, out of cube order: a list that keeps the loop."""
    x = B.x()
    mn, mx = np.array([x - 1.0, -1.0, -1.0]), np.array([x + 1.0, 1.0, 1.0])
    dx, dy, dz = np.array([2.0, 0, 0]), np.array([0, 2.0, 0]), np.array([0, 0, 2.0])
    faces = [((mn[0], mn[1], mx[2]), dx, dy), ((mx[0], mn[1], mx[2]), -dz, dy), ((mx[0], mn[1], mn[2]), -dx, dy),
             ((mn[0], mn[1], mn[2]), dz, dy), ((mn[0], mx[1], mx[2]), dx, -dz), ((mn[0], mn[1], mn[2]), dx, dz)]
    order = [4, 0, 5, 2, 1, 3]
    mats = [B.mat() for _ in order]
    members = [B.b.quad(tuple(faces[f][0]), tuple(faces[f][1]), tuple(faces[f][2]), m) for f, m in zip(order, mats)]
    return B.add(B.b.hittable_list(members), Obj("list", label, mats, (0, tuple(map(float, faces[order[0]][0]))),
                                                  (x, 0.0, 0.0), 1.75))


def add_list_mixed(B, label, depth=0):
    x = B.x()
    x0 = x if depth == 0 else 2.0 ** -6 * len(B.objs)
    mats = [B.mat() for _ in range(4)]
    members = [B.b.sphere((x0 - 1.5, 0.0, 0.0), 1.0, mats[0]),
               B.b.quad((x0 - 1.0, -1.0, -0.5), (2.0, 0.0, 0.5), (0.0, 2.0, 0.0), mats[1]),
               B.b.triangle((x0 - 1.0, -1.0, 0.5), (x0 + 2.0, -1.0, 0.75), (x0, 1.5, 0.5), mats[2]),
               B.b.moving_sphere((x0 + 1.5, 0.0, 0.0), (x0 + 1.5, 0.5, 0.0), 1.0, mats[3])]
    chain = _chain(depth, x) if depth else []
    return B.add(_wrap(B.b, B.b.hittable_list(members), chain),
                 Obj("list", label, mats, (0, (x0 - 1.5, 0.0, 0.0)), to_world(chain, (x0, 0.0, 0.0)), 2.5,
                     _need_of_depth(depth), depth=depth))


def add_list_coincident(B, label):
    """Two coincident quads: on every hit both accept the same t, and the later one wins."""
    x = B.x()
    mats = [B.mat(), B.mat()]
    q, u, v = (x - 1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
    return B.add(B.b.hittable_list([B.b.quad(q, u, v, m) for m in mats]),
                 Obj("list", label, mats, (0, q), (x, 0.0, 0.0), 1.6, later=mats[1]))


def add_list_tri_between(B, label):
    """[a quad at z = 0, a triangle at z = -2, a quad at z = -1]: for a ray along -z the triangle,
    which ignores its interval, overrides the nearer quad before it, and the quad after it is
    tested against the triangle's t."""
    x = B.x()
    mats = [B.mat() for _ in range(3)]
    u, v = (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
    members = [B.b.quad((x - 1.0, -1.0, 0.0), u, v, mats[0]),
               # (b - a) x (c - a) along -z: rays along -z pass Triangle::hit's one-sided test (det > 0)
               B.b.triangle((x - 2.0, -2.0, -2.0), (x, 2.0, -2.0), (x + 2.0, -2.0, -2.0), mats[1]),
               B.b.quad((x - 1.0, -1.0, -1.0), u, (0.0, 1.0, 0.0), mats[2])]
    return B.add(B.b.hittable_list(members), Obj("list", label, mats, (0, (x - 1.0, -1.0, 0.0)), (x, 0.0, -1.0), 2.0,
                                                  exact=True, x0=x))


def add_bvh(B, label, depth, need=F_NESTED):
    """A chain that ends in a BVH of three spheres and a quad: leaf_other enters it."""
    x = B.x()
    x0 = 2.0 ** -6 * len(B.objs)
    cs = [(x0 - 2.0, 0.0, 0.0), (x0 + 2.0, 0.5, 0.0), (x0, -0.5, 2.0)]
    members = [B.b.sphere(c, 1.0, B.mat()) for c in cs]
    q = (x0 - 1.0, -1.0, -2.0)
    members.append(B.b.quad(q, (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), B.mat()))
    chain = _chain(depth, x)
    return B.add(_wrap(B.b, B.b.bvh(members), chain),
                 Obj("bvh", label, [], (0, min([tuple(map(float, c)) for c in cs] + [tuple(map(float, q))])),
                     to_world(chain, (x0, 0.0, 0.0)), 3.0, _need_of_depth(depth, need), depth=depth))


def add_medium(B, label, boundary, density, boundary_depth=0, depth=0):
    """A medium and, before it, its boundary as an object of its own (the twin), at the same place.
    boundary: sphere | cube | quad | bvh | medium (a medium around a sphere, itself with a twin)."""
    x = B.x()
    bchain = _chain(boundary_depth, 0.0, 1) if boundary_depth else []
    chain = _chain(depth, 0.0, 2) if depth else []
    phase = B.b.isotropic((0.5, 0.25 + 0.001 * len(B.objs), 0.75))
    need = F_MEDIA
    if boundary == "sphere":
        c = (x, 0.0, 0.0)

        def shape():
            m = B.mat()
            return _wrap(B.b, B.b.sphere(c, 2.0, m), bchain), [m]
        key, kind, r = (0, c), "sphere", 2.0
    elif boundary == "cube":
        lo, hi = (x - 1.0, -1.0, -1.0), (x + 1.0, 1.0, 1.0)

        def shape():
            h, mats, _ = _cube(B, lo, hi)
            return _wrap(B.b, h, bchain), mats
        key, kind, r = (0, (lo[0], lo[1], hi[2])), "cube", 1.75
    elif boundary == "quad":
        q = (x - 1.0, -1.0, 0.0)

        def shape():
            m = B.mat()
            return _wrap(B.b, B.b.quad(q, (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), m), bchain), [m]
        key, kind, r = (0, q), "quad", 1.6
    elif boundary == "bvh":  # cubes and a sphere in a BVH (tree_test): no twin
        los = [(x - 2.0, -1.0, -1.0), (x + 0.5, -0.5, -0.5)]
        his = [(x - 0.5, 1.0, 1.0), (x + 2.0, 1.0, 0.75)]
        sc = (x, 0.0, 2.5)
        h = B.b.bvh([_cube(B, lo, hi)[0] for lo, hi in zip(los, his)] + [B.b.sphere(sc, 1.0, B.mat())])
        key = (1, min([(lo[0], lo[1], hi[2]) for lo, hi in zip(los, his)] + [sc]))
        return B.add(_wrap(B.b, B.b.medium(h, density, phase), chain),
                     Obj("medium", label, [phase], key, to_world(chain, (x, 0.0, 0.5)), 3.0, F_GENERAL, depth=depth,
                         levels=1, density=density))
    else:
        raise ValueError(boundary)
    h, mats = shape()  # (the twin under the medium's chain too: the same ray reaches it, bit for bit)
    twin = B.add(_wrap(B.b, h, chain), Obj(kind, label + "_boundary", mats, key, to_world(bchain + chain, (x, 0.0, 0.0)), r,
                                           _need_of_depth(boundary_depth + depth), depth=boundary_depth + depth))
    h, _ = shape()
    c_world = to_world(bchain + chain, (x, 0.0, 0.0))
    if max(depth, boundary_depth) > 4:
        need = F_GENERAL
    return B.add(_wrap(B.b, B.b.medium(h, density, phase), chain),
                 Obj("medium", label, [phase], (1, key[1]), c_world, r, need, twin=twin, depth=depth, levels=1,
                     density=density))


def add_medium_pair(B, label, inner_density, outer_density):
    """A medium whose boundary is a medium around a sphere (LEVEL 1), after its two twins."""
    x = B.x()
    c = (x, 0.0, 0.0)
    m0 = B.mat()
    t0 = B.add(B.b.sphere(c, 2.0, m0), Obj("sphere", label + "_sphere", [m0], (0, c), c, 2.0))
    p1 = B.b.isotropic((0.25, 0.5, 0.001 * len(B.objs)))
    t1 = B.add(B.b.medium(B.b.sphere(c, 2.0, B.mat()), inner_density, p1),
               Obj("medium", label + "_inner", [p1], (1, c), c, 2.0, F_MEDIA, twin=t0, levels=1, density=inner_density))
    p2 = B.b.isotropic((0.75, 0.5, 0.001 * len(B.objs)))
    inner = B.b.medium(B.b.sphere(c, 2.0, B.mat()), inner_density, B.b.isotropic((0.3, 0.3, 0.3)))
    return B.add(B.b.medium(inner, outer_density, p2),
                 Obj("medium", label, [p2], (2, c), c, 2.0, F_GENERAL, twin=t1, levels=2, density=outer_density))


class LeafScene:
    def __init__(self, B):
        self.name, self.objs = B.name, B.objs
        B.b.background_solid((0.5, 0.5, 0.5))
        self.spec = B.b.build()
        assert self.spec.n_world == len(self.objs)
        self.need = max(o.need for o in self.objs)


def scene_plain():
    B = Builder("plain")
    add_sphere(B, "sphere")
    add_sphere(B, "msphere", moving=True)
    add_quad(B, "quad_aa")
    add_quad(B, "quad_oblique", oblique=True)
    add_tri(B, "tri")
    add_sphere(B, "sphere_chain1", depth=1)
    add_sphere(B, "msphere_chain4", depth=4, moving=True)
    add_quad(B, "quad_chain4", depth=4)
    add_quad(B, "quad_oblique_chain1", depth=1, oblique=True)
    add_tri(B, "tri_chain4", depth=4)
    add_list_mixed(B, "list_mixed")
    add_list_mixed(B, "list_mixed_chain1", depth=1)
    add_list_coincident(B, "list_coincident")
    add_list_tri_between(B, "list_tri_between")
    add_cube(B, "cube")
    add_cube(B, "cube_b")   # (a second and third plain cube: a strict prefix of the cube mirror splits them)
    add_cube(B, "cube_c")
    add_cube(B, "cube_chain4", depth=4)
    add_cube(B, "cube_flat", flat=True)
    add_loose_cube(B, "cube_loose")
    add_quad(B, "quad_last")  # (a quad after the cubes': a strict prefix of the quad mirror leaves it out)
    return LeafScene(B)


def scene_media():
    B = Builder("media")
    for j, density in enumerate((0.01, 0.1, 1.0, 8.0)):
        add_medium(B, "medium_sphere_%d" % j, "sphere", density)
    add_medium(B, "medium_cube", "cube", 0.5)
    add_medium(B, "medium_cube_thin", "cube", 0.05)
    add_medium(B, "medium_quad", "quad", 1.0)
    add_medium(B, "medium_sphere_bchain2", "sphere", 0.3, boundary_depth=2)
    add_medium(B, "medium_cube_bchain1_chain2", "cube", 0.7, boundary_depth=1, depth=2)
    add_sphere(B, "sphere")
    add_quad(B, "quad_aa")
    add_cube(B, "cube")
    return LeafScene(B)


def scene_nested():
    B = Builder("nested")
    add_bvh(B, "bvh_chain1", 1)
    add_bvh(B, "bvh_chain2", 2)
    add_bvh(B, "bvh_chain4", 4)
    add_sphere(B, "sphere_chain1", depth=1)
    add_cube(B, "cube")
    add_quad(B, "quad_aa")
    add_tri(B, "tri")
    return LeafScene(B)


def scene_general():
    B = Builder("general")
    add_sphere(B, "sphere_chain16", depth=16)
    add_quad(B, "quad_chain16", depth=16, oblique=True)
    add_tri(B, "tri_chain16", depth=16)
    add_sphere(B, "msphere_chain16", depth=16, moving=True)
    add_cube(B, "cube_chain16", depth=16)
    add_list_mixed(B, "list_mixed_chain16", depth=16)
    add_bvh(B, "bvh_chain16", 16)
    add_bvh(B, "bvh_chain2", 2)
    add_medium(B, "medium_bvh", "bvh", 0.4)
    add_medium(B, "medium_bvh_thin", "bvh", 0.02)
    add_medium(B, "medium_bvh_chain2", "bvh", 0.4, depth=2)
    add_medium_pair(B, "medium_pair", 0.6, 0.5)
    add_medium_pair(B, "medium_pair_thin", 0.05, 0.2)
    add_medium_pair(B, "medium_pair_dense", 4.0, 3.0)
    add_medium(B, "medium_sphere_bchain16", "sphere", 0.3, boundary_depth=16)
    add_medium(B, "medium_cube", "cube", 0.5)
    add_sphere(B, "sphere")
    add_cube(B, "cube")
    return LeafScene(B)


SCENES = {"plain": scene_plain, "media": scene_media, "nested": scene_nested, "general": scene_general}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def world(name):
    return oracle.World(scene(name).spec)


# --------------------------------------------------------------------------------- rays
class _Rays:
    def __init__(self):
        self.k, self.o, self.d, self.time, self.tag, self.iv = [], [], [], [], [], []

    def add(self, k, o, d, tag, time=None, iv=None):
        """iv: (tmin, tmax) of an exact case (default: the open interval, and a variant later)."""
        o, d = np.atleast_2d(np.asarray(o, dtype=np.float64)), np.atleast_2d(np.asarray(d, dtype=np.float64))
        assert o.shape == d.shape
        n = len(o)
        self.k.append(np.full(n, k, dtype=np.int32))
        self.o.append(o)
        self.d.append(d)
        self.time.append(np.full(n, np.nan) if time is None else np.broadcast_to(np.asarray(time, dtype=np.float64), (n,)))
        self.tag += [tag] * n
        self.iv.append(np.broadcast_to(np.array([np.nan, np.nan] if iv is None else iv, dtype=np.float64), (n, 2)))


def _ball_rays(R, rng, k, ob, n_out, n_in):
    """Rays from outside at points all over the object's ball, and rays from inside it."""
    o = ob.c + ob.r * rng.uniform(1.5, 4.0, (n_out, 1)) * _dirs(rng, n_out)
    t = ob.c + 0.9 * ob.r * rng.random((n_out, 1)) ** (1.0 / 3.0) * _dirs(rng, n_out)
    R.add(k, o, _scaled(rng, t - o), "rand")
    o = ob.c + 0.5 * ob.r * rng.random((n_in, 1)) ** (1.0 / 3.0) * _dirs(rng, n_in)
    R.add(k, o, _scaled(rng, _dirs(rng, n_in)), "inside")


def _msphere_rays(R, rng, k, ob):
    """A moving sphere at times 0, 1 and between (sphere.rs:51-53); the list's too."""
    for time in (0.0, 1.0):
        n = 16
        o = ob.c + ob.r * rng.uniform(1.5, 4.0, (n, 1)) * _dirs(rng, n)
        t = ob.c + 0.6 * ob.r * _dirs(rng, n)
        R.add(k, o, _scaled(rng, t - o), "time%d" % time, time=time)


def _quad_exact(R, k, ob):
    """The unit-interval edges of Quad::hit on q = (x - 1, -1, 0), u = (2, 0, 0), v = (0, 2, 0): the
    point (x + a, b, 0) has alpha = (a + 1) / 2 and beta = (b + 1) / 2 exactly; the plane is
    z = 0 and a ray from z = 2 along (0, 0, -s) meets it at t = 2 / s exactly."""
    x = ob.x0
    for s in (0.5, 1.0, 2.0):
        for tag, a, b in (("alpha0", -1.0, 0.25), ("alpha1", 1.0, -0.5), ("beta0", 0.5, -1.0), ("beta1", -0.25, 1.0),
                          ("corner", 1.0, 1.0), ("corner", -1.0, -1.0)):
            R.add(k, (x + a, b, 2.0), (0.0, 0.0, -s), tag)
            R.add(k, (x + a, b, -2.0), (0.0, 0.0, s), tag)  # (the back face)
        for tag, a, b in (("alpha_out", -1.0 - EPS, 0.25), ("alpha_out", 1.0 + EPS, -0.5), ("beta_out", 0.5, -1.0 - EPS),
                          ("beta_out", -0.25, 1.0 + EPS)):
            R.add(k, (x + a, b, 2.0), (0.0, 0.0, -s), tag)
        # the interval's ends, closed (plane.rs:26): t = 2 / s
        R.add(k, (x + 0.5, 0.5, 2.0), (0.0, 0.0, -s), "t_eq_tmin", iv=(2.0 / s, DMAX))
        R.add(k, (x + 0.5, 0.5, 2.0), (0.0, 0.0, -s), "t_eq_tmax", iv=(TMIN, 2.0 / s))
        R.add(k, (x + 0.5, 0.5, 2.0), (0.0, 0.0, -s), "t_lt_tmin", iv=(np.nextafter(2.0 / s, 9.0), DMAX))
        R.add(k, (x + 0.5, 0.5, 2.0), (0.0, 0.0, -s), "t_gt_tmax", iv=(TMIN, np.nextafter(2.0 / s, 0.0)))
    # |n . d| either side of 1e-8 (plane.rs:22): n = (0, 0, 1), t = 1 / |d.z|
    for sign in (1.0, -1.0):
        for tag, dz in (("den_below", np.nextafter(DEN, 0.0)), ("den_at", DEN), ("den_above", np.nextafter(DEN, 1.0))):
            R.add(k, (x + 0.25, -0.5, -sign), (0.0, 0.0, sign * dz), tag)
            R.add(k, (x - 0.5, 0.75, -sign), (0.0, -0.0, sign * dz), tag)


def _sphere_exact(R, k, ob):
    """Sphere::hit's open interval (sphere.rs:79-84), radius 1: from (x, 0, 5) along (0, 0, -s)."""
    x = ob.c[0]
    for s in (1.0, 0.5, 2.0, 0.25):  # a = s^2, h = 5 s, disc = s^2: roots 4 / s and 6 / s exactly
        o, d, near, far = (x, 0.0, 5.0), (0.0, 0.0, -s), 4.0 / s, 6.0 / s
        R.add(k, o, d, "root_eq_tmin", iv=(near, DMAX))              # the near root rejected, the far one taken
        R.add(k, o, d, "root_eq_tmin_tmax", iv=(near, far))          # both rejected
        R.add(k, o, d, "root_eq_tmax", iv=(TMIN, near))              # rejected; the far root is outside too
        R.add(k, o, d, "root_in", iv=(np.nextafter(near, 0.0), far))  # the near root accepted
        R.add(k, o, d, "root_far_in", iv=(near, np.nextafter(far, np.inf)))
    d = (0.0, 0.0, -1.0)
    for y in (0.5, -0.25):  # (and off the axis: the same equalities through the oracle's own t, below)
        R.add(k, (x, y, 5.0), d, "rand")


def _cube_exact(R, k, ob):
    """The cube (x - 1, -1, -1) .. (x + 1, 1, 1).  Faces in list order: z = 1, x = x + 1, z = -1,
    x = x - 1, y = 1, y = -1 (quad.rs:62-78)."""
    x = ob.x0
    for s in (1.0, 0.5):
        # through an edge shared by two faces, and a corner shared by three: equal t, the later face wins
        R.add(k, (x + 3.0, 0.25, 3.0), (-s, 0.0, -s), "edge")        # faces z = 1 and x = x + 1 at t = 2 / s
        R.add(k, (x - 3.0, 0.25, 3.0), (s, 0.0, -s), "edge")         # z = 1 and x = x - 1
        R.add(k, (x + 0.5, 3.0, 3.0), (0.0, -s, -s), "edge")         # z = 1 and y = 1
        R.add(k, (x + 0.5, -3.0, -3.0), (0.0, s, s), "edge")         # z = -1 and y = -1
        R.add(k, (x + 3.0, 3.0, 3.0), (-s, -s, -s), "corner")        # z = 1, x = x + 1, y = 1
        R.add(k, (x - 3.0, -3.0, -3.0), (s, s, s), "corner")
        R.add(k, (x + 3.0, -3.0, 3.0), (-s, s, -s), "corner")
        R.add(k, (x - 3.0, 3.0, -3.0), (s, -s, s), "corner")
        # from inside towards an edge and a corner
        R.add(k, (x, 0.25, 0.0), (s, 0.0, s), "edge")
        R.add(k, (x, 0.0, 0.0), (s, s, -s), "corner")
        # parallel to four faces (a zero of either sign in the direction)
        for z in (0.0, -0.0):
            R.add(k, (x + 3.0, 0.25, 3.0), (z, z, -s), "parallel")      # ... and past the cube
            R.add(k, (x + 0.5, 1.0 + EPS, 3.0), (z, z, -s), "parallel")
            R.add(k, (x + 0.5, 0.25, 3.0), (z, z, -s), "parallel")
            R.add(k, (x + 3.0, 0.25, -0.5), (-s, z, z), "parallel")
            R.add(k, (x - 0.25, -3.0, 0.5), (z, s, z), "parallel")
            R.add(k, (x + 0.5, 0.25, 0.5), (z, s, z), "parallel")       # ... from inside
            R.add(k, (x + 1.0, 0.25, 3.0), (z, z, -s), "parallel")      # ... in the plane of the face x = x + 1
        # the interval's ends on a face, closed: the face z = 1 at t = 2 / s, z = -1 at 4 / s
        o, d = (x + 0.5, 0.25, 3.0), (0.0, 0.0, -s)
        R.add(k, o, d, "t_eq_tmin", iv=(2.0 / s, DMAX))
        R.add(k, o, d, "t_eq_tmax", iv=(TMIN, 2.0 / s))
        R.add(k, o, d, "t_lt_tmin", iv=(np.nextafter(2.0 / s, 9.0), DMAX))   # the far face instead
        R.add(k, o, d, "t_eq_tmin", iv=(4.0 / s, DMAX))
        R.add(k, o, d, "t_gt_tmax", iv=(TMIN, np.nextafter(2.0 / s, 0.0)))
    # |d_axis| either side of 1e-8 (the face's plane test), from inside: the face ahead is hit
    # at t = 1 / |d_axis| when it passes
    for axis in range(3):
        for sign in (1.0, -1.0):
            for tag, v in (("den_below", np.nextafter(DEN, 0.0)), ("den_at", DEN), ("den_above", np.nextafter(DEN, 1.0))):
                d = np.zeros(3)
                d[axis] = sign * v
                R.add(k, (x, 0.0, 0.0), d, tag)
                o = np.array([x + 0.25, 0.5, -0.5])
                o[axis] = (x, 0.0, 0.0)[axis]
                R.add(k, o, d, tag)


def _tri_between_exact(R, k, ob):
    """Points (x + a, b) inside the first quad and the triangle; those with b <= 0 inside the last quad too."""
    x = ob.x0
    low = ((0.0, 0.0), (0.5, -0.5), (-0.75, -0.25), (0.25, -0.875))
    high = ((0.5, 0.5), (-0.5, 0.75), (0.0, 0.25), (0.75, 0.125))
    for s in (1.0, 2.0):
        for a, b in low:
            R.add(k, (x + a, b, 3.0), (0.0, 0.0, -s), "tri_overrides")   # quad 3 / s, triangle 5 / s, quad 4 / s: the last
            R.add(k, (x + a, b, -3.0), (0.0, 0.0, s), "tri_culled")      # from behind: the triangle is one-sided
        for a, b in high:
            R.add(k, (x + a, b, 3.0), (0.0, 0.0, -s), "tri_wins")        # the triangle, the farthest, stays
        for a, b in low + high:
            R.add(k, (x + a, b, -3.0), (0.0, 0.0, -s), "tri_behind_in_list")  # all three behind: only the triangle accepts


def _rays(name):
    sc = scene(name)
    rng = np.random.default_rng([SEED, sorted(SCENES).index(name)])
    R = _Rays()
    for k, ob in enumerate(sc.objs):
        small = ob.label.endswith("_boundary") or ob.label.endswith("_sphere") or ob.label.endswith("_inner")
        n_out, n_in = (24, 8) if small else (64, 24)
        if ob.kind == "medium":
            n_out, n_in = 96, 64
        if ob.kind == "tri":  # (one-sided: half the rays are culled)
            n_out, n_in = 160, 32
        _ball_rays(R, rng, k, ob, n_out, n_in)
        if ob.kind == "msphere" or ob.label.startswith("list_mixed"):
            _msphere_rays(R, rng, k, ob)
        if ob.kind == "quad" and getattr(ob, "exact", False):
            _quad_exact(R, k, ob)
        if ob.kind == "sphere" and getattr(ob, "exact", False) and not small:
            _sphere_exact(R, k, ob)
        if ob.kind == "cube" and getattr(ob, "exact", False):
            _cube_exact(R, k, ob)
        if ob.label == "list_tri_between":
            _tri_between_exact(R, k, ob)
    k, o, d = np.concatenate(R.k), np.vstack(R.o), np.vstack(R.d)
    time = np.concatenate(R.time)
    time = np.where(np.isnan(time), rng.random(len(k)), time)
    return sc, rng, k, np.column_stack([o, d, time]), np.array(R.tag), np.vstack(R.iv)


def boundary_hits(name, k, ray, s0):
    """A medium case's two boundary hits as ConstantMedium::hit takes them (volume.rs:36-41), by the
    oracle on the medium's twin: (has1, t1, has2, t2, the stream state before the medium's own draw).
    NaN / False where the object has no twin."""
    sc, W = scene(name), world(name)
    twin = np.array([-1 if o.twin is None else o.twin for o in sc.objs])[k]
    m = twin >= 0
    n = len(k)
    has1, has2 = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    t1, t2 = np.full(n, np.nan), np.full(n, np.nan)
    state = s0.copy()
    if m.any():
        a = W.hit(twin[m], ray[m], -DMAX, DMAX, s0[m])
        has1[m], t1[m], state[m] = a["hit"], np.where(a["hit"], a["t"], np.nan), a["state"]
        m2 = m & has1
        if m2.any():
            b = W.hit(twin[m2], ray[m2], t1[m2] + 0.0001, DMAX, state[m2])
            has2[m2], t2[m2], state[m2] = b["hit"], np.where(b["hit"], b["t"], np.nan), b["state"]
    return has1, t1, has2, t2, state


INTERVALS = ("closest_below", "closest_equal", "closest_above", "tmin_equal", "tmin_above")
MEDIUM_INTERVALS = ("closest_inside", "tmin_past_t1", "crossed", "closest_equal", "closest_above", "closest_below")


@functools.lru_cache(maxsize=None)
def cases(name):
    """{"k", "ray" [n,7], "tmin", "tmax", "s0", "tag", "iv", "label"}: the scene's cases in the mixed
    order (every run of 64 holds many objects and kinds).  tag: how the ray was made; iv: how the
    interval was ("open": (0.001, f64::MAX); "exact": the tag's own; else a name of INTERVALS /
    MEDIUM_INTERVALS, drawn around the oracle's answer over the open interval)."""
    sc, rng, k, ray, tag, iv0 = _rays(name)
    W = world(name)
    n = len(k)
    s0 = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    exact = ~np.isnan(iv0[:, 0])
    tmin, tmax = np.where(exact, iv0[:, 0], TMIN), np.where(exact, iv0[:, 1], DMAX)
    iv = np.where(exact, "exact", "open").astype("U16")
    a0 = W.hit(k, ray, tmin, tmax, s0)
    kind = np.array([o.kind for o in sc.objs])[k]
    more = {key: [] for key in ("k", "ray", "tmin", "tmax", "s0", "tag", "iv")}

    def variant(idx, new_tmin, new_tmax, names, new_ray=None, new_tag=None):
        more["k"].append(k[idx])
        more["ray"].append(ray[idx] if new_ray is None else new_ray)
        more["tmin"].append(new_tmin)
        more["tmax"].append(new_tmax)
        more["s0"].append(s0[idx])
        more["tag"].append(tag[idx] if new_tag is None else np.full(len(idx), new_tag))
        more["iv"].append(np.asarray(names).astype("U16"))

    # primitives, lists, cubes: the interval around the oracle's own t
    idx = np.flatnonzero(a0["hit"] & ~exact & (kind != "medium") & (kind != "bvh"))
    t = a0["t"][idx]
    which = np.arange(len(idx)) % len(INTERVALS)
    lo = np.select([which == 3, which == 4], [t, np.nextafter(t, np.inf)], TMIN)
    hi = np.select([which == 0, which == 1, which == 2], [np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)], DMAX)
    variant(idx, lo, hi, np.array(INTERVALS)[which])
    # the triangle ignores its interval (triangle.rs:34): beyond closest, and behind the origin
    idx = np.flatnonzero(a0["hit"] & ~exact & (kind == "tri") & (a0["t"] > 2.0 * TMIN))
    variant(idx, np.full(len(idx), TMIN), 0.5 * a0["t"][idx], np.full(len(idx), "tri_beyond"))
    moved = ray[idx].copy()
    moved[:, 0:3] += 2.0 * a0["t"][idx, None] * moved[:, 3:6]
    variant(idx, np.full(len(idx), TMIN), np.full(len(idx), DMAX), np.full(len(idx), "open"), moved, "tri_behind")
    # media: the interval against the boundary's t1 and t2, and around the medium's own t
    has1, t1, has2, t2, _ = boundary_hits(name, k, ray, s0)
    idx = np.flatnonzero((kind == "medium") & has1 & has2)
    which = np.arange(len(idx)) % len(MEDIUM_INTERVALS)
    which = np.where((which >= 3) & ~a0["hit"][idx], which - 3, which)
    a, b, t = t1[idx], t2[idx], a0["t"][idx]
    span = b - a
    lo = np.select([which == 1, which == 2], [a + 0.25 * span, a + 0.75 * span], TMIN)
    hi = np.select([which == 0, which == 2, which == 3, which == 4, which == 5],
                   [a + 0.5 * span, a + 0.25 * span, t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)], DMAX)
    variant(idx, lo, hi, np.array(MEDIUM_INTERVALS)[which])
    # media without a twin (a BVH as the boundary): closest at fractions of the medium's own t
    twinless = np.array([o.kind == "medium" and o.twin is None for o in sc.objs])[k]
    idx = np.flatnonzero(twinless & a0["hit"])
    which = np.arange(len(idx)) % 3
    t = a0["t"][idx]
    variant(idx, np.where(which == 2, 0.5 * t, TMIN), np.select([which == 0, which == 1], [t, 0.75 * t], DMAX),
            np.array(["closest_equal", "closest_inside", "tmin_past_t1"])[which])

    k = np.concatenate([k] + more["k"])
    ray = np.vstack([ray] + more["ray"])
    tmin, tmax = np.concatenate([tmin] + more["tmin"]), np.concatenate([tmax] + more["tmax"])
    s0 = np.concatenate([s0] + more["s0"])
    tag = np.concatenate([tag.astype("U32")] + [x.astype("U32") for x in more["tag"]])
    iv = np.concatenate([iv] + more["iv"])
    order = S._interleave(k)
    out = {"k": k[order], "ray": np.ascontiguousarray(ray[order]), "tmin": tmin[order], "tmax": tmax[order],
           "s0": s0[order], "tag": tag[order], "iv": iv[order],
           "label": np.array([sc.objs[i].label for i in k[order]]), "kind": np.array([sc.objs[i].kind for i in k[order]])}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def answers(name):
    """The oracle's answer to every case (oracle.World.hit), once, with "draws": how many numbers
    the case drew from its stream."""
    c = cases(name)
    a = world(name).hit(c["k"], c["ray"], c["tmin"], c["tmax"], c["s0"])
    a["draws"] = S.draws(c["s0"], a["state"], most=8)
    for v in a.values():
        v.setflags(write=False)
    return a


def uniform_layout(k, wave=64):
    """The cases in an order where every run of `wave` holds one object only: indices into the
    cases, -1 for a padding lane."""
    out = []
    for v in np.unique(k):
        idx = np.flatnonzero(k == v)
        out.append(idx)
        out.append(np.full(-len(idx) % wave, -1, dtype=idx.dtype))
    return np.concatenate(out)
