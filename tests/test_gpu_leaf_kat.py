"""Known-answer tests of the leaf stage: leaf_other<FEAT, UNI> of grayshift_amd/csrc/device/leaf.hpp
-- the primitive, chain, list, cube and medium tests a leaf pass runs -- case by case through
the test-only harness (tests/hip/kat_device.hip, k_leaf) on the records the product itself
uploads (gs_debug_device_scene_record, gs_debug_leaf_stage_record: the host-built TQuad and cube
records are under test too), against the CPU oracle's Hittable::hit of the same object over the
same interval (oracle.World.hit).

The scenes and cases are tests/leaf_cases.py's; tests/test_leaf_cases_host.py asserts, on the
oracle's answers alone, that they reach the edges (interval ends, ties, face edges, the plane
threshold, the triangle outside its interval, every medium clip and draw).

Compared, per case and for every instantiation that compiles the case's leaf kind in
(FEAT projected onto {MEDIA, NESTED, GENERAL}, five sets): hit; t bit for bit; the lane's stream
state after, bit for bit; the eight test counters, exactly (a cube list counts six quad tests,
chain_count's second walk shows in the instance tests); the HitRec that reconstruct makes of the
result -- p, n, front, the material, and u, v for quads and triangles -- bit for bit, which
names the accepted list member and cube face.  A sphere's u, v are the shading KAT's.  A chain
that ends in a BVH: `enter` names the tree (its root's box against the flat scene's node) and
the ray is the chain applied in numpy f64.

Device-only choices must not show: UNI (scalar loads, one ref per wave) against per-lane loads;
the quad and cube mirrors in LDS empty, whole, and a strict prefix that splits single waves;
gs_debug_set_cube_lists on and off -- identical outputs, counters included.

libm enters in one place, log(wy_f64(rng)) in medium_test, on an argument that is exact given
the stream state.  Where the device's log (kat_math) returns glibc's bits for every draw of a
case, t is compared bit for bit; elsewhere the case is left out of that comparison only: hit,
state and counters are still compared, and t must lie within 4 ulp of hit_dist / ray_len per
draw plus the rounding of the sum.  With a differing log the decision hit_dist > dist_inside_boundary
itself may go the other way, but only on the knife edge (closest drawn at the medium's own t): the
t of the side that hit must then lie within that tolerance of closest.  The share of medium cases
left out must stay under 5% (observed: test_log_share's docstring)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N

import oracle

from tests import leaf_cases as L
from tests.shade_cases import REF_INST, REF_LIST, REF_MASK, REF_NODE, REF_NONE, REF_QUAD, REF_SHIFT, REF_TRI

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LAUNCH = 4096  # cases per harness launch (whole waves)
NAMES = sorted(L.SCENES)
# the feature sets that compile an object's leaf kind in, by the least one that does
COVERS = {L.F_NONE: (0, 1, 2, 3, 4), L.F_MEDIA: (1, 3, 4), L.F_NESTED: (2, 3, 4), L.F_MEDIA_NESTED: (3, 4),
          L.F_GENERAL: (4,)}
LOG_CAP = 0.05


def ptr(a):
    return a.ctypes.data


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ok(rc):
    """A harness call's status: after a HIP error nothing more is launched."""
    if rc != 0:
        pytest.exit("a harness kernel failed (status %d): no further launches" % rc, returncode=3)


@pytest.fixture(scope="module")
def kat(built):
    lib = C.CDLL(os.path.join(HERE, "hip", "libkat_device.so"))
    P, I, U = C.c_void_p, C.c_int, C.c_uint32
    for f, args in {"kat_math": [I, I, P, P, P], "kat_dev_scene_bytes": [], "kat_counters": [], "kat_leaf_flags": [],
                    "kat_leaf_out": [], "kat_tquad_bytes": [], "kat_leaf_counter_slot": [I],
                    "kat_leaf": [I, I, P, P, U, U, U, U, P, P, P, P, P, P, P, P, P]}.items():
        getattr(lib, f).argtypes = args
        getattr(lib, f).restype = I
    assert lib.kat_tquad_bytes() == 128
    lib.slots = [lib.kat_leaf_counter_slot(j) for j in range(8)]
    assert len(set(lib.slots)) == 8 and min(lib.slots) >= 0 and max(lib.slots) < lib.kat_counters()
    assert lib.kat_leaf_counter_slot(8) == -1
    return lib


class Dev:
    """A scene of leaf_cases on the device (uploaded with gs_debug_set_cube_lists(cube_lists)): the
    device scene's record and leaf-stage record, and each object's leaf ref and materials."""

    def __init__(self, kat, name, cube_lists):
        self.name, self.sc = name, L.scene(name)
        self.host = g.HostScene(self.sc.spec)
        d = C.c_void_p()
        N.check(N.lib.gs_debug_set_cube_lists(cube_lists))
        try:
            N.check(N.lib.gs_device_scene_create(self.host.flat_ptr, C.byref(d)))
        finally:
            N.check(N.lib.gs_debug_set_cube_lists(1))
        self.dev = d
        nbytes = kat.kat_dev_scene_bytes()
        self.record = np.zeros(nbytes, dtype=np.uint8)
        N.check(N.lib.gs_debug_device_scene_record(d, ptr(self.record), nbytes))
        self.stage = N.gs_debug_leaf_stage()
        assert N.lib.gs_debug_leaf_stage_record(d, C.byref(self.stage), C.sizeof(self.stage) - 4) == N.GS_ERR_ARG
        N.check(N.lib.gs_debug_leaf_stage_record(d, C.byref(self.stage), C.sizeof(self.stage)))
        assert self.stage.n_quads == self.host.flat.n_quads and self.stage.lds_quads <= self.stage.n_quads
        assert self.stage.lds_cubes <= self.stage.n_cubes and (self.stage.n_cubes > 0) == (cube_lists != 0)
        self.F = L.Flat(self.host.flat)
        self.obj_ref = np.array([self.F.leaves[o.key] for o in self.sc.objs], dtype=np.uint32)
        self.mat_of = {}
        for o, ref in zip(self.sc.objs, self.obj_ref):
            self.mat_of.update(zip(o.mats, self.F.materials(int(ref))))
        self.need = np.array([o.need for o in self.sc.objs])

    def close(self):
        N.lib.gs_device_scene_destroy(self.dev)
        self.host.close()

    def fed(self, f):
        """The cases whose leaf kind instantiation f compiles in."""
        return np.array([f in COVERS[n] for n in self.need])[L.cases(self.name)["k"]]

    def run(self, kat, f, uni, n_lds, n_lcubes):
        """Every fed case through leaf_other<f, uni>; the outputs in the cases' order."""
        c = L.cases(self.name)
        n = len(c["k"])
        lay = L.uniform_layout(c["k"]) if uni else np.arange(n)
        src = np.maximum(lay, 0)
        live = (lay >= 0) & self.fed(f)[src]
        refs = np.ascontiguousarray(np.where(live, self.obj_ref[c["k"][src]], np.uint32(REF_NONE)), dtype=np.uint32)
        ray = np.ascontiguousarray(c["ray"][src])
        iv = np.ascontiguousarray(np.column_stack([c["tmin"][src], c["tmax"][src]]))
        rng = np.ascontiguousarray(c["s0"][src])
        m = len(lay)
        NF, NO, NC = kat.kat_leaf_flags(), kat.kat_leaf_out(), kat.kat_counters()
        flags, out = np.zeros((m, NF), dtype=np.uint32), np.zeros((m, NO))
        rng_out, cnt = np.zeros(m, dtype=np.uint64), np.zeros((m, NC), dtype=np.uint64)
        nonuni = np.zeros(1, dtype=np.uint32)
        flag_any = 0
        for i in range(0, m, LAUNCH):
            j = min(m, i + LAUNCH)
            _ok(kat.kat_leaf(j - i, 2 * f + int(uni), ptr(self.record), self.stage.tquads, self.stage.n_quads,
                             self.stage.n_cubes, n_lds, n_lcubes, ptr(refs[i:]), ptr(ray[i:]), ptr(iv[i:]), ptr(rng[i:]),
                             ptr(flags[i:]), ptr(out[i:]), ptr(rng_out[i:]), ptr(cnt[i:]), ptr(nonuni)))
            flag_any |= int(nonuni[0])
        res = {"flags": np.zeros((n, NF), dtype=np.uint32), "out": np.zeros((n, NO)),
               "rng": np.zeros(n, dtype=np.uint64), "cnt": np.zeros((n, NC), dtype=np.uint64)}
        for key, arr in (("flags", flags), ("out", out), ("rng", rng_out), ("cnt", cnt)):
            res[key][lay[live]] = arr[live]
        res["nonuni"] = flag_any
        return res


@pytest.fixture(scope="module")
def devs(kat):
    made = {}

    def get(name, cube_lists=1):
        if (name, cube_lists) not in made:
            made[name, cube_lists] = Dev(kat, name, cube_lists)
        return made[name, cube_lists]
    yield get
    for d in made.values():
        d.close()
    N.lib.gs_debug_set_cube_lists(1)


@pytest.fixture(scope="module")
def runs(kat, devs):
    """Each (scene, f, uni, mirror, cube_lists) run once.  mirror: "all", "none", "prefix" or "scene" (the
    prefixes the scene's own placement mirrors)."""
    made = {}

    def get(name, f, uni=False, mirror="all", cube_lists=1):
        key = (name, f, uni, mirror, cube_lists)
        if key not in made:
            dv = devs(name, cube_lists)
            nq, ncb = dv.stage.n_quads, dv.stage.n_cubes
            n_lds, n_lc = {"all": lambda: (nq, ncb), "none": lambda: (0, 0), "prefix": lambda: prefix(dv),
                           "scene": lambda: (dv.stage.lds_quads, dv.stage.lds_cubes)}[mirror]()
            made[key] = dv.run(kat, f, uni, n_lds, n_lc)
        return made[key]
    return get


def prefix(dv):
    """A strict prefix of both mirrors that leaves out tested records: up to the middle one of the
    quads the quad test reads (not a cube's, which are read from the cube records), half the cubes."""
    F = dv.F
    single = set()
    for o, ref in zip(dv.sc.objs, dv.obj_ref):
        if o.kind in ("quad", "list") or (o.kind == "cube" and (getattr(o, "flat", False) or dv.stage.n_cubes == 0)):
            _, end = F.chain(int(ref))
            members = F.members(end) if (end >> REF_SHIFT) == REF_LIST else [end]
            single |= {m & REF_MASK for m in members if (m >> REF_SHIFT) == REF_QUAD}
    single = sorted(single)
    return (single[len(single) // 2] if single else 0), dv.stage.n_cubes // 2


def same(a, b):
    for key in ("flags", "rng", "cnt"):
        if not np.array_equal(a[key], b[key]):
            return False
    return np.array_equal(_bits(a["out"]), _bits(b["out"]))


# --------------------------------------------------------------------------- the device's log
_libm_log = {}


def _draw_densities(sc, k, draws):
    """The density behind each number a medium case drew, in the stream's order: the medium's own;
    for a medium whose boundary is a medium (volume.rs:36-41 calls boundary.hit twice) the inner
    one's for the boundary's draws and its own for the third, which it takes only after both."""
    ob = sc.objs[k]
    if getattr(ob, "levels", 0) == 2:
        return [sc.objs[ob.twin].density] * min(draws, 2) + [ob.density] * (draws - 2)
    return [ob.density] * draws


def log_agrees(kat, name):
    """Per case: the device's log equals glibc's on every number the case drew (True where it drew
    none); and the case's tolerance on t where it does not -- per differing draw, 4 ulp of that
    draw's hit_dist / ray_len = |log| / density / |d| (the case's own density and ray; a rotation
    changes |d| by rounding only) -- with the number of differing draws (one rounding of the sum
    each is added where the tolerance is used)."""
    if name not in _libm_log:
        c, a, sc = L.cases(name), L.answers(name), L.scene(name)
        idx = np.flatnonzero(a["draws"] > 0)
        args = [oracle.wyrand(int(c["s0"][i]), int(a["draws"][i]))[0] for i in idx]
        x = np.ascontiguousarray(np.concatenate(args)) if args else np.zeros(0)
        dev = np.zeros(len(x))
        if len(x):
            _ok(kat.kat_math(len(x), 5, ptr(x), None, ptr(dev)))
        ref = np.array([math.log(v) if v > 0.0 else -math.inf for v in x])
        eq = _bits(dev) == _bits(ref)
        n = len(c["k"])
        ok, ulps, differ = np.ones(n, dtype=bool), np.zeros(n), np.zeros(n, dtype=np.int64)
        length = np.sqrt((c["ray"][:, 3:6] ** 2).sum(1))
        at = 0
        for i, v in zip(idx, args):
            e = eq[at:at + len(v)]
            ok[i] = e.all()
            if not ok[i]:
                dens = np.array(_draw_densities(sc, int(c["k"][i]), len(v)))
                q = np.abs(ref[at:at + len(v)]) / dens / length[i]
                ulps[i] = (4.0 * np.spacing(q[~e])).sum()
                differ[i] = int((~e).sum())
            at += len(v)
        _libm_log[name] = (ok, ulps, differ, int(len(x)), int(np.count_nonzero(~eq)))
    return _libm_log[name]


# ------------------------------------------------------------------------------ the comparison
def check(kat, dv, res, f):
    name = dv.name
    c, a, sc = L.cases(name), L.answers(name), dv.sc
    fed = dv.fed(f)
    assert fed.any()
    bvh = c["kind"] == "bvh"
    flags, out = res["flags"], res["out"]
    hit, ref, inst, enter, mat, front = (flags[:, j] for j in range(6))
    leaf = dv.obj_ref[c["k"]]
    slots = kat.slots

    # ---- chains that end in a BVH: entered, not walked
    m = fed & bvh
    if m.any():
        assert not hit[m].any() and (enter[m] >= 1).all() and np.array_equal(res["rng"][m], c["s0"][m])
        other = [j for j in range(res["cnt"].shape[1]) if j != slots[5]]
        assert not res["cnt"][m][:, other].any()
        for k in np.unique(c["k"][m]):
            mk = m & (c["k"] == k)
            o, d, end = dv.F.forward(int(dv.obj_ref[k]), c["ray"][mk, 0:3], c["ray"][mk, 3:6])
            assert (end >> REF_SHIFT) == REF_NODE
            assert np.array_equal(_bits(out[mk, 1:4]), _bits(o)) and np.array_equal(_bits(out[mk, 4:7]), _bits(d))
            node = dv.F.nodes[end & REF_MASK]
            box = np.array(list(node.min) + list(node.max))
            assert np.array_equal(_bits(out[mk, 15:21]), _bits(np.broadcast_to(box, (mk.sum(), 6)))), sc.objs[k].label
            assert len(set(enter[mk])) == 1 and (res["cnt"][mk, slots[5]] == sc.objs[k].depth).all()
        trees = {int(enter[m & (c["k"] == k)][0]) for k in np.unique(c["k"][m])}
        assert len(trees) == len(np.unique(c["k"][m]))  # a tree of its own per chain

    # ---- everything else against the oracle
    m = fed & ~bvh
    ok, ulps, differ, _, _ = log_agrees(kat, name)

    def tol(at, where):
        """4 ulp of hit_dist / ray_len and one rounding of the sum, per draw whose log differs."""
        return ulps[where] + differ[where] * np.spacing(np.abs(at[where]))
    # hit: the oracle's wherever the device's log is glibc's.  Elsewhere hit_dist moves by ulps, and the
    # decision hit_dist > dist_inside_boundary may go the other way only on the knife edge -- closest drawn
    # at the medium's own t: the t of the side that hit lies within the tolerance of the interval's end
    flip = m & ((hit != 0) != a["hit"])
    assert not (flip & ok).any(), _first(c, flip & ok)
    if flip.any():
        print("%s f=%d: %d medium decisions on the knife edge go the other way with the device's log"
              % (name, f, flip.sum()))
        t_hit = np.where(hit != 0, out[:, 0], a["t"])
        assert (np.abs(t_hit - c["tmax"])[flip] <= tol(c["tmax"], flip)).all(), _first(c, flip)
        assert flip.sum() <= 0.005 * m.sum()
    assert not enter[m].any()
    assert np.array_equal(res["rng"][m], a["state"][m]), _first(c, m & (res["rng"] != a["state"]))
    for j, key in enumerate(oracle.World.HIT_COUNTERS):
        bad = m & (res["cnt"][:, slots[j]] != a[key])
        assert not bad.any(), (key, _first(c, bad))
    other = [j for j in range(res["cnt"].shape[1]) if j not in slots]
    assert not res["cnt"][m][:, other].any()
    # the ray as leaf_other left it: the leaf's chain applied in f64
    for k in np.unique(c["k"][m]):
        if sc.objs[k].depth:
            mk = m & (c["k"] == k)
            o, d, _ = dv.F.forward(int(dv.obj_ref[k]), c["ray"][mk, 0:3], c["ray"][mk, 3:6])
            assert np.array_equal(_bits(out[mk, 1:4]), _bits(o)) and np.array_equal(_bits(out[mk, 4:7]), _bits(d))
    h = m & a["hit"] & ~flip
    is_inst = (leaf >> REF_SHIFT) == REF_INST
    assert np.array_equal(inst[h], np.where(is_inst, leaf, np.uint32(REF_NONE))[h])
    want_mat = np.array([dv.mat_of.get(int(x), -1) for x in a["mat"]])
    assert np.array_equal(mat[h].astype(np.int64), want_mat[h]), _first(c, h & (mat.astype(np.int64) != want_mat))
    assert np.array_equal(front[h] != 0, a["front"][h]), _first(c, h & ((front != 0) != a["front"]))
    # t, and what reconstruct makes of it: bit for bit where the device's log is libm's
    e = h & ok
    bad = e & (_bits(out[:, 0]) != _bits(a["t"]))
    assert not bad.any(), _first(c, bad)
    for cols, key in ((slice(7, 10), "p"), (slice(10, 13), "n")):
        bad = e & (_bits(out[:, cols]) != _bits(a[key])).any(1)
        assert not bad.any(), (key, _first(c, bad))
    uv = e & np.isin(ref >> REF_SHIFT, (REF_QUAD, REF_TRI))
    assert uv.any() or name == "media"
    assert np.array_equal(_bits(out[uv, 13]), _bits(a["u"][uv])) and np.array_equal(_bits(out[uv, 14]), _bits(a["v"][uv]))
    med = h & (c["kind"] == "medium")
    assert (out[med, 13] == 0.0).all() and (out[med, 14] == 0.0).all()
    # the cases left out of the bit comparison of t
    left = h & ~ok
    assert (np.abs(out[:, 0] - a["t"])[left] <= tol(a["t"], left)).all(), _first(c, left)


def _first(c, bad):
    """The first few failing cases, for the assertion's message."""
    idx = np.flatnonzero(bad)[:5]
    return [(int(i), str(c["label"][i]), str(c["tag"][i]), str(c["iv"][i])) for i in idx]


def _feats(name):
    return COVERS[L.scene(name).need]


@pytest.mark.parametrize("name", NAMES)
def test_leaf_other_matches_the_oracle(kat, devs, runs, name):
    """Per-lane loads, both mirrors whole, cube lists on: every instantiation against the oracle."""
    for f in _feats(name):
        check(kat, devs(name), runs(name, f), f)


@pytest.mark.parametrize("name", NAMES)
def test_uniform_loads_equal_per_lane_loads(kat, devs, runs, name):
    """UNI = true -- one ref per wave, taken by readfirstlane, scalar loads -- gives what UNI = false
    gives on waves that mix refs, kinds and mirrored and unmirrored records."""
    for f in _feats(name):
        u = runs(name, f, uni=True)
        assert u["nonuni"] == 0
        assert same(u, runs(name, f)), f
        assert same(u, runs(name, f, mirror="prefix")), f


@pytest.mark.parametrize("name", NAMES)
def test_mirror_settings_give_identical_outputs(kat, devs, runs, name):
    """The quad and cube mirrors empty, whole, a strict prefix that leaves some of the tested quads and
    cubes in global memory while every wave holds both kinds of lanes, and the scene's own prefixes."""
    dv = devs(name)
    n_lds, n_lc = prefix(dv)
    if name == "plain":
        assert 0 < n_lds < dv.stage.n_quads and 0 < n_lc < dv.stage.n_cubes
    for f in _feats(name):
        full = runs(name, f)
        assert same(full, runs(name, f, mirror="none")), f
        assert same(full, runs(name, f, mirror="prefix")), f
        assert same(full, runs(name, f, mirror="scene")), f


@pytest.mark.parametrize("name", NAMES)
def test_cube_lists_off_gives_identical_outputs(kat, devs, runs, name):
    """cube_test's straight-line faces against the generic loop over the same six TQuad records
    (gs_debug_set_cube_lists(0) at upload): identical outputs, counters included."""
    assert devs(name, 0).stage.n_cubes == 0 and devs(name).stage.n_cubes > 0
    for f in _feats(name):
        off = runs(name, f, cube_lists=0)
        assert same(off, runs(name, f)), f
        assert same(off, runs(name, f, mirror="none", cube_lists=0)), f
    check(kat, devs(name, 0), runs(name, _feats(name)[-1], cube_lists=0), _feats(name)[-1])


def test_log_share(kat):
    """The share of medium cases left out of the bit comparison of t -- a case one of whose draws'
    log differs between the device and glibc -- stays under 5%.  Observed on MI355X: 164 of 5518
    medium cases (2.97%); 168 of 5404 log arguments differ; 6 knife-edge decisions go the other way."""
    cases = left = 0
    for name in NAMES:
        c, a = L.cases(name), L.answers(name)
        ok, _, _, n_args, n_diff = log_agrees(kat, name)
        med = c["kind"] == "medium"
        cases += int(med.sum())
        left += int((med & ~ok).sum())
        print("%s: %d medium cases, %d left out; %d log arguments, %d differ" % (name, med.sum(), (med & ~ok).sum(),
                                                                               n_args, n_diff))
    print("left out: %d of %d medium cases (%.2f%%)" % (left, cases, 100.0 * left / cases))
    assert cases >= 4000 and left / cases < LOG_CAP
