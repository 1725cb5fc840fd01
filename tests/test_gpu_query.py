"""Ray queries on the device (gs_query_rays, gs_query_rays_async; csrc/device/query.hip) against the
reference's world.hit, which is the oracle's hit of the scene's *twin* (tests/query_cases.py): one
BVH of the world's members in their order.

Closest, per ray, bit for bit: hit, t, p, n, front, the stream after, a quad's and a triangle's
u, v, and all eight test counters; the material through the flat scene's numbering (the anchors
the shading KAT matches leaves by).  A sphere's u, v pass through acos / atan2: equal, or within
4 * 2^-52.  A ray whose walk took a free-flight draw passes through log: state and
counters stay exact, t is equal or within 4 ulp of hit_dist / ray_len plus the sum's rounding
(DESIGN.md §2.5), and at most 5% of the draw-taking rays may differ in bits at all (measured on
MI355X: test_closest_matches_the_twin's docstring).  A NaN is compared as a NaN (_bits).

Any: the same walk up to its first acceptance.  Then what must not matter: a ray's place in its
batch, the batch's size, what else runs on the scene."""
import ctypes as C

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import query as GQ
from grayshift_amd import scenes
from grayshift_amd.scene import camera_spec, fixed_spp

import oracle

from tests import query_cases as Q
from tests.shade_cases import REF_MEDIUM, REF_MSPHERE, REF_QUAD, REF_SHIFT, REF_SPHERE, REF_TRI

pytestmark = pytest.mark.gpu
DRAW_CAP = 0.05
WY_C0 = 0x2d358dccaa6c78a5
COUNTERS = oracle.World.HIT_COUNTERS
DENSITY = {"media": (0.6, 0.3), "fog": (0.4,), "nested_medium": (1.2,), "bvh_boundary": (0.8,),
           "bvh_boundary_chain": (0.8,), "nested_media": (1.5, 0.7, 2.0, 0.9), "general_all": (1.0,)}


def _bits(a):
    """The f64 bit patterns, every NaN as one pattern: a NaN's sign and payload are not arithmetic
    (x86 and gfx950 make different default NaNs), that it is a NaN is (a NaN direction makes the
    reference's triangle, which ignores ray_t, a hit at t = NaN)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def _ulp(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(np.isfinite(x), np.nextafter(x, np.inf) - x, 0.0)


@pytest.fixture(scope="module")
def devs(built):
    made = {}

    def get(name):
        if name not in made:
            rq = g.RayQuery(Q.scene(name).spec)
            rq.mat = Q.material_map(Q.scene(name), rq.host.flat)
            info = N.gs_scene_info()
            N.check(N.lib.gs_device_scene_info(rq.dev, C.byref(info)))
            rq.feat = info.feat
            made[name] = rq
        return made[name]
    yield get
    for rq in made.values():
        rq.close()


@pytest.fixture(scope="module")
def closest(devs):
    """Each scene's whole ray set through gs_query_rays once (closest, with counters)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = devs(name).closest(Q.rays(name)[0], seed=Q.SEED, counts=True)
        return made[name]
    return get


def _draw_tolerance(name, r, a):
    """Per ray that drew: the bound on |t - t_ref| -- per draw 4 ulp of that draw's hit_dist / ray_len
    = |log u| / density / |d| (the scene's thinnest medium: an upper bound for every draw), plus one
    rounding of the sum at t each."""
    s0 = Q.seeds(len(r))
    moved = np.flatnonzero(a["state"] != s0)
    tol = np.zeros(len(r))
    dens = min(DENSITY[name])
    for i in moved:
        step = (int(a["state"][i]) - int(s0[i])) % (1 << 64)  # wyrand adds its constant once per draw
        k = next(k for k in range(1, 257) if (k * WY_C0) % (1 << 64) == step)  # draws taken
        f, _ = oracle.wyrand(int(s0[i]), k)
        v = np.abs(np.log(f[:k])) / dens / np.linalg.norm(r[i, 3:6])
        tol[i] = (4.0 * _ulp(v)).sum() + k * _ulp(a["t"][i])
    return moved, tol


@pytest.mark.parametrize("name", sorted(Q.SCENES) + sorted(Q.GENERAL))
def test_closest_matches_the_twin(name, devs, closest):
    """The share of the draw-taking rays whose record differs from the twin's in any bit is printed
    per scene.  MI355X: media 2 of 554, fog 5 of 1386, nested_medium 1 of 139, the other media
    scenes 0."""
    r, tags = Q.rays(name)
    a, d, rq = Q.answers(name), closest(name), devs(name)
    if name in Q.SCENES:
        assert rq.feat & (1 | 2 | 512) == Q.FEAT_BITS[name]
    else:
        assert rq.feat & 512
    off = np.flatnonzero((d["hit"] != a["hit"]) | (d["state"] != a["state"]))
    assert len(off) == 0, (len(off), off[:8], [tags[i] for i in off[:8]])
    for j, c in enumerate(COUNTERS):
        off = np.flatnonzero(d[c].astype(np.uint64) != a[c])
        assert len(off) == 0, (c, len(off), off[:8], [tags[i] for i in off[:8]], d[c][off[:8]], a[c][off[:8]])
    hit = a["hit"]
    t_ref = np.where(hit, a["t"], r[:, 8])  # a miss: the tmax given
    moved, tol = (np.zeros(0, dtype=int), np.zeros(len(r))) if name not in DENSITY else _draw_tolerance(name, r, a)
    differs = _bits(d["t"]) != _bits(t_ref)
    for key in ("p", "n"):
        differs |= (_bits(d[key]) != _bits(np.where(hit[:, None], a[key], 0.0))).any(axis=1)
    drew = np.zeros(len(r), dtype=bool)
    drew[moved] = True
    print("%s: %d rays, %d hits, %d drew, %d of them differ in bits" % (name, len(r), hit.sum(), drew.sum(),
                                                                       (differs & drew).sum()))
    assert not (differs & ~drew).any(), np.flatnonzero(differs & ~drew)[:8]
    if drew.any():
        assert (differs & drew).sum() <= DRAW_CAP * drew.sum()
        bad = differs & drew
        assert (np.abs(d["t"][bad] - t_ref[bad]) <= tol[bad]).all()
        dn = np.linalg.norm(r[bad, 3:6], axis=1)
        assert (np.abs(d["p"][bad] - a["p"][bad]).max(axis=1, initial=0.0) <= 2.0 * dn * tol[bad] + 4.0 * _ulp(a["p"][bad]).max(axis=1, initial=0.0)).all()
        assert np.array_equal(_bits(d["n"][bad]), _bits(a["n"][bad]))
    assert np.array_equal(d["front"][hit], a["front"][hit]) and not d["front"][~hit].any()
    kind = d["ref"] >> REF_SHIFT
    assert (kind[hit] != 0).all() and (d["ref"][~hit] == 0).all() and (d["inst"][~hit] == 0).all()
    assert (d["material"][~hit] == 0).all()
    exact_uv = hit & np.isin(kind, (REF_QUAD, REF_TRI, REF_MEDIUM)) & ~(differs & drew)
    round_uv = hit & np.isin(kind, (REF_SPHERE, REF_MSPHERE))
    assert (exact_uv | round_uv)[hit & ~(differs & drew)].all()
    for key in ("u", "v"):
        assert np.array_equal(_bits(d[key][exact_uv]), _bits(a[key][exact_uv])), key
        du = np.abs(d[key][round_uv] - a[key][round_uv])
        assert ((du <= 4.0 * 2.0 ** -52) | (np.isnan(d[key][round_uv]) & np.isnan(a[key][round_uv]))).all(), key
        assert (_bits(d[key][~hit]) == 0).all()
    mapped = np.array([rq.mat.get(int(m), -1) for m in d["material"]])
    known = hit & (mapped >= 0)
    assert np.array_equal(mapped[known], a["mat"][known])
    if name in Q.SCENES:
        assert known[hit].all()  # every material of these scenes is matched
    else:
        assert known[hit].mean() > 0.5


@pytest.mark.parametrize("name", sorted(Q.SCENES) + ["nested_medium", "bvh_boundary_chain", "general_all"])
def test_any_is_the_same_walk_up_to_its_first_acceptance(name, devs, closest):
    r, _ = Q.rays(name)
    c = closest(name)
    y = devs(name).any(r, seed=Q.SEED, counts=True)
    assert np.array_equal(y["hit"], c["hit"])
    hit = y["hit"]
    kind = y["ref"] >> REF_SHIFT
    h = hit & (kind != REF_TRI)  # (Triangle::hit ignores ray_t: triangle.rs:34-68)
    h &= ~np.isnan(r[:, 7]) & ~np.isnan(r[:, 8])  # (a NaN end bounds nothing: a medium's clips never take it)
    # the reference's own interval ends: a sphere's root must lie inside (sphere.rs:76-81, surrounds);
    # a quad's plane hit and a medium's clipped span may sit on them (plane.rs:20-32, contains;
    # volume.rs:43-44) -- the tmax = t rays of the set do
    op = h & np.isin(kind, (REF_SPHERE, REF_MSPHERE))
    assert (r[op, 7] < y["t"][op]).all() and (y["t"][op] < r[op, 8]).all()
    assert (r[h, 7] <= y["t"][h]).all() and (y["t"][h] <= r[h, 8]).all()
    h2 = h & ((c["ref"] >> REF_SHIFT) != REF_TRI)  # (closest's own answer may be a farther triangle)
    assert (y["t"][h2] >= c["t"][h2]).all()
    assert np.array_equal(_bits(y["t"][~hit]), _bits(r[~hit, 8]))
    assert (y["node_visits"] <= c["node_visits"]).all()
    for k in COUNTERS:
        assert (y[k] <= c[k]).all(), k
    if (c["node_visits"] > 1).any():
        assert y["node_visits"].sum() < c["node_visits"].sum()
    else:  # tiny1, tiny2: one node is the whole tree, so every walk visits it and nothing else
        assert np.array_equal(y["node_visits"], c["node_visits"])
        total = lambda q: sum(int(q[k].sum()) for k in COUNTERS)
        assert total(y) < total(c) if name != "tiny1" else total(y) == total(c)  # (one member: nothing follows a hit)
    # a ray whose first acceptance ends the closest walk too has the closest record
    same = hit & (y["node_visits"] == c["node_visits"]) & (y["ref"] == c["ref"])
    assert np.array_equal(_bits(y["t"][same]), _bits(c["t"][same]))


FIELDS = ("hit", "front", "t", "p", "n", "u", "v", "material", "ref", "inst") + tuple(COUNTERS)


def _same(a, ia, b, ib, fields=FIELDS):
    for k in fields:
        x, y = a[k][ia], b[k][ib]
        if x.dtype == np.float64:
            x, y = _bits(x), _bits(y)
        if not np.array_equal(x, y):
            return k
    return None


def test_a_rays_place_in_its_batch_does_not_matter(devs, closest):
    """mixed takes no draws: 257 rays alone, at offset 1000 of the whole set, and reversed -- every
    record identical field by field; the stream word is the ray's own untouched stream."""
    r, _ = Q.rays("mixed")
    rq, whole = devs("mixed"), closest("mixed")
    part = np.ascontiguousarray(r[1000:1257])
    alone = rq.closest(part, seed=Q.SEED, counts=True)
    rev = rq.closest(np.ascontiguousarray(part[::-1]), seed=Q.SEED, counts=True)
    idx = np.arange(257)
    assert _same(alone, idx, whole, idx + 1000) is None
    assert _same(alone, idx, rev, idx[::-1]) is None
    assert np.array_equal(alone["state"], Q.seeds(257)) and np.array_equal(rev["state"], Q.seeds(257))
    assert np.array_equal(whole["state"][1000:1257], Q.seeds(257, first=1000))
    assert alone["hit"].any() and not alone["hit"].all()


def test_media_records_depend_on_the_index_through_the_stream_only(devs, closest):
    r, _ = Q.rays("media")
    rq, whole = devs("media"), closest("media")
    again = rq.closest(r, seed=Q.SEED, counts=True)
    idx = np.arange(len(r))
    assert _same(again, idx, whole, idx, FIELDS + ("state",)) is None
    # the same rays at other indices: the answer is the twin's at those indices' streams
    part = np.ascontiguousarray(r[3000:3257])
    d = rq.closest(part, seed=Q.SEED, counts=True)
    a = Q.twin_hit("media", part, Q.seeds(257))
    assert np.array_equal(d["hit"], a["hit"]) and np.array_equal(d["state"], a["state"])
    moved = a["state"] != Q.seeds(257)
    assert moved.any()
    assert np.array_equal(_bits(d["t"][~moved]), _bits(np.where(a["hit"], a["t"], part[:, 8])[~moved]))
    other = rq.closest(part, seed=Q.SEED + 1)
    assert not np.array_equal(other["state"], d["state"])


class DevBuf:
    def __init__(self, nbytes, fill=None):
        self.p = C.c_void_p()
        self.n = nbytes
        N.check(N.lib.gs_device_alloc(max(nbytes, 8), C.byref(self.p)))
        if fill is not None:
            self.put(np.full(nbytes, fill, dtype=np.uint8))

    def put(self, a):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            N.check(N.lib.gs_device_upload(self.p, a.ctypes.data, a.nbytes))

    def get(self):
        out = np.zeros(self.n, dtype=np.uint8)
        if self.n:
            N.check(N.lib.gs_device_download(out.ctypes.data, self.p, self.n))
        return out

    def free(self):
        N.lib.gs_device_free(self.p)


@pytest.mark.parametrize("mode", [N.GS_QUERY_CLOSEST, N.GS_QUERY_ANY])
@pytest.mark.parametrize("n", Q.BATCHES)
def test_batch_edges_write_nothing_past_n(n, mode, devs):
    """The async form on caller buffers, over-allocated and poisoned: the first n records equal the
    synchronous form's, nothing after them is touched (a block is 256 lanes, a wave 64)."""
    rq = devs("mixed")
    r = np.ascontiguousarray(Q.rays("mixed")[0][:n])
    pad, poison = 70, 0xA5
    d_r, d_h, d_c = DevBuf(max(n, 1) * 72), DevBuf((n + pad) * 104, poison), DevBuf((n + pad) * 32, poison)
    try:
        d_r.put(r)
        N.check(N.lib.gs_query_rays_async(rq.dev, d_r.p, n, mode, Q.SEED, d_h.p, d_c.p, None))
        hb, cb = d_h.get(), d_c.get()  # (the download synchronises)
    finally:
        for b in (d_r, d_h, d_c):
            b.free()
    assert (hb[n * 104:] == poison).all() and (cb[n * 32:] == poison).all()
    if n == 0:
        return
    ref = rq._run(r, mode, Q.SEED, True)
    hits = hb[:n * 104].view(GQ.HIT_DTYPE)
    cnt = cb[:n * 32].view(np.uint32).reshape(n, 8)
    assert np.array_equal(hits["hit"] != 0, ref["hit"]) and np.array_equal(_bits(hits["t"]), _bits(ref["t"]))
    assert np.array_equal(_bits(hits["p"]), _bits(ref["p"])) and np.array_equal(hits["state"], ref["state"])
    assert np.array_equal(hits["ref"], ref["ref"]) and (hits["pad"] == 0).all()
    assert np.array_equal(cnt[:, 0], ref["node_visits"]) and np.array_equal(cnt[:, 7], ref["medium_tests"])
    a = Q.answers("mixed")
    if mode == N.GS_QUERY_CLOSEST:
        assert np.array_equal(hits["hit"] != 0, a["hit"][:n])


@pytest.mark.parametrize("name", ["mixed", "media", "tiny1", "tiny2", "tiny3"])
def test_malformed_rays_complete_with_the_references_answer(name, devs, closest):
    """NaN, infinities, a zero direction and empty intervals are inputs the entry accepts by contract:
    the walk ends and the record is what the reference's arithmetic gives."""
    r, tags = Q.rays(name)
    sel = np.isin(np.array(tags), ("empty", "zero_dir", "bad_o", "bad_d", "bad_iv", "bad_all", "axis", "face"))
    assert sel.sum() > 40
    a, d = Q.answers(name), closest(name)
    assert np.array_equal(d["hit"][sel], a["hit"][sel])
    assert np.array_equal(d["state"][sel], a["state"][sel])
    for c in COUNTERS:
        assert np.array_equal(d[c][sel].astype(np.uint64), a[c][sel]), c
    t_ref = np.where(a["hit"], a["t"], r[:, 8])
    nodraw = sel & (a["state"] == Q.seeds(len(r)))
    assert np.array_equal(_bits(d["t"][nodraw]), _bits(t_ref[nodraw]))  # (a NaN tmax comes back as given)
    y = devs(name).any(np.ascontiguousarray(r[sel]), seed=Q.SEED)
    assert y["hit"].shape == (int(sel.sum()),)


def _frame_scene():
    sc = Q.scene("media")
    cam = camera_spec(1.0, 96, 8, 40.0, (0.0, 2.0, 26.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 10.0)
    return scenes.Scene("query_media", sc.spec, cam, fixed_spp(4))


def _last_feat(m):
    d, f = C.c_void_p(), C.c_int32()
    N.check(N.lib.gs_multi_scene(m.handle, 0, C.byref(d)))
    N.check(N.lib.gs_debug_last_launch_feat(d, C.byref(f)))
    return f.value


def test_a_query_beside_renders_changes_nothing(closest):
    """One frame context (one device scene): query, render, query, render -- both frames, their
    counters and the last launched render instantiation equal a context's that never queried; the
    query, which shares the scene's records with the renders, answers as on a scene of its own,
    before and between them."""
    sc = _frame_scene()
    r = np.ascontiguousarray(Q.rays("media")[0][:1500])
    want = closest("media")
    plain = g.MultiRenderer(sc, num_gpus=1)
    try:
        p1 = plain.render(seed=3, rgb=True)
        p2 = plain.render(seed=3, rgb=True)
        feat = _last_feat(plain)
    finally:
        plain.close()
    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        q = m.query()
        f0 = _last_feat(m)
        before = q.closest(r, seed=Q.SEED, counts=True)
        assert _last_feat(m) == f0                         # a query is no render launch
        f1 = m.render(seed=3, rgb=True)
        f_after = _last_feat(m)
        mid = q.closest(r, seed=Q.SEED, counts=True)
        assert _last_feat(m) == f_after
        f2 = m.render(seed=3, rgb=True)
        q.close()
    finally:
        m.close()
    assert feat == f_after and feat >= 0
    for a, b in ((p1, f1), (p2, f2)):
        assert np.array_equal(a["rgb"], b["rgb"]) and a["counters"] == b["counters"]
    idx = np.arange(len(r))
    assert _same(before, idx, want, idx, FIELDS + ("state",)) is None
    assert _same(mid, idx, want, idx, FIELDS + ("state",)) is None


@pytest.mark.parametrize("name", sorted(Q.GENERAL))
def test_general_scenes_launch_the_catch_all_set(name, devs, closest):
    """GS_FEAT_GENERAL scenes are supported: their instantiation compiles without scratch
    (tests/test_code_object.py asserts that of every kernel in the library), so the compositions of
    tests/test_gpu_composition.py are cases of test_closest_matches_the_twin; here, that they reach
    the paths they are for."""
    rq, d = devs(name), closest(name)
    assert rq.feat & 512
    assert d["instance_tests"].sum() > 0 or name.startswith("bvh_boundary") or name == "nested_media"
    if name in DENSITY:
        assert d["medium_tests"].sum() > 0
    if name.startswith("bvh_boundary") or name == "general_all":
        a = Q.answers(name)
        assert (a["node_visits"] > 3).any()  # (a medium boundary's tree is walked and counted too)
