"""The cases of the leaf stage's known-answer tests (tests/leaf_cases.py) reach the branches they
are for -- asserted on the oracle's answers alone, no GPU: what keeps tests/test_gpu_leaf_kat.py
from being a comparison over easy rays.  At least 16 cases per branch; at least 4 where the case
is built, not drawn (an exact equality)."""
import numpy as np
import pytest

import ctypes as C

import grayshift_amd as g
from grayshift_amd import _native as N

from tests import leaf_cases as L

NAMES = sorted(L.SCENES)


def _all(key, source=L.cases):
    return np.concatenate([source(n)[key] for n in NAMES])


def _count(mask):
    return int(np.count_nonzero(mask))


def test_leaf_stage_record_checks_its_arguments():
    out = N.gs_debug_leaf_stage()
    assert C.sizeof(out) == 24
    assert N.lib.gs_debug_leaf_stage_record(None, C.byref(out), C.sizeof(out)) == N.GS_ERR_ARG
    assert b"null" in N.lib.gs_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_every_object_has_its_leaf_and_its_materials(name):
    sc = L.scene(name)
    host = g.HostScene(sc.spec)
    try:
        F = L.Flat(host.flat)
        assert len(F.leaves) == len(sc.objs)
        pairs = set()
        for ob in sc.objs:
            ref = F.leaves[ob.key]
            flat_mats = F.materials(ref)
            assert len(flat_mats) == len(ob.mats), ob.label
            pairs |= set(zip(ob.mats, flat_mats))
            assert len(F.chain(ref)[0]) == ob.depth, ob.label
        # the spec's and the flat scene's material numbers correspond one to one
        assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs})
    finally:
        host.close()


@pytest.mark.parametrize("name", NAMES)
def test_scenes_are_small_and_waves_are_mixed(name):
    c, sc = L.cases(name), L.scene(name)
    assert len(sc.objs) <= 40 and 1000 <= len(c["k"]) <= 6000
    # the mixed order: every run of 64 holds several objects
    per_wave = [len(set(c["k"][i:i + 64])) for i in range(0, len(c["k"]) - 63, 64)]
    assert min(per_wave) >= min(4, len(sc.objs))
    lay = L.uniform_layout(c["k"])
    assert len(lay) % 64 == 0 and sorted(lay[lay >= 0]) == list(range(len(c["k"])))
    for i in range(0, len(lay), 64):
        w = lay[i:i + 64]
        assert len(set(c["k"][w[w >= 0]])) == 1


def test_every_kind_hits_and_misses():
    kind, hit = _all("kind"), _all("hit", L.answers)
    for k in ("sphere", "msphere", "quad", "tri", "list", "cube", "medium"):
        assert _count((kind == k) & hit) >= 16 and _count((kind == k) & ~hit) >= 16, k


def test_chains_of_depth_1_4_and_16():
    for name, labels in (("plain", ("sphere_chain1", "msphere_chain4", "quad_chain4", "quad_oblique_chain1", "tri_chain4",
                                    "cube_chain4", "list_mixed_chain1")),
                         ("general", ("sphere_chain16", "msphere_chain16", "quad_chain16", "tri_chain16", "cube_chain16",
                                      "list_mixed_chain16", "medium_sphere_bchain16")),
                         ("nested", ("bvh_chain1", "bvh_chain2", "bvh_chain4")), ("general", ("bvh_chain16", "bvh_chain2"))):
        c, a = L.cases(name), L.answers(name)
        for lab in labels:
            m = c["label"] == lab
            assert _count(m & a["hit"]) >= 16 and _count(m & ~a["hit"]) >= 16, lab
            assert a["instance_tests"][m].min() >= int("".join(ch for ch in lab.split("chain")[-1] if ch.isdigit())), lab
    ob = {o.label: o for o in L.scene("general").objs}
    assert ob["sphere_chain16"].depth == 16 and ob["bvh_chain16"].depth == 16


def test_interval_ends():
    kind, iv, tag, hit = _all("kind"), _all("iv"), _all("tag"), _all("hit", L.answers)
    t, tmin, tmax = _all("t", L.answers), _all("tmin"), _all("tmax")
    closed = np.isin(kind, ("quad", "cube"))
    # closest drawn below, at and above the oracle's own t; tmin at and above it
    for k in ("sphere", "msphere", "quad", "tri", "list", "cube"):
        for name in L.INTERVALS:
            assert _count((kind == k) & (iv == name)) >= 16, (k, name)
    # the closed interval of quads and cube faces: t == tmax and t == tmin are hits, at that t
    m = closed & (iv == "closest_equal")
    assert _count(m) >= 16 and hit[m].all() and np.array_equal(t[m], tmax[m])
    m = closed & (iv == "tmin_equal")
    assert _count(m) >= 16 and hit[m].all() and np.array_equal(t[m], tmin[m])
    # the open one of spheres: the root at an end is not taken (the other root may be)
    m = np.isin(kind, ("sphere", "msphere")) & (iv == "closest_equal")
    assert _count(m) >= 16 and not (hit[m] & (t[m] == tmax[m])).any() and _count(m & ~hit) >= 16
    m = np.isin(kind, ("sphere", "msphere")) & (iv == "tmin_equal")
    assert _count(m) >= 16 and not (hit[m] & (t[m] == tmin[m])).any() and _count(m & hit) >= 16
    # an ulp inside: taken again
    for k in ("sphere", "quad", "cube", "list"):
        m = (kind == k) & (iv == "closest_above")
        assert _count(m) >= 16 and hit[m].all(), k
    # the built ones
    for k in ("quad", "cube"):
        for name, want in (("t_eq_tmin", True), ("t_eq_tmax", True), ("t_gt_tmax", False)):
            m = (kind == k) & (tag == name) & (iv == "exact")
            assert _count(m) >= 4 and (hit[m] == want).all(), (k, name)
        m = (kind == k) & (tag == "t_eq_tmin") & (iv == "exact")
        assert np.array_equal(t[m], tmin[m])
        m = (kind == k) & (tag == "t_eq_tmax") & (iv == "exact")
        assert np.array_equal(t[m], tmax[m])
    m = (kind == "quad") & (tag == "t_lt_tmin") & (iv == "exact")
    assert _count(m) >= 4 and not hit[m].any()
    m = (kind == "cube") & (tag == "t_lt_tmin") & (iv == "exact")  # the far face instead
    assert _count(m) >= 4 and hit[m].all() and (t[m] > tmin[m]).all()
    for name, want in (("root_eq_tmin", True), ("root_eq_tmin_tmax", False), ("root_eq_tmax", False), ("root_in", True),
                       ("root_far_in", True)):
        m = (kind == "sphere") & (tag == name)
        assert _count(m) >= 4 and (hit[m] == want).all(), name
    m = (kind == "sphere") & (tag == "root_eq_tmin")
    assert (t[m] == 1.5 * tmin[m]).all()  # the far root, 6 / s


def test_face_edges_and_the_plane_threshold():
    kind, iv, tag, hit = _all("kind"), _all("iv"), _all("tag"), _all("hit", L.answers)
    u, v = _all("u", L.answers), _all("v", L.answers)
    base = (kind == "quad") & (iv == "open")
    for name, arr, val in (("alpha0", u, 0.0), ("alpha1", u, 1.0), ("beta0", v, 0.0), ("beta1", v, 1.0)):
        m = base & (tag == name)
        assert _count(m) >= 4 and hit[m].all() and (arr[m] == val).all(), name
    m = base & (tag == "corner")
    assert _count(m) >= 4 and hit[m].all() and np.isin(u[m], (0.0, 1.0)).all() and np.isin(v[m], (0.0, 1.0)).all()
    for name in ("alpha_out", "beta_out"):
        m = base & (tag == name)
        assert _count(m) >= 4 and not hit[m].any(), name
    for k in ("quad", "cube"):
        for name, want in (("den_below", False), ("den_at", True), ("den_above", True)):
            m = (kind == k) & (tag == name) & (iv == "open")
            assert _count(m) >= 4 and (hit[m] == want).all(), (k, name)
    m = (kind == "cube") & (tag == "parallel") & (iv == "open")
    assert _count(m & hit) >= 4 and _count(m & ~hit) >= 4  # (in the plane of a face: the edge's alpha / beta decides)


def test_ties():
    c, a, sc = L.cases("plain"), L.answers("plain"), L.scene("plain")
    # two coincident quads: every hit is the later one's
    ob = next(o for o in sc.objs if o.label == "list_coincident")
    m = (c["label"] == "list_coincident") & a["hit"]
    assert _count(m) >= 16 and (a["mat"][m] == ob.later).all()
    assert (a["quad_tests"][c["label"] == "list_coincident"] == 2).all()
    # a ray through an edge of the cube lies in two faces at one t, through a corner in three: the
    # later face of the list wins, which the normal names (faces: +z, +x, -z, -x, +y, -y)
    m = np.isin(c["label"], ("cube", "cube_b", "cube_c")) & (c["iv"] == "open") & a["hit"]
    e, k = m & (c["tag"] == "edge"), m & (c["tag"] == "corner")
    assert _count(e) >= 4 and _count(k) >= 4
    on_faces = (np.abs(np.abs(a["p"] - np.round(a["p"] / L.STEP) * L.STEP) - 1.0) == 0.0).sum(1)
    assert (on_faces[e] == 2).all() and (on_faces[k] == 3).all()
    from_outside = a["front"]
    assert (np.abs(a["n"][e & from_outside, 2]) == 0.0).all()  # +z lost to the later x or y face
    assert (np.abs(a["n"][k & from_outside, 1]) == 1.0).all()  # the y face, the last of the three
    # the flat cube: its two y faces coincide, the later one (-y, normal against the ray) wins
    m = (c["label"] == "cube_flat") & a["hit"]
    assert _count(m) >= 16 and (a["quad_tests"][c["label"] == "cube_flat"] == 6).all()


def test_the_triangle_ignores_its_interval():
    kind, iv, tag, hit = _all("kind"), _all("iv"), _all("tag"), _all("hit", L.answers)
    t, tmax = _all("t", L.answers), _all("tmax")
    m = (kind == "tri") & (iv == "tri_beyond")
    assert _count(m) >= 16 and hit[m].all() and (t[m] > tmax[m]).all()
    m = (kind == "tri") & (tag == "tri_behind")
    assert _count(m) >= 16 and hit[m].all() and (t[m] < 0.0).all()
    m = (kind == "tri") & (iv == "closest_below")
    assert _count(m) >= 16 and hit[m].all()
    # in a list: after a nearer quad (it overrides it) and before one (tested against the triangle's t)
    c, a, sc = L.cases("plain"), L.answers("plain"), L.scene("plain")
    ob = next(o for o in sc.objs if o.label == "list_tri_between")
    base = (c["label"] == "list_tri_between") & (c["iv"] == "open")
    m = base & (c["tag"] == "tri_overrides")
    assert _count(m) >= 4 and a["hit"][m].all() and (a["mat"][m] == ob.mats[2]).all()
    assert (a["t"][m] * -c["ray"][m, 5] == 4.0).all()  # farther than the first quad's 3 / s
    m = base & (c["tag"] == "tri_wins")
    assert _count(m) >= 4 and (a["mat"][m] == ob.mats[1]).all() and (a["t"][m] * -c["ray"][m, 5] == 5.0).all()
    m = base & (c["tag"] == "tri_culled")
    assert _count(m) >= 4 and (a["mat"][m] == ob.mats[2]).all()
    m = base & (c["tag"] == "tri_behind_in_list")
    assert _count(m) >= 4 and a["hit"][m].all() and (a["t"][m] * -c["ray"][m, 5] == -1.0).all()
    assert (a["mat"][m] == ob.mats[1]).all()
    m = (c["label"] == "list_tri_between") & (c["tag"] == "rand") & a["hit"]
    assert _count(m & (a["mat"] == ob.mats[1])) >= 16


def _medium_branches(name):
    c, a, sc = L.cases(name), L.answers(name), L.scene(name)
    has1, t1, has2, t2, before = L.boundary_hits(name, c["k"], c["ray"], c["s0"])
    twin = np.array([o.kind == "medium" and o.twin is not None for o in sc.objs])[c["k"]]
    both = twin & has1 & has2
    c1, c2 = np.where(t1 < c["tmin"], c["tmin"], t1), np.where(t2 > c["tmax"], c["tmax"], t2)
    own = L.S.draws(before, a["state"], most=2)  # the medium's own draw, after its boundary's
    out = {"no_first_hit": twin & ~has1, "no_second_hit": twin & has1 & ~has2, "t1_below_tmin": both & (t1 < c["tmin"]),
           "t2_above_closest": both & (t2 > c["tmax"]), "crossed": both & (c1 >= c2),
           "drawn_rejected": both & (own == 1) & ~a["hit"], "drawn_accepted": both & (own == 1) & a["hit"],
           "no_draw": twin & (own == 0)}
    # the draw is taken exactly when both hits exist and the clipped interval is not empty
    assert np.array_equal(own[twin] == 1, (both & ~(c1 >= c2))[twin])
    assert not (a["hit"] & twin & (own == 0)).any()
    return c, a, sc, out


def test_medium_clips_and_draws():
    total = {}
    for name in ("media", "general"):
        c, a, sc, br = _medium_branches(name)
        for key, m in br.items():
            total[key] = total.get(key, 0) + _count(m)
        if name == "media":
            for key, m in br.items():
                assert _count(m) >= 16, key
            # every kind of boundary: a sphere, a cube, a single quad (never a second hit)
            for lab in ("medium_sphere_0", "medium_sphere_3", "medium_cube", "medium_sphere_bchain2",
                        "medium_cube_bchain1_chain2"):
                m = c["label"] == lab
                assert _count(m & br["drawn_accepted"]) >= 4 and _count(m & br["drawn_rejected"]) >= 4, lab
            m = c["label"] == "medium_quad"
            assert _count(m & br["no_second_hit"]) >= 16 and not a["hit"][m].any() and (a["draws"][m] == 0).all()
            # origins outside and inside (t1 < 0 < tmin), densities over three decades
            assert _count(br["t1_below_tmin"] & (c["tag"] == "inside") & (c["iv"] == "open")) >= 16
            dens = sorted(o.density for o in sc.objs if o.kind == "medium")
            assert dens[-1] / dens[0] >= 500.0
            for name_iv in L.MEDIUM_INTERVALS:
                assert _count((c["kind"] == "medium") & (c["iv"] == name_iv)) >= 16, name_iv
    assert all(v >= 16 for v in total.values())


def test_media_of_the_general_kernel():
    c, a, sc = L.cases("general"), L.answers("general"), L.scene("general")
    W = L.world("general")
    # a BVH as the boundary: node visits inside the medium's test
    for lab in ("medium_bvh", "medium_bvh_chain2"):
        m = c["label"] == lab
        assert _count(m & a["hit"]) >= 16 and _count(m & ~a["hit"] & (a["draws"] == 1)) >= 16, lab
        assert (a["node_visits"][m] >= 1).all() and (a["medium_tests"][m] == 1).all()
    # a medium as the boundary: up to three draws a case, the outer one last
    pair = np.isin(c["label"], ("medium_pair", "medium_pair_thin", "medium_pair_dense"))
    for n in (1, 2, 3):
        assert _count(pair & (a["draws"] == n)) >= 16, n
    assert _count(pair & a["hit"]) >= 16 and (a["medium_tests"][pair] >= 2).all()
    # the t1 < 0 clamp, reached only with tmin = -f64::MAX: the origin inside the inner medium's sphere
    objs = sc.objs
    sphere_of = np.array([objs[o.twin].twin if getattr(o, "levels", 0) == 2 else -1 for o in objs])[c["k"]]
    m = sphere_of >= 0
    b1 = W.hit(sphere_of[m], c["ray"][m], -L.DMAX, L.DMAX, c["s0"][m])
    inside = np.zeros(len(m), dtype=bool)
    inside[m] = b1["hit"] & (b1["t"] < 0.0)
    b2 = W.hit(sphere_of[inside], c["ray"][inside], b1["t"][inside[m]] + 0.0001, L.DMAX, c["s0"][inside])
    assert b2["hit"].all() and (b2["t"] > 0.0).all()
    assert _count(inside) >= 16 and (a["draws"][inside] >= 1).all() and _count(inside & a["hit"]) >= 4
    assert (c["tag"][inside] == "inside").all()


def test_nested_entries():
    for name in ("nested", "general"):
        c, a = L.cases(name), L.answers(name)
        m = c["kind"] == "bvh"
        assert _count(m) >= 64 and (c["iv"][m] == "open").all()
        assert _count(m & a["hit"]) >= 16 and _count(m & ~a["hit"]) >= 16
