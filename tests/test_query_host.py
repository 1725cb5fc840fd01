"""Ray queries, without a device: the cases of tests/query_cases.py reach what they are meant to
reach (asserted on the oracle's answers alone), the twin is a different reference from the
brute-force fold, the bindings agree on the two records, and the entry points reject bad arguments
before anything touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from grayshift_amd import _native as N
from grayshift_amd import query as GQ

from tests import query_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _random(name):
    r, tags = Q.rays(name)
    n = tags.count("random")
    return r[:n], {k: v[:n] for k, v in Q.answers(name).items()}


@pytest.mark.parametrize("name,want", [
    ("mixed", {"sphere", "msphere", "quad", "triangle", "cube", "nested"}),
    ("media", {"sphere", "msphere", "quad", "triangle", "cube", "nested", "medium_sphere", "medium_cube"}),
    ("spheres", {"sphere"}), ("tiny1", {"tiny0"}), ("tiny2", {"tiny0", "tiny1"}), ("tiny3", {"tiny0", "tiny1", "tiny2"}),
    ("fog", {"sphere", "medium_sphere"})])
def test_every_object_kind_is_the_accepted_hit_of_some_ray(name, want):
    labels = set(Q.hit_label(Q.scene(name), Q.answers(name)))
    assert want <= labels, want - labels


@pytest.mark.parametrize("name", sorted(Q.SCENES))
def test_misses_are_a_fair_share_of_the_random_rays(name):
    _, a = _random(name)
    miss = 1.0 - a["hit"].mean()
    assert 0.2 <= miss <= 0.8, miss


@pytest.mark.parametrize("name", sorted(Q.GENERAL))
def test_composition_scenes_hit_and_miss(name):
    _, a = _random(name)
    assert 0.1 <= 1.0 - a["hit"].mean() <= 0.9
    assert a["node_visits"].max() > 1


@pytest.mark.parametrize("name", ["media", "fog"])
def test_media_draws_taken_and_accepted_taken_and_rejected_and_not_taken(name):
    r, tags = Q.rays(name)
    a = Q.answers(name)
    moved = a["state"] != Q.seeds(len(r))
    at_medium = np.array([str(x).startswith("medium") for x in Q.hit_label(Q.scene(name), a)])
    tested = a["medium_tests"] > 0
    assert (moved & at_medium).any()             # a draw taken and accepted
    assert (moved & ~at_medium).any()            # taken and rejected (or overtaken by a nearer hit)
    assert (moved & ~a["hit"]).any()             # ... rejected outright: the ray misses everything
    assert (tested & ~moved).any()               # the medium tested, no draw taken
    assert not (moved & ~tested).any()


@pytest.mark.parametrize("name", ["mixed", "media"])
def test_the_twin_is_not_the_brute_force_fold(name):
    """Reach: order-dependent rays exist (the triangle that ignores ray_t; with media, the draws), so
    a fold over the top-level objects is not the reference's answer.  The twin is."""
    r, a = _random(name)
    f = Q.fold(name, r, Q.seeds(len(r)))
    differ = (f["hit"] != a["hit"]) | (f["t"].view(np.uint64) != np.where(a["hit"], a["t"], r[:, 8]).view(np.uint64))
    assert differ.any()
    assert differ.mean() < 0.1  # (they agree on nearly every ray)


@pytest.mark.parametrize("name", ["mixed", "tiny1"])
def test_the_edge_rays_reach_their_edges(name):
    r, tags = Q.rays(name)
    a = Q.answers(name)
    tags = np.array(tags)
    nr = int((tags == "random").sum())
    base_hits = np.flatnonzero(a["hit"][:nr])[:256]
    var = np.flatnonzero((tags == "tmax") | (tags == "tmin"))
    assert len(var) == 6 * len(base_hits) and len(base_hits) > 0
    flips = 0
    for j, i in enumerate(base_hits):
        at, below, above = (var[6 * j + k] for k in range(3))  # tmax = t, one ulp below, one above
        assert r[at, 8] == a["t"][i] and r[below, 8] < r[at, 8] < r[above, 8]
        flips += int(not (a["hit"][at] and a["t"][at] == a["t"][i])) + int(a["hit"][above] and a["t"][above] == a["t"][i])
    assert flips >= len(base_hits)  # the interval is open: tmax = t loses the hit, one ulp above keeps it
    for tag in ("axis", "face", "inside"):
        sel = tags == tag
        assert sel.sum() > 0 and a["hit"][sel].any()
    assert (~a["hit"][tags == "face"]).any()
    for tag in ("empty", "zero_dir", "bad_o", "bad_d", "bad_iv", "bad_all"):
        assert (tags == tag).any()
    if name == "mixed":
        mv = tags == "moving"
        assert a["hit"][mv].any() and a["msphere_tests"][mv].sum() > 0
        assert len(set(r[mv, 6])) >= 3 and {0.0, 1.0} <= set(r[mv, 6])


# ----------------------------------------------------------------------------- the records
_C_SIZES = {"double": 8, "uint32_t": 4, "uint64_t": 8, "f64": 8, "u32": 4, "u64": 8}


def _layout(fields):
    """[(name, type, count)] -> ({name: offset}, size) under the C rules for naturally aligned scalars."""
    off, out, align = 0, {}, 1
    for name, typ, count in fields:
        sz = _C_SIZES[typ]
        off = (off + sz - 1) // sz * sz
        out[name] = off
        off += sz * count
        align = max(align, sz)
    return out, (off + align - 1) // align * align


def _header_fields(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = decl.split(None, 1)
        for part in rest.split(","):
            m = re.match(r"\s*([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[(\d+)\])?\s*$", part)
            out.append((m.group(1), typ, int(m.group(2) or 1)))
    return out


def _rust_fields(name):
    src = open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read()
    body = re.search(r"pub struct %s \{(.*?)\n\}" % name, src, re.S).group(1)
    out = []
    for fname, arr_t, arr_n, typ in re.findall(r"pub (?:r#)?([a-z_0-9]+)\s*:\s*(?:\[([a-z0-9]+);\s*(\d+)\]|([a-z0-9]+))", body):
        out.append((fname, arr_t or typ, int(arr_n or 1)))
    return out


@pytest.mark.parametrize("name,size", [("gs_ray", 72), ("gs_ray_hit", 104)])
def test_record_layouts_agree_in_header_ctypes_and_rust(name, size):
    hdr, rs = _header_fields(name), _rust_fields(name)
    assert [f[0] for f in hdr] == [f[0] for f in rs]
    h_off, h_size = _layout(hdr)
    r_off, r_size = _layout(rs)
    T = getattr(N, name)
    assert h_size == r_size == C.sizeof(T) == size
    assert [f[0] for f in T._fields_] == [f[0] for f in hdr]
    for fname, _, _ in hdr:
        assert getattr(T, fname).offset == h_off[fname] == r_off[fname], fname
    dt = {"gs_ray": GQ.RAY_DTYPE, "gs_ray_hit": GQ.HIT_DTYPE}[name]
    assert dt.itemsize == size and {k: dt.fields[k][1] for k in dt.names} == h_off
    rust = open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read()
    assert "pub const GS_QUERY_CLOSEST: i32 = 0;" in rust and "pub const GS_QUERY_ANY: i32 = 1;" in rust
    assert (N.GS_QUERY_CLOSEST, N.GS_QUERY_ANY) == (0, 1)


def test_query_entry_points_reject_bad_arguments_before_the_device():
    """Every argument check answers GS_ERR_ARG on the arguments alone: the scene pointer below is
    not a scene and is never read."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    rays = (N.gs_ray * 2)()
    hits = (N.gs_ray_hit * 2)()
    stream = None
    for fn, tail in ((N.lib.gs_query_rays_async, (None, stream)), (N.lib.gs_query_rays, (None,))):
        def call(sc, r, n, mode, h):
            return fn(sc, r, n, mode, 1, h, *tail)
        assert call(None, rays, 2, 0, hits) == N.GS_ERR_ARG
        assert b"null" in N.lib.gs_last_error()
        assert call(scene, None, 2, 0, hits) == N.GS_ERR_ARG
        assert call(scene, rays, 2, 0, None) == N.GS_ERR_ARG
        assert call(scene, rays, -1, 0, hits) == N.GS_ERR_ARG
        assert b"n must be" in N.lib.gs_last_error()
        assert call(scene, rays, 1 << 31, 0, hits) == N.GS_ERR_ARG
        assert call(scene, rays, 1 << 40, 1, hits) == N.GS_ERR_ARG
        for mode in (-1, 2, 7):
            assert call(scene, rays, 2, mode, hits) == N.GS_ERR_ARG
            assert b"mode" in N.lib.gs_last_error()
        assert call(scene, rays, 0, 0, hits) == N.GS_OK   # nothing to do: no launch, the scene not read
        assert call(scene, rays, 0, 1, hits) == N.GS_OK
        assert call(None, rays, 0, 0, hits) == N.GS_ERR_ARG  # (the checks come first)


def test_query_kernels_run_without_scratch_in_a_library_of_their_own():
    """Every gs_query_kernel instantiation (four feature sets and the catch-all, two modes) launches
    without private memory; they live in libgrayshift_query.so, so the product's code objects --
    and the hash that keys its committed profiles -- hold none of them."""
    from grayshift_amd import build, codeobj
    scratch = codeobj.kernel_scratch(build.QUERY_LIB)
    q = {k: v for k, v in scratch.items() if "gs_query_kernel" in k}
    assert len(q) == 10 and set(q.values()) == {0}
    for feat in (0, 1, 2, 3, 515):
        for mode in (0, 1):
            assert any("gs_query_kernelILi%dELb%dE" % (feat, mode) in k for k in q), (feat, mode)
    assert not [k for k in codeobj.kernel_scratch(N.LIB_PATH) if "gs_query" in k]
    assert hasattr(C.CDLL(N.LIB_PATH), "gs_query_rays_async")


def test_the_abi_number_stays():
    assert N.lib.gs_version() == N.GS_ABI_VERSION == 11


def test_pack_rays_and_camera_rays():
    a = np.arange(18, dtype=np.float64).reshape(2, 9)
    assert GQ.pack_rays(a) is a or np.array_equal(GQ.pack_rays(a), a)
    d = {"o": a[:, 0:3], "d": a[:, 3:6], "time": a[:, 6], "tmin": 0.5, "tmax": a[:, 8]}
    p = GQ.pack_rays(d)
    assert p.shape == (2, 9) and np.array_equal(p[:, [0, 3, 6, 8]], a[:, [0, 3, 6, 8]]) and (p[:, 7] == 0.5).all()
    with pytest.raises(ValueError):
        GQ.pack_rays(np.zeros((3, 7)))
    import grayshift_amd as g
    from grayshift_amd import scenes
    cam = g.camera(scenes.config("C4", width=16, spp=1).camera)
    r = GQ.camera_rays(cam)
    W, H = cam.image_width, cam.image_height
    assert r.shape == (W * H, 9) and (r[:, 7] == 0.001).all() and (r[:, 8] == Q.DMAX).all()
    c, p0 = np.array(cam.center[:]), np.array(cam.starting_pixel_pos[:])
    du, dv = np.array(cam.pixel_delta_u[:]), np.array(cam.pixel_delta_v[:])
    assert np.array_equal(r[0, 0:3], c) and np.array_equal(r[0, 3:6], p0 - c)
    j, i = 3, 5
    assert np.array_equal(r[j * W + i, 3:6], ((p0 + du * float(i)) + dv * float(j)) - c)
