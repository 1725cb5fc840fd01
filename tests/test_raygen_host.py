"""Generated radiance queries, without a device: the bindings agree on gs_raygen and the two entries,
the entries reject bad arguments before anything touches a device, the built library holds the five
gs_raygen_kernel instantiations (the four non-general ones without scratch) and the product none,
and the numpy restatement of tests/raygen_cases.py reaches what the GPU tests lean on it for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from grayshift_amd import _native as N
from grayshift_amd import query as GQ

from tests import raygen_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SIZES = {"double": 8, "int32_t": 4, "uint32_t": 4, "f64": 8, "i32": 4, "u32": 4}


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


# ----------------------------------------------------------------------------- the struct, the entries
def _layout(fields, nested):
    """[(name, type, count)] -> ({name: (offset, size)}, size): C's rules for naturally aligned members;
    `nested`: {type: (size, alignment)} of the structs among them."""
    off, out, align = 0, {}, 1
    for name, typ, count in fields:
        sz, al = nested[typ] if typ in nested else (_SIZES[typ], _SIZES[typ])
        off = (off + al - 1) // al * al
        out[name] = (off, sz * count)
        off += sz * count
        align = max(align, al)
    return out, (off + align - 1) // align * align


def _header_fields(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            typ, rest = decl.split(None, 1)
            for part in rest.split(","):
                m = re.match(r"\s*([A-Za-z_][A-Za-z0-9_]*)\s*((?:\[\d+\])*)\s*$", part)
                out.append((m.group(1), typ, int(np.prod([int(x) for x in re.findall(r"\d+", m.group(2))] or [1]))))
    return out


def _rust_fields(name):
    src = open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read()
    body = re.search(r"pub struct %s \{(.*?)\n\}" % name, src, re.S).group(1)
    out = []
    for fname, typ in re.findall(r"pub ([a-z_0-9]+)\s*:\s*([^,\n]+?)\s*,", body + ","):
        count = int(np.prod([int(x) for x in re.findall(r";\s*(\d+)\]", typ)] or [1]))
        out.append((fname, re.search(r"[a-z_][a-z_0-9]*", typ).group(0), count))
    return out


def test_gs_raygen_agrees_in_header_ctypes_and_rust():
    cam_h, cam_r = _header_fields("gs_camera"), _rust_fields("gs_camera")
    _, cam_size = _layout(cam_h, {})
    assert cam_size == _layout(cam_r, {})[1] == C.sizeof(N.gs_camera) == 168
    hdr, rs = _header_fields("gs_raygen"), _rust_fields("gs_raygen")
    assert [f[0] for f in hdr] == [f[0] for f in rs] == [f[0] for f in N.gs_raygen._fields_]
    assert [f[0] for f in hdr] == ["kind", "width", "height", "pad", "cam", "origin", "axis"]
    assert [f[2] for f in hdr] == [f[2] for f in rs] == [1, 1, 1, 1, 1, 3, 9]
    h_off, h_size = _layout(hdr, {"gs_camera": (cam_size, 8)})
    r_off, r_size = _layout(rs, {"gs_camera": (cam_size, 8)})
    assert h_size == r_size == C.sizeof(N.gs_raygen) == 280
    for fname, _, _ in hdr:
        f = getattr(N.gs_raygen, fname)
        assert (f.offset, f.size) == h_off[fname] == r_off[fname], fname
    header = open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for k, name in enumerate(("GS_GEN_CAMERA", "GS_GEN_PANORAMA", "GS_GEN_ORTHO", "GS_GEN_HEMISPHERE")):
        assert "#define %s %d\n" % (name, k) in header and "pub const %s: i32 = %d;" % (name, k) in rust
        assert getattr(N, name) == k
    for fn in ("gs_query_radiance_gen_async", "gs_query_radiance_gen"):
        assert "pub fn %s(" % fn in rust and fn in doc and fn in N.SIGNATURES and hasattr(C.CDLL(N.LIB_PATH), fn)
    # the two entries' parameter lists, type by type, against the ctypes signatures
    kinds = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for fn in ("gs_query_radiance_gen_async", "gs_query_radiance_gen"):
        params = re.search(r"gs_status %s\((.*?)\);" % fn, plain, re.S).group(1).split(",")
        want = [N._P if "*" in p else kinds[p.split()[0]] for p in params]
        assert N.SIGNATURES[fn] == (C.c_int32, want), fn
        assert len(re.search(r"pub fn %s\((.*?)\)" % fn, rust, re.S).group(1).split(",")) == len(params)
    assert N.lib.gs_version() == N.GS_ABI_VERSION == 11


def test_gen_entry_points_reject_bad_arguments_before_the_device():
    """Every argument check answers GS_ERR_ARG on the arguments alone: the scene pointer below is not
    a scene and is never read, and neither are the device pointers."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    out = (N.gs_ray_radiance * 16)()
    pts = (N.gs_ray * 16)()
    scratch = C.cast(C.create_string_buffer(4096), C.c_void_p)

    def raw(kind, w=2, h=2):
        g = N.gs_raygen()
        g.kind, g.width, g.height = kind, w, h
        g.cam.image_width, g.cam.image_height = w, h
        return g

    def a_sync(sc, g, p, samples, first, chunk, o, scr=scratch, nbytes=4096):
        return N.lib.gs_query_radiance_gen_async(sc, C.addressof(g) if g is not None else None, p, samples, first, chunk,
                                                 50, 1, o, None, None, None, scr, nbytes, None)

    def sync(sc, g, p, samples, first, chunk, o, scr=None, nbytes=0):
        return N.lib.gs_query_radiance_gen(sc, C.addressof(g) if g is not None else None, p, samples, first, chunk, 50, 1,
                                           o, None, None, None)
    pano = raw(N.GS_GEN_PANORAMA)
    for call in (a_sync, sync):
        assert call(None, pano, None, 1, 0, 0, out) == N.GS_ERR_ARG
        assert b"null" in N.lib.gs_last_error()
        assert call(scene, None, None, 1, 0, 0, out) == N.GS_ERR_ARG
        assert call(scene, pano, None, 1, 0, 0, None) == N.GS_ERR_ARG
        for kind in (-1, 4, 1 << 20):
            assert call(scene, raw(kind), pts, 1, 0, 0, out) == N.GS_ERR_ARG
            assert b"kind" in N.lib.gs_last_error()
        for kind in (N.GS_GEN_CAMERA, N.GS_GEN_PANORAMA, N.GS_GEN_ORTHO, N.GS_GEN_HEMISPHERE):
            for w, h in ((0, 2), (2, 0), (-3, 2), (2, -1)):
                assert call(scene, raw(kind, w, h), pts, 1, 0, 0, out) == N.GS_ERR_ARG, (kind, w, h)
                assert b"width" in N.lib.gs_last_error()
        cam = raw(N.GS_GEN_CAMERA)  # a camera's dimensions are its own: width and height are not read
        cam.cam.image_width = 0
        assert call(scene, cam, None, 1, 0, 0, out) == N.GS_ERR_ARG
        assert b"width" in N.lib.gs_last_error()
        assert call(scene, raw(N.GS_GEN_HEMISPHERE, 4, 1), None, 1, 0, 0, out) == N.GS_ERR_ARG
        assert b"points" in N.lib.gs_last_error()
        assert call(scene, raw(N.GS_GEN_HEMISPHERE, 4, 2), pts, 1, 0, 0, out) == N.GS_ERR_ARG  # height is 1
        assert call(scene, pano, None, 0, 0, 0, out) == N.GS_ERR_ARG
        assert b"samples" in N.lib.gs_last_error()
        assert call(scene, pano, None, 2, 0xFFFFFFFF, 0, out) == N.GS_ERR_ARG
        assert b"first_sample" in N.lib.gs_last_error()
        assert call(scene, pano, None, 0xFFFFFFFF, 2, 0xFFFFFFFF, out) == N.GS_ERR_ARG
        assert b"first_sample" in N.lib.gs_last_error()
        assert call(scene, raw(N.GS_GEN_ORTHO, 1 << 16, 1 << 15), None, 1, 0, 0, out) == N.GS_ERR_ARG  # 2^31 items
        assert b"2^31" in N.lib.gs_last_error()
        assert call(scene, raw(N.GS_GEN_ORTHO, 1 << 15, 1 << 15), None, 2, 0, 1, out) == N.GS_ERR_ARG  # 2^30 x 2 chunks
        assert b"2^31" in N.lib.gs_last_error()
        assert call(None, raw(7), None, 0, 0, 0, None) == N.GS_ERR_ARG
        assert b"null" in N.lib.gs_last_error()  # (the null check comes first)
    # the async form's scratch: gs_query_radiance_scratch_bytes(n, samples, chunk), needed with more than one chunk
    need = N.lib.gs_query_radiance_scratch_bytes(4, 5, 2)
    assert need == 4 * 3 * 40
    assert a_sync(scene, pano, None, 5, 0, 2, out, None, 0) == N.GS_ERR_ARG
    assert b"scratch" in N.lib.gs_last_error()
    assert a_sync(scene, pano, None, 5, 0, 2, out, None, 1 << 20) == N.GS_ERR_ARG
    assert a_sync(scene, pano, None, 5, 0, 2, out, scratch, need - 1) == N.GS_ERR_ARG
    assert a_sync(scene, pano, None, 17, 0, 0, out, scratch, 4 * 2 * 40 - 8) == N.GS_ERR_ARG
    assert b"scratch" in N.lib.gs_last_error()
    # the synchronous form's emitted arrays: 2^30 items of 2^32 - 1 samples in one chunk pass the item
    # count, but 2^62 rays of 72 B cannot be counted in a size_t, let alone allocated
    big, stub = raw(N.GS_GEN_ORTHO, 1 << 15, 1 << 15), C.cast(C.create_string_buffer(72), C.c_void_p)
    for r_out, s_out in ((stub, None), (None, stub), (stub, stub)):
        assert N.lib.gs_query_radiance_gen(scene, C.addressof(big), None, 0xFFFFFFFF, 0, 0xFFFFFFFF, 50, 1, out, None,
                                           r_out, s_out) == N.GS_ERR_ARG
        assert b"do not fit" in N.lib.gs_last_error()


# ----------------------------------------------------------------------------- the code objects
def test_raygen_kernels_of_the_reference_scenes_carry_no_scratch():
    """Five gs_raygen_kernel instantiations in libgrayshift_query.so, the four non-general ones (MEDIA x
    NESTED) without private memory; the catch-all's figure is reported (profiles/raygen/
    resource_usage.txt).  The product's code objects hold none of them."""
    from grayshift_amd import build, codeobj
    assert os.path.exists(build.QUERY_LIB)
    scratch = codeobj.kernel_scratch(build.QUERY_LIB)
    gen = {k: v for k, v in scratch.items() if "gs_raygen_kernel" in k}
    assert len(gen) == 5, sorted(gen)
    for feat in (0, 1, 2, 3):
        ks = [k for k in gen if "gs_raygen_kernelILi%dEE" % feat in k]
        assert len(ks) == 1 and gen[ks[0]] == 0, (feat, ks, gen)
    general = [k for k in gen if "gs_raygen_kernelILi515EE" in k]
    assert len(general) == 1
    print("catch-all scratch: %d B per lane" % gen[general[0]])
    assert len([k for k in scratch if "gs_radiance_combine_kernel" in k]) == 1  # (the one combine serves both)
    assert not [k for k in codeobj.kernel_scratch(N.LIB_PATH) if "gs_raygen" in k]


# ----------------------------------------------------------------------------- the restatement's reach
def test_an_unjittered_panorama_is_panorama_rays_and_an_unjittered_ortho_is_ortho_rays():
    for w, h in G.IMAGES + ((64, 32),):
        pano = G.restate(GQ.RayGen.panorama((1.0, 2.0, 3.0), w, h), 2, G.SEED, jitter=False)["rays"]
        want = np.repeat(GQ.panorama_rays((1.0, 2.0, 3.0), w, h), 2, axis=0)
        for col in (0, 1, 2, 3, 4, 5, 7, 8):
            assert np.array_equal(pano[:, col].view(np.uint64), want[:, col].view(np.uint64)), (w, h, col)
        args = ((-9.0, 7.0, 22.0), (18.0, 0.0, 1.0), (0.0, -14.0, 0.5), (0.1, 0.0, -1.5))
        orth = G.restate(GQ.RayGen.ortho(*args, w, h), 2, G.SEED, jitter=False)["rays"]
        want = np.repeat(GQ.ortho_rays(*args, w, h), 2, axis=0)
        for col in (0, 1, 2, 3, 4, 5, 7, 8):
            assert np.array_equal(orth[:, col].view(np.uint64), want[:, col].view(np.uint64)), (w, h, col)
        # the time is drawn third, from the (item, sample) stream
        t = np.array([G.oracle.wyrand(G.oracle.stream_seed(G.SEED, q, s), 3)[0][2] for q in range(w * h) for s in range(2)])
        assert np.array_equal(pano[:, 6], t) and np.array_equal(orth[:, 6], t)


def test_jitter_stays_inside_the_cell_and_moves_every_ray():
    w, h = G.IMAGES[1]
    j = G.restated("ortho", "media_sky", w, h, 5)["rays"]
    c = G.restate(G.gen("ortho", "media_sky", w, h), 5, G.SEED, jitter=False)["rays"]
    raw = G.gen("ortho", "media_sky", w, h).raw
    eu, ev = np.array(raw.axis[0][:]), np.array(raw.axis[1][:])
    d = j[:, 0:3] - c[:, 0:3]
    a = d @ eu / (eu @ eu) * w  # (eu and ev: nearly orthogonal)
    assert (np.abs(a) <= 0.5 + 1e-3).all() and (a != 0.0).all() and a.std() > 0.2
    assert len(np.unique(j[:, 0])) == len(j)


def test_a_defocus_cameras_origins_lie_on_the_disk_and_its_loop_rejects():
    w, h = G.IMAGES[1]
    r = G.restated("camera_defocus", "media_sky", w, h, 5)
    plain = G.restated("camera", "media_sky", w, h, 5)
    cam = G.gen("camera_defocus", "media_sky", w, h).raw.cam
    assert cam.defocus_angle == G.DEFOCUS
    c, ku, kv = (np.array(v[:]) for v in (cam.center, cam.defocus_disk_u, cam.defocus_disk_v))
    off = r["rays"][:, 0:3] - c
    x, y = off @ ku / (ku @ ku), off @ kv / (kv @ kv)
    assert (x * x + y * y < 1.0 + 1e-9).all() and (np.abs(off).max(axis=1) > 0.0).all()
    assert (x * x + y * y).max() > 0.9 and len(np.unique(r["rays"][:, 0])) == len(off)
    assert (plain["rays"][:, 0:3] == c).all() and plain["retries"] == 0
    # the loop's rounds show in the streams: 5 draws without a retry, two more per retry
    draws = ((r["states"].astype(object) - np.array([G.oracle.stream_seed(G.SEED, q, s) for q in range(w * h)
                                                      for s in range(5)], dtype=object)) % (1 << 64))
    counts = np.array([int(v) * pow(G.WY_C0, -1, 1 << 64) % (1 << 64) for v in draws])
    print("defocus: %d retries over %d samples; draws per sample %s" % (r["retries"], len(off), sorted(set(counts))))
    assert r["retries"] >= 1 and counts.min() == 5 and counts.max() >= 7 and ((counts - 5) % 2 == 0).all()
    assert int(((counts - 5) // 2).sum()) == r["retries"]
    # the pixel's point on the focus plane does not move with the origin: o + d is the plain camera's
    assert np.abs((r["rays"][:, 0:3] + r["rays"][:, 3:6]) - (plain["rays"][:, 0:3] + plain["rays"][:, 3:6])).max() < 1e-12


def test_the_hemisphere_restatement_is_cosine_weighted_about_both_kinds_of_normal():
    w, h = 272, 1
    rg = G.gen("hemisphere", "media_sky", w, h)
    r = G.restate(rg, 33, G.SEED)
    assert rg.shape == (1, 272) and r["retries"] == 0
    nrm = np.repeat(rg.points[:, 3:6] / np.linalg.norm(rg.points[:, 3:6], axis=1, keepdims=True), 33, axis=0)
    cos = (r["rays"][:, 3:6] * nrm).sum(axis=1)
    assert np.abs(np.linalg.norm(r["rays"][:, 3:6], axis=1) - 1.0).max() < 1e-15 and (cos > 0.0).all()
    # (x, y, z) = (cos phi r2^(1/4), sin phi r2^(1/4), sqrt(1 - r2)) is normalised afterwards, so the
    # cosine to the normal is sqrt(1 - r2) / sqrt(sqrt(r2) + 1 - r2) with r2 uniform: its mean, by quadrature
    r2 = (np.arange(200000) + 0.5) / 200000
    want = (np.sqrt(1.0 - r2) / np.sqrt(np.sqrt(r2) + 1.0 - r2)).mean()
    assert abs(cos.mean() - want) < 0.02, (cos.mean(), want)  # (8 976 samples of spread < 0.3: sigma 0.003)
    assert (np.abs(nrm[:, 0]) > 0.9).any() and (np.abs(nrm[:, 0]) <= 0.9).any()
    assert np.array_equal(np.repeat(rg.points[:, 0:3], 33, axis=0), r["rays"][:, 0:3])
    assert np.array_equal(np.repeat(rg.points[:, 6], 33), r["rays"][:, 6])
    first = np.array([G.oracle.stream_seed(G.SEED, q, s) for q in range(w) for s in range(33)], dtype=np.uint64)
    assert np.array_equal(r["states"], first + np.uint64(2 * G.WY_C0 % (1 << 64)))  # two draws, no time draw

