"""Radiance queries, without a device: the reference fold of tests/radiance_cases.py agrees with the
reference's own recursion, the lit scenes reach what they are meant to reach (asserted on the oracle
alone), the bindings agree on the record, the entry points reject bad arguments before anything
touches a device, the ray generators follow their documented conventions, and the four non-general
kernel sets carry no scratch."""
import ctypes as C
import os

import numpy as np
import pytest

from grayshift_amd import _native as N
from grayshift_amd import query as GQ

import oracle

from tests import query_cases as Q
from tests import radiance_cases as R
from tests.test_query_host import _header_fields, _layout, _rust_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


# ----------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("name", sorted(R.LIT))
def test_the_forward_fold_agrees_with_the_references_recursion(name):
    """T = (1 a1) a2 ... ended by T c, against emitted + colour * attenuation from the last level
    back (camera.rs:193-195): the same products in another order, 1e-12 relative."""
    r = R.rays(name)
    f = R.ray_color_fold(R.scene(name).twin, r, R.seeds(len(r)), 50, trail=True)
    back = R.ray_color_recursive(len(r), f["trail"])
    assert np.isfinite(f["rgb"]).all() and np.isfinite(back).all()
    rel = np.abs(f["rgb"] - back) / np.maximum(np.abs(back), 1e-300)
    rel[(f["rgb"] == 0.0) & (back == 0.0)] = 0.0
    print("%s: largest relative difference %.3g, bit-equal rays %.1f%%" % (
        name, rel.max(), 100.0 * (f["rgb"] == back).all(axis=1).mean()))
    assert rel.max() <= 1e-12
    plain = R.answers(name, 50)  # (the shared answer is the same fold)
    assert np.array_equal(plain["rgb"], f["rgb"]) and np.array_equal(plain["state"], f["state"])


@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("name", sorted(R.LIT))
def test_the_lit_scenes_reach_every_way_a_path_ends(name, depth):
    """Per scene and depth, every end its geometry can give (radiance_cases.ENDS): the sky and the
    depth limit everywhere, a light where the scene holds one, an absorbed ray where it holds a fuzzy
    metal.  Where the random rays fell short, the scene's rays were changed (radiance_cases.aimed):
    `mixed`'s metals have fuzz 0.1 and absorb only a grazing ray; `nested_media` and `outer_light`
    hold no specular material, and their only paths of 50 segments run inside the ground sphere.  The
    ends left out cannot occur: no light in the scene, or no metal (`fog`, `nested_media`).  At depth
    50: at least 95% non-zero colours and at least 1.4 rays a path."""
    a = R.answers(name, depth)
    nonzero = (a["rgb"] != 0.0).any(axis=1).mean()
    ends = {k: int((a["end"] == k).sum()) for k in (R.SKY, R.LIGHT, R.ABSORBED, R.DEPTH)}
    print("%s depth %d: non-zero %.1f%%, rays/path %.2f, ends %s" % (name, depth, 100.0 * nonzero, a["rays"].mean(), ends))
    assert a["rays"].max() <= depth and (a["end"] != 0).all()
    if depth == 50:
        assert nonzero >= 0.95
        assert a["rays"].mean() >= 1.4
    for k in (R.SKY, R.LIGHT, R.ABSORBED, R.DEPTH):
        if k in R.ENDS[name]:
            assert ends[k] > 0, (name, depth, k, ends)
        else:
            assert k in (R.LIGHT, R.ABSORBED) and ends[k] == 0  # (the named exceptions: it cannot occur)


def test_the_expected_ends_follow_the_scenes_materials():
    """ENDS is not tuned to the answers: a light end is expected exactly where the builder makes a
    light that emits, an absorbed end exactly where it makes a metal with fuzz (or `textured`'s dark
    light)."""
    import grayshift_amd as g
    for name in sorted(R.LIT):
        made = {"light": False, "fuzzy": False}

        class Spy(g.SceneBuilder):
            def diffuse_light(self, rgb):
                made["light"] |= any(x != 0.0 for x in rgb)
                made["fuzzy"] |= all(x == 0.0 for x in rgb)
                return super().diffuse_light(rgb)

            def metal(self, albedo, fuzz):
                made["fuzzy"] |= fuzz > 0.0
                return super().metal(albedo, fuzz)
        R._builder(R.LIT[name][0])(Spy())
        assert (R.LIGHT in R.ENDS[name]) == made["light"], name
        assert (R.ABSORBED in R.ENDS[name]) == made["fuzzy"], name
        assert {R.SKY, R.DEPTH} <= R.ENDS[name]


@pytest.mark.parametrize("name", R.HDRI_SCENES)
def test_hdri_colours_tell_directions_apart(name):
    a = R.answers(name, 50)
    distinct = len(np.unique(a["rgb"].view(np.uint64).reshape(-1, 3), axis=0))
    print("%s: %d distinct colours over %d rays" % (name, distinct, len(a["rgb"])))
    assert distinct >= 1000


def test_the_hdri_map_survives_rgbe8():
    m = R.hdri_map().reshape(-1, 3).astype(np.float64)
    assert len(np.unique(m, axis=0)) == R.HDRI_W * R.HDRI_H
    mx = m.max(axis=1)
    assert (mx >= 0.5).all() and (mx < 1.0).all()       # one exponent: 2^0
    assert np.array_equal(np.floor(m * 256.0), m * 256.0)  # 8-bit mantissas hold every channel


def test_the_textured_scene_reaches_its_textures_and_its_light():
    a = R.answers("textured_hdri", 50)
    c = a["counters"]
    assert c["image_texels"] > 100 and c["noise_evals"] > 100 and c["hdri_texels"] > 1000
    assert (a["end"] == R.LIGHT).sum() > 10 and a["noise"].any() and not a["noise"].all()
    free = R.answers("mirrors_sky", 50)
    assert (free["end"] == R.ABSORBED).any() and (free["end"] == R.DEPTH).sum() > 0


# ----------------------------------------------------------------------------- the record, the entries
def test_record_layout_agrees_in_header_ctypes_and_rust():
    hdr, rs = _header_fields("gs_ray_radiance"), _rust_fields("gs_ray_radiance")
    assert [f[0] for f in hdr] == [f[0] for f in rs] == ["rgb", "rays", "state"]
    h_off, h_size = _layout(hdr)
    r_off, r_size = _layout(rs)
    T = N.gs_ray_radiance
    assert h_size == r_size == C.sizeof(T) == 40
    assert [f[0] for f in T._fields_] == [f[0] for f in hdr]
    for fname, _, _ in hdr:
        assert getattr(T, fname).offset == h_off[fname] == r_off[fname], fname
    dt = GQ.RADIANCE_DTYPE
    assert dt.itemsize == 40 and {k: dt.fields[k][1] for k in dt.names} == h_off
    rust = open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in ("gs_query_radiance_scratch_bytes", "gs_query_radiance_async", "gs_query_radiance"):
        assert "pub fn %s(" % fn in rust and fn in doc and fn in N.SIGNATURES
    assert N.lib.gs_version() == N.GS_ABI_VERSION == 11


def test_scratch_bytes():
    sb = N.lib.gs_query_radiance_scratch_bytes
    assert sb(0, 1, 0) == 0 and sb(1000, 1, 0) == 0 and sb(1000, 16, 0) == 0 and sb(1000, 16, 16) == 0
    assert sb(1000, 17, 0) == 1000 * 2 * 40 and sb(1000, 64, 4) == 1000 * 16 * 40 and sb(7, 5, 2) == 7 * 3 * 40
    assert sb(0, 64, 4) == 0
    assert sb(1, 0xFFFFFFFF, 0xFFFFFFFF) == 0 and sb(1, 0xFFFFFFFF, 0) == 268435456 * 40
    assert sb(-1, 1, 0) == -1 and sb(10, 0, 0) == -1
    assert sb(1 << 31, 1, 0) == -1 and sb((1 << 31) - 1, 1, 0) == 0
    assert sb(1 << 30, 2, 1) == -1 and sb((1 << 30) - 1, 2, 1) == ((1 << 31) - 2) * 40
    assert sb(1, 0xFFFFFFFF, 1) == -1  # 2^32 - 1 items


def test_radiance_entry_points_reject_bad_arguments_before_the_device():
    """Every argument check answers GS_ERR_ARG on the arguments alone: the scene pointer below is
    not a scene and is never read."""
    fake = C.create_string_buffer(64)
    scene = C.cast(fake, C.c_void_p)
    rays = (N.gs_ray * 2)()
    out = (N.gs_ray_radiance * 2)()
    scratch = C.create_string_buffer(2 * 3 * 40)

    def a_sync(sc, r, n, samples, chunk, o, scr=None, nbytes=0):
        return N.lib.gs_query_radiance_async(sc, r, n, samples, chunk, 50, 1, None, o, None, scr, nbytes, None)

    def sync(sc, r, n, samples, chunk, o, scr=None, nbytes=0):
        return N.lib.gs_query_radiance(sc, r, n, samples, chunk, 50, 1, None, o, None)
    for call in (a_sync, sync):
        assert call(None, rays, 2, 1, 0, out) == N.GS_ERR_ARG
        assert b"null" in N.lib.gs_last_error()
        assert call(scene, None, 2, 1, 0, out) == N.GS_ERR_ARG
        assert call(scene, rays, 2, 1, 0, None) == N.GS_ERR_ARG
        assert call(scene, rays, -1, 1, 0, out) == N.GS_ERR_ARG
        assert b"negative" in N.lib.gs_last_error()
        assert call(scene, rays, 2, 0, 0, out) == N.GS_ERR_ARG
        assert b"samples" in N.lib.gs_last_error()
        assert call(scene, rays, 1 << 31, 1, 0, out) == N.GS_ERR_ARG
        assert b"2^31" in N.lib.gs_last_error()
        assert call(scene, rays, 1 << 30, 2, 1, out) == N.GS_ERR_ARG
        assert call(scene, rays, 1 << 40, 1, 0, out) == N.GS_ERR_ARG
        assert call(scene, rays, 0, 1, 0, out) == N.GS_OK      # nothing to do: no launch, the scene not read
        assert call(scene, rays, 0, 64, 4, out) == N.GS_OK     # (no rays need no scratch)
        assert call(None, rays, 0, 1, 0, out) == N.GS_ERR_ARG  # (the checks come first)
        assert call(scene, rays, 0, 0, 0, out) == N.GS_ERR_ARG
    # the async form's scratch: needed with more than one chunk per ray
    assert a_sync(scene, rays, 2, 5, 2, out, None, 0) == N.GS_ERR_ARG
    assert b"scratch" in N.lib.gs_last_error()
    assert a_sync(scene, rays, 2, 5, 2, out, None, 1 << 20) == N.GS_ERR_ARG
    assert a_sync(scene, rays, 2, 5, 2, out, C.cast(scratch, C.c_void_p), 2 * 3 * 40 - 1) == N.GS_ERR_ARG
    assert a_sync(scene, rays, 2, 17, 0, out, C.cast(scratch, C.c_void_p), 2 * 2 * 40 - 8) == N.GS_ERR_ARG
    assert b"scratch" in N.lib.gs_last_error()


def test_the_shade_batch_hook_checks_its_argument():
    assert N.lib.gs_debug_set_radiance_batch(-1) == N.GS_ERR_ARG
    assert b"shade_batch" in N.lib.gs_last_error()
    assert N.lib.gs_debug_set_radiance_batch(65) == N.GS_ERR_ARG
    assert N.lib.gs_debug_set_radiance_batch(64) == N.GS_OK
    assert N.lib.gs_debug_set_radiance_batch(0) == N.GS_OK  # (the default again)


# ----------------------------------------------------------------------------- the ray generators
def test_panorama_rays_are_unit_rows_over_the_sphere():
    W, H = 16, 8
    r = GQ.panorama_rays((1.0, 2.0, 3.0), W, H, time=0.25)
    assert r.shape == (W * H, 9) and (r[:, 0:3] == (1.0, 2.0, 3.0)).all() and (r[:, 6] == 0.25).all()
    assert (r[:, 7] == 0.001).all() and (r[:, 8] == Q.DMAX).all()
    assert np.abs(np.linalg.norm(r[:, 3:6], axis=1) - 1.0).max() <= 2.0 ** -52
    d = r[:, 3:6].reshape(H, W, 3)
    # row order: z falls from the +z pole's row to the -z pole's, the same for every column
    assert (np.diff(d[:, :, 2], axis=0) < 0.0).all() and np.abs(d[:, :, 2] - d[:, :1, 2]).max() < 1e-15
    assert d[0, 0, 2] == pytest.approx(np.cos(np.pi / 16.0)) and d[-1, 0, 2] == pytest.approx(-np.cos(np.pi / 16.0))
    # column order: the azimuth atan2(y, x) rises from -pi to pi along a row
    az = np.arctan2(d[:, :, 1], d[:, :, 0])
    assert (np.diff(az, axis=1) > 0.0).all() and az[3, 0] == pytest.approx(-np.pi + np.pi / 16.0)
    tall = GQ.panorama_rays((0.0, 0.0, 0.0), 4, 512)  # rows half a texel from the poles: still unit, still ordered
    assert np.abs(np.linalg.norm(tall[:, 3:6], axis=1) - 1.0).max() <= 2.0 ** -52
    assert tall[0, 5] > 0.99999 and tall[-1, 5] < -0.99999


def test_a_panorama_of_an_empty_world_is_the_sky_map_itself():
    """The documented correspondence with HDRI::sample: under an unrotated W x H map, pixel (j, i) of
    panorama_rays(., W, H) reads texel (i, j) -- here through the oracle's Camera::sample_background."""
    import grayshift_amd as g
    b = g.SceneBuilder()
    b.add(b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian((0.5, 0.5, 0.5))))  # (the background does not look at the world)
    m = R.hdri_map()
    b.background_hdri(m, (0.0, 0.0, 0.0))
    w = oracle.World(b.build())
    try:
        r = GQ.panorama_rays((0.0, 5.0, 0.0), R.HDRI_W, R.HDRI_H)
        col, texels = w.background(r[:, 3:6])
    finally:
        w.close()
    assert (texels == 1).all()
    assert np.array_equal(col.reshape(R.HDRI_H, R.HDRI_W, 3), m.astype(np.float64))


def test_ortho_rays():
    W, H = 5, 3
    r = GQ.ortho_rays((1.0, 1.0, 1.0), (10.0, 0.0, 0.0), (0.0, 0.0, 6.0), (0.0, -2.0, 0.0), W, H, time=0.5)
    assert r.shape == (W * H, 9) and (r[:, 3:6] == (0.0, -2.0, 0.0)).all() and (r[:, 6] == 0.5).all()
    assert (r[:, 7] == 0.001).all() and (r[:, 8] == Q.DMAX).all()
    o = r[:, 0:3].reshape(H, W, 3)
    assert np.array_equal(o[0, 0], (2.0, 1.0, 2.0)) and np.array_equal(o[2, 4], (10.0, 1.0, 6.0))
    assert np.array_equal(o[1, 2], (6.0, 1.0, 4.0)) and (o[:, :, 1] == 1.0).all()


# ----------------------------------------------------------------------------- the code objects
def test_radiance_kernels_of_the_reference_scenes_carry_no_scratch():
    """The four non-general gs_radiance_kernel instantiations (MEDIA x NESTED) launch without private
    memory; the catch-all's figure is reported (profiles/radiance_query/resource_usage.txt).  They
    live in libgrayshift_query.so: the product's code objects hold none of them."""
    from grayshift_amd import build, codeobj
    if not os.path.exists(build.QUERY_LIB):
        pytest.skip("libgrayshift_query.so is not built")
    scratch = codeobj.kernel_scratch(build.QUERY_LIB)
    rad = {k: v for k, v in scratch.items() if "gs_radiance_kernel" in k}
    assert len(rad) == 5, sorted(rad)
    for feat in (0, 1, 2, 3):
        ks = [k for k in rad if "gs_radiance_kernelILi%dEE" % feat in k]
        assert len(ks) == 1 and rad[ks[0]] == 0, (feat, ks, rad)
    general = [k for k in rad if "gs_radiance_kernelILi515EE" in k]
    assert len(general) == 1
    print("catch-all scratch: %d B per lane" % rad[general[0]])
    combine = [k for k in scratch if "gs_radiance_combine_kernel" in k]
    assert len(combine) == 1 and scratch[combine[0]] == 0
    assert not [k for k in codeobj.kernel_scratch(N.LIB_PATH) if "gs_radiance" in k]
    assert hasattr(C.CDLL(N.LIB_PATH), "gs_query_radiance_async")
