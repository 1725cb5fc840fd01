"""Every instantiation of the render kernel against the CPU oracle, at bit parity.

kernel_for (csrc/device/render.hip) holds 27 base feature sets, each in two to four launch forms:
the per-lane adaptive loop (F), the fixed-spp kernel (F | FIXED), its views form (F | FIXED | VIEWS;
the GS_K and GS_KR lines) and the split batch round (F | FIXED | RSPLIT; the GS_KR lines).
choose_feat (csrc/host/scene.cpp) picks F from facts about the scene, and the launch may clear
LDSTREE and adds the form's bits.

ROWS has one row per base feature set: the smallest scene that selects it (its builder steers
choose_feat's own inputs: media, a BVH under a Translate, a quad or triangle among the spheres,
three shading cases, a uv-needing material, a tree larger than the LDS mirror, the share of
sibling sphere-leaf pairs), or the reason no scene can.  Every case renders a 32 x 32 frame,
asserts the exact feature word the launch passed to kernel_for (gs_debug_last_launch_feat) and
compares the frame with the oracle through tests/parity.py and the counters through
counters_match (paths and pixels exactly).  Forms:

  loop    adaptive settings (batch 4, max 16, tolerance 0.05), gs_set_adaptive_mode(0);
  fixed   fixed_spp(8), auto chunks (one chunk per pixel: the oracle's association);
  rounds  (GS_KR rows) the loop's settings in batch rounds, split items (the RSPLIT kernel) and
          whole-batch items (the loop's kernel): frame and counters equal the loop's bit for bit;
  views   (GS_K and GS_KR rows) two cameras x 8 samples in one launch: each view equals its own
          fixed render bit for bit, and the oracle's through the helper.

tests/test_kernel_table_sync.py keeps ROWS and kernel_for's table in step without a GPU.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import camera_spec, fixed_spp, sample_settings
import oracle

from tests import parity

pytestmark = pytest.mark.gpu

# kernel_abi.hpp's GS_FEAT_*
MEDIA, NESTED, LEAFRUN, LDSTREE, MIXED, VISITS, SPHLEAF, FIXED, PLAIN, GENERAL, RSPLIT, VIEWS = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
GENERAL_KERNEL = GENERAL | MEDIA | NESTED | LEAFRUN | MIXED
FEAT_BITS = {"GS_FEAT_MEDIA": MEDIA, "GS_FEAT_NESTED": NESTED, "GS_FEAT_LEAFRUN": LEAFRUN, "GS_FEAT_LDSTREE": LDSTREE,
             "GS_FEAT_MIXED": MIXED, "GS_FEAT_VISITS": VISITS, "GS_FEAT_SPHLEAF": SPHLEAF, "GS_FEAT_FIXED": FIXED,
             "GS_FEAT_PLAIN": PLAIN, "GS_FEAT_GENERAL": GENERAL, "GS_FEAT_RSPLIT": RSPLIT, "GS_FEAT_VIEWS": VIEWS,
             "GS_FEAT_GENERAL_KERNEL": GENERAL_KERNEL}

W = 32
SEED = 7
ADAPTIVE = (0.95, 0.05, 4, 16)  # confidence, tolerance, batch, max samples: up to five batches
SPP = 8
FORMS = {"GS_K0": ("loop", "fixed"), "GS_K": ("loop", "fixed", "views"), "GS_KR": ("loop", "fixed", "rounds", "views")}


# ------------------------------------------------------------------ scene parts
def _camera(look_from=(0.0, 3.0, 9.0)):
    return camera_spec(1.0, W, 12, 50.0, look_from, (0.0, 0.3, -1.0), (0.0, 1.0, 0.0), 0.0, 9.0)


def _mats(b, kinds):
    """Materials by name: L Lambertian, M metal, D dielectric, U a uv-needing (image) Lambertian,
    E a solid light."""
    out = []
    for k in kinds:
        if k == "L":
            out.append(b.lambertian((0.7, 0.4, 0.3)))
        elif k == "M":
            out.append(b.metal((0.8, 0.8, 0.9), 0.2))
        elif k == "D":
            out.append(b.dielectric(1.5))
        elif k == "E":
            out.append(b.diffuse_light((2.0, 1.5, 1.0)))
        else:
            img = (np.arange(4 * 8 * 3, dtype=np.uint32) * 37 % 256).astype(np.uint8).reshape(4, 8, 3)
            out.append(b.lambertian_texture(b.image_texture(b.image(img))))
    return out


def _sky(b):
    """A small HDRI (8 x 4 texels, values that survive the RGBE round trip or not alike)."""
    t = (0.25 + (np.arange(4 * 8 * 3, dtype=np.float32) * 29 % 17) / 8.0).reshape(4, 8, 3)
    b.background_hdri(t, (0.3, 0.2, 0.0))


def _sphere(b, center, radius, m, single):
    """A sphere added to the world: as it is, or (single) as a BVH of its own.  The flattening inlines
    such a BVH as a node with one child, so the threaded records run node, sphere, node, sphere:
    no two sphere leaves are neighbours (has_leaf_runs counts no pair: LEAFRUN off) while every
    top-level leaf is still a stationary sphere (SPHLEAF)."""
    s = b.sphere(center, radius, m)
    return b.add(b.bvh([s]) if single else s)


def _row_of_spheres(b, mats, n, y=0.5, z=0.0, single=False):
    """n spheres side by side along x: sorted by x, the BVH pairs them up (leaf runs)."""
    return [_sphere(b, (1.1 * (k - (n - 1) / 2.0), y, z), 0.5, mats[k % len(mats)], single) for k in range(n)]


def _field(b, mats, prim, nx=46, nz=46, single=False):
    """nx x nz = 2116 small primitives on the ground: 2116 leaf records and at least as many node
    records, 165 KiB of threaded tree or more, more than any LDS mirror holds (GS_FEAT_LDSTREE off)."""
    for i in range(nx):
        for j in range(nz):
            x, z, m = 0.25 * (i - nx / 2.0), 2.5 - 0.25 * j, mats[(i + j) % len(mats)]
            if prim == "sphere":
                _sphere(b, (x, 0.1, z), 0.1, m, single)
            else:
                b.add(b.triangle((x - 0.1, 0.0, z + 0.1), (x + 0.1, 0.0, z + 0.1), (x, 0.2, z - 0.1), m))


def _alternating(b, mats, n=3):
    """Spheres and small quads alternating along x: no two sphere leaves are neighbours (no
    leaf runs), and the tree has a leaf that is no sphere."""
    for k in range(n):
        x = 2.4 * (k - (n - 1) / 2.0)
        b.add(b.sphere((x - 0.6, 0.5, 0.0), 0.5, mats[k % len(mats)]))
        b.add(b.quad((x + 0.1, 0.0, -0.4), (0.9, 0.0, 0.0), (0.0, 1.0, 0.3), mats[(k + 1) % len(mats)]))


def _backdrop(b, m):
    """One quad behind everything (its box's min x is the smallest: the BVH's first leaf)."""
    b.add(b.quad((-7.0, 0.0, -10.0), (14.0, 0.0, 0.0), (0.0, 5.0, 0.0), m))


def _flat(kinds, spheres=0, field=None, alternating=False, backdrop=False, sky=False, lone=False, single=False):
    def build():
        b = g.SceneBuilder()
        mats = _mats(b, kinds)
        b.background_solid((0.6, 0.7, 0.9))
        if sky:
            _sky(b)
        if lone:
            b.add(b.sphere((0.0, 0.3, -1.0), 1.5, mats[0]))
        if spheres:
            _row_of_spheres(b, mats, spheres, single=single)
        if field:
            _field(b, mats, field, single=single)
        if alternating:
            _alternating(b, mats)
        if backdrop:
            _backdrop(b, mats[0])
        return b
    return build


def _nonflat(media, nested, spheres):
    def build():
        b = g.SceneBuilder()
        white, red = b.lambertian((0.7, 0.7, 0.7)), b.lambertian((0.8, 0.3, 0.2))
        b.background_solid((0.6, 0.7, 0.9))
        _backdrop(b, white)
        if media:
            b.add(b.medium_isotropic(b.sphere((-2.0, 0.8, 1.0), 0.8, white), 1.5, (0.9, 0.9, 0.9)))
        if nested:
            members = [b.quad((-0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.2), red),
                       b.sphere((0.0, 0.5, 0.6), 0.3, b.metal((0.9, 0.9, 0.9), 0.0)),
                       b.triangle((-0.8, 0.0, 0.9), (0.8, 0.0, 0.9), (0.0, 0.9, 0.9), white)]
            b.add(b.translate(b.bvh(members), (2.0, 0.0, 1.0)))
        if spheres:
            _row_of_spheres(b, [white, red], spheres, z=-1.5)
        return b
    return build


def _general():
    b = g.SceneBuilder()
    white = b.lambertian((0.7, 0.7, 0.7))
    b.background_solid((0.6, 0.7, 0.9))
    obj = b.sphere((0.0, 0.5, 0.0), 0.5, b.metal((0.8, 0.8, 0.9), 0.1))
    for k in range(5):  # a chain deeper than 4: only the catch-all kernel walks it (validate)
        obj = b.rotate_y(obj, 9.0 * (k + 1)) if k % 2 == 0 else b.translate(obj, (0.1 * k, 0.05, -0.07 * k))
    b.add(obj)
    b.add(b.cube((-2.0, 0.0, -1.0), (-1.0, 1.0, 0.0), white))
    _backdrop(b, white)
    return b


@dataclasses.dataclass
class Row:
    feat: int
    macro: str        # the kernel_for line the set sits under: GS_K0, GS_K or GS_KR
    name: str
    build: object = None      # () -> SceneBuilder, or None when no scene validate accepts selects the set
    libm_free: bool = False   # no libm call on the colour path: every pixel equals the oracle's
    unreachable: str = ""

    @property
    def forms(self):
        return FORMS[self.macro]


ROWS = [
    # ---- media / BVHs under instances (never LDSTREE, MIXED or SPHLEAF)
    Row(MEDIA, "GS_K", "a medium and a backdrop quad", _nonflat(True, False, 0)),
    Row(NESTED, "GS_K", "a BVH under a Translate", _nonflat(False, True, 0)),
    Row(MEDIA | NESTED, "GS_K", "a medium and a BVH under a Translate", _nonflat(True, True, 0)),
    Row(LEAFRUN | MEDIA, "GS_K", "a medium and a row of 12 spheres", _nonflat(True, False, 12)),
    Row(LEAFRUN | NESTED, "GS_K", "a BVH under a Translate and a row of 12 spheres", _nonflat(False, True, 12)),
    Row(LEAFRUN | MEDIA | NESTED, "GS_K", "a medium, a BVH under a Translate, 12 spheres", _nonflat(True, True, 12)),
    # ---- flat trees with a leaf that is no sphere
    Row(0, "GS_KR", "2116 Lambertian triangles and a sphere", _flat("L", field="triangle", lone=True)),
    Row(LEAFRUN, "GS_KR", "2116 metal / dielectric spheres and a quad", _flat("MD", field="sphere", backdrop=True),
        libm_free=True),
    Row(LDSTREE, "GS_KR", "3 spheres and 3 quads alternating, Lambertian", _flat("L", alternating=True)),
    Row(LDSTREE | LEAFRUN, "GS_KR", "8 Lambertian / light spheres and a quad", _flat("LE", spheres=8, backdrop=True)),
    Row(MIXED, "GS_KR", "2116 triangles, Lambertian / metal, HDRI sky, a sphere",
        _flat("LM", field="triangle", lone=True, sky=True)),
    Row(MIXED | LEAFRUN, "GS_KR", "2116 spheres of three materials and a quad",
        _flat("LMD", field="sphere", backdrop=True)),
    Row(MIXED | LDSTREE, "GS_KR", "3 spheres and 3 quads alternating, three materials", _flat("LMD", alternating=True)),
    Row(MIXED | LDSTREE | LEAFRUN, "GS_KR", "8 spheres of three materials and a quad",
        _flat("LMD", spheres=8, backdrop=True)),
    # ---- sphere-only trees with leaf runs
    Row(SPHLEAF | LEAFRUN, "GS_KR", "2116 metal / dielectric spheres", _flat("MD", field="sphere"), libm_free=True),
    Row(SPHLEAF | LEAFRUN | LDSTREE, "GS_KR", "8 metal / dielectric / light spheres", _flat("MDE", spheres=8),
        libm_free=True),
    Row(SPHLEAF | LEAFRUN | MIXED, "GS_KR", "2116 spheres: Lambertian, metal, dielectric, image texture",
        _flat("LMDU", field="sphere")),
    Row(SPHLEAF | LEAFRUN | MIXED | LDSTREE, "GS_KR", "8 spheres: Lambertian, metal, dielectric, image texture",
        _flat("LMDU", spheres=8)),
    Row(SPHLEAF | LEAFRUN | MIXED | PLAIN, "GS_KR", "2116 spheres: Lambertian, metal, HDRI sky",
        _flat("LM", field="sphere", sky=True)),
    Row(SPHLEAF | LEAFRUN | MIXED | PLAIN | LDSTREE, "GS_KR", "8 spheres: Lambertian, metal, dielectric",
        _flat("LMD", spheres=8)),
    # ---- the catch-all kernel
    Row(GENERAL_KERNEL, "GS_K0", "a sphere under a chain of five instances", _general),
    # ---- sphere-only trees without leaf runs: a lone sphere, or every sphere in a BVH of its own
    Row(SPHLEAF, "GS_KR", "2116 metal spheres, each a BVH of its own", _flat("M", field="sphere", single=True),
        libm_free=True),
    Row(SPHLEAF | LDSTREE, "GS_KR", "a lone metal sphere", _flat("M", lone=True), libm_free=True),
    Row(SPHLEAF | MIXED, "GS_KR", "2116 single-sphere BVHs: Lambertian, metal, dielectric, image texture",
        _flat("LMDU", field="sphere", single=True)),
    Row(SPHLEAF | MIXED | LDSTREE, "GS_KR", "8 single-sphere BVHs: Lambertian, metal, dielectric, image texture",
        _flat("LMDU", spheres=8, single=True)),
    Row(SPHLEAF | MIXED | PLAIN, "GS_KR", "2116 single-sphere BVHs: Lambertian, metal, dielectric",
        _flat("LMD", field="sphere", single=True)),
    Row(SPHLEAF | MIXED | PLAIN | LDSTREE, "GS_KR", "8 single-sphere BVHs: Lambertian, metal, dielectric",
        _flat("LMD", spheres=8, single=True)),
]
BY_FEAT = {r.feat: r for r in ROWS}
REACHABLE = [r for r in ROWS if r.build is not None]


# ------------------------------------------------------------------ rendering
class _knobs:
    """gs_set_adaptive_mode / gs_debug_set_round_items for one block.  The library has no getters:
    on exit both go back to the library's defaults (adaptive mode 1, auto; round items 0, split),
    which is also what every other test module leaves set."""
    def __init__(self, mode, items=0):
        self.mode, self.items = mode, items

    def __enter__(self):
        N.check(N.lib.gs_set_adaptive_mode(self.mode))
        N.check(N.lib.gs_debug_set_round_items(self.items))

    def __exit__(self, *a):
        N.check(N.lib.gs_set_adaptive_mode(1))
        N.check(N.lib.gs_debug_set_round_items(0))


def _scene(row, settings, cam=None):
    return scenes.Scene("feat%d" % row.feat, _spec(row), cam or _camera(), settings)


_SPECS, _ORACLE, _GPU = {}, {}, {}


def _spec(row):
    if row.feat not in _SPECS:
        _SPECS[row.feat] = row.build().build()
    return _SPECS[row.feat]


def _oracle(row, key, sc, seed):
    """The oracle's frame and counters, rendered once per (row, settings, camera) and shared."""
    if (row.feat, key) not in _ORACLE:
        _ORACLE[(row.feat, key)] = oracle.render(sc, seed=seed)
    return _ORACLE[(row.feat, key)]


def _last_feat(r):
    d, f = C.c_void_p(), C.c_int32(-2)
    N.check(N.lib.gs_multi_scene(r.handle, 0, C.byref(d)))
    N.check(N.lib.gs_debug_last_launch_feat(d, C.byref(f)))
    return f.value


def _render(sc, seed=SEED):
    """One frame on a fresh one-device context: (frame, counters, the launched feature word,
    scene_info)."""
    r = g.MultiRenderer(sc, num_gpus=1, plan=False)
    try:
        out = r.render(seed=seed, rgb=True)
        return out["rgb"], out["counters"], _last_feat(r), r.scene_info()
    finally:
        r.close()


def _gpu(row, form):
    """The loop's and the fixed form's renders, shared by the forms that compare with them."""
    if (row.feat, form) not in _GPU:
        if form == "loop":
            with _knobs(0):
                _GPU[(row.feat, form)] = _render(_scene(row, sample_settings(*ADAPTIVE)))
        else:
            _GPU[(row.feat, form)] = _render(_scene(row, fixed_spp(SPP)))
    return _GPU[(row.feat, form)]


def counters_match(gpu, ref, rel=1e-4):
    """tests/test_gpu_parity.py's: paths and pixels exactly, traversal work within `rel`."""
    if gpu["paths"] != ref["paths"] or gpu["pixels"] != ref["pixels"]:
        return False
    return all(abs(gpu[k] - v) <= rel * max(v, 1) + 2 for k, v in ref.items())


def _launched(row, info, form_bits):
    """The word the launch must pass: the scene's choice plus the form's bits.  The rows' trees either
    fit every launch's mirror whole or fit none (asserted here), so no row's launch clears LDSTREE;
    that path has its own case, test_launch_clears_ldstree_for_the_larger_lane_state."""
    assert info["feat"] == row.feat, "choose_feat took %d, the row means %d" % (info["feat"], row.feat)
    whole = info["lds_nodes"] == info["node_records"] and info["lds_leaves"] == info["leaf_records"]
    assert whole == bool(row.feat & LDSTREE) or row.feat & (MEDIA | NESTED), (info, row.feat)
    return row.feat | form_bits


def _ids(rows):
    return ["feat%d" % r.feat for r in rows]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("row", REACHABLE, ids=_ids(REACHABLE))
def test_loop(row):
    out, gc, feat, info = _gpu(row, "loop")
    assert feat == _launched(row, info, 0)
    sc = _scene(row, sample_settings(*ADAPTIVE))
    ref, rc = _oracle(row, "adaptive", sc, SEED)
    assert gc["pixels"] == W * W and counters_match(gc, rc), (gc, rc)
    parity.check(out, ref, same_association=True, libm_free=row.libm_free, label="feat %d loop" % row.feat)


@pytest.mark.parametrize("row", REACHABLE, ids=_ids(REACHABLE))
def test_fixed(row):
    out, gc, feat, info = _gpu(row, "fixed")
    assert feat == _launched(row, info, FIXED)
    sc = _scene(row, fixed_spp(SPP))
    ref, rc = _oracle(row, "fixed", sc, SEED)
    assert gc["paths"] == W * W * SPP and counters_match(gc, rc), (gc, rc)
    parity.check(out, ref, same_association=True, libm_free=row.libm_free, label="feat %d fixed" % row.feat)


_KR = [r for r in REACHABLE if "rounds" in r.forms]


@pytest.mark.parametrize("items", [0, 1])
@pytest.mark.parametrize("row", _KR, ids=_ids(_KR))
def test_rounds(row, items):
    """Batch rounds in split items (the F | FIXED | RSPLIT kernel) and in whole-batch items (F):
    the loop's frame and counters bit for bit, hence the oracle's as test_loop found them."""
    loop, lc, _, _ = _gpu(row, "loop")
    with _knobs(2, items):
        out, gc, feat, info = _render(_scene(row, sample_settings(*ADAPTIVE)))
    assert feat == _launched(row, info, 0 if items else FIXED | RSPLIT)
    assert np.array_equal(out.view(np.int32), loop.view(np.int32)) and gc == lc
    ref, rc = _oracle(row, "adaptive", _scene(row, sample_settings(*ADAPTIVE)), SEED)
    assert counters_match(gc, rc)
    parity.check(out, ref, same_association=True, libm_free=row.libm_free,
                 label="feat %d rounds items %d" % (row.feat, items))


_K = [r for r in REACHABLE if "views" in r.forms]


@pytest.mark.parametrize("row", _K, ids=_ids(_K))
def test_views(row):
    """Two cameras x 8 samples in one launch.  View 0 is the fixed form's camera and seed; view 1
    looks from elsewhere with another seed."""
    cams = [_camera(), _camera((2.5, 2.0, 8.0))]
    seeds = [SEED, SEED + 4]
    sc = _scene(row, fixed_spp(SPP))
    r = g.MultiRenderer(sc, num_gpus=1, plan=False)
    try:
        got = r.render_views(cams, SPP, seeds)
        feat, info = _last_feat(r), r.scene_info()
    finally:
        r.close()
    assert feat == _launched(row, info, FIXED | VIEWS)
    one0, c0, _, _ = _gpu(row, "fixed")
    one1, c1, f1, _ = _render(_scene(row, fixed_spp(SPP), cams[1]), seed=seeds[1])
    assert f1 == row.feat | FIXED
    assert np.array_equal(got["rgb"][0].view(np.int32), one0.view(np.int32))
    assert np.array_equal(got["rgb"][1].view(np.int32), one1.view(np.int32))
    assert got["counters"] == {k: c0[k] + c1[k] for k in c0}
    for v, key in ((0, "fixed"), (1, "fixed_view1")):
        ref, rc = _oracle(row, key, _scene(row, fixed_spp(SPP), cams[v]), seeds[v])
        assert counters_match((c0, c1)[v], rc)
        parity.check(got["rgb"][v], ref, same_association=True, libm_free=row.libm_free,
                     label="feat %d view %d" % (row.feat, v))


def test_launch_clears_ldstree_for_the_larger_lane_state():
    """1250 spheres: ~100 KiB of threaded records, which fit the mirror beside a fixed-spp launch's
    lane state (~112 KiB of room) and not beside an adaptive launch's, 24 KiB larger.  The scene's
    choice has LDSTREE; the fixed launch keeps it and the loop's launch clears it (launch.cpp's
    launch shapes), and both frames are the oracle's."""
    def build():
        b = g.SceneBuilder()
        mats = _mats(b, "MD")
        b.background_solid((0.6, 0.7, 0.9))
        _field(b, mats, "sphere", nx=50, nz=25)
        return b
    row = Row(SPHLEAF | LEAFRUN | LDSTREE, "GS_KR", "1250 metal / dielectric spheres", build, libm_free=True)
    spec = build().build()
    for form, settings, want in (("fixed", fixed_spp(SPP), row.feat | FIXED),
                                 ("loop", sample_settings(*ADAPTIVE), row.feat & ~LDSTREE)):
        sc = scenes.Scene("prefix", spec, _camera(), settings)
        with _knobs(0):
            out, gc, feat, info = _render(sc)
        assert info["feat"] == row.feat
        assert info["lds_nodes"] == info["node_records"] and info["lds_leaves"] == info["leaf_records"]
        assert feat == want, (form, feat, want)
        ref, rc = oracle.render(sc, seed=SEED)
        assert counters_match(gc, rc)
        parity.check(out, ref, same_association=True, libm_free=True, label="prefix %s" % form)
