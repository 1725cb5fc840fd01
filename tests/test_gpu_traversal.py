"""Every flavour of the traversal loop (render.hip, "traverse") in checked frames.

The loop between the shading stage and the leaf stage is written into gs_render_kernel's body:
whole frames are its only test.  Its variants are chosen by facts that the kernel matrix's scenes
never vary, so this module varies them, on the matrix's own rows (tests/test_gpu_kernel_matrix.py:
ROWS, 32 x 32 frames, 8 spp fixed, the ADAPTIVE settings for the per-lane loop).  None of them
changes a ray, the tree or a decision of the reference's, so every comparison between two device
renders is exact: the frames' f32 bits with np.array_equal, the counter dicts with ==.

  a  test_cert_boxes_off*      gs_debug_set_cert_boxes(0): every node step takes the reference's f64
                               box test (node_step(slow_t, mixed_t)) where the default takes the
                               certified f32 one.  Every row, fixed and loop; rounds and views on
                               four rows (sets 68, 28, 3, 7).
  b  test_mirror_cuts          gs_debug_set_mirror_budget: the LDS mirror cut at 0, 32, 80, 32 + 2 x 48,
                               T / 2, T - 1 and T bytes (T: the whole tree, quads and cubes); the
                               prefixes asserted from scene_info, the launched feature word with
                               LDSTREE exactly when the tree is whole; the smallest and the largest
                               budget again with cert_boxes off (the f64 flavour reading global
                               memory and LDS).
  c  test_wave_knobs*          shade batch, leaf batch, node steps, camera batch and blocks per CU:
                               they only regroup lanes.
  d  test_noncert_camera_rays  camera rays of 2^-60 and 2^-460 times the unit camera's (no cert rays;
                               at 2^-460 the sphere roots' division flavour) among cert bounce rays:
                               the unit camera's frame and counters (tests/traversal_cases.py).
  e  test_the_1e15_rule        a box maximum of exactly 1e15 keeps cert_boxes, one ulp more clears
                               it; both frames and all counters are the oracle's exactly.

test_default_fixed_is_the_oracles compares the fixed form's default with the oracle as the matrix's
test_fixed does, so the module stands on its own.  Every hook and knob is set by `_set`, which puts
all of them back to the library's defaults on exit; test_zz_settings_are_restored renders one row
again after everything else and finds the scene record, the launch and the frame of a render made
before the module's first test.  Each comparison prints its differing pixels and counters
(pytest -s): DESIGN.md §2.6's table.
"""
import collections
import ctypes as C

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import renderer
from grayshift_amd.scene import fixed_spp, sample_settings
import oracle

from tests import parity
from tests import test_gpu_kernel_matrix as KM
from tests import traversal_cases as TC

pytestmark = pytest.mark.gpu

ROWS, REACHABLE, BY_FEAT = KM.ROWS, KM.REACHABLE, KM.BY_FEAT
LDSTREE, FIXED, RSPLIT, VIEWS = KM.LDSTREE, KM.FIXED, KM.RSPLIT, KM.VIEWS
NONFLAT = KM.MEDIA | KM.NESTED | KM.GENERAL  # rows whose kernels never take LDSTREE (choose_feat)
W, SPP, SEED, ADAPTIVE = KM.W, KM.SPP, KM.SEED, KM.ADAPTIVE

# form -> (gs_set_adaptive_mode, gs_debug_set_round_items, the bits the launch adds to the scene's word)
FORMS = {"fixed": (1, 0, FIXED), "loop": (0, 0, 0), "rounds0": (2, 0, FIXED | RSPLIT), "rounds1": (2, 1, 0),
         "views": (1, 0, FIXED | VIEWS)}
VIEW_SEEDS = [SEED, SEED + 4]
FOUR = [BY_FEAT[f] for f in (68, 28, 3, 7)]  # the rows that also run rounds and views
# (shade_batch, leaf_batch, node_steps, cam_batch, blocks_per_cu); sample_chunk stays -1
WAVE_KNOBS = [(1, 1, 1, 1, 0), (64, 64, 8, 64, 0), (52, 12, 3, 7, 1), (44, 24, 5, 33, 8)]

Shot = collections.namedtuple("Shot", "rgb counters feat info stage")
Stage = collections.namedtuple("Stage", "n_quads n_cubes lds_quads lds_cubes")


class _set:
    """The process-wide hooks and knobs for one block: cert boxes, the mirror budget, the wave knobs,
    the adaptive mode and the rounds' items.  The library has no getters: on exit every one goes back
    to the library's default, which is also what every other test module leaves set."""
    def __init__(self, cert=1, budget=-1, wave=None, mode=1, items=0):
        self.cert, self.budget, self.wave, self.mode, self.items = cert, budget, wave, mode, items

    def __enter__(self):
        try:
            N.check(N.lib.gs_debug_set_cert_boxes(self.cert))
            N.check(N.lib.gs_debug_set_mirror_budget(self.budget))
            if self.wave is not None:
                shade, leaf, steps, cam, per_cu = self.wave
                N.check(N.lib.gs_set_tuning(shade, per_cu, leaf, -1))
                N.check(N.lib.gs_set_node_steps(steps))
                N.check(N.lib.gs_set_camera_batch(cam))
            N.check(N.lib.gs_set_adaptive_mode(self.mode))
            N.check(N.lib.gs_debug_set_round_items(self.items))
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        N.check(N.lib.gs_debug_set_cert_boxes(1))
        N.check(N.lib.gs_debug_set_mirror_budget(-1))
        N.check(N.lib.gs_set_tuning(0, 0, 0, -1))
        N.check(N.lib.gs_set_node_steps(0))
        N.check(N.lib.gs_set_camera_batch(0))
        N.check(N.lib.gs_set_adaptive_mode(1))
        N.check(N.lib.gs_debug_set_round_items(0))


def _stage(r):
    d, s = C.c_void_p(), N.gs_debug_leaf_stage()
    N.check(N.lib.gs_multi_scene(r.handle, 0, C.byref(d)))
    N.check(N.lib.gs_debug_leaf_stage_record(d, C.byref(s), C.sizeof(s)))
    return Stage(s.n_quads, s.n_cubes, s.lds_quads, s.lds_cubes)


def _shoot(sc, seed=SEED, views=None, **settings):
    """One render of a scene uploaded under `settings` (_set's arguments), on a fresh one-device
    context.  views: a list of cameras for one views launch (seeds VIEW_SEEDS), frames [V, H, W, 3]."""
    with _set(**settings):
        r = g.MultiRenderer(sc, num_gpus=1, plan=False)
        try:
            got = r.render_views(views, SPP, VIEW_SEEDS) if views else r.render(seed=seed, rgb=True)
            return Shot(got["rgb"], got["counters"], KM._last_feat(r), r.scene_info(), _stage(r))
        finally:
            r.close()


def _run(row, form, **settings):
    mode, items, _ = FORMS[form]
    sc = KM._scene(row, fixed_spp(SPP) if form in ("fixed", "views") else sample_settings(*ADAPTIVE))
    views = [KM._camera(), KM._camera((2.5, 2.0, 8.0))] if form == "views" else None
    return _shoot(sc, views=views, mode=mode, items=items, **settings)


_DEFAULT = {}


def _default(row, form):
    """The row's render under the library's defaults, once per form.  The fixed and the loop forms
    share the kernel matrix's renders (KM._gpu); rounds and views are rendered here."""
    if (row.feat, form) not in _DEFAULT:
        if form in ("fixed", "loop"):
            _DEFAULT[row.feat, form] = Shot(*KM._gpu(row, form), None)
        else:
            _DEFAULT[row.feat, form] = _run(row, form)
    return _DEFAULT[row.feat, form]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _equal(label, got, base):
    """Frame and counters of two device renders, exactly; the differing counts first."""
    diff_px = int((_bits(got.rgb) != _bits(base.rgb)).any(axis=-1).sum()) if got.rgb.shape == base.rgb.shape else -1
    diff_c = sorted(k for k in base.counters if got.counters.get(k) != base.counters[k])
    print("traversal %s: diff_px %d diff_counters %d %s" % (label, diff_px, len(diff_c), " ".join(diff_c)))
    assert np.array_equal(_bits(got.rgb), _bits(base.rgb)), "%s: %d pixels differ" % (label, diff_px)
    assert got.counters == base.counters, "%s: %s" % (label, {k: (got.counters[k], base.counters[k]) for k in diff_c})


def _ids(cases):
    return ["feat%d-%s" % (r.feat, f) for r, f in cases]


BOTH = [(r, f) for r in REACHABLE for f in ("fixed", "loop")]
# rounds where the row's kernel has them (the GS_KR lines), views on all four
MORE = [(r, f) for r in FOUR for f in ("rounds0", "rounds1", "views") if f.rstrip("01") in r.forms]


# ------------------------------------------------------------------ the module's own footing
def _bare(sc):
    """A render that sets nothing: under the process's settings as they stand."""
    r = g.MultiRenderer(sc, num_gpus=1, plan=False)
    try:
        out = r.render(seed=SEED, rgb=True)
        return Shot(out["rgb"], out["counters"], KM._last_feat(r), r.scene_info(), _stage(r))
    finally:
        r.close()


@pytest.fixture(scope="module", autouse=True)
def before():
    """One row's fixed render and records before the module's first test (test_zz_settings_are_restored)."""
    return _bare(KM._scene(BY_FEAT[28], fixed_spp(SPP)))


@pytest.mark.parametrize("row", REACHABLE, ids=KM._ids(REACHABLE))
def test_default_fixed_is_the_oracles(row):
    d = _default(row, "fixed")
    assert d.feat == KM._launched(row, d.info, FIXED)
    ref, rc = KM._oracle(row, "fixed", KM._scene(row, fixed_spp(SPP)), SEED)
    assert d.counters["paths"] == W * W * SPP and KM.counters_match(d.counters, rc), (d.counters, rc)
    parity.check(d.rgb, ref, same_association=True, libm_free=row.libm_free, label="feat %d fixed" % row.feat)


# ------------------------------------------------------------------ a. certified versus f64 node test
def _cert_off(row, form):
    base = _default(row, form)
    assert base.info["cert_boxes"] == 1 and base.info["feat"] == row.feat
    got = _run(row, form, cert=0)
    assert got.info["cert_boxes"] == 0
    assert got.info["feat"] == row.feat and got.feat == base.feat == row.feat | FORMS[form][2]
    _equal("feat %d %s cert_boxes 0" % (row.feat, form), got, base)


@pytest.mark.parametrize("row,form", BOTH, ids=_ids(BOTH))
def test_cert_boxes_off(row, form):
    _cert_off(row, form)


@pytest.mark.parametrize("row,form", MORE, ids=_ids(MORE))
def test_cert_boxes_off_rounds_and_views(row, form):
    _cert_off(row, form)


# ------------------------------------------------------------------ b. mirror cuts
def _mirror_bytes(s):
    return 32 * s.info["lds_nodes"] + 48 * s.info["lds_leaves"] + 128 * s.stage.lds_quads + 96 * s.stage.lds_cubes


def _mirror(s):
    return (s.info["lds_nodes"], s.info["lds_leaves"], s.stage.lds_quads, s.stage.lds_cubes)


@pytest.mark.parametrize("row,form", BOTH, ids=_ids(BOTH))
def test_mirror_cuts(row, form):
    """T = 32 node_records + 48 leaf_records + 128 n_quads + 96 n_cubes.  place_records fills node and
    leaf records first, then a prefix of the quads, then the cube records, so under a budget B the
    tree is whole exactly when B >= 32 node_records + 48 leaf_records (T for the sphere-only rows:
    whole at T, cut at T - 1), and the mirror is the default's exactly when B holds the default's
    bytes.  The rows of 2116 primitives exceed the block's own budget, which caps the hook's: they
    stay cut at every budget, and T itself is not among theirs."""
    base = _default(row, form)
    full = _run(row, form)  # (the default again, for the leaf stage's record)
    _equal("feat %d %s default again" % (row.feat, form), full, base)
    nodes, leaves = full.info["node_records"], full.info["leaf_records"]
    tree = 32 * nodes + 48 * leaves
    T = tree + 128 * full.stage.n_quads + 96 * full.stage.n_cubes
    fits = full.info["lds_nodes"] == nodes and full.info["lds_leaves"] == leaves  # T within the auto budget
    flat = not row.feat & NONFLAT
    assert fits == bool(row.feat & LDSTREE) or not flat
    assert _mirror_bytes(full) <= T
    budgets = sorted({0, 32, 80, 32 + 2 * 48, T // 2, T - 1} | ({T} if fits else set()))
    for b in budgets:
        for cert in ((1, 0) if b in (budgets[0], budgets[-1]) else (1,)):
            got = _run(row, form, budget=b, cert=cert)
            label = "feat %d %s budget %d%s" % (row.feat, form, b, "" if cert else " cert_boxes 0")
            i = got.info
            assert i["cert_boxes"] == cert and (i["node_records"], i["leaf_records"]) == (nodes, leaves)
            assert _mirror_bytes(got) <= b, (label, _mirror(got))
            if b == 0:
                assert _mirror(got) == (0, 0, 0, 0), label
            if b == 32:
                assert _mirror(got) == (min(1, nodes), 0, 0, 0), label
            whole = i["lds_nodes"] == nodes and i["lds_leaves"] == leaves
            if fits:
                assert whole == (b >= tree), (label, _mirror(got))
                assert (_mirror(got) == _mirror(full)) == (b >= _mirror_bytes(full)), (label, _mirror(got), _mirror(full))
            else:  # more records than the block's own budget holds, whatever the hook allows
                assert not whole and _mirror_bytes(got) <= _mirror_bytes(full), (label, _mirror(got))
            # choose_feat saw the mirror: LDSTREE exactly with a whole tree (flat rows), and the launch kept the word
            want = (row.feat & ~LDSTREE) | (LDSTREE if whole and flat else 0)
            assert i["feat"] == want and got.feat == want | FORMS[form][2], (label, i["feat"], got.feat, want)
            _equal(label, got, base)


# ------------------------------------------------------------------ c. wave knobs
def _knobs(row, form):
    base = _default(row, form)
    for wave in WAVE_KNOBS:
        got = _run(row, form, wave=wave)
        assert got.info["feat"] == row.feat and got.feat == base.feat
        assert got.info["node_steps"] <= wave[2]  # (the knob reached the launch: its steps, or the kernel's unroll limit)
        _equal("feat %d %s knobs %s" % (row.feat, form, "/".join(map(str, wave))), got, base)


@pytest.mark.parametrize("row,form", BOTH, ids=_ids(BOTH))
def test_wave_knobs(row, form):
    _knobs(row, form)


@pytest.mark.parametrize("row,form", MORE, ids=_ids(MORE))
def test_wave_knobs_rounds_and_views(row, form):
    _knobs(row, form)


# ------------------------------------------------------------------ d. non-cert rays among cert rays
@pytest.mark.parametrize("name", list(TC.SCALE_SCENES))
def test_noncert_camera_rays(name):
    """tests/traversal_cases.py: the camera's rays at focus distance 2^-60 and 2^-460 are the unit
    camera's scaled by a power of two, so frame and counters are the unit camera's bit for bit;
    they are no cert rays (the bound below) in a scene of certified boxes, whose bounce rays are."""
    one = _shoot(TC.scale_scene(name, 1.0))
    assert one.info["cert_boxes"] == 1
    ref, rc = oracle.render(TC.scale_scene(name, 1.0), seed=SEED)
    assert one.counters["paths"] == W * W * SPP and KM.counters_match(one.counters, rc), (one.counters, rc)
    parity.check(one.rgb, ref, same_association=True, label="scale %s focus 1" % name)
    for scale, s in TC.SCALES.items():
        sc = TC.scale_scene(name, s)
        bound = TC.camera_ray_bound(renderer.camera(sc.camera))
        assert max(bound) < TC.NONCERT, bound
        got = _shoot(sc)
        assert got.info["cert_boxes"] == 1 and got.feat == one.feat
        _equal("scale %s focus %s" % (name, scale), got, one)
        sref, src = oracle.render(sc, seed=SEED)
        assert KM.counters_match(got.counters, src), (got.counters, src)
        parity.check(got.rgb, sref, same_association=True, label="scale %s focus %s" % (name, scale))
    off = _shoot(TC.scale_scene(name, 1.0), cert=0)
    assert off.info["cert_boxes"] == 0 and off.feat == one.feat
    _equal("scale %s focus 1 cert_boxes 0" % name, off, one)


# ------------------------------------------------------------------ e. the 1e15 rule
@pytest.mark.parametrize("name", list(TC.BIG_X))
def test_the_1e15_rule(name):
    sc = TC.big_scene(name)
    got = _shoot(sc)
    assert got.info["cert_boxes"] == TC.BIG_CERT[name]
    ref, rc = oracle.render(sc, seed=SEED)
    print("traversal big %s: differing counters %s" % (name, sorted(k for k in rc if got.counters[k] != rc[k])))
    parity.check(got.rgb, ref, same_association=True, libm_free=True, label="big %s" % name)
    assert got.counters == rc, {k: (got.counters[k], v) for k, v in rc.items() if got.counters[k] != v}


# ------------------------------------------------------------------ the settings are restored
def test_zz_settings_are_restored(before):
    """The module's last test: a render under the settings as the module leaves them is the one
    made before its first test -- the scene record (cert_boxes, the mirror's prefixes, node_steps,
    the feature word), the leaf stage's record, the launched word, the frame and the counters."""
    after = _bare(KM._scene(BY_FEAT[28], fixed_spp(SPP)))
    assert after.info == before.info and after.stage == before.stage and after.feat == before.feat
    assert after.info["cert_boxes"] == 1 and after.feat == 28 | FIXED
    _equal("feat 28 fixed after the module", after, before)
