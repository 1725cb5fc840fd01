"""Adaptive views (gs_render_tiles_views_rounds_async, gs_multi_views_adapt_*, ViewsAdaptiveRenderer;
include/grayshift_gpu.h "Adaptive views"): a batch of cameras under one set of adaptive settings, in
batch rounds on the tall frame.  View v's f32 frame, rgb8 bytes, `samples` map and `rel_error` map
equal those of AdaptiveRenderer on that camera alone, bit for bit, and the counters are the sums --
whatever the number and order of the views, the split into passes, the segment count, the sample
chunk, the rank count or a checkpoint in between.

Shapes: V = 3 views of 40 x 24 pixels in 16 x 8 tiles (a padding column; three tile rows per view),
batch 4, max_samples 16: five rounds, in whose late rounds a wave holds pixels of several views."""
import ctypes as C
import functools

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import camera_spec, sample_settings
import oracle

from tests import parity
from tests import test_gpu_kernel_matrix as M
from tests.test_gpu_parity import TOL, counters_match, maxdiff

pytestmark = pytest.mark.gpu

W, H, V = 40, 24, 3
TILE = (16, 8)
BS, MAXS = 4, 16
R = MAXS // BS + 1
SETTINGS = (0.95, 0.05, BS, MAXS)
SEEDS = [3, 4, 5]
# per view: max_depth, vfov, defocus angle (views 0 and 2 are pinholes)
DEPTH, VFOV, DEFOCUS = (12, 6, 9), (50.0, 40.0, 55.0), (0.0, 1.5, 0.0)


def _cams(look_from, look_at, focus):
    cams = [camera_spec(W / H, W, DEPTH[v], VFOV[v], look_from[v], look_at, (0.0, 1.0, 0.0), DEFOCUS[v], focus)
            for v in range(V)]
    for c in cams:
        gc = g.camera(c)
        assert (gc.image_width, gc.image_height) == (W, H)
    return cams


def _spheres():
    """Metal and dielectric spheres under a solid sky: no libm call on the colour path (the kernel
    matrix's libm_free rows), so the device's OCML and the oracle's glibc cannot differ by an ulp,
    no frame of it at a fixed spp differs from the oracle's in a bit.

    The oracle check (test_one_family_against_the_oracle) needs more: that the one-shot adaptive
    render of each camera, which the batch must equal bit for bit, takes the oracle's stop decisions.
    At batch 4 that render (the parent's code, per-lane loop and rounds alike) and the oracle can
    disagree on one pixel's stop test where f64 sample colours differ below f32 resolution: measured
    on MI355X with these three cameras and a ground sphere of radius 100, view 1 stopped pixel
    (12, 20) after 4 samples where the oracle took 20 (paths 11816 / 11832, |delta| 0.0525), and
    without a ground sphere one or two pixels per view differed; with the ground sphere of radius 20
    used here all three views have the oracle's paths and bits.  (With the radius-100 ground the
    batch equalled the one-shot renders bit for bit all the same: the difference is the one-shot
    render's, not the batch's.)"""
    b = g.SceneBuilder()
    b.add(b.sphere((0, 0, 0), 1.0, b.metal((0.5, 0.6, 0.7), 0.6)))
    b.add(b.sphere((1.6, -0.3, 0.5), 0.7, b.metal((0.8, 0.8, 0.8), 0.3)))
    b.add(b.sphere((-1.5, -0.4, 0.8), 0.6, b.dielectric(1.5)))
    b.add(b.sphere((0, -21, 0), 20.0, b.metal((0.4, 0.5, 0.3), 0.9)))
    b.background_solid((0.7, 0.8, 1.0))
    return b.build()


@functools.lru_cache(maxsize=None)
def _family(name):
    """(spec, cameras) of one kernel family: a sphere-only scene (the F | FIXED | RSPLIT | VIEWS form),
    a small cornell_smoke (media, the loop form F | VIEWS), a BVH under a Translate (nested, loop form)."""
    if name == "spheres":
        return _spheres(), _cams([(0, 1, 6), (4, 2, 4), (-3, 0.5, 5)], (0, 0, 0), 6.0)
    if name == "smoke":
        return (scenes.cornell_smoke(width=W).spec,
                _cams([(278, 278, -800), (100, 350, -760), (450, 200, -780)], (278, 278, 0), 800.0))
    assert name == "nested"
    return (M._nonflat(False, True, 0)().build(),
            _cams([(0.0, 3.0, 9.0), (2.5, 2.0, 8.0), (-3.0, 1.5, 7.0)], (0.0, 0.3, -1.0), 9.0))


FAMILIES = ["spheres", "smoke", "nested"]


def _scene(name, v=0, settings=SETTINGS):
    spec, cams = _family(name)
    return scenes.Scene(name, spec, cams[v], sample_settings(*settings))


def _single(name, v, rounds=None, settings=SETTINGS):
    """AdaptiveRenderer of view v's camera alone, `rounds` rounds (None: to the end)."""
    with g.AdaptiveRenderer(_scene(name, v, settings), seed=SEEDS[v], tile=TILE, plan=False) as ar:
        res = ar.render_rounds(R if rounds is None else rounds, rgb=True, rgb8=True)
        out = {"rgb": res["rgb"], "rgb8": res["rgb8"], "samples": ar.sample_counts(), "rel_error": ar.error_map(),
               "counters": res["info"]["counters"], "info": res["info"]}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, v, rounds=None):
    """Computed once, shared, never written to."""
    return _single(name, v, rounds)


def _batch(name, views=(0, 1, 2), passes=(R,), settings=SETTINGS, **kw):
    """The batch of `views` (indices into the family's cameras) in passes of `passes` rounds."""
    _, cams = _family(name)
    with g.ViewsAdaptiveRenderer(_scene(name, 0, settings), [cams[v] for v in views], seeds=[SEEDS[v] for v in views],
                                 tile=TILE, **kw) as r:
        res = None
        for n in passes:
            res = r.render_rounds(n, rgb=True, rgb8=True)
        return {"rgb": res["rgb"], "rgb8": res["rgb8"], "samples": r.sample_counts(), "rel_error": r.error_map(),
                "counters": res["info"]["counters"], "info": res["info"], "full": r.info()}


def _assert_views(got, name, views=(0, 1, 2), rounds=None, ref=None):
    refs = [ref(v) if ref else _reference(name, v, rounds) for v in views]
    for k, one in enumerate(refs):
        assert np.array_equal(got["rgb"][k].view(np.int32), one["rgb"].view(np.int32)), (name, views[k])
        assert np.array_equal(got["rgb8"][k], one["rgb8"]), (name, views[k])
        assert np.array_equal(got["samples"][k], one["samples"]), (name, views[k])
        assert np.array_equal(got["rel_error"][k], one["rel_error"], equal_nan=True), (name, views[k])
    assert got["counters"] == {c: sum(one["counters"][c] for one in refs) for c in refs[0]["counters"]}
    return refs


class _knobs:
    def __init__(self, chunk=-1, budget=0):
        self.chunk, self.budget = chunk, budget

    def __enter__(self):
        g.set_tuning(0, 0, 0, self.chunk)
        N.check(N.lib.gs_debug_set_partial_budget(self.budget))

    def __exit__(self, *a):
        g.set_tuning(0, 0, 0, -1)
        N.check(N.lib.gs_debug_set_partial_budget(0))


class _same_device:
    """N ranks on device 0 (gs_debug_set_multi_same_device): the N-rank frame loop on one GPU."""

    def __enter__(self):
        N.check(N.lib.gs_debug_set_multi_same_device(1))

    def __exit__(self, *a):
        N.check(N.lib.gs_debug_set_multi_same_device(0))


# ------------------------------------------------------------------ per-view parity
@pytest.mark.parametrize("name", FAMILIES)
def test_every_view_equals_its_own_adaptive_render(name):
    got = _batch(name)
    assert got["info"]["finished"] and got["info"]["active_pixels"] == 0
    refs = _assert_views(got, name)
    assert got["info"]["samples_total"] == got["counters"]["paths"]
    assert got["full"]["active_fractions"] == [0.0] * V and got["full"]["tile_h"] == TILE[1]
    for v, one in enumerate(refs):
        # (the frame context's one-shot render, g.render, gives AdaptiveRenderer's bits too)
        sc = _scene(name, v)
        rgb, cnt = g.render(sc, seed=SEEDS[v])
        assert np.array_equal(rgb.view(np.int32), one["rgb"].view(np.int32)) and cnt == one["counters"]


@pytest.mark.parametrize("name", FAMILIES)
def test_the_adaptive_logic_runs_in_every_view(name):
    """In each view the reference stops some pixels early and runs others on: the oracle's `paths`
    lies strictly between one batch and R batches of every pixel -- and so do the samples the batch
    took for the view, which are the one-shot render's."""
    got = _batch(name)
    for v in range(V):
        _, rc = oracle.render(_scene(name, v), seed=SEEDS[v])
        assert W * H * BS < rc["paths"] < W * H * R * BS, (name, v, rc["paths"])
        taken = int(got["samples"][v].sum())
        assert taken == _reference(name, v)["counters"]["paths"] and W * H * BS < taken < W * H * R * BS
        assert got["samples"][v].min() >= BS and got["samples"][v].max() <= R * BS


def test_one_family_against_the_oracle():
    got = _batch("spheres")
    total = None
    for v in range(V):
        ref, rc = oracle.render(_scene("spheres", v), seed=SEEDS[v])
        assert maxdiff(got["rgb"][v], ref) < TOL, v
        parity.check(got["rgb"][v], ref, same_association=True, label="adaptive views, view %d" % v)
        total = rc if total is None else {k: total[k] + rc[k] for k in rc}
    assert counters_match(got["counters"], total)


# ------------------------------------------------------------------ invariance
@pytest.mark.parametrize("name", FAMILIES)
def test_the_batch_reversed_and_one_view_alone(name):
    _assert_views(_batch(name, views=(2, 1, 0)), name, views=(2, 1, 0))
    _assert_views(_batch(name, views=(1,)), name, views=(1,))


@pytest.mark.parametrize("name", FAMILIES)
def test_passes_of_1_1_3_rounds(name):
    got = _batch(name, passes=(1, 1, 3))
    assert got["info"]["finished"]
    _assert_views(got, name)


@pytest.mark.parametrize("name", ["spheres", "smoke"])
def test_a_segment_boundary_inside_a_view(name):
    """A partial budget of 1000 pixels' batches: the 3456 packed pixels of the tall frame run in four
    segments, whose boundaries fall inside views."""
    with _knobs(budget=1000 * BS * 24):
        got = _batch(name)
    _assert_views(got, name)


@pytest.mark.parametrize("name", ["spheres", "smoke"])
def test_a_sample_chunk(name):
    with _knobs(chunk=2):
        got = _batch(name)
    _assert_views(got, name)


@pytest.mark.parametrize("name", FAMILIES)
def test_eight_same_device_ranks(name):
    with _same_device():
        got = _batch(name, devices=[0] * 8)
    _assert_views(got, name)


# ------------------------------------------------------------------ after k rounds
@pytest.mark.parametrize("name", FAMILIES)
def test_after_two_rounds_every_view_is_its_own_preview(name):
    got = _batch(name, passes=(2,))
    assert got["info"]["rounds"] == 2 and not got["info"]["finished"]
    refs = _assert_views(got, name, rounds=2)
    assert got["counters"]["pixels"] == sum(W * H - one["info"]["active_pixels"] for one in refs)
    assert got["info"]["active_pixels"] == sum(one["info"]["active_pixels"] for one in refs)
    assert got["full"]["active_fractions"] == [one["info"]["active_pixels"] / (W * H) for one in refs]


# ------------------------------------------------------------------ checkpoint
@pytest.mark.parametrize("name", ["spheres", "nested"])
def test_checkpoint_on_one_rank_resumes_on_eight(name, tmp_path):
    _, cams = _family(name)
    sc = _scene(name)
    path = str(tmp_path / "batch.vackpt")
    with g.ViewsAdaptiveRenderer(sc, cams, seeds=SEEDS, tile=TILE) as r:
        r.render_rounds(2)
        r.save(path)
        sums, state = r.state()
    assert sums.shape == (V, H, W, 5) and state.shape == (V, H, W)
    with _same_device():
        with g.ViewsAdaptiveRenderer.resume(sc, path, cams, tile=TILE, devices=[0] * 8) as r:
            assert r._info().rounds == 2
            s2, st2 = r.state()
            assert np.array_equal(s2, sums) and np.array_equal(st2, state)
            res = r.render_rounds(R, rgb=True, rgb8=True)
            got = {"rgb": res["rgb"], "rgb8": res["rgb8"], "samples": r.sample_counts(),
                   "rel_error": r.error_map(), "counters": res["info"]["counters"]}
    assert res["info"]["finished"]
    _assert_views(got, name)


# ------------------------------------------------------------------ refusals
def test_a_scene_of_the_catch_all_kernel_is_unsupported():
    spec = M._general().build()
    cams = _cams([(0.0, 3.0, 9.0), (2.5, 2.0, 8.0), (-3.0, 1.5, 7.0)], (0.0, 0.3, -1.0), 9.0)
    sc = scenes.Scene("general", spec, cams[0], sample_settings(*SETTINGS))
    mr = g.MultiRenderer(sc, num_gpus=1, tile=TILE, plan=False)
    try:
        assert mr.scene_info()["feat"] & 512
        views = (N.gs_view * V)()
        for v in range(V):
            views[v].cam, views[v].seed = g.camera(cams[v]), SEEDS[v]
        assert N.lib.gs_multi_views_adapt_begin(mr.handle, views, V, C.byref(mr.settings)) == N.GS_ERR_UNSUPPORTED
        assert b"catch-all" in N.lib.gs_last_error()
        assert N.lib.gs_multi_views_adapt_end(mr.handle) == N.GS_ERR_ARG  # (nothing was opened)
    finally:
        mr.close()
    with pytest.raises(N.GrayshiftError) as e:
        g.render_views_adaptive(sc, cams, seeds=SEEDS, tile=TILE)
    assert e.value.code == N.GS_ERR_UNSUPPORTED


def test_open_states_exclude_each_other():
    _, cams = _family("spheres")
    sc = _scene("spheres")
    mr = g.MultiRenderer(sc, num_gpus=1, tile=TILE, plan=False)
    L, h, ss = N.lib, None, None
    try:
        h, ss = mr.handle, C.byref(mr.settings)
        views = (N.gs_view * V)()
        for v in range(V):
            views[v].cam, views[v].seed = g.camera(cams[v]), SEEDS[v]
        cam = C.byref(mr.cam)
        info, ainfo = N.gs_views_adapt_info(), N.gs_adapt_info()
        # no views adaptation open: its calls refuse
        assert L.gs_multi_views_adapt_pass(h, 1, None, None) == N.GS_ERR_ARG and b"no views adaptation" in L.gs_last_error()
        assert L.gs_multi_views_adapt_info(h, C.byref(info), None) == N.GS_ERR_ARG
        assert L.gs_multi_views_adapt_maps(h, None, None) == N.GS_ERR_ARG
        assert L.gs_multi_views_adapt_end(h) == N.GS_ERR_ARG
        # open: every other frame call and begin refuses, and the plain adaptation's calls do not see it
        N.check(L.gs_multi_views_adapt_begin(h, views, V, ss))
        for status in (L.gs_multi_views_adapt_begin(h, views, V, ss), L.gs_multi_adapt_begin(h, cam, ss, 1),
                       L.gs_multi_accum_begin(h, cam, 1, 4), L.gs_multi_views_accum_begin(h, views, V, 4),
                       L.gs_multi_render(h, cam, ss, 1, None, None),
                       L.gs_multi_render_views(h, views, V, 8, 4, None, None)):
            assert status == N.GS_ERR_ARG and b"views adaptation is open" in L.gs_last_error()
        assert L.gs_multi_adapt_pass(h, 1, None, None) == N.GS_ERR_ARG and b"no adaptation" in L.gs_last_error()
        assert L.gs_multi_adapt_info(h, C.byref(ainfo)) == N.GS_ERR_ARG
        assert L.gs_multi_adapt_end(h) == N.GS_ERR_ARG
        assert L.gs_multi_views_adapt_pass(h, 0, None, None) == N.GS_ERR_ARG and b"0 rounds" in L.gs_last_error()
        N.check(L.gs_multi_views_adapt_info(h, C.byref(info), None))
        assert (info.width, info.height, info.n_views, info.tile_h, info.rounds, info.max_rounds) == (W, H, V, 8, 0, R)
        assert info.active_pixels == V * W * H
        N.check(L.gs_multi_views_adapt_end(h))
        # ... and in the other direction: it refuses while any of the other three is open
        for begin, end, what in ((lambda: L.gs_multi_adapt_begin(h, cam, ss, 1), L.gs_multi_adapt_end, b"an adaptation"),
                                 (lambda: L.gs_multi_accum_begin(h, cam, 1, 4), L.gs_multi_accum_end, b"an accumulation"),
                                 (lambda: L.gs_multi_views_accum_begin(h, views, V, 4), L.gs_multi_views_accum_end,
                                  b"a views accumulation")):
            N.check(begin())
            assert L.gs_multi_views_adapt_begin(h, views, V, ss) == N.GS_ERR_ARG and what in L.gs_last_error()
            assert L.gs_multi_views_adapt_pass(h, 1, None, None) == N.GS_ERR_ARG
            N.check(end(h))
        # the context renders on as before
        assert mr.render(seed=1, rgb=True)["counters"]["pixels"] == W * H
    finally:
        mr.close()


# ------------------------------------------------------------------ batch size 1
def test_batch_size_1_maps_hold_nan():
    """Batch 1: after the first round n - 1 = 0, the variance is 0/0 and the map NaN."""
    settings = (0.95, 0.5, 1, 5)
    got = _batch("spheres", passes=(1,), settings=settings)
    assert np.isnan(got["rel_error"]).all() and (got["samples"] == 1).all()
    _assert_views(got, "spheres", ref=lambda v: _single("spheres", v, rounds=1, settings=settings))
    got = _batch("spheres", passes=(6,), settings=settings)
    assert got["info"]["finished"]
    _assert_views(got, "spheres", ref=lambda v: _single("spheres", v, rounds=6, settings=settings))


def test_one_call_forms():
    """render_views_adaptive and MultiRenderer.render_views_adaptive: the renderer's bits."""
    _, cams = _family("spheres")
    sc = _scene("spheres")
    res = g.render_views_adaptive(sc, cams, seeds=SEEDS, tile=TILE, rgb8=True, maps=True)
    _assert_views(res, "spheres")
    mr = g.MultiRenderer(sc, num_gpus=1, tile=TILE, plan=False)
    try:
        res2 = mr.render_views_adaptive(cams, seeds=SEEDS)
    finally:
        mr.close()
    assert np.array_equal(res2["rgb"].view(np.int32), res["rgb"].view(np.int32)) and res2["counters"] == res["counters"]
