"""Views on the device: a batch of cameras of one scene in a single launch.

The contract (include/grayshift_gpu.h, DESIGN.md "Views"): view v's f32 and rgb8 frames are, bit
for bit, a one-shot fixed-spp render of camera v with seed seeds[v] and the same coarse chunk, and
the call's counters are the exact sums of those renders' -- whatever the number of views, their
order, the other cameras in the batch, the rank count, the tile size and the guided tail.

Checked with V = 3 views of 72 x 40 at 32 samples, c = 4, tile 64: the tall frame is 72 x 120, so
tile row 0 straddles views 0 and 1, the second tile column is partial and the last tile row is
mostly padding.  Each view has its own seed and look_from; view 1 has a defocus disk, view 2
max_depth 3 (the others 0 and 50): lanes of one wave mix all three.  One scene per kernel family,
built as tests/test_gpu_progressive.py builds them.
"""
import dataclasses

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import fixed_spp
import oracle

from tests.test_gpu_progressive import (_composition, _guided_tail, _same_device, counters_match, maxdiff, TOL)

pytestmark = pytest.mark.gpu
W, H, V = 72, 40, 3
CHUNK, TOTAL = 4, 32
SEEDS = [5, 9, 23]
ASPECT = 16.0 / 9.0  # 72 / (16 / 9) = 40.5 -> 40 rows, as Camera::new truncates

# name -> (scene at fixed_spp(32), the guided tail's forced percentage or 0)
SCENES = {
    "C4": (lambda: scenes.config("C4", width=W, spp=TOTAL), 0),                # the plain sphere kernel
    "C1_tail": (lambda: scenes.config("C1", width=W, spp=TOTAL), 10),          # coarse and fine regions of `partial`
    "cornell_smoke": (lambda: scenes.cornell_smoke(width=W, settings=fixed_spp(TOTAL)), 0),  # media
    "final_scene": (lambda: scenes.final_scene(width=W, boxes_per_side=4, n_balls=40,
                                               settings=fixed_spp(TOTAL)), 0),  # nested BVHs
}


def _cameras(sc, n=V):
    """n camera specs from the scene's: view v looks from a point of its own; view 1 through a
    defocus disk, the others through a pinhole; view 2 with max_depth 3, the others 50."""
    out = []
    for v in range(n):
        c = N.gs_camera_spec.from_buffer_copy(sc.camera)
        c.aspect_ratio = ASPECT
        c.image_width = W
        c.look_from[0] = sc.camera.look_from[0] * (1.0 + 0.07 * v) + 0.2 * v
        c.look_from[1] = sc.camera.look_from[1] * (1.0 + 0.04 * v) + 0.3 * v
        c.defocus_angle = 0.6 if v % 3 == 1 else 0.0
        if c.focus_distance <= 0.0:
            c.focus_distance = 10.0
        c.max_depth = 3 if v % 3 == 2 else 50
        out.append(c)
    return out


def _with_camera(sc, cam):
    return dataclasses.replace(sc, camera=cam)


def _views(sc, cams, seeds, tail=0, chunk=CHUNK, samples=TOTAL, **kw):
    """One views call on a fresh context (**kw: devices, tile, plan)."""
    with _guided_tail(tail):
        r = g.MultiRenderer(sc, **kw)
        try:
            return r.render_views(cams, samples, seeds, chunk=chunk, rgb=True, rgb8=True)
        finally:
            r.close()


def _sum_counters(cs):
    return {k: sum(c[k] for c in cs) for k in cs[0]}


_CACHE = {}


def _case(name):
    """The scene, its cameras, the one-shot render of each (f32, rgb8, counters) and the views call
    on one rank with tile 64, computed once and shared (never modified) by the tests below."""
    if name not in _CACHE:
        build, tail = SCENES[name]
        sc = build()
        cams = _cameras(sc)
        one, one8, oc = [], [], []
        g.set_tuning(0, 0, 0, CHUNK)
        try:
            with _guided_tail(tail):
                for cam, seed in zip(cams, SEEDS):
                    sv = _with_camera(sc, cam)
                    rgb, cnt = g.render(sv, seed=seed)
                    one.append(rgb)
                    oc.append(cnt)
                    one8.append(g.render_multi(sv, num_gpus=1, seed=seed, rgb=False, rgb8=True)["rgb8"])
        finally:
            g.set_tuning(0, 0, 0, -1)
        _CACHE[name] = {"scene": sc, "tail": tail, "cams": cams, "one": one, "one8": one8, "one_counters": oc,
                        "views": _views(sc, cams, SEEDS, tail)}
    return _CACHE[name]


def _same_bits(a, b):
    return (np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["rgb8"], b["rgb8"]) and
            a["counters"] == b["counters"])


# ------------------------------------------------------------ 1. each view == its one-shot render
@pytest.mark.parametrize("name", list(SCENES))
def test_each_view_equals_its_one_shot_render(name):
    c = _case(name)
    got = c["views"]
    assert got["rgb"].shape == (V, H, W, 3) and got["rgb8"].shape == (V, H, W, 3)
    for v in range(V):
        assert c["one"][v].shape == (H, W, 3)
        assert np.array_equal(got["rgb"][v], c["one"][v]), v
        assert np.array_equal(got["rgb8"][v], c["one8"][v]), v
    assert got["counters"] == _sum_counters(c["one_counters"])
    assert got["counters"]["paths"] == V * W * H * TOTAL and got["counters"]["pixels"] == V * W * H
    # the views differ (another camera, another seed): no view is a copy of another
    assert not np.array_equal(got["rgb"][0], got["rgb"][1]) and not np.array_equal(got["rgb"][0], got["rgb"][2])
    if name == "cornell_smoke":
        assert got["counters"]["medium_tests"] > 0


# ------------------------------------------------------------ 2. against the oracle
def test_views_match_the_oracle():
    c = _case("C4")
    refs = [oracle.render(_with_camera(c["scene"], cam), seed=seed) for cam, seed in zip(c["cams"], SEEDS)]
    for v in range(V):
        assert maxdiff(c["views"]["rgb"][v], refs[v][0]) < TOL, v
        assert counters_match(c["one_counters"][v], refs[v][1]), v
    assert counters_match(c["views"]["counters"], _sum_counters([r[1] for r in refs]))


# ------------------------------------------------------------ 3. nothing else moves a bit
def test_reversed_batch_gives_the_same_views():
    c = _case("C4")
    got = _views(c["scene"], c["cams"][::-1], SEEDS[::-1])
    assert np.array_equal(got["rgb"][::-1], c["views"]["rgb"])
    assert np.array_equal(got["rgb8"][::-1], c["views"]["rgb8"])
    assert got["counters"] == c["views"]["counters"]


def test_single_view_calls_give_the_same_views():
    c = _case("C4")
    r = g.MultiRenderer(c["scene"])
    try:
        parts = [r.render_views([cam], TOTAL, [seed], chunk=CHUNK, rgb=True, rgb8=True)
                 for cam, seed in zip(c["cams"], SEEDS)]
    finally:
        r.close()
    for v in range(V):
        assert np.array_equal(parts[v]["rgb"][0], c["views"]["rgb"][v]), v
        assert np.array_equal(parts[v]["rgb8"][0], c["views"]["rgb8"][v]), v
        assert parts[v]["counters"] == c["one_counters"][v], v
    assert _sum_counters([p["counters"] for p in parts]) == c["views"]["counters"]


def test_three_ranks_give_one_ranks_bits():
    """3 ranks on device 0 (same-device hook): the tall frame's 4 tiles round-robin, whatever the
    context's plan setting says."""
    c = _case("C4")
    for plan in (True, False):
        with _same_device():
            got = _views(c["scene"], c["cams"], SEEDS, devices=[0] * 3, tile=64, plan=plan)
        assert _same_bits(got, c["views"]), plan


@pytest.mark.parametrize("name", ["C4", "C1_tail"])
def test_tile_32_gives_tile_64s_bits(name):
    c = _case(name)
    assert _same_bits(_views(c["scene"], c["cams"], SEEDS, c["tail"], tile=32), c["views"])


def test_guided_tail_moves_no_bit():
    c = _case("C4")
    assert _same_bits(_views(c["scene"], c["cams"], SEEDS, tail=10), c["views"])


def test_render_views_groups_what_exceeds_the_partial_budget():
    """The one-call wrapper splits the cameras into consecutive groups whose chunk sums fit."""
    c = _case("C4")
    # one view's 72 x 40 frame: 2 tiles of 64 x 64, 8 chunks per pixel; two views' 72 x 80: 4 tiles
    N.check(N.lib.gs_debug_set_partial_budget(2 * 64 * 64 * (TOTAL // CHUNK) * 24))
    try:
        got = g.render_views(c["scene"], c["cams"], TOTAL, SEEDS, chunk=CHUNK, rgb=True, rgb8=True)
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))
    assert isinstance(got["stats"], list) and len(got["stats"]) == 3  # groups of 2, then 1, 1, 1
    assert _same_bits(got, c["views"])


# ------------------------------------------------------------ 4. the default chunk
def test_default_chunk_equals_plain_renders():
    """render_views(chunk=0) of C1-sized views (400 x 225 x 100: the small-frame rule gives a
    one-shot render c = 4; the tall frame's own size would give 16) equals plain render() calls
    with no tuning set."""
    sc = scenes.config("C1")
    cams = []
    for v in range(2):
        cam = N.gs_camera_spec.from_buffer_copy(sc.camera)
        cam.look_from[0] = sc.camera.look_from[0] + 1.5 * v
        cams.append(cam)
    r = g.MultiRenderer(sc)
    try:
        assert r.views_chunk(g.camera(cams[0]), 100) == 4
        got = r.render_views(cams, 100, [3, 4])
    finally:
        r.close()
    cnt = []
    for v in range(2):
        one, oc = g.render(_with_camera(sc, cams[v]), seed=3 + v)
        assert np.array_equal(got["rgb"][v], one), v
        cnt.append(oc)
    assert got["counters"] == _sum_counters(cnt)


# ------------------------------------------------------------ 5. the general kernel has no views form
def test_a_general_kernel_scene_is_unsupported():
    sc = _composition()
    r = g.MultiRenderer(sc)
    try:
        assert r.scene_info()["feat"] & 512  # GS_FEAT_GENERAL
        with pytest.raises(N.GrayshiftError) as e:
            r.render_views([sc.camera, sc.camera], TOTAL, chunk=CHUNK)
        assert e.value.code == N.GS_ERR_UNSUPPORTED
        # the context is still good for plain frames
        assert r.render(seed=1, rgb=True)["rgb"].shape == (r.height, r.width, 3)
    finally:
        r.close()
