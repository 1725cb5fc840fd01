"""CPU tests of the views calls (a batch of cameras in one launch): every argument rule returns
GS_ERR_ARG before any device work -- with a scene pointer that would fault if it were read and
no device in the machine -- gs_views_chunk follows the one-view chunk rule, and the ctypes
records match the library's.  No compute on a device."""
import ctypes as C

import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes

P = C.c_void_p
OK = P(0x1000)  # a non-null pointer that must never be followed
W, H = 72, 40


@pytest.fixture(scope="module")
def cam():
    c = g.camera(scenes.config("C4", width=W, spp=1).camera)
    assert (c.image_width, c.image_height) == (W, H)
    return c


def _views(cam, n=3):
    v = (N.gs_view * n)()
    for k in range(n):
        v[k].cam = cam
        v[k].seed = k + 1
    return v


def _call(views, n, samples, chunk, scene=OK, part="rr", outs="rgb"):
    part = {"rr": N.gs_partition(0, 1, 64, 64, None, 0, 0), "bad": N.gs_partition(2, 2, 64, 64, None, 0, 0),
            "null": None}[part]
    o = {"rgb": N.gs_render_outputs(0x2000, None, None), "rgb8": N.gs_render_outputs(None, 0x2000, None),
         "none": N.gs_render_outputs(None, None, None), "visits": N.gs_render_outputs(0x2000, None, 0x3000),
         "null": None}[outs]
    return N.lib.gs_render_tiles_views_async(scene, views, n, samples, chunk,
                                             C.byref(part) if part is not None else None,
                                             C.byref(o) if o is not None else None, None, None)


def _err():
    return N.lib.gs_last_error()


def test_views_reject_null_pointers_and_empty_batches(cam):
    v = _views(cam)
    assert _call(v, 3, 8, 4, scene=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(None, 3, 8, 4) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, part="null") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, outs="null") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, outs="none") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, outs="visits") == N.GS_ERR_ARG and b"visit" in _err()
    assert _call(v, 0, 8, 4) == N.GS_ERR_ARG and b"0 views" in _err()
    assert _call(v, 3, 8, 4, part="bad") == N.GS_ERR_ARG and b"partition" in _err()


def test_views_reject_views_of_another_size_or_depth_0(cam):
    v = _views(cam)
    v[2].cam.image_width = W + 1
    assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"view 2 differs" in _err()
    v = _views(cam)
    v[1].cam.image_height = H - 1
    assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"view 1 differs" in _err()
    v = _views(cam)
    v[1].cam.max_depth = 0
    assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"view 1 has max_depth 0" in _err()
    v = _views(cam)
    v[0].cam.image_width = 0
    assert _call(v, 1, 8, 4) == N.GS_ERR_ARG and b"image size" in _err()


def test_views_reject_bad_sample_counts(cam):
    v = _views(cam)
    assert _call(v, 3, 0, 4) == N.GS_ERR_ARG and b"0 samples" in _err()
    assert _call(v, 3, 10, 4) == N.GS_ERR_ARG and b"multiple" in _err()
    assert _call(v, 3, 24, 0) == N.GS_ERR_ARG and b"multiple" in _err()  # chunk 0 = 16
    assert _call(v, 3, 65 * 4, 4) == N.GS_ERR_ARG and b"64 chunks" in _err()
    assert _call(v, 3, 65, 1) == N.GS_ERR_ARG and b"64 chunks" in _err()


def test_views_reject_what_does_not_fit_32_bits(cam):
    big = N.gs_camera.from_buffer_copy(cam)
    big.image_width, big.image_height = 65536, 32768
    v = _views(big, 2)
    assert _call(v, 2, 8, 4) == N.GS_ERR_ARG and b"32-bit pixel" in _err()  # V W H = 2^32
    big.image_width, big.image_height = 1, 1 << 30
    assert _call(_views(big, 2), 2, 8, 4) == N.GS_ERR_ARG and b"32-bit pixel" in _err()  # V H = 2^31: no i32 height
    # the item count: capacity x samples / c, with the budget out of the way
    N.check(N.lib.gs_debug_set_partial_budget(1 << 62))
    try:
        mid = N.gs_camera.from_buffer_copy(cam)
        mid.image_width, mid.image_height = 16384, 16384  # x 3 views: 3 * 2^28 pixels, x 8 chunks >= 2^32
        assert _call(_views(mid, 3), 3, 32, 4) == N.GS_ERR_ARG and b"work items" in _err()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


def test_views_reject_chunk_sums_beyond_the_partial_budget(cam):
    """capacity of the tall W x 3H frame x (samples / c) x 24 bytes against the budget."""
    tall = N.gs_camera.from_buffer_copy(cam)
    tall.image_height = 3 * H
    cap = N.lib.gs_partition_capacity(C.byref(tall), C.byref(N.gs_partition(0, 1, 64, 64, None, 0, 0)))
    assert cap == 2 * 2 * 64 * 64  # 2 tile columns, 120 rows: 2 tile rows
    v = _views(cam)
    N.check(N.lib.gs_debug_set_partial_budget(cap * 2 * 24 - 1))
    try:
        assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"partial budget" in _err()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


def test_multi_render_views_rejects_a_null_context(cam):
    st = N.gs_stats()
    assert N.lib.gs_multi_render_views(None, _views(cam), 3, 8, 4, None, C.byref(st)) == N.GS_ERR_ARG
    assert b"null" in _err()


def test_views_chunk_is_the_one_view_rule():
    """gs_views_chunk: the coarse chunk of a one-shot render of ONE view's frame.  A small frame
    of a simple scene (C1's own 400 x 225 x 100: at most 4 x 256 CUs x 1024 lanes x c samples)
    takes 4, a larger one 16 -- however many views a call stacks."""
    small = g.camera(scenes.config("C1").camera)
    assert (small.image_width, small.image_height) == (400, 225)
    assert N.lib.gs_views_chunk(None, C.byref(small), 100) == 4
    large = g.camera(scenes.config("C1", width=1920).camera)
    assert N.lib.gs_views_chunk(None, C.byref(large), 100) == 16
    assert N.lib.gs_views_chunk(None, C.byref(large), 8) == 8      # (never more than the samples)
    assert N.lib.gs_views_chunk(None, C.byref(large), 6400) == 100  # (at most 64 chunks per pixel)
    g.set_tuning(0, 0, 0, 4)  # an explicit chunk
    try:
        assert N.lib.gs_views_chunk(None, C.byref(large), 100) == 4
    finally:
        g.set_tuning(0, 0, 0, -1)
    assert N.lib.gs_views_chunk(None, None, 100) == 0 and N.lib.gs_views_chunk(None, C.byref(small), 0) == 0


def test_native_struct_sizes_match_the_library():
    assert N.lib.gs_host_struct_size(b"gs_view") == C.sizeof(N.gs_view) == C.sizeof(N.gs_camera) + 8
    assert N.lib.gs_host_struct_size(b"gs_camera") == C.sizeof(N.gs_camera)
    assert N.lib.gs_version() == 11
