"""CPU tests of progressive views (a batch of cameras refined in passes, view by view): every
argument rule of the tile-level pass returns its status and message before any device work --
with a scene pointer that would fault if it were read and no device in the machine -- the frame
context's calls refuse a NULL context, gs_views_tile_h gives the documented tile heights, the
ctypes records match the library's, and checkpoint format 3 round-trips and is told apart from
formats 1 and 2.  No compute on a device."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import checkpoint, scenes

P = C.c_void_p
OK = P(0x1000)  # a non-null pointer that must never be followed
W, H = 72, 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _call(views, n, samples, chunk, counts=(0, 0, 0), selected=None, scene=OK, part="rr", outs="rgb", sums=OK):
    """gs_render_tiles_views_pass_async; tile height 20 divides H = 40."""
    part = {"rr": N.gs_partition(0, 1, 64, 20, None, 0, 0), "bad": N.gs_partition(2, 2, 64, 20, None, 0, 0),
            "straddle": N.gs_partition(0, 1, 64, 64, None, 0, 0), "null": None}[part]
    o = {"rgb": N.gs_render_outputs(0x2000, None, None), "rgb8": N.gs_render_outputs(None, 0x2000, None),
         "none": N.gs_render_outputs(None, None, None), "visits": N.gs_render_outputs(0x2000, None, 0x3000),
         "null": None}[outs]
    ns = np.array(list(counts), dtype=np.uint32) if counts is not None else None
    sel = np.array(list(selected), dtype=np.uint8) if selected is not None else None
    return N.lib.gs_render_tiles_views_pass_async(
        scene, views, n, ns.ctypes.data if ns is not None else None, sel.ctypes.data if sel is not None else None,
        samples, chunk, C.byref(part) if part is not None else None, sums,
        C.byref(o) if o is not None else None, None, None, None)


def _err():
    return N.lib.gs_last_error()


# ------------------------------------------------------------ the tile-level pass's argument rules
def test_pass_rejects_null_pointers_and_empty_batches(cam):
    v = _views(cam)
    assert _call(v, 3, 8, 4, scene=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(None, 3, 8, 4) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, counts=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, sums=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, part="null") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, outs="null") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, outs="none") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, 8, 4, outs="visits") == N.GS_ERR_ARG and b"visit" in _err()
    assert _call(v, 0, 8, 4) == N.GS_ERR_ARG and b"0 views" in _err()
    assert _call(v, 3, 8, 4, part="bad") == N.GS_ERR_ARG and b"partition" in _err()


def test_pass_rejects_views_of_another_size_or_depth_0(cam):
    v = _views(cam)
    v[2].cam.image_width = W + 1
    assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"view 2 differs" in _err()
    v = _views(cam)
    v[1].cam.image_height = H - 1
    assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"view 1 differs" in _err()
    v = _views(cam)
    v[1].cam.max_depth = 0
    assert _call(v, 3, 8, 4) == N.GS_ERR_ARG and b"view 1 has max_depth 0" in _err()


def test_pass_rejects_bad_sample_counts(cam):
    v = _views(cam)
    assert _call(v, 3, 0, 4) == N.GS_ERR_ARG and b"0 samples" in _err()
    assert _call(v, 3, 10, 4) == N.GS_ERR_ARG and b"multiple" in _err()
    assert _call(v, 3, 24, 0) == N.GS_ERR_ARG and b"multiple" in _err()  # chunk 0 = 16
    assert _call(v, 3, 65 * 4, 4) == N.GS_ERR_ARG and b"64 chunks" in _err()
    # a view's stored samples are whole chunks too, selected or not
    assert _call(v, 3, 8, 4, counts=(8, 6, 8), selected=(1, 0, 1)) == N.GS_ERR_ARG and b"view 1's samples" in _err()
    # ... and stay below 2^32
    top = (1 << 32) - 4
    assert _call(v, 3, 8, 4, counts=(top, top, top)) == N.GS_ERR_ARG and b"overflow 32 bits" in _err()


def test_pass_rejects_an_empty_or_mixed_selection(cam):
    v = _views(cam)
    assert _call(v, 3, 8, 4, selected=(0, 0, 0)) == N.GS_ERR_ARG and b"empty selection" in _err()
    assert _call(v, 3, 8, 4, counts=(8, 16, 8), selected=(1, 1, 0)) == N.GS_ERR_ARG and b"different sample counts" in _err()
    assert _call(v, 3, 8, 4, counts=(8, 16, 8)) == N.GS_ERR_ARG and b"different sample counts" in _err()  # NULL = all


def test_pass_rejects_tiles_that_straddle_views(cam):
    assert _call(_views(cam), 3, 8, 4, part="straddle") == N.GS_ERR_ARG and b"straddle" in _err()


def test_pass_rejects_what_does_not_fit_32_bits(cam):
    big = N.gs_camera.from_buffer_copy(cam)
    big.image_width, big.image_height = 65536, 32768
    assert _call(_views(big, 2), 2, 8, 4, counts=(0, 0)) == N.GS_ERR_ARG and b"32-bit pixel" in _err()
    N.check(N.lib.gs_debug_set_partial_budget(1 << 62))
    try:
        mid = N.gs_camera.from_buffer_copy(cam)
        mid.image_width, mid.image_height = 16384, 16384  # x 3 views: 3 * 2^28 pixels, x 8 chunks >= 2^32
        assert _call(_views(mid, 3), 3, 32, 4) == N.GS_ERR_ARG and b"work items" in _err()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


def test_pass_rejects_chunk_sums_beyond_the_partial_budget(cam):
    tall = N.gs_camera.from_buffer_copy(cam)
    tall.image_height = 3 * H
    cap = N.lib.gs_partition_capacity(C.byref(tall), C.byref(N.gs_partition(0, 1, 64, 20, None, 0, 0)))
    assert cap == 2 * 6 * 64 * 20  # 2 tile columns, 120 rows: 6 tile rows of 20
    N.check(N.lib.gs_debug_set_partial_budget(cap * 2 * 24 - 1))
    try:
        assert _call(_views(cam), 3, 8, 4) == N.GS_ERR_ARG and b"partial budget" in _err()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


# ------------------------------------------------------------ the frame context's calls
def test_context_calls_reject_a_null_context(cam):
    v = _views(cam)
    info = N.gs_views_accum_info()
    ns = np.zeros(3, dtype=np.uint32)
    sums = np.zeros((3, H, W, 3))
    cnt = N.gs_counters()
    L = N.lib
    assert L.gs_multi_views_accum_begin(None, v, 3, 4) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_accum_pass(None, 8, None, None, None) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_accum_info(None, C.byref(info), None, None) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_accum_download(None, sums.ctypes.data) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_accum_upload(None, v, 3, 4, ns.ctypes.data, sums.ctypes.data,
                                         C.byref(cnt)) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_accum_end(None) == N.GS_ERR_ARG and b"null" in _err()


# ------------------------------------------------------------ gs_views_tile_h
@pytest.mark.parametrize("h,t,want", [(225, 64, 45), (1080, 64, 60), (24, 16, 12), (64, 64, 64), (719, 64, 1)])
def test_views_tile_h(h, t, want):
    got = N.lib.gs_views_tile_h(h, t)
    assert got == want and h % got == 0 and got <= t
    assert all(h % k for k in range(got + 1, min(h, t) + 1))  # the largest such divisor


def test_views_tile_h_rejects_bad_arguments():
    assert N.lib.gs_views_tile_h(0, 64) == 0 and N.lib.gs_views_tile_h(64, 0) == 0 and N.lib.gs_views_tile_h(-3, 4) == 0
    assert N.lib.gs_views_tile_h(8, 64) == 8  # a tile taller than the view: the view's height


# ------------------------------------------------------------ records
def test_native_struct_sizes_match_the_library():
    assert N.lib.gs_host_struct_size(b"gs_views_accum_info") == C.sizeof(N.gs_views_accum_info)
    assert N.lib.gs_host_struct_size(b"gs_view") == C.sizeof(N.gs_view)
    assert N.lib.gs_host_struct_size(b"gs_counters") == C.sizeof(N.gs_counters)
    assert N.lib.gs_version() == 11


def test_info_record_follows_the_header():
    """gs_views_accum_info's fields, in the header's order, in bindings/grayshift_gpu.rs and in _native."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gs_views_accum_info \{(.*?)\} gs_views_accum_info;", hdr, re.S).group(1)
    c_names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
               for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    rs = re.search(r"pub struct gs_views_accum_info \{(.*?)\}",
                   open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read(), re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+)\s*:", rs) == c_names
    assert [k for k, _ in N.gs_views_accum_info._fields_] == c_names


# ------------------------------------------------------------ checkpoint format 3
V = 3


def _meta(cam):
    cams = []
    for v in range(V):
        c = N.gs_camera.from_buffer_copy(cam)
        c.center[0] += v
        cams.append(bytes(c))
    return {"samples": [8, 24, 0], "seeds": [1, 2, 3], "cameras": cams, "chunk": 4, "width": W, "height": H,
            "counters": {n: 7 * k + 1 for k, n in enumerate(checkpoint.COUNTER_NAMES)}, "passes": 5,
            "deltas": [0.25, 0.125, 0.0]}


def _file(write, *args):
    f = io.BytesIO()
    write(f, *args)
    f.seek(0)
    return f


def test_views_checkpoint_round_trip(cam):
    meta = _meta(cam)
    sums = np.random.default_rng(3).random((V, H, W, 3))
    sums[2] = 0.0
    got, m = checkpoint.read_views_checkpoint(_file(checkpoint.write_views_checkpoint, sums, meta))
    assert got.dtype == np.float64 and got.tobytes() == sums.tobytes()
    assert m == meta
    checkpoint.check_views_compatible(m, W, H, 4, [1, 2, 3], meta["cameras"])
    checkpoint.check_views_compatible(m, W, H, 4, [1, 2, 3], meta["cameras"], samples=[8, 24, 0])


def test_views_checkpoint_write_rejects_bad_records(cam):
    meta = _meta(cam)
    sums = np.zeros((V, H, W, 3))
    for bad in ({"samples": [8, 6, 0]}, {"samples": [8, 24]}, {"seeds": [1, 2]}, {"chunk": 0}):
        with pytest.raises(checkpoint.CheckpointError):
            checkpoint.write_views_checkpoint(io.BytesIO(), sums, dict(meta, **bad))
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_views_checkpoint(io.BytesIO(), np.zeros((V, H, W + 1, 3)), meta)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_views_checkpoint(io.BytesIO(), sums, {k: v for k, v in meta.items() if k != "cameras"})


def test_the_three_readers_reject_each_others_files(cam):
    meta = _meta(cam)
    f3 = _file(checkpoint.write_views_checkpoint, np.zeros((V, H, W, 3)), meta)
    m1 = {"samples": 8, "seed": 1, "chunk": 4, "width": W, "height": H, "camera": bytes(cam), "counters": meta["counters"]}
    f1 = _file(checkpoint.write_checkpoint, np.zeros((H, W, 3)), m1)
    m2 = {"rounds": 0, "seed": 1, "width": W, "height": H, "confidence": 1.96, "tolerance": 0.05, "batch_size": 4,
          "max_samples": 16, "camera": bytes(cam), "counters": meta["counters"]}
    f2 = _file(checkpoint.write_adaptive_checkpoint, np.zeros((H, W, 5)), np.zeros((H, W), dtype=np.uint32), m2)
    for f in (f1, f2):
        with pytest.raises(checkpoint.CheckpointError):
            checkpoint.read_views_checkpoint(f)
        f.seek(0)
    for read in (checkpoint.read_checkpoint, checkpoint.read_adaptive_checkpoint):
        with pytest.raises(checkpoint.CheckpointError):
            read(f3)
        f3.seek(0)
    checkpoint.read_checkpoint(f1)
    checkpoint.read_adaptive_checkpoint(f2)
    checkpoint.read_views_checkpoint(f3)


def test_views_checkpoint_rejects_any_mismatch(cam):
    meta = _meta(cam)
    _, m = checkpoint.read_views_checkpoint(_file(checkpoint.write_views_checkpoint, np.zeros((V, H, W, 3)), meta))
    cams = meta["cameras"]
    other = N.gs_camera.from_buffer_copy(cam)
    other.max_depth += 1
    cases = {
        "seed": (W, H, 4, [1, 9, 3], cams, None),
        "camera": (W, H, 4, [1, 2, 3], [cams[0], bytes(other), cams[2]], None),
        "chunk": (W, H, 8, [1, 2, 3], cams, None),
        "width": (W + 1, H, 4, [1, 2, 3], cams, None),
        "height": (W, H + 1, 4, [1, 2, 3], cams, None),
        "view count": (W, H, 4, [1, 2], cams[:2], None),
        "sample vector": (W, H, 4, [1, 2, 3], cams, [8, 24, 4]),
    }
    for what, (w, h, c, seeds, cs, ns) in cases.items():
        with pytest.raises(checkpoint.CheckpointError):  # (a changed `what`)
            checkpoint.check_views_compatible(m, w, h, c, seeds, cs, samples=ns)
