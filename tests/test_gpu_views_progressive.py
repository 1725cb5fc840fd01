"""Progressive views on the device: a batch of cameras refined in passes, view by view.

The contract (include/grayshift_gpu.h, DESIGN.md "Progressive views"): after any sequence of passes
in which view v received n_v samples, its f64 sums, f32 frame and rgb8 frame are bit for bit those
of a one-shot fixed-spp render of camera v with seed v, n_v samples and the same chunk, and the
cumulative counters are the exact sums of those renders' -- so no sample of an unselected view is
ever traced.  The comparison targets are independent paths through existing code: render_views
(gs_multi_render_views) and ProgressiveRenderer (gs_multi_accum_*).

Checked with V = 3 views of 40 x 24, c = 4, tile 16: the accumulation's tile height becomes 12
(gs_views_tile_h(24, 16)), so every view is 3 x 2 tiles, the third tile column is half padding, and
the tall frame has 18 tiles.  Each view has its own seed (1..3) and look_from; view 1 has a defocus
disk, view 2 max_depth 3 (the others 50).  One scene per kernel family with a views form, and one
with a forced guided tail (the combine's fine region).
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import fixed_spp

from tests.test_gpu_progressive import _composition, _guided_tail, _same_device

pytestmark = pytest.mark.gpu
W, H, V = 40, 24, 3
TILE, TILE_H = 16, 12
CHUNK, TOTAL = 4, 32
SEEDS = [1, 2, 3]
ASPECT = 1.66  # 40 / 1.66 = 24.1 -> 24 rows, as Camera::new truncates
PLANS = [(8, 8, 8, 8), (16, 16), (4, 28), (32,)]

# name -> (scene, the guided tail's forced percentage or 0)
SCENES = {
    "C4": (lambda: scenes.config("C4", width=W, spp=TOTAL), 0),                # the plain sphere kernel
    "C1_tail": (lambda: scenes.config("C1", width=W, spp=TOTAL), 10),          # coarse and fine regions of `partial`
    "cornell_box": (lambda: scenes.cornell_box(width=W, settings=fixed_spp(TOTAL)), 0),      # quads, cube lists
    "cornell_smoke": (lambda: scenes.cornell_smoke(width=W, settings=fixed_spp(TOTAL)), 0),  # media
    "final_scene": (lambda: scenes.final_scene(width=W, boxes_per_side=4, n_balls=40,
                                               settings=fixed_spp(TOTAL)), 0),  # nested BVHs
}


def _cameras(sc):
    out = []
    for v in range(V):
        c = N.gs_camera_spec.from_buffer_copy(sc.camera)
        c.aspect_ratio = ASPECT
        c.image_width = W
        c.look_from[0] = sc.camera.look_from[0] * (1.0 + 0.07 * v) + 0.2 * v
        c.look_from[1] = sc.camera.look_from[1] * (1.0 + 0.04 * v) + 0.3 * v
        c.defocus_angle = 0.6 if v == 1 else 0.0
        if c.focus_distance <= 0.0:
            c.focus_distance = 10.0
        c.max_depth = 3 if v == 2 else 50
        out.append(c)
    return out


def _sum_counters(cs):
    return {k: sum(c[k] for c in cs) for k in cs[0]}


def _open(sc, cams, **kw):
    kw.setdefault("tile", TILE)
    return g.ViewsProgressiveRenderer(sc, cams, seeds=SEEDS, chunk=CHUNK, **kw)


def _run(sc, cams, plan, tail=0, **kw):
    """plan: (samples, views or None) steps.  -> dict(rgb, rgb8, sums, info) after the last."""
    with _guided_tail(tail):
        p = _open(sc, cams, **kw)
        try:
            for n, views in plan[:-1]:
                p.render_pass(n, views, rgb=False)  # (the frames stay on the device)
            res = p.render_pass(plan[-1][0], plan[-1][1], rgb=True, rgb8=True)
            return {"rgb": res["rgb"], "rgb8": res["rgb8"], "sums": p.sums(), "info": p.info}
        finally:
            p.close()


def _one_shot(mr, cams, counts):
    """Each view alone through gs_multi_render_views at its own count: (rgb, rgb8, counters) lists;
    a view with 0 samples is zeros and no work."""
    rgb, rgb8, cnt = [], [], []
    for v, n in enumerate(counts):
        if n == 0:
            rgb.append(np.zeros((H, W, 3), np.float32))
            rgb8.append(np.zeros((H, W, 3), np.uint8))
            continue
        r = mr.render_views([cams[v]], n, [SEEDS[v]], chunk=CHUNK, rgb=True, rgb8=True)
        rgb.append(r["rgb"][0])
        rgb8.append(r["rgb8"][0])
        cnt.append(r["counters"])
    return rgb, rgb8, _sum_counters(cnt)


_CACHE = {}


def _case(name):
    """The scene, its cameras, the one-shot batch (render_views at 32 spp), each camera's
    ProgressiveRenderer sums, and the (8, 8, 8, 8) passes over all views on one rank: computed once
    and shared (never modified) by the tests below."""
    if name not in _CACHE:
        build, tail = SCENES[name]
        sc = build()
        cams = _cameras(sc)
        with _guided_tail(tail):
            mr = g.MultiRenderer(sc, tile=TILE, plan=False)
            try:
                views = mr.render_views(cams, TOTAL, SEEDS, chunk=CHUNK, rgb=True, rgb8=True)
            finally:
                mr.close()
            psums = []
            for cam, seed in zip(cams, SEEDS):
                with g.ProgressiveRenderer(dataclasses.replace(sc, camera=cam), seed=seed, chunk=CHUNK) as p:
                    p.render_pass(TOTAL, rgb=False)
                    psums.append(p.sums())
        _CACHE[name] = {"scene": sc, "tail": tail, "cams": cams, "views": views, "psums": np.stack(psums),
                        "passes": _run(sc, cams, [(n, None) for n in PLANS[0]], tail)}
    return _CACHE[name]


def _same_bits(a, b):
    return (np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["rgb8"], b["rgb8"]) and
            a["sums"].tobytes() == b["sums"].tobytes() and a["info"]["counters"] == b["info"]["counters"] and
            a["info"]["samples"] == b["info"]["samples"])


# ------------------------------------------------------------ 1. pass plans
@pytest.mark.parametrize("name", list(SCENES))
def test_pass_plans_equal_the_one_shot_batch(name):
    c = _case(name)
    ref = c["views"]
    assert ref["rgb"].shape == (V, H, W, 3)
    for plan in PLANS:
        got = c["passes"] if plan == PLANS[0] else _run(c["scene"], c["cams"], [(n, None) for n in plan], c["tail"])
        assert got["info"]["samples"] == [TOTAL] * V and got["info"]["passes"] == len(plan), plan
        assert got["info"]["tile_h"] == TILE_H and got["info"]["chunk"] == CHUNK
        assert np.array_equal(got["rgb"], ref["rgb"]), plan
        assert np.array_equal(got["rgb8"], ref["rgb8"]), plan
        assert got["sums"].shape == (V, H, W, 3) and got["sums"].tobytes() == c["psums"].tobytes(), plan
        assert got["info"]["counters"] == ref["counters"], plan
    assert ref["counters"]["pixels"] == V * W * H and ref["counters"]["paths"] == V * W * H * TOTAL
    # the sums are the frames': colour = sums / n, the division the resolve takes
    assert np.array_equal((c["passes"]["sums"] / float(TOTAL)).astype(np.float32), ref["rgb"])
    if name == "cornell_smoke":
        assert ref["counters"]["medium_tests"] > 0


# ------------------------------------------------------------ 2. per-view budgets
def test_per_view_budgets_trace_only_the_selected_views():
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    mr = g.MultiRenderer(sc, tile=TILE, plan=False)
    try:
        want, want8, want_cnt = _one_shot(mr, cams, [24, 8, 24])
        full24 = mr.render_views(cams, 24, SEEDS, chunk=CHUNK, rgb=True, rgb8=True)
    finally:
        mr.close()
    p = _open(sc, cams)
    try:
        p.render_pass(8, rgb=False)
        p.render_pass(8, [0, 2], rgb=False)
        res = p.render_pass(8, [0, 2], rgb=True, rgb8=True)
        assert list(p.samples) == [24, 8, 24]
        for v in range(V):
            assert np.array_equal(res["rgb"][v], want[v]), v
            assert np.array_equal(res["rgb8"][v], want8[v]), v
        # exactly the three renders' work: a traced row of view 1 would show here
        assert res["info"]["counters"] == want_cnt
        assert res["info"]["counters"]["paths"] == W * H * (24 + 8 + 24) and res["info"]["counters"]["pixels"] == V * W * H
        assert res["counters"]["paths"] == 2 * W * H * 8  # (this pass alone)
        # a pass over views whose counts differ is refused by the library (the Python layer groups them)
        sel = np.array([1, 1, 0], dtype=np.uint8)
        assert N.lib.gs_multi_views_accum_pass(p._mr.handle, 8, sel.ctypes.data, None, None) == N.GS_ERR_ARG
        assert b"different sample counts" in N.lib.gs_last_error()
        assert list(p.samples) == [24, 8, 24]
        # re-selecting the stopped view
        res = p.render_pass(16, [1], rgb=True, rgb8=True)
        assert list(p.samples) == [24, 24, 24]
        assert np.array_equal(res["rgb"], full24["rgb"]) and np.array_equal(res["rgb8"], full24["rgb8"])
        assert res["info"]["counters"] == full24["counters"]
    finally:
        p.close()


def test_python_layer_groups_views_by_count():
    """render_pass over views of different counts runs one launch per count; the result is the
    one-shot render of each view at its count."""
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    p = _open(sc, cams)
    try:
        p.render_pass(8, [0, 1], rgb=False)
        res = p.render_pass(8, None, rgb=True, rgb8=True)  # views 0, 1 at 8 and view 2 at 0: two launches
        assert list(p.samples) == [16, 16, 8] and len(res["stats"]) == 2
    finally:
        p.close()
    mr = g.MultiRenderer(sc, tile=TILE, plan=False)
    try:
        want, want8, want_cnt = _one_shot(mr, cams, [16, 16, 8])
    finally:
        mr.close()
    for v in range(V):
        assert np.array_equal(res["rgb"][v], want[v]) and np.array_equal(res["rgb8"][v], want8[v]), v
    assert res["info"]["counters"] == want_cnt


# ------------------------------------------------------------ 3. fresh output buffers
def test_every_pass_fills_a_fresh_buffer():
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    mr = g.MultiRenderer(sc, tile=TILE, plan=False)
    try:
        want, want8, _ = _one_shot(mr, cams, [16, 0, 8])
    finally:
        mr.close()
    for devices in (None, [0, 0]):  # (one rank writes the frames itself; two go through packed tiles)
        with _same_device():
            p = _open(sc, cams, **({"devices": devices} if devices else {}))
            try:
                a = p.render_pass(8, [0, 2], rgb=True, rgb8=True)   # new numpy buffers every call
                assert not a["rgb"][1].any() and not a["rgb8"][1].any()  # n_v = 0: all zeros
                assert np.array_equal(a["rgb"][2], want[2])
                b = p.render_pass(8, [0], rgb=True, rgb8=True)
                for v in range(V):  # views 1 and 2 unselected, still delivered
                    assert np.array_equal(b["rgb"][v], want[v]), (devices, v)
                    assert np.array_equal(b["rgb8"][v], want8[v]), (devices, v)
            finally:
                p.close()


# ------------------------------------------------------------ 4. per-view delta
def test_deltas_are_the_mean_change_per_view_and_deterministic():
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]

    def run():
        p = _open(sc, cams)
        try:
            out = []
            before, n0 = np.zeros((V, H, W, 3)), np.zeros(V, dtype=np.int64)
            last = np.zeros(V)
            for n, views in ((8, None), (4, [0, 2]), (12, [1]), (8, [0, 2])):
                info = p.render_pass(n, views, rgb=False)["info"]
                after = p.sums()
                sel = range(V) if views is None else views
                for v in range(V):
                    if v not in sel:
                        assert info["deltas"][v] == last[v], v  # an unselected view keeps its value
                        assert after[v].tobytes() == before[v].tobytes()
                        continue
                    old = before[v] / float(n0[v]) if n0[v] else np.zeros_like(before[v])
                    want = float(np.abs(after[v] / float(n0[v] + n) - old).mean())
                    # N = 40 * 24 * 3 = 2880 non-negative terms: N * 2^-53 = 3.2e-13 bounds the reassociation
                    assert abs(info["deltas"][v] - want) <= 1e-12 * want, (v, info["deltas"][v], want)
                    if n0[v] == 0:  # the first pass's delta is the mean |colour|
                        assert abs(info["deltas"][v] - float(np.abs(after[v] / float(n)).mean())) <= 1e-12 * want
                    n0[v] += n
                    last[v] = info["deltas"][v]
                before = after
                out.append(list(info["deltas"]))
            return out
        finally:
            p.close()

    a, b = run(), run()
    assert a == b  # the same bits run to run
    assert all(d > 0.0 for d in a[0])


# ------------------------------------------------------------ 5. ranks and checkpoint
def test_three_ranks_give_one_ranks_bits():
    c = _case("C4")
    plan = [(8, None), (8, [0, 2]), (8, [1]), (16, None)]
    one = _run(c["scene"], c["cams"], plan)
    with _same_device():
        three = _run(c["scene"], c["cams"], plan, devices=[0] * 3)
    assert _same_bits(three, one)
    assert _same_bits(one, c["passes"])
    # the tile size moves no bit either: tile 64 gives tile_h 24, one tile per view
    big = _run(c["scene"], c["cams"], plan, tile=64)
    assert big["info"]["tile_h"] == 24 and _same_bits(big, one)


@pytest.mark.parametrize("first,second", [(1, 2), (2, 1)])
def test_resume_on_another_rank_count(first, second, tmp_path):
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    path = str(tmp_path / "views.npz")
    with _same_device():
        p = _open(sc, cams, devices=[0] * first)
        try:
            p.render_pass(8, rgb=False)
            p.render_pass(8, [0, 2], rgb=False)
            assert list(p.samples) == [16, 8, 16]
            p.save(path)
            saved = p.info
        finally:
            p.close()
        q = g.ViewsProgressiveRenderer.resume(sc, path, cams, devices=[0] * second, tile=TILE)
        try:
            i = q.info
            assert i["samples"] == [16, 8, 16] and i["counters"] == saved["counters"] and i["deltas"] == saved["deltas"]
            assert q.seeds == SEEDS and q.chunk == CHUNK
            q.render_pass(8, [1], rgb=False)
            res = q.render_pass(16, rgb=True, rgb8=True)
            got = {"rgb": res["rgb"], "rgb8": res["rgb8"], "sums": q.sums(), "info": q.info}
        finally:
            q.close()
    assert _same_bits(got, c["passes"])
    assert got["info"]["passes"] == 4
    # a changed batch is rejected before any device work
    from grayshift_amd import checkpoint
    with pytest.raises(checkpoint.CheckpointError):
        g.ViewsProgressiveRenderer.resume(sc, path, cams, seeds=[1, 2, 4], tile=TILE)
    with pytest.raises(checkpoint.CheckpointError):
        g.ViewsProgressiveRenderer.resume(sc, path, cams[:2], tile=TILE)


# ------------------------------------------------------------ the tile primitive
def test_tile_primitive_with_a_callers_order_equals_the_context():
    """gs_render_tiles_views_pass_async on 2 ranks whose partition carries a tile order of the
    caller's (the tall frame's 18 tiles reversed, 9 slots a rank): the frames are the context's,
    the per-slot partials add up to its deltas, the counters to its counters."""
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    plan = [(8, None), (8, [0, 2])]
    want = _run(sc, cams, plan)
    gcams = [g.camera(s) for s in cams]
    views = (N.gs_view * V)()
    for v in range(V):
        views[v].cam, views[v].seed = gcams[v], SEEDS[v]
    tall = N.gs_camera.from_buffer_copy(gcams[0])
    tall.image_height = V * H
    tiles, world = (W + TILE - 1) // TILE * (V * H // TILE_H), 2
    assert tiles == 18
    order = np.arange(tiles, dtype=np.int32)[::-1].copy()
    slots, tpx = tiles // world, TILE * TILE_H
    cap = slots * tpx
    r = g.Renderer(sc, tile=TILE)  # (the device scene)
    bufs = []

    def alloc(nbytes):
        d = C.c_void_p()
        N.check(N.lib.gs_device_alloc(nbytes, C.byref(d)))
        bufs.append(d)
        z = np.zeros(nbytes, dtype=np.uint8)
        N.check(N.lib.gs_device_upload(d, z.ctypes.data, nbytes))
        return d.value

    try:
        d_order = alloc(order.nbytes)
        N.check(N.lib.gs_device_upload(C.c_void_p(d_order), order.ctypes.data, order.nbytes))
        gathered, frame = alloc(world * cap * 12), alloc(V * H * W * 12)
        per_rank = [(alloc(cap * 24), alloc(slots * 8), alloc(C.sizeof(N.gs_counters))) for _ in range(world)]
        total = {k: 0 for k in N.COUNTER_NAMES}
        change = np.zeros(V)
        counts = np.zeros(V, dtype=np.uint32)
        for n, sel_views in plan:
            sel = np.ones(V, dtype=np.uint8) if sel_views is None else np.isin(np.arange(V), sel_views).astype(np.uint8)
            change[sel != 0] = 0.0
            for k in range(world):
                part = N.gs_partition(k, world, TILE, TILE_H, d_order, slots, 0)
                assert N.lib.gs_partition_capacity(C.byref(tall), C.byref(part)) == cap
                sums, dpart, cnt = per_rank[k]
                out = N.gs_render_outputs(gathered + k * cap * 12, None, None)
                N.check(N.lib.gs_render_tiles_views_pass_async(r.dev, views, V, counts.ctypes.data, sel.ctypes.data, n,
                                                               CHUNK, C.byref(part), sums, C.byref(out), dpart, cnt,
                                                               None))
                parts = np.zeros(slots)
                N.check(N.lib.gs_device_download(parts.ctypes.data, C.c_void_p(dpart), parts.nbytes))
                for s in range(slots):  # rank after rank, each rank's partials in slot order
                    v = (int(order[k + s * world]) // 3) * TILE_H // H
                    if sel[v]:
                        change[v] += parts[s]
                    else:
                        assert parts[s] == 0.0
            counts[sel != 0] += n
        for k in range(world):
            got = N.gs_counters()
            N.check(N.lib.gs_device_download(C.byref(got), C.c_void_p(per_rank[k][2]), C.sizeof(N.gs_counters)))
            for name, v in got.as_dict().items():
                total[name] += v
        part0 = N.gs_partition(0, world, TILE, TILE_H, d_order, slots, 0)
        N.check(N.lib.gs_unpack_tiles_part_async(C.byref(tall), C.byref(part0), cap, C.c_void_p(gathered),
                                                 C.c_void_p(frame), 12, None))
        rgb = np.zeros((V, H, W, 3), dtype=np.float32)
        N.check(N.lib.gs_device_download(rgb.ctypes.data, C.c_void_p(frame), rgb.nbytes))
    finally:
        for d in bufs:
            N.lib.gs_device_free(d)
        r.close()
    assert list(counts) == want["info"]["samples"] == [16, 8, 16]
    assert np.array_equal(rgb, want["rgb"])
    for v in range(V):  # (another order of the additions: N = 2880 terms, N * 2^-53 = 3.2e-13)
        d = change[v] / (W * H * 3.0)
        assert abs(d - want["info"]["deltas"][v]) <= 1e-12 * d, v
    # the kernel counts the selected views' pixels at chunk 0 of every pass; everything else adds up
    assert total["pixels"] == (V + 2) * W * H
    total["pixels"] = V * W * H
    assert total == want["info"]["counters"]


# ------------------------------------------------------------ 6. render_until with min_delta
def test_render_until_stops_views_by_their_change():
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    rec = []
    with _open(sc, cams) as p:
        p.render_until(total_samples=TOTAL, pass_samples=8, on_pass=lambda info, fr: rec.append(list(info["deltas"])))
    assert len(rec) == 4

    def stops(thr):  # the samples each view ends with under threshold thr, by the recorded deltas
        out = []
        for v in range(V):
            k = next((k for k in range(4) if rec[k][v] < thr), 3)
            out.append(8 * (k + 1))
        return out

    # the threshold from the recorded run: the first midpoint between two recorded values under which
    # at least one view stops early and at least one runs to the end
    vals = sorted({d for r in rec for d in r})
    thr = next((0.5 * (a + b) for a, b in zip(vals, vals[1:])
                if min(stops(0.5 * (a + b))) < TOTAL and max(stops(0.5 * (a + b))) == TOTAL), None)
    assert thr is not None, rec
    want_n = stops(thr)
    with _open(sc, cams) as p:
        info, frames = p.render_until(total_samples=TOTAL, min_delta=thr, pass_samples=8)
        assert info["samples"] == want_n, (info["samples"], want_n, thr)
    mr = g.MultiRenderer(sc, tile=TILE, plan=False)
    try:
        want, _, want_cnt = _one_shot(mr, cams, want_n)
    finally:
        mr.close()
    for v in range(V):
        assert np.array_equal(frames[v], want[v]), v
    assert info["counters"] == want_cnt


# ------------------------------------------------------------ 7. exclusion
def test_an_open_views_accumulation_excludes_the_other_calls():
    c = _case("C4")
    sc, cams = c["scene"], c["cams"]
    p = _open(sc, cams)
    try:
        mr = p._mr
        st = N.gs_stats()
        L = N.lib
        assert L.gs_multi_render(mr.handle, C.byref(mr.cam), C.byref(mr.settings), 1, None, C.byref(st)) == N.GS_ERR_ARG
        assert b"views accumulation is open" in L.gs_last_error()
        with pytest.raises(N.GrayshiftError) as e:
            mr.render_views(cams, 8, SEEDS, chunk=CHUNK)
        assert e.value.code == N.GS_ERR_ARG
        assert L.gs_multi_accum_begin(mr.handle, C.byref(mr.cam), 1, CHUNK) == N.GS_ERR_ARG
        assert L.gs_multi_adapt_begin(mr.handle, C.byref(mr.cam), C.byref(scenes.config("A1").settings), 1) == N.GS_ERR_ARG
        assert L.gs_multi_views_accum_begin(mr.handle, p._views, V, CHUNK) == N.GS_ERR_ARG
        p.render_pass(8, rgb=False)
        N.check(L.gs_multi_views_accum_end(mr.handle))
        p._open = False
        assert L.gs_multi_views_accum_pass(mr.handle, 8, None, None, None) == N.GS_ERR_ARG
        assert b"no views accumulation is open" in L.gs_last_error()
        assert L.gs_multi_views_accum_end(mr.handle) == N.GS_ERR_ARG
        # after _end the context renders again: plain frames and views, with the context's own tiles
        assert mr.render(seed=1, rgb=True)["rgb"].shape == (mr.height, mr.width, 3)
        got = mr.render_views(cams, TOTAL, SEEDS, chunk=CHUNK, rgb=True, rgb8=True)
        assert np.array_equal(got["rgb"], c["views"]["rgb"]) and got["counters"] == c["views"]["counters"]
        # ... and the other accumulations exclude a views accumulation
        N.check(L.gs_multi_accum_begin(mr.handle, C.byref(mr.cam), 1, CHUNK))
        assert L.gs_multi_views_accum_begin(mr.handle, p._views, V, CHUNK) == N.GS_ERR_ARG
        N.check(L.gs_multi_accum_end(mr.handle))
    finally:
        p.close()


def test_a_general_kernel_scene_is_unsupported_at_begin():
    sc = _composition()
    with pytest.raises(N.GrayshiftError) as e:
        g.ViewsProgressiveRenderer(sc, [sc.camera, sc.camera], chunk=CHUNK)
    assert e.value.code == N.GS_ERR_UNSUPPORTED
