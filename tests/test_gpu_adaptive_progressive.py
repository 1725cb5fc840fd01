"""Progressive adaptive passes (gs_render_tiles_rounds_async, gs_multi_adapt_*, AdaptiveRenderer;
DESIGN.md §3.2): a frame's batch rounds split over passes on persistent state.  Whatever the
split, the rank count, the tile plan, the sample chunk, the partial budget or a checkpoint in
between, the finished frame, its rgb8 bytes and the counters are the one-shot render's, bit for
bit; after k rounds the frame is the one-shot frame with max_samples = k * batch - 1; the maps
and the state in image order follow the contract in include/grayshift_gpu.h."""
import ctypes as C
import functools

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import checkpoint, scenes
from grayshift_amd.scene import camera_spec, sample_settings

pytestmark = pytest.mark.gpu
STOPPED = np.uint32(0x80000000)


class _knobs:
    def __init__(self, chunk=-1, budget=0, items=0):
        self.chunk, self.budget, self.items = chunk, budget, items

    def __enter__(self):
        g.set_tuning(0, 0, 0, self.chunk)
        N.check(N.lib.gs_debug_set_partial_budget(self.budget))
        N.check(N.lib.gs_debug_set_round_items(self.items))

    def __exit__(self, *a):
        g.set_tuning(0, 0, 0, -1)
        N.check(N.lib.gs_debug_set_partial_budget(0))
        N.check(N.lib.gs_debug_set_round_items(0))


class _same_device:
    """N ranks on device 0 (gs_debug_set_multi_same_device): the N-rank frame loop on one GPU."""

    def __enter__(self):
        N.check(N.lib.gs_debug_set_multi_same_device(1))

    def __exit__(self, *a):
        N.check(N.lib.gs_debug_set_multi_same_device(0))


def _edge(width, batch, maxs, tol):
    b = g.SceneBuilder()
    m = b.lambertian((0.5, 0.6, 0.7))
    b.add(b.sphere((0, 0, 0), 1.0, m))
    b.add(b.sphere((0, -101, 0), 100.0, b.metal((0.8, 0.8, 0.8), 0.3)))
    b.add(b.quad((-2, -1, -2), (4, 0, 0), (0, 3, 0), b.dielectric(1.5)))
    b.background_solid((0.7, 0.8, 1.0))
    cam = camera_spec(1.0, width, 50, 40.0, (0, 1, 6), (0, 0, 0), (0, 1, 0), 0.0, 6.0)
    return scenes.Scene("edge", b.build(), cam, sample_settings(0.95, tol, batch, maxs))


def _sky(batch, maxs):
    """Every primary ray sees the solid sky (the sphere is behind the camera): the variance is 0
    and the first stop test passes."""
    b = g.SceneBuilder()
    b.add(b.sphere((0, 0, 60), 1.0, b.lambertian((0.5, 0.5, 0.5))))
    b.background_solid((0.7, 0.8, 1.0))
    cam = camera_spec(1.0, 48, 50, 20.0, (0, 0, 30), (0, 0, 0), (0, 1, 0), 0.0, 30.0)
    return scenes.Scene("sky", b.build(), cam, sample_settings(0.95, 0.05, batch, maxs))


@functools.lru_cache(maxsize=None)
def _scene(name, width=40):
    if name.startswith("edge"):
        _, batch, maxs, tol = name.split(":")
        return _edge(24, int(batch), int(maxs), float(tol))
    kw = {"final_scene": {"boxes_per_side": 4, "n_balls": 60}}.get(name, {})
    return scenes.SCENES[name](width=width, **kw)


def _with_max(sc, maxs):
    s = sc.settings
    return scenes.Scene(sc.name, sc.spec, sc.camera, sample_settings(s.confidence, s.tolerance, s.batch_size, maxs))


def _rounds_of(sc):
    return sc.settings.max_samples // sc.settings.batch_size + 1


def _one_shot(sc, seed, chunk=-1):
    with _knobs(chunk=chunk):
        r = g.render_multi(sc, num_gpus=1, seed=seed, rgb=True, rgb8=True)
    return r["rgb"], r["rgb8"], r["counters"]


@functools.lru_cache(maxsize=None)
def _reference(name, seed, width=40):
    """The one-shot render of a cached scene: computed once, shared, never written to."""
    rgb, rgb8, cnt = _one_shot(_scene(name, width), seed)
    rgb.setflags(write=False)
    rgb8.setflags(write=False)
    return rgb, rgb8, cnt


def _run_plan(ar, plan, R):
    """plan: 'ones', '3+rest' or 'all'.  Returns the last pass's result."""
    steps = {"ones": [1] * R, "3+rest": [3, R], "all": [R]}[plan]
    res = None
    for n in steps:
        res = ar.render_rounds(n, rgb=True, rgb8=True)
        if res["info"]["finished"]:
            break
    assert res["info"]["finished"] and res["info"]["active_pixels"] == 0
    return res


def _assert_final(res, ref):
    rgb, rgb8, cnt = ref
    assert np.array_equal(res["rgb"], rgb)
    assert np.array_equal(res["rgb8"], rgb8)
    assert res["info"]["counters"] == cnt


# ------------------------------------------------------------------ 1. final frame
@pytest.mark.parametrize("plan", ["ones", "3+rest", "all"])
@pytest.mark.parametrize("scene", ["hdri", "cornell_box", "cornell_smoke", "final_scene", "triangles"])
def test_final_frame_equals_the_one_shot_render(scene, plan):
    """The sphere-leaf, staged, media and nested kernel families, with and without a split-round
    instantiation, with the scenes' own settings."""
    sc = _scene(scene)
    with g.AdaptiveRenderer(sc, seed=2) as ar:
        res = _run_plan(ar, plan, _rounds_of(sc))
        assert ar.finished and ar.info.rounds <= _rounds_of(sc)
    _assert_final(res, _reference(scene, 2))


@pytest.mark.parametrize("plan", ["ones", "3+rest", "all"])
@pytest.mark.parametrize("batch,maxs,tol", [(1, 5, 0.5), (3, 17, 0.1), (7, 7, 0.2), (64, 200, 0.05)])
def test_final_frame_edge_settings(batch, maxs, tol, plan):
    """batch 1 (the first stop test is NaN), max_samples equal to the batch (two rounds), small
    and large tolerances."""
    name = "edge:%d:%d:%r" % (batch, maxs, tol)
    sc = _scene(name)
    with g.AdaptiveRenderer(sc, seed=5) as ar:
        res = _run_plan(ar, plan, _rounds_of(sc))
    _assert_final(res, _reference(name, 5))


def test_single_batch_settings_are_refused():
    """(batch 1, max_samples 0): max_samples < batch_size runs one batch -- not adaptive by the
    contract's own definition -- so the adaptation is refused with the pointer to the fixed-spp
    passes, and the context renders on as before."""
    sc = _edge(24, 1, 0, 0.0)
    mr = g.MultiRenderer(sc, num_gpus=1)
    try:
        assert N.lib.gs_multi_adapt_begin(mr.handle, C.byref(mr.cam), C.byref(mr.settings), 5) == N.GS_ERR_ARG
        assert b"one batch" in N.lib.gs_last_error()
        assert mr.render(seed=5, rgb=True)["counters"]["paths"] == sc.width * sc.height
    finally:
        mr.close()
    with pytest.raises(N.GrayshiftError):
        g.AdaptiveRenderer(sc, seed=5)


# ------------------------------------------------------------------ 2. preview
@pytest.mark.parametrize("name,width", [("cornell_box", 48), ("edge:3:17:0.1", 24)])
def test_preview_after_k_rounds_is_the_capped_one_shot_render(name, width):
    """After k rounds the frame is the one-shot frame with max_samples = k * bs - 1 (every pixel
    still active stops on that cap with Σrgb / (k bs)), and so are the counters but `pixels`,
    which counts the stopped pixels.  k = 1 compares with the per-lane loop over one batch
    (sample chunk 0: the additions in sample order)."""
    sc = _scene(name, width)
    bs, R = sc.settings.batch_size, _rounds_of(sc)
    ks = sorted({1, 2, 3, R - 1})
    got = {}
    with g.AdaptiveRenderer(sc, seed=7) as ar:
        for k in range(1, R):
            res = ar.render_rounds(1, rgb=True, rgb8=True)
            assert res["info"]["rounds"] == k
            if k in ks:
                got[k] = res
    for k in ks:
        rgb, rgb8, cnt = _one_shot(_with_max(sc, k * bs - 1), 7, chunk=0 if k == 1 else -1)
        info = got[k]["info"]
        assert np.array_equal(got[k]["rgb"], rgb), k
        assert np.array_equal(got[k]["rgb8"], rgb8), k
        mine = dict(info["counters"])
        assert cnt.pop("pixels") == sc.width * sc.height
        assert mine.pop("pixels") == sc.width * sc.height - info["active_pixels"]
        assert mine == cnt, k


# ------------------------------------------------------------------ 3. maps
def _error_reference(sums, state, ss):
    n = (state & ~STOPPED).astype(np.float64) * float(ss.batch_size)
    lsum, lsq = sums[..., 3], sums[..., 4]
    c2 = np.float64(ss.confidence) * np.float64(ss.confidence)
    with np.errstate(all="ignore"):
        mean = lsum / n
        var = 1.0 / (n - 1.0) * (lsq - lsum * lsum / n)
        return np.sqrt(c2 * var / n / (mean * mean)).astype(np.float32)


@pytest.mark.parametrize("name,width", [("cornell_box", 48), ("edge:1:5:0.5", 24), ("edge:1:1:0.5", 24)])
def test_maps_follow_the_state(name, width):
    """Batch 1: the first stop test is inf * 0 = NaN for every pixel (1 / (1 - 1) times an exact
    0), so nothing stops in round 0; from the second sample on the variance is finite and a
    pixel may stop (max_samples 5: the one-shot render stops them too,
    test_final_frame_edge_settings).  With max_samples 1 the second round is the cap, so every
    pixel takes R * bs = 2 samples."""
    sc = _scene(name, width)
    bs, R = sc.settings.batch_size, _rounds_of(sc)
    with g.AdaptiveRenderer(sc, seed=3) as ar:
        assert ar.sample_counts().max() == 0  # before the first pass
        for k in range(1, R + 1):
            res = ar.render_rounds(1, rgb=False)
            info = ar.info
            if k not in (1, 2, R) and not info.finished:
                continue
            samples, (sums, state) = ar.sample_counts(), ar.state()
            cnt = info.counters.as_dict()
            assert samples.dtype == np.uint32 and samples.shape == (sc.height, sc.width)
            assert int(samples.sum(dtype=np.uint64)) == cnt["paths"] == info.samples_total
            assert int(samples.max()) == info.samples_max
            assert np.all(samples % bs == 0) and samples.min() >= bs and samples.max() <= R * bs
            assert np.array_equal(samples, (state & ~STOPPED) * np.uint32(bs))
            stopped = (state & STOPPED) != 0
            assert int(((samples <= k * bs) & stopped).sum()) == cnt["pixels"]
            assert int((~stopped).sum()) == info.active_pixels
            assert np.all(samples[~stopped] == k * bs)
            assert np.array_equal(ar.error_map(), _error_reference(sums, state, sc.settings), equal_nan=True)
            if info.finished:
                break
        assert ar.finished and res["info"]["finished"]
        if name == "edge:1:1:0.5":  # round 0 cannot stop, round 1 is the cap
            assert np.all(ar.sample_counts() == R * bs) and ar.info.rounds == R
            assert ar.info.samples_total == R * bs * sc.width * sc.height == ar.info.counters.paths


def test_a_frame_that_stops_after_one_round():
    """Every pixel stops after its first batch while the settings allow 257 rounds: finished is
    set, a later pass renders nothing and delivers the same frame, and rounds stays 1."""
    sc = _sky(4, 1024)
    rgb, rgb8, cnt = _one_shot(sc, 4)
    with g.AdaptiveRenderer(sc, seed=4) as ar:
        first = ar.render_rounds(1, rgb=True, rgb8=True)
        assert ar.finished and ar.info.rounds == 1 and ar.info.active_pixels == 0
        assert np.all(ar.sample_counts() == 4)
        again = ar.render_rounds(5, rgb=True, rgb8=True)
        assert ar.info.rounds == 1 and again["counters"]["paths"] == 0
        info, frame = ar.render_until(rounds=9)
        assert frame is None and info["rounds"] == 1
        assert ar.info.counters.as_dict() == cnt
    for r in (first, again):
        assert np.array_equal(r["rgb"], rgb) and np.array_equal(r["rgb8"], rgb8)


# ------------------------------------------------------------------ 4. ranks and plans
def _trace(sc, seed, pass_rounds, **kw):
    """Everything observable of a run in passes of `pass_rounds` rounds."""
    frames = []
    with g.AdaptiveRenderer(sc, seed=seed, **kw) as ar:
        while not ar.finished:
            r = ar.render_rounds(pass_rounds, rgb=True, rgb8=True)
            frames.append((r["rgb"], r["rgb8"], ar.sample_counts(), ar.error_map()))
        sums, state = ar.state()
        return frames, sums, state, ar.info.counters.as_dict(), ar.info.rounds


def _assert_same_trace(a, b):
    assert len(a[0]) == len(b[0]) and a[4] == b[4]
    for fa, fb in zip(a[0], b[0]):
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
        assert np.array_equal(fa[2], fb[2]) and np.array_equal(fa[3], fb[3], equal_nan=True)
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    assert a[3] == b[3]


@pytest.fixture(scope="module")
def one_rank_trace():
    return _trace(_scene("cornell_box", 56), 3, 2, num_gpus=1)


@pytest.mark.parametrize("plan", [True, False])
def test_three_ranks_equal_one(one_rank_trace, plan):
    """3 ranks at tile 16 (16 tiles of a 56 x 56 frame, the last row and column half outside it:
    ranks of 6, 5 and 5 tiles, so padding slots and an empty slot), planned and round-robin: the frame after every pass, both maps, the state in
    image order and the counters are one rank's."""
    with _same_device():
        three = _trace(_scene("cornell_box", 56), 3, 2, devices=[0, 0, 0], tile=16, plan=plan)
    _assert_same_trace(three, one_rank_trace)
    assert np.array_equal(one_rank_trace[0][-1][0], _reference("cornell_box", 3, 56)[0])


# ------------------------------------------------------------------ 5. knobs
@pytest.mark.parametrize("knobs", [{"chunk": 1}, {"chunk": 3}, {"chunk": 32},
                                   {"budget": 100 * 32 * 24}, {"chunk": 3, "budget": 100 * 32 * 24}, {"items": 1}])
def test_knobs_change_no_bit(one_rank_trace, knobs):
    """Sample chunks per work item, a partial budget of 100 pixels' batches (the active list in
    segments) and whole-batch round items (ignored: the pass form always splits)."""
    sc = _scene("cornell_box", 56)
    assert sc.settings.batch_size == 32
    with _knobs(**knobs):
        t = _trace(sc, 3, 2, num_gpus=1)
    _assert_same_trace(t, one_rank_trace)


# ------------------------------------------------------------------ 6. checkpoint
def test_checkpoint_resumes_on_another_rank_count(one_rank_trace, tmp_path):
    sc = _scene("cornell_box", 56)
    path = str(tmp_path / "adapt.ckpt")
    with g.AdaptiveRenderer(sc, seed=3) as ar:
        ar.render_rounds(2, rgb=False)
        ar.save(path)
    with _same_device():
        with g.AdaptiveRenderer.resume(sc, path, devices=[0, 0], tile=16) as ar:
            assert ar.info.rounds == 2 and ar.seed == 3
            assert np.array_equal(ar.state()[1], checkpoint.read_adaptive_checkpoint(path)[1])
            res = None
            while not ar.finished:
                res = ar.render_rounds(3, rgb=True, rgb8=True)
            sums, state = ar.state()
            assert ar.info.rounds == one_rank_trace[4]
    ref = _reference("cornell_box", 3, 56)
    _assert_final(res, ref)
    assert sums.tobytes() == one_rank_trace[1].tobytes() and np.array_equal(state, one_rank_trace[2])


def test_resume_rejects_a_changed_scene(tmp_path):
    sc = _scene("cornell_box", 56)
    path = str(tmp_path / "adapt.ckpt")
    with g.AdaptiveRenderer(sc, seed=3) as ar:
        ar.render_rounds(1, rgb=False)
        ar.save(path)
    s = sc.settings
    moved = scenes.cornell_box(width=56)
    moved.camera.v_fov += 1.0
    others = {"tolerance": scenes.Scene(sc.name, sc.spec, sc.camera, sample_settings(s.confidence, 0.4, 32, 1000)),
              "batch_size": scenes.Scene(sc.name, sc.spec, sc.camera, sample_settings(s.confidence, 0.5, 16, 1000)),
              "max_samples": scenes.Scene(sc.name, sc.spec, sc.camera, sample_settings(s.confidence, 0.5, 32, 999)),
              "width": scenes.cornell_box(width=48), "camera": moved}
    for field, other in others.items():
        with pytest.raises(checkpoint.CheckpointError) as e:
            g.AdaptiveRenderer.resume(other, path)
        assert field in str(e.value)
    with pytest.raises(checkpoint.CheckpointError) as e:
        g.AdaptiveRenderer.resume(sc, path, seed=4)
    assert "seed" in str(e.value)
    with pytest.raises(checkpoint.CheckpointError):
        g.ProgressiveRenderer.resume(sc, path)  # the fixed-spp renderer cannot resume it


# ------------------------------------------------------------------ 7. the stateless primitive
def test_stateless_primitive_with_caller_blobs():
    """Two ranks rendered one after the other through Renderer.render_rounds_async, each on its
    own caller-owned blob, in passes of 2 rounds and the rest; the last pass gets output buffers
    it has never seen and must fill them whole (stopped pixels resolve from their stored sums)."""
    import torch
    sc = _scene("cornell_box", 56)
    full, full8, fc = _reference("cornell_box", 3, 56)
    R, world, tile = _rounds_of(sc), 2, 16
    dev = torch.device("cuda", 0)
    cam = g.camera(sc.camera)
    cap0 = N.lib.gs_partition_capacity(C.byref(cam), C.byref(N.gs_partition(0, world, tile, tile)))
    gathered = torch.full((world * cap0 * 3,), float("nan"), dtype=torch.float32, device=dev)
    gathered8 = torch.full((world * cap0 * 3,), 7, dtype=torch.uint8, device=dev)
    counters = torch.zeros(16, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    total = 0
    for r in range(world):
        rr = g.Renderer(sc, rank=r, world_size=world, tile=tile)
        nbytes = rr.round_state_bytes()
        blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        first = torch.zeros(rr.capacity * 3, dtype=torch.float32, device=dev)
        samples = torch.zeros(rr.capacity, dtype=torch.int32, device=dev)
        err = torch.zeros(rr.capacity, dtype=torch.float32, device=dev)
        rr.render_rounds_async(0, 2, blob.data_ptr(), nbytes, d_rgb=first.data_ptr(), d_counters=counters.data_ptr(),
                               stream=stream, seed=3)
        rr.render_rounds_async(2, R - 2, blob.data_ptr(), nbytes, d_rgb=gathered.data_ptr() + r * cap0 * 12,
                               d_rgb8=gathered8.data_ptr() + r * cap0 * 3, d_samples=samples.data_ptr(),
                               d_rel_error=err.data_ptr(), d_counters=counters.data_ptr(), stream=stream, seed=3)
        torch.cuda.synchronize()
        total += int(samples.cpu().numpy().astype(np.int64).sum())
        rr.close()
    frame = torch.zeros(cam.image_height * cam.image_width * 3, dtype=torch.float32, device=dev)
    frame8 = torch.zeros(cam.image_height * cam.image_width * 3, dtype=torch.uint8, device=dev)
    rr = g.Renderer(sc, rank=0, world_size=world, tile=tile)
    rr.unpack_async(gathered.data_ptr(), frame.data_ptr(), world, stream)
    rr.unpack_u8_async(gathered8.data_ptr(), frame8.data_ptr(), world, stream)
    torch.cuda.synchronize()
    rr.close()
    c = counters.cpu().numpy()
    assert np.array_equal(frame.view(cam.image_height, cam.image_width, 3).cpu().numpy(), full)
    assert np.array_equal(frame8.view(cam.image_height, cam.image_width, 3).cpu().numpy(), full8)
    assert {n: int(c[i]) for i, n in enumerate(N.COUNTER_NAMES)} == fc
    assert total == fc["paths"]


# ------------------------------------------------------------------ 8. exclusion
def test_open_adaptation_and_accumulation_exclude_other_frames():
    sc = _scene("cornell_box", 56)
    mr = g.MultiRenderer(sc, num_gpus=1)
    h, cam, ss = mr.handle, mr.cam, mr.settings
    try:
        assert N.lib.gs_multi_adapt_pass(h, 1, None, None) == N.GS_ERR_ARG  # none open
        assert N.lib.gs_multi_adapt_end(h) == N.GS_ERR_ARG
        N.check(N.lib.gs_multi_adapt_begin(h, C.byref(cam), C.byref(ss), 3))
        st = N.gs_stats()
        assert N.lib.gs_multi_render(h, C.byref(cam), C.byref(ss), 3, None, C.byref(st)) == N.GS_ERR_ARG
        assert b"adaptation is open" in N.lib.gs_last_error()
        assert N.lib.gs_multi_accum_begin(h, C.byref(cam), 3, 0) == N.GS_ERR_ARG
        assert b"adaptation is open" in N.lib.gs_last_error()
        assert N.lib.gs_multi_adapt_begin(h, C.byref(cam), C.byref(ss), 3) == N.GS_ERR_ARG
        N.check(N.lib.gs_multi_adapt_pass(h, 1, None, C.byref(st)))
        N.check(N.lib.gs_multi_adapt_end(h))
        full = mr.render(seed=3, rgb=True)  # works again
        assert np.array_equal(full["rgb"], _reference("cornell_box", 3, 56)[0])
        N.check(N.lib.gs_multi_accum_begin(h, C.byref(cam), 3, 0))
        assert N.lib.gs_multi_adapt_begin(h, C.byref(cam), C.byref(ss), 3) == N.GS_ERR_ARG
        assert b"accumulation is open" in N.lib.gs_last_error()
        N.check(N.lib.gs_multi_accum_end(h))
        N.check(N.lib.gs_multi_adapt_begin(h, C.byref(cam), C.byref(ss), 3))  # destroy frees an open one
    finally:
        mr.close()
