"""Progressive rendering on the device: passes over device-resident f64 sums.

The contract (include/grayshift_gpu.h, DESIGN.md "Progressive passes"): passes of n_1, n_2, ...
samples give the f32 frame, the rgb8 frame, the sums and the cumulative counters of ONE render
of their total with the same seed and chunk, bit for bit -- for any split into passes, any rank
count, and across a checkpoint.  Checked here with c = 4 and N = 32 samples on one scene per
kernel family that sets a work item's first sample, against the one-shot render (gs_render
under set_tuning(0, 0, 0, 4): N / c = 8 <= 64 and N > c, so its coarse chunk stays 4) and against
the CPU oracle (per-channel |delta| < 1e-3, counters as tests/test_gpu_parity.py).

Frames are 64-160 px wide: partial tiles, padding slots and two or more tile slots all occur.
"""
import ctypes as C
import math

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import checkpoint, scenes
from grayshift_amd.scene import fixed_spp
import oracle

from tests.test_gpu_composition import _nested_scene

pytestmark = pytest.mark.gpu
TOL = 1e-3  # per-channel absolute, the project's own (tests/test_gpu_parity.py)
CHUNK, TOTAL, SEED = 4, 32, 5
PLANS = [(8, 8, 8, 8), (16, 16), (4, 28), (32,)]


def maxdiff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


def counters_match(gpu, ref, rel=1e-4):
    """tests/test_gpu_parity.py's rule: paths and pixels exactly; traversal work within `rel`
    (the device's OCML trigonometry can differ from glibc's by an ulp, and a grazing ray then
    takes another route through the BVH to the same hit)."""
    if gpu["paths"] != ref["paths"] or gpu["pixels"] != ref["pixels"]:
        return False
    for k, v in ref.items():
        if abs(gpu[k] - v) > rel * max(v, 1) + 2:
            return False
    return True


class _same_device:
    """gs_debug_set_multi_same_device: N frame-context ranks on the one device (test hook)."""
    def __enter__(self):
        N.check(N.lib.gs_debug_set_multi_same_device(1))

    def __exit__(self, *a):
        N.check(N.lib.gs_debug_set_multi_same_device(0))


class _guided_tail:
    """gs_debug_set_guided_tail(1, pct): force a tail of 1-sample items (scheduling only)."""
    def __init__(self, pct):
        self.pct = pct

    def __enter__(self):
        if self.pct:
            N.check(N.lib.gs_debug_set_guided_tail(1, self.pct))

    def __exit__(self, *a):
        N.check(N.lib.gs_debug_set_guided_tail(0, 0))


def _composition():
    """A medium under a chain inside a BVH under a chain: the general kernel."""
    def inner(b):
        m = b.lambertian((0.9, 0.5, 0.1))
        med = b.medium(b.cube((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m), 1.2, b.isotropic((0.8, 0.8, 0.8)))
        return [b.translate(b.rotate_y(med, 15.0), (0.4, 0.0, 0.2))]
    return _nested_scene(inner, width=72, spp=TOTAL)


# name -> (scene at fixed_spp(32), the guided tail's forced percentage or 0)
SCENES = {
    "C4": (lambda: scenes.config("C4", width=96, spp=TOTAL), 0),                # the plain sphere kernel
    "C1_tail": (lambda: scenes.config("C1", width=160, spp=TOTAL), 10),         # coarse and fine regions of `partial`
    "cornell_smoke": (lambda: scenes.cornell_smoke(width=64, settings=fixed_spp(TOTAL)), 0),  # media
    "final_scene": (lambda: scenes.final_scene(width=64, boxes_per_side=4, n_balls=40,
                                               settings=fixed_spp(TOTAL)), 0),  # nested BVHs
    "composition": (_composition, 0),                                           # the general kernel
}


def _run_passes(sc, passes, tail=0, **kw):
    """-> dict(rgb, rgb8, sums, info) after the passes (outputs taken from the last); **kw: the
    context's (devices, tile, plan)."""
    with _guided_tail(tail):
        p = g.ProgressiveRenderer(sc, seed=SEED, chunk=CHUNK, **kw)
        try:
            for n in passes[:-1]:
                p.render_pass(n, rgb=False)  # (the frame stays on the device)
            res = p.render_pass(passes[-1], rgb=True, rgb8=True)
            return {"rgb": res["rgb"], "rgb8": res["rgb8"], "sums": p.sums(), "info": p.info(),
                    "feat": p.scene_info()["feat"]}
        finally:
            p.close()


_CACHE = {}


def _case(name):
    """The scene, its one-shot render and its (8, 8, 8, 8) passes on one rank, computed once and
    shared (never modified) by the tests below."""
    if name not in _CACHE:
        build, tail = SCENES[name]
        sc = build()
        g.set_tuning(0, 0, 0, CHUNK)
        try:
            with _guided_tail(tail):
                one, oc = g.render(sc, seed=SEED)
                one8 = g.render_multi(sc, num_gpus=1, seed=SEED, rgb=False, rgb8=True)["rgb8"]
        finally:
            g.set_tuning(0, 0, 0, -1)
        _CACHE[name] = {"scene": sc, "tail": tail, "one": one, "one8": one8, "one_counters": oc,
                        "passes": _run_passes(sc, PLANS[0], tail)}
    return _CACHE[name]


def _same_bits(a, b):
    return (np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(a["rgb8"], b["rgb8"]) and
            a["sums"].tobytes() == b["sums"].tobytes() and a["info"]["counters"] == b["info"]["counters"] and
            a["info"]["samples"] == b["info"]["samples"])


# ------------------------------------------------------------ 1. passes == the one-shot render
@pytest.mark.parametrize("name", list(SCENES))
def test_passes_equal_the_one_shot_render(name):
    c = _case(name)
    base = c["passes"]
    assert base["info"]["samples"] == TOTAL and base["info"]["passes"] == len(PLANS[0])
    assert base["info"]["chunk"] == CHUNK and base["info"]["seed"] == SEED
    for plan in PLANS[1:]:
        got = _run_passes(c["scene"], plan, c["tail"])
        assert got["info"]["passes"] == len(plan)
        assert _same_bits(got, base), plan
    assert np.array_equal(base["rgb"], c["one"])
    assert np.array_equal(base["rgb8"], c["one8"])
    assert base["info"]["counters"] == c["one_counters"]
    # the sums are the frame's: colour = sums / N, the division the resolve takes
    assert np.array_equal((base["sums"] / float(TOTAL)).astype(np.float32), c["one"])
    if name == "composition":
        assert base["feat"] & 512  # GS_FEAT_GENERAL
    if name == "cornell_smoke":
        assert base["info"]["counters"]["medium_tests"] > 0


# ------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("name", list(SCENES))
def test_last_pass_matches_the_oracle(name):
    c = _case(name)
    ref, rc = oracle.render(c["scene"], seed=SEED)
    assert maxdiff(c["passes"]["rgb"], ref) < TOL
    assert counters_match(c["passes"]["info"]["counters"], rc)


# ------------------------------------------------------------ 3. device count
def test_three_ranks_give_one_ranks_bits():
    """3 ranks on device 0 (same-device hook), a planned partition of 32-px tiles: 6 tiles of
    the 96 x 54 frame, partial ones among them."""
    c = _case("C4")
    with _same_device():
        got = _run_passes(c["scene"], PLANS[0], devices=[0] * 3, tile=32, plan=True)
    assert _same_bits(got, c["passes"])
    with _same_device():  # round-robin, and more ranks than 64-px tiles: a rank with nothing to render
        got = _run_passes(c["scene"], (16, 16), devices=[0] * 3, tile=64, plan=False)
    assert _same_bits(got, c["passes"])


# ------------------------------------------------------------ 4. resume
@pytest.mark.parametrize("first,second", [(1, 2), (2, 1)])
def test_resume_on_another_rank_count(first, second, tmp_path):
    """2 passes, save, close; resume on a context of another rank count; 2 more passes: the
    frame, the sums and info() are those of 4 uninterrupted passes."""
    c = _case("C4")
    sc = c["scene"]
    path = str(tmp_path / "frame.npz")

    def ctx(n, **kw):
        return dict(devices=[0] * n, tile=32, plan=True, **kw)

    with _same_device():
        p = g.ProgressiveRenderer(sc, seed=SEED, chunk=CHUNK, **ctx(first))
        try:
            p.render_pass(8, rgb=False)
            p.render_pass(8, rgb=False)
            p.save(path)
        finally:
            p.close()
        _, meta = checkpoint.read_checkpoint(path)
        assert meta["samples"] == 16 and meta["passes"] == 2 and meta["camera"] == bytes(g.camera(sc.camera))
        q = g.ProgressiveRenderer.resume(sc, path, **ctx(second))
        try:
            assert q.samples == 16 and q.info()["passes"] == 2 and len(q.devices) == second
            q.render_pass(8, rgb=False)
            res = q.render_pass(8, rgb=True, rgb8=True)
            got = {"rgb": res["rgb"], "rgb8": res["rgb8"], "sums": q.sums(), "info": q.info()}
        finally:
            q.close()
        # 4 uninterrupted passes on the resumed context's rank count: info() and all, bit for bit
        whole = _run_passes(sc, PLANS[0], **ctx(second))
        # a checkpoint of another seed or chunk is rejected
        with pytest.raises(checkpoint.CheckpointError):
            g.ProgressiveRenderer.resume(sc, path, seed=SEED + 1, **ctx(1))
        with pytest.raises(checkpoint.CheckpointError):
            g.ProgressiveRenderer.resume(sc, path, chunk=8, **ctx(1))
        with pytest.raises(checkpoint.CheckpointError):
            g.ProgressiveRenderer.resume(scenes.config("C4", width=100, spp=TOTAL), path, **ctx(1))
    assert _same_bits(got, whole) and got["info"] == whole["info"]
    assert _same_bits(got, c["passes"])  # ... and the one-rank frame's bits


# ------------------------------------------------------------ 5. last_delta
def test_last_delta_is_the_mean_change_and_deterministic():
    c = _case("C4")
    sc = c["scene"]
    W, H = sc.width, sc.height

    def run():
        p = g.ProgressiveRenderer(sc, seed=SEED, chunk=CHUNK)
        try:
            out = []
            before, n0 = np.zeros((H, W, 3)), 0
            for n in (8, 4, 12):
                info = p.render_pass(n, rgb=False)["info"]
                after = p.sums()
                old = before / float(n0) if n0 else np.zeros_like(before)
                terms = np.abs(after / float(n0 + n) - old)
                out.append((info["last_delta"], math.fsum(terms.ravel().tolist()) / (W * H * 3.0)))
                before, n0 = after, n0 + n
            return out
        finally:
            p.close()

    a, b = run(), run()
    assert [x[0] for x in a] == [x[0] for x in b]  # identical run to run
    for got, want in a:
        print("last_delta", got, "numpy", want, "rel", abs(got - want) / want)
        assert want > 0.0 and abs(got - want) / want <= W * H * 3 * 2.0 ** -52
    assert a[0][0] > a[1][0]  # (the first pass's change is the frame itself)


# ------------------------------------------------------------ 6. the tile primitive
def test_tile_primitive_on_two_ranks_equals_the_context():
    c = _case("C4")
    sc = c["scene"]
    want = _run_passes(sc, (8, 8))
    rs = [g.Renderer(sc, rank=k, world_size=2, tile=32) for k in range(2)]
    bufs = []

    def alloc(nbytes, zero=True):
        d = C.c_void_p()
        N.check(N.lib.gs_device_alloc(nbytes, C.byref(d)))
        bufs.append(d)
        if zero:
            z = np.zeros(nbytes, dtype=np.uint8)
            N.check(N.lib.gs_device_upload(d, z.ctypes.data, nbytes))
        return d.value

    try:
        cap = rs[0].capacity  # (rank 0 holds the most tiles)
        assert rs[1].capacity <= cap
        gathered = alloc(2 * cap * 12)
        frame = alloc(sc.width * sc.height * 12)
        total = {k: 0 for k in N.COUNTER_NAMES}
        for k, r in enumerate(rs):
            sums, cnt = alloc(r.capacity * 24), alloc(C.sizeof(N.gs_counters))
            for base in (0, 8):
                r.render_pass_async(8, base, sums, d_rgb=gathered + k * cap * 12, d_counters=cnt, seed=SEED, chunk=CHUNK)
            got = N.gs_counters()
            N.check(N.lib.gs_device_download(C.byref(got), C.c_void_p(cnt), C.sizeof(N.gs_counters)))
            for name, v in got.as_dict().items():
                total[name] += v
        rs[0].unpack_async(gathered, frame, 2)
        out = np.zeros((sc.height, sc.width, 3), dtype=np.float32)
        N.check(N.lib.gs_device_download(out.ctypes.data, C.c_void_p(frame), out.nbytes))
    finally:
        for d in bufs:
            N.lib.gs_device_free(d)
        for r in rs:
            r.close()
    assert np.array_equal(out, want["rgb"])
    # the kernel counts `pixels` at chunk 0 of every pass; everything else adds up
    assert total["pixels"] == 2 * sc.width * sc.height
    total["pixels"] //= 2
    assert total == want["info"]["counters"]


# ------------------------------------------------------------ 7. PPM
def test_pass_ppm_is_the_oracles_text():
    c = _case("C4")
    p = g.ProgressiveRenderer(c["scene"], seed=SEED, chunk=CHUNK)
    try:
        p.render_pass(16, rgb=False)
        res = p.render_pass(16, rgb=False, rgb8=True, ppm=True)
    finally:
        p.close()
    assert np.array_equal(res["rgb8"], c["passes"]["rgb8"])
    assert res["ppm"] == oracle.ppm_text(res["rgb8"])


# ------------------------------------------------------------ the frame context's rules
def test_open_and_closed_accumulation_rules():
    c = _case("C4")
    m = g.MultiRenderer(c["scene"], num_gpus=1)
    try:
        st = N.gs_stats()
        info = N.gs_accum_info()
        assert N.lib.gs_multi_accum_pass(m.handle, 8, None, C.byref(st)) == N.GS_ERR_ARG  # never opened
        assert N.lib.gs_multi_accum_info(m.handle, C.byref(info)) == N.GS_ERR_ARG
        assert N.lib.gs_multi_accum_end(m.handle) == N.GS_ERR_ARG
        N.check(N.lib.gs_multi_accum_begin(m.handle, C.byref(m.cam), SEED, CHUNK))
        assert N.lib.gs_multi_accum_begin(m.handle, C.byref(m.cam), SEED, CHUNK) == N.GS_ERR_ARG
        # one-shot frames are refused while the packed sums live
        assert N.lib.gs_multi_render(m.handle, C.byref(m.cam), C.byref(m.settings), SEED, None,
                                     C.byref(st)) == N.GS_ERR_ARG
        assert b"accumulation" in N.lib.gs_last_error()
        for bad in (0, 6, 65 * CHUNK):
            assert N.lib.gs_multi_accum_pass(m.handle, bad, None, C.byref(st)) == N.GS_ERR_ARG
        N.check(N.lib.gs_multi_accum_pass(m.handle, 8, None, C.byref(st)))
        assert st.counters.paths == 8 * m.width * m.height  # stats: this pass alone
        N.check(N.lib.gs_multi_accum_pass(m.handle, 4, None, C.byref(st)))
        assert st.counters.paths == 4 * m.width * m.height
        N.check(N.lib.gs_multi_accum_info(m.handle, C.byref(info)))
        assert info.samples == 12 and info.passes == 2 and info.counters.pixels == m.width * m.height
        N.check(N.lib.gs_multi_accum_end(m.handle))
        assert N.lib.gs_multi_accum_pass(m.handle, 8, None, C.byref(st)) == N.GS_ERR_ARG  # closed
        res = m.render(seed=SEED, rgb=True)  # the context renders one-shot frames again
        assert res["rgb"].shape == (m.height, m.width, 3)
    finally:
        m.close()


def test_render_until_stops_at_the_first_bound():
    c = _case("C4")
    seen = []
    with g.ProgressiveRenderer(c["scene"], seed=SEED, chunk=CHUNK) as p:
        info, frame = p.render_until(total_samples=TOTAL, pass_samples=7, on_pass=lambda i, f: seen.append(i["samples"]))
        assert seen == [8, 16, 24, 32] and info["samples"] == TOTAL  # (7 rounds up to 2 chunks)
        assert np.array_equal(frame, c["one"])
        info, frame = p.render_until(total_samples=TOTAL)  # already there: no pass
        assert frame is None and info["samples"] == TOTAL
        info, _ = p.render_until(min_delta=1e9, pass_samples=4)  # any change is below it: one pass
        assert info["samples"] == TOTAL + 4
        info, _ = p.render_until(seconds=0.0, pass_samples=4)  # a time budget still renders one pass
        assert info["samples"] == TOTAL + 8
        with pytest.raises(ValueError):
            p.render_until()
        with pytest.raises(ValueError):
            p.render_until(total_samples=TOTAL + 9)
