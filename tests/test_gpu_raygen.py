"""Generated radiance queries on the device (gs_query_radiance_gen, gs_query_radiance_gen_async;
csrc/device/raygen.hip): a ray drawn for every sample from the sample's own stream, then ray_color.

1. The generators against tests/raygen_cases.py's numpy restatement: CAMERA (without and with the
   defocus disk) and ORTHO use no libm and are equal to the bit; PANORAMA and HEMISPHERE are equal in
   streams, origins and times and within 1e-13 in a direction's component.
2. The tracing, device against device and exact: the emitted rays and streams through
   gs_query_radiance at one sample each, folded in the call's chunks.
3. The render: a frame of gs_render is the CAMERA generator's sum / spp, with and without defocus.
4. The oracle directly: the fold of the restated rays (tests/radiance_cases.py).
5. A known answer: a panorama under an HDRI of its own size reads the sky map back.
6. Progressive ranges of samples; 7. the edges."""
import ctypes as C
import time

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import query as GQ
from grayshift_amd import scenes
from grayshift_amd.scene import fixed_spp

import oracle

from tests import parity
from tests import query_cases as Q
from tests import radiance_cases as R
from tests import raygen_cases as G
from tests.test_gpu_query import DevBuf, _bits

pytestmark = pytest.mark.gpu
T0 = time.time()
DIR_TOL = 1e-13  # PANORAMA, HEMISPHERE: a direction's component against glibc's sines and cosines


@pytest.fixture(scope="module")
def devs(built):
    made = {}

    def get(name):
        if name not in made:
            rq = g.RayQuery(R.scene(name).spec)
            info = N.gs_scene_info()
            N.check(N.lib.gs_device_scene_info(rq.dev, C.byref(info)))
            rq.feat = info.feat
            made[name] = rq
        return made[name]
    yield get
    for rq in made.values():
        rq.close()
    print("tests/test_gpu_raygen.py: %.1f s from import to teardown" % (time.time() - T0))


def _same(a, b, keys=("sum", "rays", "state")):
    for k in keys:
        x, y = (_bits(a[k]), _bits(b[k])) if k == "sum" else (a[k], b[k])
        assert np.array_equal(x, y), k


# ----------------------------------------------------------------------------- 1. generation
@pytest.mark.parametrize("kind", G.KINDS)
def test_generated_rays_and_streams_are_the_restatements(kind, devs):
    """Measured on MI355X: the largest direction difference against glibc is 2.22e-16
    for PANORAMA and for HEMISPHERE, 0 for the kinds without libm."""
    rq = devs("spheres_sky")
    worst = 0.0
    for w, h in G.IMAGES:
        for (samples, chunk), first in zip(G.SAMPLES, (0, 0, 7)):
            want = G.restated(kind, "spheres_sky", w, h, samples, G.SEED, first)
            d = rq.radiance_gen(G.gen(kind, "spheres_sky", w, h), samples, max_depth=2, seed=G.SEED, chunk=chunk,
                                first_sample=first, emit=True)
            assert d["gen_rays"].shape == (w * h * samples, 9) and d["sum"].shape == G.gen(kind, "spheres_sky", w, h).shape + (3,)
            assert np.array_equal(d["gen_states"], want["states"])
            assert (d["gen_rays"][:, 7] == 0.001).all() and (d["gen_rays"][:, 8] == Q.DMAX).all()
            for col in (0, 1, 2, 6):  # origins and times: no libm in any kind
                assert np.array_equal(d["gen_rays"][:, col].view(np.uint64), want["rays"][:, col].view(np.uint64)), col
            delta = float(np.abs(d["gen_rays"][:, 3:6] - want["rays"][:, 3:6]).max())
            worst = max(worst, delta)
            if kind in G.LIBM_FREE_KINDS:
                assert np.array_equal(d["gen_rays"].view(np.uint64), want["rays"].view(np.uint64))
            else:
                assert delta <= DIR_TOL, delta
    print("%s: largest |direction difference| against the restatement %.3g" % (kind, worst))
    if kind == "camera_defocus":
        assert G.restated(kind, "spheres_sky", 17, 16, 33, G.SEED, 7)["retries"] > 0


# ----------------------------------------------------------------------------- 2. tracing, device against device
@pytest.mark.parametrize("name", G.SCENES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_generated_paths_are_radiance_queries_of_the_emitted_rays(kind, name, devs):
    rq = devs(name)
    assert rq.feat & (1 | 2 | 512) == R.FEAT_BITS[name] or (R.FEAT_BITS[name] == 512 and rq.feat & 512)
    for w, h in G.IMAGES:
        for samples, chunk in G.SAMPLES:
            n = w * h
            d = rq.radiance_gen(G.gen(kind, name, w, h), samples, max_depth=12, seed=G.SEED, chunk=chunk, counters=True,
                                emit=True)
            one = rq.radiance(d["gen_rays"], samples=1, max_depth=12, seed=99, states=d["gen_states"], counters=True)
            assert np.array_equal(_bits(d["sum"].reshape(n, 3)), _bits(G.fold_chunks(one["sum"], samples, chunk)))
            assert np.array_equal(_bits(d["rgb"]), _bits(d["sum"] / float(samples)))
            assert np.array_equal(d["rays"].reshape(n), one["rays"].reshape(n, samples).sum(axis=1))
            assert np.array_equal(d["state"].reshape(n), one["state"].reshape(n, samples)[:, -1])
            assert d["counters"] == one["counters"], (d["counters"], one["counters"])
            assert d["counters"]["paths"] == n * samples and d["counters"]["rays"] == int(d["rays"].sum())
            assert (d["sum"] != 0.0).any() and (d["counters"]["hits"] > 0 or n * samples < 1000)
            if chunk == 16:  # chunk 0 means 16
                z = rq.radiance_gen(G.gen(kind, name, w, h), samples, max_depth=12, seed=G.SEED, chunk=0)
                _same(z, d)


# ----------------------------------------------------------------------------- 3. the render
FRAME = {"mixed_sky": ((0.0, 2.0, 26.0), 40.0), "textured_hdri": ((2.0, 3.0, 24.0), 45.0)}
W, SPP, FRAME_SEED, FRAME_DEPTH = 32, 8, 5, 12


@pytest.mark.parametrize("defocus", [0.0, G.DEFOCUS])
@pytest.mark.parametrize("name", sorted(FRAME))
def test_a_render_is_the_camera_generators_mean(name, defocus, devs):
    """Device against device, exact: the generator draws the megakernel's camera rays, the defocus
    disk's rejection loop included, and the query walks and shades the megakernel's paths."""
    assert G.VIEW[name] == FRAME[name]
    cs, cam = G.camera(name, W, W, defocus, FRAME_DEPTH)
    sc = scenes.Scene("raygen_" + name, R.scene(name).spec, cs, fixed_spp(SPP))
    g.set_tuning(0, 0, 0, SPP)
    try:
        frame, counters = g.render(sc, seed=FRAME_SEED)
    finally:
        g.set_tuning(0, 0, 0, -1)
    d = devs(name).radiance_gen(GQ.RayGen.camera(cam), SPP, max_depth=FRAME_DEPTH, seed=FRAME_SEED, chunk=SPP, counters=True)
    mine = (d["sum"] / float(SPP)).astype(np.float32)
    assert (frame != 0.0).any() and mine.shape == frame.shape == (W, W, 3)
    assert np.array_equal(mine.view(np.uint32), np.ascontiguousarray(frame).view(np.uint32))
    got = d["counters"]
    for k, v in counters.items():
        if k != "pixels":
            assert got[k] == v, (k, got[k], v)
    assert got["pixels"] == 0 and counters["pixels"] == W * W


# ----------------------------------------------------------------------------- 4. the oracle, directly
@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_generated_radiance_matches_the_fold_of_the_restated_rays(kind, depth, devs):
    """Judged as tests/test_gpu_radiance.py::test_radiance_matches_the_fold: items that differ in the
    colour's bits, the ray count or the stream are at most parity.cap_for(items), and such an item
    still lies within parity.MAX_ABS per sample and channel."""
    name, (w, h), (samples, chunk) = "media_sky", G.IMAGES[1], G.SAMPLES[1]
    n = w * h
    want = G.restated(kind, name, w, h, samples)
    a = R.ray_color_fold(R.scene(name).twin, want["rays"], want["states"], depth)
    ref = {"sum": G.fold_chunks(a["rgb"], samples, chunk), "rays": a["rays"].reshape(n, samples).sum(axis=1),
           "state": a["state"].reshape(n, samples)[:, -1]}
    d = devs(name).radiance_gen(G.gen(kind, name, w, h), samples, max_depth=depth, seed=G.SEED, chunk=chunk)
    got = {"sum": d["sum"].reshape(n, 3), "rays": d["rays"].reshape(n), "state": d["state"].reshape(n)}
    off = (_bits(got["sum"]) != _bits(ref["sum"])).any(axis=1) | (got["rays"] != ref["rays"]) | (got["state"] != ref["state"])
    cap = parity.cap_for(n)
    worst = float(np.abs(got["sum"] - ref["sum"]).max())
    print("%s depth %d: %d items of %d samples, %d differ (cap %d), max |delta| %.3g" % (
        kind, depth, n, samples, int(off.sum()), cap, worst))
    assert np.isfinite(got["sum"]).all() and (got["sum"] != 0.0).any()
    assert (a["end"] == R.SKY).any() and ((a["rays"] > 1).any() or depth == 1)
    assert off.sum() <= cap, np.flatnonzero(off)[:8]
    assert worst <= parity.MAX_ABS * samples


# ----------------------------------------------------------------------------- 5. a known answer
def test_a_jittered_panorama_under_its_own_sky_map_reads_the_map_back(built):
    """One small sphere under the unrotated 64 x 32 HDRI, a 64 x 32 panorama from outside it at 4
    samples: a pixel whose four rays miss (the oracle's world.hit on the restated rays) sees its own
    texel four times, and sum / 4 is that texel exactly."""
    b = g.SceneBuilder()
    b.add(b.sphere((0.0, 0.0, 0.0), 0.5, b.lambertian((0.5, 0.5, 0.5))))
    m = R.hdri_map()
    b.background_hdri(m, (0.0, 0.0, 0.0))
    spec = b.build()
    rg = GQ.RayGen.panorama((0.0, 3.0, 0.0), R.HDRI_W, R.HDRI_H)
    want = G.restate(rg, 4, G.SEED)
    w = oracle.World(spec)
    try:
        nr = len(want["rays"])
        hit = w.hit(np.zeros(nr, dtype=np.int32), want["rays"][:, 0:7], 0.001, Q.DMAX, want["states"])["hit"]
    finally:
        w.close()
    clear = ~hit.reshape(R.HDRI_H, R.HDRI_W, 4).any(axis=2)
    print("known answer: %d of %d pixels clear of the sphere" % (int(clear.sum()), clear.size))
    assert clear.mean() >= 0.9 and not clear.all()
    with g.RayQuery(spec) as rq:
        d = rq.radiance_gen(rg, 4, max_depth=50, seed=G.SEED, counters=True)
    assert np.array_equal((d["sum"] / 4.0)[clear], m.astype(np.float64)[clear])
    assert (d["rays"][clear] == 4).all() and (d["rays"][~clear] > 4).all()
    assert d["counters"]["hdri_texels"] >= 4 * int(clear.sum())


# ----------------------------------------------------------------------------- 6. progressive
@pytest.mark.parametrize("kind", ["camera_defocus", "hemisphere"])
def test_ranges_of_samples_add_up_to_the_whole(kind, devs):
    """Samples [0, 8) at chunk 4 in one call are (0 + A) + B to the bit, A and B two calls of 4 samples
    at first_sample 0 and 4."""
    name, (w, h) = "media_sky", G.IMAGES[1]
    rq, rg = devs(name), G.gen(kind, name, w, h)
    whole = rq.radiance_gen(rg, 8, seed=G.SEED, chunk=4, counters=True)
    a = rq.radiance_gen(rg, 4, seed=G.SEED, chunk=4, first_sample=0, counters=True)
    b = rq.radiance_gen(rg, 4, seed=G.SEED, chunk=4, first_sample=4, counters=True)
    assert np.array_equal(_bits(whole["sum"]), _bits((0.0 + a["sum"]) + b["sum"]))
    assert np.array_equal(whole["rays"], a["rays"] + b["rays"]) and np.array_equal(whole["state"], b["state"])
    assert whole["counters"] == {k: a["counters"][k] + b["counters"][k] for k in whole["counters"]}
    assert (a["sum"] != b["sum"]).any() and not np.array_equal(a["state"], b["state"])
    hi = rq.radiance_gen(rg, 4, seed=G.SEED, chunk=4, first_sample=0xFFFFFFFC)  # the last four samples there are
    assert np.isfinite(hi["sum"]).all() and (hi["state"] != a["state"]).any()


# ----------------------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_hemisphere_batch_edges_write_nothing_past_n(n, devs):
    """The async form on caller buffers, over-allocated and poisoned, three chunks per point: the first
    n records, n * samples rays and streams equal the synchronous form's and nothing after them is
    touched, nor the scratch past its 3 n records; the totals are added to the caller's counters."""
    name, samples, chunk, chunks = "media_sky", 5, 2, 3
    rq, rg = devs(name), G.gen("hemisphere", name, n, 1)
    pad, poison = 70, 0xA5
    need = N.lib.gs_query_radiance_scratch_bytes(n, samples, chunk)
    assert need == n * chunks * 40
    d_p, d_o, d_s, d_c = DevBuf(n * 72), DevBuf((n + pad) * 40, poison), DevBuf(need + pad * 40, poison), DevBuf(128)
    d_r, d_t = DevBuf((n * samples + pad) * 72, poison), DevBuf((n * samples + pad) * 8, poison)
    try:
        d_p.put(rg.points)
        d_c.put(np.full(16, 1000, dtype=np.uint64))
        N.check(N.lib.gs_query_radiance_gen_async(rq.dev, C.addressof(rg.raw), d_p.p, samples, 0, chunk, 50, G.SEED, d_o.p,
                                                  d_c.p, d_r.p, d_t.p, d_s.p, need, None))
        ob, sb, cb = d_o.get(), d_s.get(), d_c.get().view(np.uint64)  # (the download synchronises)
        rb, tb = d_r.get(), d_t.get()
    finally:
        for buf in (d_p, d_o, d_s, d_c, d_r, d_t):
            buf.free()
    assert (ob[n * 40:] == poison).all() and (sb[need:] == poison).all()
    assert (rb[n * samples * 72:] == poison).all() and (tb[n * samples * 8:] == poison).all()
    ref = rq.radiance_gen(rg, samples, max_depth=50, seed=G.SEED, chunk=chunk, counters=True, emit=True)
    out = ob[:n * 40].view(GQ.RADIANCE_DTYPE)
    assert np.array_equal(_bits(out["rgb"]), _bits(ref["sum"].reshape(n, 3)))
    assert np.array_equal(out["rays"], ref["rays"].reshape(n)) and np.array_equal(out["state"], ref["state"].reshape(n))
    assert np.array_equal(rb[:n * samples * 72].view(np.uint64), ref["gen_rays"].view(np.uint64).reshape(-1))
    assert np.array_equal(tb[:n * samples * 8].view(np.uint64), ref["gen_states"])
    cnt = dict(zip(N.COUNTER_NAMES, (int(x) - 1000 for x in cb)))
    assert cnt == ref["counters"] and cnt["paths"] == n * samples and cnt["pixels"] == 0
    assert int(cb[15]) == 1000  # (the reserved word is not a counter)
    part = sb[:need].view(GQ.RADIANCE_DTYPE).reshape(n, chunks)
    assert np.array_equal(part["rays"].sum(axis=1), out["rays"]) and np.array_equal(part["state"][:, -1], out["state"])


@pytest.mark.parametrize("kind", G.KINDS)
def test_depth_zero_draws_nothing_and_traces_nothing(kind, devs):
    name, (w, h), samples = "media_sky", G.IMAGES[1], 5
    z = devs(name).radiance_gen(G.gen(kind, name, w, h), samples, max_depth=0, seed=G.SEED, chunk=2, first_sample=3,
                                counters=True, emit=True)
    assert (_bits(z["sum"]) == 0).all() and (z["rays"] == 0).all()  # +0.0
    last = np.array([oracle.stream_seed(G.SEED, q, 3 + samples - 1) for q in range(w * h)], dtype=np.uint64)
    assert np.array_equal(z["state"].reshape(-1), last)
    assert z["counters"]["paths"] == w * h * samples
    assert all(v == 0 for k, v in z["counters"].items() if k != "paths")
    assert not z["gen_rays"].any() and not z["gen_states"].any()  # nothing is generated


def test_nan_normals_and_empty_rectangles_complete_with_the_restatements_answer(devs):
    name = "media_sky"
    rq = devs(name)
    p, nrm, t = G.hemisphere_points(name, 64)
    nrm = nrm.copy()
    nrm[::3] = np.nan
    nrm[1::9] = 0.0  # (a zero normal: unit() divides by zero)
    nrm[2::9, 1] = np.inf
    flat = GQ.RayGen.ortho((0.0, 6.0, 20.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, -0.2, -1.0), 8, 8)
    for rg in (GQ.RayGen.hemisphere(p, nrm, t), flat):
        want = G.restate(rg, 3, G.SEED)
        d = rq.radiance_gen(rg, 3, max_depth=4, seed=G.SEED, chunk=2, counters=True, emit=True)
        assert np.array_equal(d["gen_states"], want["states"])
        assert np.array_equal(np.isnan(d["gen_rays"]), np.isnan(want["rays"]))
        with np.errstate(invalid="ignore"):
            delta = np.abs(d["gen_rays"] - want["rays"])
        assert np.nanmax(np.where(np.isfinite(delta), delta, 0.0)) <= (DIR_TOL if rg.points is not None else 0.0)
        one = rq.radiance(d["gen_rays"], samples=1, max_depth=4, seed=1, states=d["gen_states"], counters=True)
        n = len(d["gen_rays"]) // 3
        assert np.array_equal(_bits(d["sum"].reshape(n, 3)), _bits(G.fold_chunks(one["sum"], 3, 2)))
        assert np.array_equal(d["rays"].reshape(n), one["rays"].reshape(n, 3).sum(axis=1))
        assert np.array_equal(d["state"].reshape(n), one["state"].reshape(n, 3)[:, -1])
        assert d["counters"] == one["counters"] and (d["rays"] >= 3).all() and (d["rays"] <= 12).all()
    assert np.isnan(want["rays"][:, 3:6]).sum() == 0  # (the rectangle without extent: one finite ray, 64 times over)
    assert len(np.unique(d["gen_rays"][:, 0:6], axis=0)) == 1 and len(np.unique(d["gen_rays"][:, 6])) == 64 * 3


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_the_shade_batch_moves_no_bit(batch, devs):
    name, (w, h) = "media_sky", G.IMAGES[1]
    rq = devs(name)
    want = {k: rq.radiance_gen(G.gen(k, name, w, h), 7, seed=G.SEED, chunk=3, counters=True) for k in ("panorama", "hemisphere")}
    N.check(N.lib.gs_debug_set_radiance_batch(batch))
    try:
        got = {k: rq.radiance_gen(G.gen(k, name, w, h), 7, seed=G.SEED, chunk=3, counters=True) for k in want}
    finally:
        N.check(N.lib.gs_debug_set_radiance_batch(0))
    for k in want:
        _same(got[k], want[k])
        assert got[k]["counters"] == want[k]["counters"]


# ----------------------------------------------------------------------------- Python
def test_multirenderer_query_has_the_generators():
    name = "textured_hdri"
    cs, cam = G.camera(name, 32, 32, G.DEFOCUS, 8)
    sc = scenes.Scene("raygen_textured", R.scene(name).spec, cs, fixed_spp(2))
    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        q = m.query()
        a = q.radiance_gen(GQ.RayGen.camera(cam), 3, max_depth=6, seed=4, chunk=2, counters=True)
        q.close()
    finally:
        m.close()
    with g.RayQuery(R.scene(name).spec) as fresh:
        b = fresh.radiance_gen(g.RayGen.camera(cam), 3, max_depth=6, seed=4, chunk=2, counters=True)
    _same(a, b, ("sum", "rgb", "rays", "state"))
    assert a["counters"] == b["counters"] and a["counters"]["paths"] == 32 * 32 * 3
    assert set(a) == {"sum", "rgb", "rays", "state", "counters"} and a["sum"].shape == (32, 32, 3)
