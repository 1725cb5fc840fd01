"""Radiance queries on the device (gs_query_radiance, gs_query_radiance_async; csrc/device/radiance.hip)
against the reference's Camera::ray_color, which is tests/radiance_cases.py's fold of the oracle's
bounce and background entries on the scene's twin.

Per ray: the f64 colour's bits, the world.hit count and the stream after.  The rays that differ in
any of them are at most parity.cap_for(n, libm_free) -- the project's rule for whole frames, max(1,
ceil(4e-4 n)), and 0 where no libm call lies on the path -- and such a ray still lies within 1e-3
per channel.  A colour through the noise texture is compared at 1e-9 relative.

Then, device against device and exact: the same paths as the megakernel's (a render's frame rebuilt
from radiance queries of its own camera rays), the association of the sample sum, and what must not
matter: a ray's place in its batch, the batch's size, what else runs on the scene."""
import ctypes as C
import time

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import query as GQ
from grayshift_amd import scenes
from grayshift_amd.scene import camera_spec, fixed_spp

import oracle

from tests import parity
from tests import query_cases as Q
from tests import radiance_cases as R
from tests.test_gpu_parity import counters_match
from tests.test_gpu_query import DevBuf, _bits, _last_feat

pytestmark = pytest.mark.gpu
WY_C0 = 0x2d358dccaa6c78a5
M64 = (1 << 64) - 1
T0 = time.time()


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
    print("tests/test_gpu_radiance.py: %.1f s from import to teardown" % (time.time() - T0))


@pytest.fixture(scope="module")
def single(devs):
    """Each lit scene's rays through gs_query_radiance once per depth (one sample, with totals)."""
    made = {}

    def get(name, depth):
        if (name, depth) not in made:
            made[name, depth] = devs(name).radiance(R.rays(name), samples=1, max_depth=depth, seed=R.SEED, counters=True)
        return made[name, depth]
    return get


def _differs(d, a):
    return ((_bits(d["sum"]) != _bits(a["rgb"])).any(axis=1) | (d["rays"] != a["rays"]) | (d["state"] != a["state"]))


# ----------------------------------------------------------------------------- 1. against the fold
@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("name", sorted(R.LIT))
def test_radiance_matches_the_fold(name, depth, devs, single):
    """Measured on MI355X: DESIGN.md §3.7 lists the count of differing rays per scene and depth."""
    a, d, rq = R.answers(name, depth), single(name, depth), devs(name)
    n = len(a["rgb"])
    assert rq.feat & (1 | 2 | 512) == R.FEAT_BITS[name] or (R.FEAT_BITS[name] == 512 and rq.feat & 512)
    assert np.array_equal(_bits(d["rgb"]), _bits(d["sum"]))  # one sample: the mean is the sum
    noise = a["noise"]
    off = _differs(d, a)
    exact_off = off & ~noise
    # a noise colour is compared at 1e-9 relative; its ray count and stream stay exact
    noise_off = noise & ((d["rays"] != a["rays"]) | (d["state"] != a["state"]) |
                         (np.abs(d["sum"] - a["rgb"]) > 1e-9 * np.abs(a["rgb"])).any(axis=1))
    bad = exact_off | noise_off
    cap = parity.cap_for(n, name in R.LIBM_FREE)
    worst = float(np.abs(d["sum"] - a["rgb"]).max())
    print("%s depth %d: %d rays, %d differ (cap %d; %d through noise, %d of them in bits), max |delta| %.3g" % (
        name, depth, n, int(bad.sum()), cap, int(noise.sum()), int((off & noise).sum()), worst))
    assert np.isfinite(d["sum"]).all()
    assert bad.sum() <= cap, np.flatnonzero(bad)[:8]
    assert worst <= parity.MAX_ABS
    got, want = d["counters"], dict(a["counters"], pixels=0)
    assert got["paths"] == n and got["pixels"] == 0
    assert counters_match(got, want), (got, want)
    if not bad.any():
        assert got["rays"] == want["rays"] == int(a["rays"].sum()) and got["hits"] == want["hits"]


# ----------------------------------------------------------------------------- 2. the megakernel's paths
FRAME = {"mixed_sky": ((0.0, 2.0, 26.0), 40.0), "media_sky": ((0.0, 2.0, 26.0), 40.0),
         "general_all_sky": ((0.5, 2.0, 9.0), 40.0), "outer_light_sky": ((0.0, 3.0, 28.0), 40.0),
         "textured_hdri": ((2.0, 3.0, 24.0), 45.0)}
W, SPP, FRAME_SEED, FRAME_DEPTH = 32, 8, 5, 12


def _camera_rays_and_states(cam, seed):
    """Every (pixel, sample)'s get_ray (camera.rs:204-221, no defocus): two offset draws, the
    direction, the time draw -- and the stream after those three draws."""
    Wd, Hd = cam.image_width, cam.image_height
    p0, du, dv, c = (np.array(v[:], dtype=np.float64) for v in (cam.starting_pixel_pos, cam.pixel_delta_u,
                                                                cam.pixel_delta_v, cam.center))
    n = Wd * Hd * SPP
    rays = np.empty((n, 9))
    states = np.empty(n, dtype=np.uint64)
    k = 0
    for pix in range(Wd * Hd):
        pj, pi = divmod(pix, Wd)
        for s in range(SPP):
            st = oracle.stream_seed(seed, pix, s)
            f, _ = oracle.wyrand(st, 3)
            si, sj = float(pi) + (f[0] - 0.5), float(pj) + (f[1] - 0.5)
            ps = (p0 + du * si) + dv * sj
            rays[k, 0:3], rays[k, 3:6], rays[k, 6] = c, ps - c, f[2]
            states[k] = (st + 3 * WY_C0) & M64
            k += 1
    rays[:, 7], rays[:, 8] = 0.001, Q.DMAX
    return rays, states


@pytest.mark.parametrize("name", sorted(FRAME))
def test_a_frame_rebuilt_from_radiance_queries_is_the_renders_frame(name, devs):
    """Device against device, exact: the query walks and shades the very paths the megakernel does."""
    look_from, fov = FRAME[name]
    cs = camera_spec(1.0, W, FRAME_DEPTH, fov, look_from, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 10.0)
    sc = scenes.Scene("radiance_" + name, R.scene(name).spec, cs, fixed_spp(SPP))
    g.set_tuning(0, 0, 0, SPP)
    try:
        frame, counters = g.render(sc, seed=FRAME_SEED)
    finally:
        g.set_tuning(0, 0, 0, -1)
    cam = g.camera(cs)
    rays, states = _camera_rays_and_states(cam, FRAME_SEED)
    d = devs(name).radiance(rays, samples=1, max_depth=FRAME_DEPTH, seed=99, states=states, counters=True)
    col = d["sum"].reshape(-1, SPP, 3)
    chunk = np.zeros((col.shape[0], 3))
    for s in range(SPP):
        chunk = chunk + col[:, s]
    mine = ((0.0 + chunk) / float(SPP)).astype(np.float32).reshape(cam.image_height, cam.image_width, 3)
    assert (frame != 0.0).any()
    assert np.array_equal(mine.view(np.uint32), np.ascontiguousarray(frame).view(np.uint32))
    got = d["counters"]
    for k, v in counters.items():
        if k != "pixels":
            assert got[k] == v, (k, got[k], v)
    assert got["pixels"] == 0 and counters["pixels"] == cam.image_width * cam.image_height


# ----------------------------------------------------------------------------- 3. association
@pytest.mark.parametrize("samples,chunk", [(1, 1), (5, 2), (16, 16), (33, 16), (64, 4)])
def test_samples_are_summed_in_chunks_in_sample_order(samples, chunk, devs):
    name, n = "media_hdri", 150
    rq = devs(name)
    r = np.ascontiguousarray(R.rays(name)[:n])
    s0 = R.seeds(n, samples)
    one = rq.radiance(np.repeat(r, samples, axis=0), samples=1, max_depth=50, seed=3, states=s0)
    col = one["sum"].reshape(n, samples, 3)
    total = np.zeros((n, 3))
    for k0 in range(0, samples, chunk):
        c = np.zeros((n, 3))
        for s in range(k0, min(samples, k0 + chunk)):
            c = c + col[:, s]
        total = total + c
    d = rq.radiance(r, samples=samples, max_depth=50, seed=R.SEED, chunk=chunk, counters=True)
    assert np.array_equal(_bits(d["sum"]), _bits(total))
    assert np.array_equal(_bits(d["rgb"]), _bits(total / float(samples)))
    assert np.array_equal(d["rays"], one["rays"].reshape(n, samples).sum(axis=1))
    assert np.array_equal(d["state"], one["state"].reshape(n, samples)[:, -1])
    assert d["counters"]["paths"] == n * samples and d["counters"]["rays"] == int(d["rays"].sum())
    if chunk == 16:  # chunk 0 means 16
        z = rq.radiance(r, samples=samples, max_depth=50, seed=R.SEED, chunk=0)
        assert np.array_equal(_bits(z["sum"]), _bits(d["sum"])) and np.array_equal(z["state"], d["state"])
    e = rq.radiance(r, samples=samples, max_depth=50, seed=77, chunk=chunk, states=s0)  # (states win over the seed)
    assert np.array_equal(_bits(e["sum"]), _bits(d["sum"])) and np.array_equal(e["state"], d["state"])


# ----------------------------------------------------------------------------- 4. scheduling
def test_a_rays_place_in_its_batch_does_not_matter(devs, single):
    name = "media_hdri"
    rq, whole = devs(name), single(name, 50)
    part = np.ascontiguousarray(R.rays(name)[1000:1257])
    st = R.seeds(257, first=1000)
    alone = rq.radiance(part, samples=1, max_depth=50, seed=1, states=st)
    rev = rq.radiance(np.ascontiguousarray(part[::-1]), samples=1, max_depth=50, seed=2, states=st[::-1].copy())
    for k in ("sum", "rays", "state"):
        assert np.array_equal(_bits(alone[k]) if k == "sum" else alone[k],
                              _bits(whole[k][1000:1257]) if k == "sum" else whole[k][1000:1257]), k
        assert np.array_equal(_bits(alone[k]) if k == "sum" else alone[k],
                              _bits(rev[k][::-1]) if k == "sum" else rev[k][::-1]), k
    assert (alone["state"] != st).any() and (alone["sum"] != 0.0).any()
    # without states the stream is the index's: the same rays at other indices draw differently
    other = rq.radiance(part, samples=1, max_depth=50, seed=R.SEED)
    assert not np.array_equal(other["state"], alone["state"])


@pytest.mark.parametrize("batch", [1, 7, 33, 64])
def test_the_shade_batch_moves_no_bit(batch, devs, single):
    """How many lanes of a wave wait at their walk's end before the wave shades them is scheduling:
    colours, ray counts, streams and totals are those of the default."""
    name = "media_hdri"
    want = single(name, 50)
    N.check(N.lib.gs_debug_set_radiance_batch(batch))
    try:
        d = devs(name).radiance(R.rays(name), samples=1, max_depth=50, seed=R.SEED, counters=True)
        m = devs(name).radiance(R.rays(name)[:300], samples=7, max_depth=50, seed=R.SEED, chunk=3)
    finally:
        N.check(N.lib.gs_debug_set_radiance_batch(0))
    for k in ("sum", "rays", "state"):
        assert np.array_equal(d[k].view(np.uint64), want[k].view(np.uint64)), k
    assert d["counters"] == want["counters"]
    m0 = devs(name).radiance(R.rays(name)[:300], samples=7, max_depth=50, seed=R.SEED, chunk=3)
    for k in ("sum", "rays", "state"):
        assert np.array_equal(m[k].view(np.uint64), m0[k].view(np.uint64)), k


@pytest.mark.parametrize("n", Q.BATCHES)
def test_batch_edges_write_nothing_past_n(n, devs):
    """The async form on caller buffers, over-allocated and poisoned, three chunks per ray: the first
    n records equal the synchronous form's, nothing after them is touched in the output or -- past
    its 3 n records -- in the scratch; the totals are added to the caller's counters."""
    name, samples, chunk, chunks = "mixed_hdri", 5, 2, 3
    rq = devs(name)
    r = np.ascontiguousarray(R.rays(name)[:n])
    pad, poison = 70, 0xA5
    need = N.lib.gs_query_radiance_scratch_bytes(n, samples, chunk)
    assert need == n * chunks * 40
    d_r, d_o, d_s, d_c = DevBuf(max(n, 1) * 72), DevBuf((n + pad) * 40, poison), DevBuf(need + pad * 40, poison), DevBuf(128)
    try:
        d_r.put(r)
        d_c.put(np.full(16, 1000, dtype=np.uint64))
        N.check(N.lib.gs_query_radiance_async(rq.dev, d_r.p, n, samples, chunk, 50, R.SEED, None, d_o.p, d_c.p, d_s.p,
                                              need, None))
        ob, sb, cb = d_o.get(), d_s.get(), d_c.get().view(np.uint64)  # (the download synchronises)
    finally:
        for b in (d_r, d_o, d_s, d_c):
            b.free()
    assert (ob[n * 40:] == poison).all() and (sb[need:] == poison).all()
    cnt = dict(zip(N.COUNTER_NAMES, (int(x) - 1000 for x in cb)))
    if n == 0:
        assert (sb == poison).all() and all(v == 0 for v in cnt.values())
        return
    ref = rq.radiance(r, samples=samples, max_depth=50, seed=R.SEED, chunk=chunk, counters=True)
    out = ob[:n * 40].view(GQ.RADIANCE_DTYPE)
    assert np.array_equal(_bits(out["rgb"]), _bits(ref["sum"]))
    assert np.array_equal(out["rays"], ref["rays"]) and np.array_equal(out["state"], ref["state"])
    assert cnt == ref["counters"] and cnt["paths"] == n * samples and cnt["pixels"] == 0
    assert int(cb[15]) == 1000  # (the reserved word is not a counter)
    part = sb[:need].view(GQ.RADIANCE_DTYPE).reshape(n, chunks)
    assert np.array_equal(part["rays"].sum(axis=1), out["rays"]) and np.array_equal(part["state"][:, -1], out["state"])


def test_no_rays_is_ok_with_no_launch(devs):
    d = devs("mixed_sky").radiance(np.zeros((0, 9)), samples=4, counters=True)
    assert d["sum"].shape == (0, 3) and d["rays"].shape == (0,) and d["counters"]["paths"] == 0


# ----------------------------------------------------------------------------- 5. edge cases
def test_depth_zero_traces_nothing_and_depth_one_is_the_first_hit(devs):
    name, n, samples = "mixed_hdri", 300, 3
    rq = devs(name)
    r = np.ascontiguousarray(R.rays(name)[:n])
    z = rq.radiance(r, samples=samples, max_depth=0, seed=R.SEED, counters=True)
    assert (_bits(z["sum"]) == 0).all() and (z["rays"] == 0).all()  # +0.0
    assert np.array_equal(z["state"], R.seeds(n, samples).reshape(n, samples)[:, -1])
    assert z["counters"]["paths"] == n * samples
    assert all(v == 0 for k, v in z["counters"].items() if k != "paths")
    st = np.arange(1, n * samples + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    zs = rq.radiance(r, samples=samples, max_depth=0, seed=R.SEED, states=st)
    assert np.array_equal(zs["state"], st.reshape(n, samples)[:, -1]) and (_bits(zs["sum"]) == 0).all()
    one = rq.radiance(r, samples=1, max_depth=1, seed=R.SEED)
    a = R.ray_color_fold(R.scene(name).twin, r, R.seeds(n), 1)
    assert (one["rays"] == 1).all() and np.array_equal(one["state"], a["state"])
    assert (_bits(one["sum"]) != _bits(a["rgb"])).any(axis=1).sum() <= parity.cap_for(n)
    # a scattered ray is black at depth 1 (and an absorbed one at any depth)
    assert ((one["sum"] == 0.0).all(axis=1) == np.isin(a["end"], (R.DEPTH, R.ABSORBED))).all()
    assert (a["end"] == R.SKY).any() and (a["end"] == R.DEPTH).any()


@pytest.mark.parametrize("name,base", [("mixed_sky", "mixed"), ("media_hdri", "media")])
def test_malformed_rays_complete_with_the_folds_answer(name, base, devs):
    """NaN, infinities, a zero direction: inputs the entry accepts by contract.  Every path ends and
    the colour is what the reference's arithmetic gives, a NaN matched by position."""
    r, tags = Q.special_rays(base)
    r = np.ascontiguousarray(r)
    assert len(r) > 100 and {"zero_dir", "bad_o", "bad_d", "bad_all"} <= set(tags)
    d = devs(name).radiance(r, samples=1, max_depth=4, seed=R.SEED)
    a = R.ray_color_fold(R.scene(name).twin, r, R.seeds(len(r)), 4)
    assert np.array_equal(np.isnan(d["sum"]), np.isnan(a["rgb"]))
    bad = _differs(d, a)
    print("%s: %d special rays, %d NaN colours, %d differ" % (name, len(r), int(np.isnan(a["rgb"]).any(axis=1).sum()),
                                                             int(bad.sum())))
    assert bad.sum() <= parity.cap_for(len(r)), [tags[i] for i in np.flatnonzero(bad)[:8]]
    with np.errstate(invalid="ignore"):
        delta = np.abs(d["sum"] - a["rgb"])
    assert np.nanmax(np.where(np.isfinite(delta), delta, 0.0)) <= parity.MAX_ABS
    assert (d["rays"] <= 4).all() and (d["rays"] >= 1).all()


def test_tmin_and_tmax_are_not_read(devs, single):
    name = "mixed_hdri"
    r = R.rays(name).copy()
    rng = np.random.default_rng(3)
    r[:, 7] = rng.uniform(-1e9, 1e9, len(r))
    r[:, 8] = rng.uniform(-1e9, 1e9, len(r))
    r[::7, 7], r[::5, 8], r[::11, 8] = np.nan, -np.inf, 0.0
    d, want = devs(name).radiance(r, samples=1, max_depth=50, seed=R.SEED), single(name, 50)
    for k in ("sum", "rays", "state"):
        assert np.array_equal(d[k].view(np.uint64), want[k].view(np.uint64)), k


# ----------------------------------------------------------------------------- 6. general scenes, renders
@pytest.mark.parametrize("name", sorted(k for k, v in R.FEAT_BITS.items() if v == 512))
def test_general_scenes_launch_the_catch_all_set(name, devs, single):
    rq, d = devs(name), single(name, 50)
    assert rq.feat & 512
    c = d["counters"]
    assert c["node_visits"] > c["rays"] and c["hits"] > 0 and c["instance_tests"] > 0
    if name == "outer_light_sky":
        # the light and the fuzzy metal sit behind two chains: their ends are the fold's, ray by ray
        a = R.answers(name, 50)
        ends = np.isin(a["end"], (R.LIGHT, R.ABSORBED))
        assert (a["end"] == R.LIGHT).sum() > 50 and (a["end"] == R.ABSORBED).sum() > 0
        assert np.array_equal(_bits(d["sum"][ends]), _bits(a["rgb"][ends])) and (d["sum"][a["end"] == R.LIGHT] > 0.0).any()
    else:
        assert c["medium_tests"] > 0


def test_a_radiance_query_beside_renders_changes_nothing(devs, single):
    """One frame context (one device scene): query, render, query, render -- both frames and their
    counters equal a context's that never queried; the query answers as on a scene of its own."""
    name = "media_hdri"
    cs = camera_spec(1.0, 96, 8, 40.0, (0.0, 2.0, 26.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 10.0)
    sc = scenes.Scene("radiance_media", R.scene(name).spec, cs, fixed_spp(4))
    r = np.ascontiguousarray(R.rays(name)[:1500])
    want = single(name, 50)
    plain = g.MultiRenderer(sc, num_gpus=1)
    try:
        p1 = plain.render(seed=3, rgb=True)
        p2 = plain.render(seed=3, rgb=True)
        feat = _last_feat(plain)
    finally:
        plain.close()
    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        q = m.query()
        f0 = _last_feat(m)
        before = q.radiance(r, samples=1, max_depth=50, seed=R.SEED)
        assert _last_feat(m) == f0  # a query is no render launch
        f1 = m.render(seed=3, rgb=True)
        f_after = _last_feat(m)
        mid = q.radiance(r, samples=1, max_depth=50, seed=R.SEED)
        assert _last_feat(m) == f_after
        f2 = m.render(seed=3, rgb=True)
        q.close()
    finally:
        m.close()
    assert feat == f_after and feat >= 0
    for a, b in ((p1, f1), (p2, f2)):
        assert np.array_equal(a["rgb"], b["rgb"]) and a["counters"] == b["counters"]
    for got in (before, mid):
        for k in ("sum", "rays", "state"):
            assert np.array_equal(got[k].view(np.uint64), want[k][:1500].view(np.uint64)), k


# ----------------------------------------------------------------------------- 7. Python
def test_multirenderer_query_radiance_equals_a_fresh_rayquerys():
    name = "textured_hdri"
    cs = camera_spec(1.0, 32, 8, 45.0, (2.0, 3.0, 24.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 10.0)
    sc = scenes.Scene("radiance_textured", R.scene(name).spec, cs, fixed_spp(2))
    r = GQ.panorama_rays((0.0, 8.0, 0.0), 64, 32)
    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        q = m.query()
        a = q.radiance(r, samples=3, max_depth=6, seed=4, chunk=2, counters=True)
        q.close()
    finally:
        m.close()
    with g.RayQuery(R.scene(name).spec) as fresh:
        b = fresh.radiance(r, samples=3, max_depth=6, seed=4, chunk=2, counters=True)
    for k in ("sum", "rgb", "rays", "state"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert a["counters"] == b["counters"] and a["counters"]["paths"] == 64 * 32 * 3
    assert set(a) == {"sum", "rgb", "rays", "state", "counters"} and a["sum"].shape == (64 * 32, 3)
    assert np.array_equal(a["rgb"], a["sum"] / 3.0) and (a["sum"] != 0.0).any()
