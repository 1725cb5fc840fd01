"""Python entry points to the device path (libgrayshift.so, HIP for gfx950).

* ``render(scene)`` — the one-call ``Camera::render`` replacement (linear f32 frame).
* ``render_views(scene, cameras, samples)`` / ``MultiRenderer.render_views`` — a batch of
  cameras of one world in a single launch, each view bit-identical to its own render.
* ``ProgressiveRenderer`` — a fixed-spp frame as a sequence of passes over device-resident
  f64 sums: preview, add samples, checkpoint, resume (bit-identical to the one-shot render).
* ``AdaptiveRenderer`` — the scene's own adaptive SampleSettings in passes of batch rounds:
  preview, per-pixel sample-count and error maps, checkpoint, resume (bit-identical too).
* ``ViewsProgressiveRenderer`` — a batch of cameras refined in passes, view by view: per-view
  sample budgets and change, preview, checkpoint, resume (each view bit-identical to its own render).
* ``ViewsAdaptiveRenderer`` / ``render_views_adaptive`` — a batch of cameras under one set of
  adaptive SampleSettings, in batch rounds whose active lists hold every view's surviving pixels
  (each view bit-identical to its own adaptive render).
* ``Renderer`` — device-resident scene for repeated / multi-GPU rendering: upload once,
  render this rank's tiles into a caller-provided device buffer on a given stream.
  Used by bench.py with torch tensors as the device buffers (torch is plumbing only).
"""
import ctypes as C
import time

import numpy as np

from . import _native as N
from . import checkpoint


def camera(cam_spec):
    """Camera::new (camera.rs:39-98) -> gs_camera (the fields the device reads)."""
    out = N.gs_camera()
    N.check(N.lib.gs_host_camera(C.byref(cam_spec), C.byref(out)))
    return out


def render(scene, seed=1, stats=None):
    """Render a scenes.Scene on the current HIP device.  Returns (rgb [H,W,3] f32, counters);
    `stats` (a dict, optional) receives the call's gs_stats (kernel / render ms, bytes)."""
    cam = camera(scene.camera)
    out = np.zeros((cam.image_height, cam.image_width, 3), dtype=np.float32)
    st = N.gs_stats()
    N.check(N.lib.gs_host_render_spec(scene.spec.ptr(), C.byref(scene.camera), C.byref(scene.settings), seed,
                                      out.ctypes.data, C.byref(st)))
    if stats is not None:
        stats.update(st.as_dict())
    return out, st.counters.as_dict()


def render_ppm(scene, seed=1):
    """The whole of Camera::render (camera.rs:100-121): returns (PPM text as bytes, counters).
    Pixel bytes (write_color of the f64 colour) and the text are produced on the device."""
    cam = camera(scene.camera)
    cap = N.lib.gs_ppm_max_bytes(cam.image_width, cam.image_height)
    if cap < 0:
        raise ValueError("bad image size")
    buf = C.create_string_buffer(int(cap))
    n = C.c_int64()
    st = N.gs_stats()
    N.check(N.lib.gs_host_render_ppm_spec(scene.spec.ptr(), C.byref(scene.camera), C.byref(scene.settings), seed,
                                          buf, cap, C.byref(n), C.byref(st)))
    return buf.raw[:n.value], st.counters.as_dict()


def _launch(num_gpus, tile, plan, devices):
    dev = None
    if devices is not None:
        dev = (C.c_int32 * len(devices))(*devices)
        num_gpus = len(devices)
    tile_w, tile_h = tile if isinstance(tile, (tuple, list)) else (tile, tile)  # (an int: square tiles)
    launch = N.gs_launch(num_gpus=num_gpus, tile_w=tile_w, tile_h=tile_h, plan=1 if plan else 0,
                         devices=C.cast(dev, C.c_void_p) if dev is not None else None)
    return launch, dev


def _outputs(W, H, rgb, rgb8, ppm):
    """gs_multi_outputs for the requested host outputs (None: the frame stays on the device)."""
    if not (rgb or rgb8 or ppm):
        return None, {}, None
    res = {}
    out = N.gs_multi_outputs()
    if rgb:
        res["rgb"] = np.zeros((H, W, 3), dtype=np.float32)
        out.rgb = res["rgb"].ctypes.data
    if rgb8:
        res["rgb8"] = np.zeros((H, W, 3), dtype=np.uint8)
        out.rgb8 = res["rgb8"].ctypes.data
    ppm_buf = None
    if ppm:
        cap = N.lib.gs_ppm_max_bytes(W, H)
        ppm_buf = (C.create_string_buffer(int(cap)), C.c_int64(0))
        out.ppm_text = C.addressof(ppm_buf[0])
        out.ppm_capacity = cap
        out.ppm_len = C.pointer(ppm_buf[1])
    return out, res, ppm_buf


def _result(res, st, ppm_buf=None, views=None):
    """The tail of a call's result dict: the PPM text when there is one, the frames as [V,H,W,3] for
    views = (V, H, W), the call's "counters" and its "stats"."""
    if ppm_buf is not None:
        res["ppm"] = ppm_buf[0].raw[:ppm_buf[1].value]
    for k in ("rgb", "rgb8"):
        if views is not None and k in res:
            res[k] = res[k].reshape(*views, 3)
    res["counters"] = st.counters.as_dict()
    res["stats"] = {k: v for k, v in st.as_dict().items() if k != "counters"}
    return res


def render_multi(scene, num_gpus=0, seed=1, tile=64, plan=True, rgb=True, rgb8=False, ppm=False, devices=None,
                 bvh="host"):
    """camera.rs:105-114 (and with ppm=True the whole of :100-121) on `num_gpus` GPUs of
    this node (0 = every visible one) through gs_render_multi: one scene per device,
    tiles rendered concurrently, one RCCL gather to the first device.  Returns a dict
    with the requested outputs ("rgb" [H,W,3] f32, "rgb8" [H,W,3] u8, "ppm" bytes), the
    summed "counters" and the call's "stats"."""
    host = HostScene(scene.spec, bvh=bvh)
    try:
        cam = camera(scene.camera)
        out, res, ppm_buf = _outputs(cam.image_width, cam.image_height, rgb, rgb8, ppm)
        if out is None:
            out = N.gs_multi_outputs()  # none requested: the library reports GS_ERR_ARG
        launch, _dev = _launch(num_gpus, tile, plan, devices)
        st = N.gs_stats()
        N.check(N.lib.gs_render_multi(host.flat_ptr, C.byref(cam), C.byref(scene.settings), seed, C.byref(launch),
                                      C.byref(out), C.byref(st)))
        return _result(res, st, ppm_buf)
    finally:
        host.close()


class MultiRenderer:
    """The persistent N-GPU frame context (gs_multi_*): the world uploaded to every device
    and the RCCL communicator built once, then any number of frames, each one synchronous
    call (plan, render on every device, one gather, unpack).  num_gpus=0: every visible
    device; num_gpus=1: no collective."""

    def __init__(self, scene, num_gpus=1, tile=64, plan=True, devices=None, bvh="host", device_min_members=0):
        self.scene = scene
        self.host = HostScene(scene.spec, bvh=bvh, device_min_members=device_min_members)
        self.cam = camera(scene.camera)
        self.settings = scene.settings
        launch, _dev = _launch(num_gpus, tile, plan, devices)
        h = C.c_void_p()
        N.check(N.lib.gs_multi_create(self.host.flat_ptr, C.byref(launch), C.byref(h)))
        self.handle = h
        n = C.c_int32()
        ids = (C.c_int32 * 64)()
        N.check(N.lib.gs_multi_devices(h, C.byref(n), ids, 64))
        self.devices = list(ids[:n.value])

    @property
    def width(self):
        return self.cam.image_width

    @property
    def height(self):
        return self.cam.image_height

    def render(self, seed=1, rgb=False, rgb8=False, ppm=False):
        """One frame.  With no host output requested the linear f32 frame stays on the first
        device (frame_ptr()).  Returns a dict: requested outputs, "counters", "stats"."""
        out, res, ppm_buf = _outputs(self.width, self.height, rgb, rgb8, ppm)
        st = N.gs_stats()
        N.check(N.lib.gs_multi_render(self.handle, C.byref(self.cam), C.byref(self.settings), seed,
                                      C.byref(out) if out is not None else None, C.byref(st)))
        return _result(res, st, ppm_buf)

    def render_stats(self, seed, st):
        """One frame, the frame left on the first device, its gs_stats written into `st` (a
        caller-owned N.gs_stats) -- render() without the per-call Python conversions, for
        timed loops (bench.py)."""
        N.check(N.lib.gs_multi_render(self.handle, C.byref(self.cam), C.byref(self.settings), seed, None,
                                      C.byref(st)))

    def views_chunk(self, cam, samples):
        """gs_views_chunk: the coarse chunk a one-shot render of `cam` (a gs_camera) at `samples`
        spp takes under the process's knobs as they stand."""
        d = C.c_void_p()
        N.check(N.lib.gs_multi_scene(self.handle, 0, C.byref(d)))
        c = N.lib.gs_views_chunk(d, C.byref(cam), samples)
        if c == 0:
            raise N.GrayshiftError(N.GS_ERR_ARG, N.lib.gs_last_error().decode("utf-8", "replace"))
        return c

    def render_views(self, cameras, samples, seeds=None, chunk=0, rgb=True, rgb8=False):
        """V cameras (gs_camera_specs of one width and height) of the context's world in one
        launch (gs_multi_render_views), `samples` per pixel, view v with seed seeds[v] (default 1).
        View v's frames are bit for bit those of a fixed-spp render of cameras[v] with that seed
        and the same coarse chunk; chunk=0 takes gs_views_chunk, the chunk of plain render()
        calls.  Returns a dict like render(): "rgb" [V,H,W,3] f32, "rgb8" [V,H,W,3] u8, the
        summed "counters", "stats".  With no host output the frames stay on the first device
        (frame_ptr(): [V,H,W,3] f32)."""
        cams = [camera(c) for c in cameras]
        V = len(cams)
        seeds = [1] * V if seeds is None else list(seeds)
        if len(seeds) != V:
            raise ValueError("one seed per camera")
        views = (N.gs_view * max(V, 1))()
        for v in range(V):
            views[v].cam = cams[v]
            views[v].seed = seeds[v]
        if V and not chunk:
            chunk = self.views_chunk(cams[0], samples)
        W, H = (cams[0].image_width, cams[0].image_height) if V else (0, 0)
        out, res, _ = _outputs(W, V * H, rgb, rgb8, False)
        st = N.gs_stats()
        N.check(N.lib.gs_multi_render_views(self.handle, views, V, samples, chunk,
                                            C.byref(out) if out is not None else None, C.byref(st)))
        return _result(res, st, views=(V, H, W))

    def render_views_adaptive(self, cameras, seeds=None, settings=None, rgb=True, rgb8=False):
        """V cameras of the context's world under one set of adaptive SampleSettings (default: the
        scene's), run to the end in batch rounds on the tall frame (gs_multi_views_adapt_*: one
        begin, one pass of every round, end).  View v's frames are bit for bit those of an adaptive
        render of cameras[v] alone with seed seeds[v] (default 1).  Returns a dict like
        render_views(): "rgb" [V,H,W,3] f32, "rgb8", the summed "counters", "stats"."""
        cams = [camera(c) for c in cameras]
        V = len(cams)
        seeds = [1] * V if seeds is None else list(seeds)
        if len(seeds) != V:
            raise ValueError("one seed per camera")
        views = (N.gs_view * max(V, 1))()
        for v in range(V):
            views[v].cam = cams[v]
            views[v].seed = seeds[v]
        ss = self.settings if settings is None else settings
        N.check(N.lib.gs_multi_views_adapt_begin(self.handle, views, V, C.byref(ss)))
        try:
            W, H = cams[0].image_width, cams[0].image_height
            out, res, _ = _outputs(W, V * H, rgb, rgb8, False)
            st = N.gs_stats()
            N.check(N.lib.gs_multi_views_adapt_pass(self.handle, ss.max_samples // ss.batch_size + 1,
                                                    C.byref(out) if out is not None else None, C.byref(st)))
            i = N.gs_views_adapt_info()
            N.check(N.lib.gs_multi_views_adapt_info(self.handle, C.byref(i), None))
        finally:
            N.lib.gs_multi_views_adapt_end(self.handle)
        res = _result(res, st, views=(V, H, W))
        res["counters"] = i.counters.as_dict()
        return res

    def query(self):
        """A RayQuery (grayshift_amd.query) over rank 0's device scene: no second upload.  Valid
        while this context is open; the current device must be rank 0's, as for any launch."""
        from .query import RayQuery
        d = C.c_void_p()
        N.check(N.lib.gs_multi_scene(self.handle, 0, C.byref(d)))
        return RayQuery(None, _shared=d)

    def scene_info(self, rank=0):
        """gs_device_scene_info of the scene on rank `rank`'s device."""
        d = C.c_void_p()
        N.check(N.lib.gs_multi_scene(self.handle, rank, C.byref(d)))
        i = N.gs_scene_info()
        N.check(N.lib.gs_device_scene_info(d, C.byref(i)))
        return {k: getattr(i, k) for k, _ in N.gs_scene_info._fields_}

    def frame_ptr(self):
        """(device pointer of the last W*H*3 f32 frame or None, its device id)."""
        p, p8, d = C.c_void_p(), C.c_void_p(), C.c_int32()
        N.check(N.lib.gs_multi_frame(self.handle, C.byref(p), C.byref(p8), C.byref(d)))
        return p.value, d.value

    def close(self):
        if getattr(self, "handle", None):
            N.lib.gs_multi_destroy(self.handle)
            self.handle = None
        if getattr(self, "host", None):
            self.host.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: the binding may be gone)
            pass


def render_views(scene, cameras, samples, seeds=None, num_gpus=1, tile=64, devices=None, bvh="host", **kw):
    """MultiRenderer.render_views in one call: upload `scene`, render the cameras, free it.  A
    batch whose chunk sums exceed the partial budget is rendered as consecutive groups of cameras
    that fit, the results concatenated: grouping changes no bit (the views contract).  Returns
    MultiRenderer.render_views' dict; "stats" is then a list, one gs_stats dict per group.
    **kw: render_views' chunk, rgb, rgb8."""
    r = MultiRenderer(scene, num_gpus=num_gpus, tile=tile, plan=False, devices=devices, bvh=bvh)
    try:
        cameras = list(cameras)
        seeds = [1] * len(cameras) if seeds is None else list(seeds)
        if len(seeds) != len(cameras):
            raise ValueError("one seed per camera")
        group = max(1, len(cameras))
        parts, at = [], 0
        while at < len(cameras) or not parts:
            try:
                parts.append(r.render_views(cameras[at:at + group], samples, seeds[at:at + group], **kw))
            except N.GrayshiftError as e:
                if e.code != N.GS_ERR_ARG or "partial budget" not in str(e) or group == 1:
                    raise
                group = (group + 1) // 2
                continue
            at += group
        res = {k: np.concatenate([p[k] for p in parts]) for k in ("rgb", "rgb8") if k in parts[0]}
        res["counters"] = {k: sum(p["counters"][k] for p in parts) for k in parts[0]["counters"]}
        res["stats"] = [p["stats"] for p in parts] if len(parts) > 1 else parts[0]["stats"]
        return res
    finally:
        r.close()


class _Session:
    """What the four session renderers share: a frame context of their own (self._mr), on which
    their session is open (self._open) until close(), which ends it with the library's `_end`."""

    _end = None  # the name of the session's gs_multi_*_end

    @property
    def devices(self):
        return self._mr.devices

    def scene_info(self, rank=0):
        return self._mr.scene_info(rank)

    def close(self):
        mr = getattr(self, "_mr", None)
        if mr is not None:
            if self._open and mr.handle:
                getattr(N.lib, self._end)(mr.handle)
            self._open = False
            mr.close()
            self._mr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: the binding may be gone)
            pass


class ProgressiveRenderer(_Session):
    """A fixed-spp frame rendered in passes (gs_multi_accum_*): every pass adds `samples` more
    samples per pixel to f64 sums resident on the devices and returns the frame resolved so far.

    The contract: passes of n_1, n_2, ... samples give the frame, the sums and the cumulative
    counters of one render of n_1 + n_2 + ... samples with the same seed and chunk, bit for bit
    -- however the samples are split into passes, on any number of GPUs, and across save() /
    resume().  The scene's own SampleSettings are not used: a pass is a sample count (adaptive
    settings have their own pass form, AdaptiveRenderer).  chunk: the coarse sample chunk c (0 = 16); every pass is 1 to
    64 whole chunks."""

    _end = "gs_multi_accum_end"

    def __init__(self, scene, num_gpus=1, seed=1, chunk=0, tile=64, plan=True, devices=None, bvh="host",
                 _resume=None):
        self.scene = scene
        self.seed = int(seed)
        self._mr = MultiRenderer(scene, num_gpus=num_gpus, tile=tile, plan=plan, devices=devices, bvh=bvh)
        self._open = False
        self._passes0 = 0
        self._delta0 = 0.0
        try:
            if _resume is None:
                N.check(N.lib.gs_multi_accum_begin(self._mr.handle, C.byref(self._mr.cam), self.seed, int(chunk)))
            else:
                sums, meta = _resume
                cnt = N.gs_counters(**meta["counters"])
                N.check(N.lib.gs_multi_accum_upload(self._mr.handle, C.byref(self._mr.cam), self.seed, int(chunk),
                                                    meta["samples"], sums.ctypes.data, C.byref(cnt)))
                self._passes0 = meta.get("passes", 0)
                self._delta0 = meta.get("last_delta", 0.0)
            self._open = True
            self.chunk = self._info().chunk
        except Exception:
            self.close()
            raise

    @property
    def width(self):
        return self._mr.width

    @property
    def height(self):
        return self._mr.height

    def _info(self):
        i = N.gs_accum_info()
        N.check(N.lib.gs_multi_accum_info(self._mr.handle, C.byref(i)))
        return i

    @property
    def samples(self):
        """Samples per pixel accumulated so far."""
        return int(self._info().samples)

    def info(self):
        """width, height, chunk, passes, seed, samples, last_delta (the last pass's mean |change|
        of the f64 colour over W*H*3 values) and the cumulative counters.  After resume(), passes
        continues the checkpoint's count, and last_delta is the checkpoint's until a pass runs."""
        d = self._info().as_dict()
        if d["passes"] == 0:
            d["last_delta"] = self._delta0
        d["passes"] += self._passes0
        return d

    def render_pass(self, samples, rgb=True, rgb8=False, ppm=False):
        """Render `samples` more samples of every pixel (1 to 64 whole chunks) and resolve the frame.
        Returns a dict: the requested outputs ("rgb" [H,W,3] f32, "rgb8", "ppm"; with none the f32
        frame stays on the first device, frame_ptr()), this pass's "counters" and "stats", and
        "info" (info() after the pass)."""
        out, res, ppm_buf = _outputs(self.width, self.height, rgb, rgb8, ppm)
        st = N.gs_stats()
        N.check(N.lib.gs_multi_accum_pass(self._mr.handle, int(samples), C.byref(out) if out is not None else None,
                                          C.byref(st)))
        res = _result(res, st, ppm_buf)
        res["info"] = self.info()
        return res

    def render_until(self, total_samples=None, seconds=None, min_delta=None, pass_samples=None, on_pass=None):
        """Run passes until the first bound is reached: the frame holds `total_samples` samples per
        pixel (a multiple of the chunk), `seconds` of wall time have passed since the call, or a
        pass's last_delta is at most `min_delta`.  pass_samples: samples per pass, rounded up to
        whole chunks and capped at 64 chunks (default: 4 chunks).  on_pass(info, frame) is called
        after every pass with info() and the resolved [H,W,3] f32 frame (a preview).  Returns
        (info, frame) of the last pass; frame is None when no pass ran."""
        if total_samples is None and seconds is None and min_delta is None:
            raise ValueError("render_until needs a bound: total_samples, seconds or min_delta")
        c = self.chunk
        if total_samples is not None and total_samples % c:
            raise ValueError("total_samples %d is not a multiple of the chunk %d" % (total_samples, c))
        step = 4 * c if pass_samples is None else int(pass_samples)
        step = min(64 * c, max(c, (step + c - 1) // c * c))
        t0 = time.monotonic()
        info, frame = self.info(), None
        while True:
            n = step
            if total_samples is not None:
                n = min(n, total_samples - info["samples"])
                if n <= 0:
                    break
            if seconds is not None and frame is not None and time.monotonic() - t0 >= seconds:
                break
            res = self.render_pass(n)
            info, frame = res["info"], res["rgb"]
            if on_pass is not None:
                on_pass(info, frame)
            if min_delta is not None and info["last_delta"] <= min_delta:
                break
            if seconds is not None and time.monotonic() - t0 >= seconds:
                break
        return info, frame

    def sums(self):
        """The running sums, [H, W, 3] f64 in image order (a copy on the host)."""
        out = np.zeros((self.height, self.width, 3), dtype=np.float64)
        N.check(N.lib.gs_multi_accum_download(self._mr.handle, out.ctypes.data))
        return out

    def frame_ptr(self):
        """(device pointer of the last resolved W*H*3 f32 frame or None, its device id)."""
        return self._mr.frame_ptr()

    def save(self, path):
        """Write a checkpoint (grayshift_amd.checkpoint): the sums, samples, seed, chunk, frame size,
        the gs_camera bytes and the cumulative counters."""
        i = self.info()
        meta = {k: i[k] for k in ("samples", "seed", "chunk", "width", "height", "counters", "passes", "last_delta")}
        meta["camera"] = bytes(self._mr.cam)
        checkpoint.write_checkpoint(path, self.sums(), meta)

    @classmethod
    def resume(cls, scene, path, **kw):
        """Continue the checkpoint at `path` on `scene`: **kw as for the constructor (any device
        count or tile plan).  seed and chunk default to the checkpoint's; the checkpoint is
        rejected (checkpoint.CheckpointError) when its frame size, chunk, seed or gs_camera bytes
        differ from the scene's and the ones given.  Whether `scene` is otherwise the world the
        checkpoint was rendered from is the caller's responsibility."""
        sums, meta = checkpoint.read_checkpoint(path)
        cam = camera(scene.camera)
        seed = kw.pop("seed", meta["seed"])
        chunk = kw.pop("chunk", meta["chunk"]) or 16
        checkpoint.check_compatible(meta, cam.image_width, cam.image_height, chunk, seed, bytes(cam))
        return cls(scene, seed=seed, chunk=chunk, _resume=(sums, meta), **kw)


class AdaptiveRenderer(_Session):
    """The scene's own adaptive SampleSettings rendered in passes of batch rounds
    (gs_multi_adapt_*): round r renders batch r of every pixel still active, and every pass
    returns the frame resolved so far -- a stopped pixel's final colour, an active pixel's mean
    over the samples it has taken.

    The contract: whatever the split into passes, the GPU count, the tile plan or a save() /
    resume() in between, the finished frame, its rgb8 bytes and the cumulative counters are those
    of render() / render_multi() with the same settings and seed, bit for bit; after k rounds
    the frame is the one-shot frame with max_samples = k * batch_size - 1."""

    _end = "gs_multi_adapt_end"

    def __init__(self, scene, num_gpus=1, seed=1, tile=64, plan=True, devices=None, bvh="host", _resume=None):
        self.scene = scene
        self.seed = int(seed)
        self._mr = MultiRenderer(scene, num_gpus=num_gpus, tile=tile, plan=plan, devices=devices, bvh=bvh)
        self._open = False
        mr = self._mr
        try:
            if _resume is None:
                N.check(N.lib.gs_multi_adapt_begin(mr.handle, C.byref(mr.cam), C.byref(mr.settings), self.seed))
            else:
                sums, state, meta = _resume
                cnt = N.gs_counters(**meta["counters"])
                N.check(N.lib.gs_multi_adapt_upload(mr.handle, C.byref(mr.cam), C.byref(mr.settings), self.seed,
                                                    meta["rounds"], sums.ctypes.data, state.ctypes.data,
                                                    C.byref(cnt)))
            self._open = True
        except Exception:
            self.close()
            raise

    @property
    def width(self):
        return self._mr.width

    @property
    def height(self):
        return self._mr.height

    @property
    def info(self):
        """gs_adapt_info: width, height, batch, rounds, max_rounds, finished, seed, active_pixels,
        samples_total, samples_max and the cumulative counters (attributes; .as_dict())."""
        i = N.gs_adapt_info()
        N.check(N.lib.gs_multi_adapt_info(self._mr.handle, C.byref(i)))
        return i

    @property
    def finished(self):
        return bool(self.info.finished)

    def render_rounds(self, n, rgb=True, rgb8=False, ppm=False):
        """Render the next `n` rounds (clipped to what remains; none once finished) and resolve the
        frame.  Returns a dict: the requested outputs ("rgb" [H,W,3] f32, "rgb8", "ppm"; with none
        the f32 frame stays on the first device, frame_ptr), this pass's "counters" and "stats",
        and "info" (info.as_dict() after the pass)."""
        out, res, ppm_buf = _outputs(self.width, self.height, rgb, rgb8, ppm)
        st = N.gs_stats()
        N.check(N.lib.gs_multi_adapt_pass(self._mr.handle, int(n), C.byref(out) if out is not None else None,
                                          C.byref(st)))
        res = _result(res, st, ppm_buf)
        res["info"] = self.info.as_dict()
        return res

    def render_until(self, rounds=None, seconds=None, active_fraction=None, pass_rounds=1, on_pass=None):
        """Run passes of `pass_rounds` rounds until the first bound is reached: `rounds` rounds
        have run in all, `seconds` of wall time have passed since the call, at most
        `active_fraction` of the pixels are still active -- or, at the latest, the frame is
        finished.  on_pass(info, frame) is called after every pass with info.as_dict() and the
        resolved [H,W,3] f32 frame.  Returns (info, frame) of the last pass; frame is None when no
        pass ran.  pass_rounds: every pass ends with one resolve over the frame and one read of
        the active count, so a larger value trades preview rate for less overhead."""
        step = max(1, int(pass_rounds))
        t0 = time.monotonic()
        info, frame = self.info.as_dict(), None
        npx = self.width * self.height
        while not info["finished"]:
            n = step
            if rounds is not None:
                n = min(n, int(rounds) - info["rounds"])
                if n <= 0:
                    break
            if seconds is not None and frame is not None and time.monotonic() - t0 >= seconds:
                break
            res = self.render_rounds(n)
            info, frame = res["info"], res["rgb"]
            if on_pass is not None:
                on_pass(info, frame)
            if active_fraction is not None and info["active_pixels"] <= active_fraction * npx:
                break
        return info, frame

    def sample_counts(self):
        """[H, W] u32: the samples every pixel has taken so far (multiples of the batch size)."""
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        N.check(N.lib.gs_multi_adapt_maps(self._mr.handle, out.ctypes.data, None))
        return out

    def error_map(self):
        """[H, W] f32: what the stop test compares with the tolerance, sqrt(confidence² · var / n)
        / |mean| of the pixel's luminance (NaN / inf where the variance or the mean is 0/0)."""
        out = np.zeros((self.height, self.width), dtype=np.float32)
        N.check(N.lib.gs_multi_adapt_maps(self._mr.handle, None, out.ctypes.data))
        return out

    def state(self):
        """(sums [H, W, 5] f64: Σr, Σg, Σb, Σlum, Σlum²; state [H, W] u32: batches taken, the top
        bit once the pixel has stopped) in image order, copies on the host."""
        sums = np.zeros((self.height, self.width, 5), dtype=np.float64)
        state = np.zeros((self.height, self.width), dtype=np.uint32)
        N.check(N.lib.gs_multi_adapt_download(self._mr.handle, sums.ctypes.data, state.ctypes.data))
        return sums, state

    @property
    def frame_ptr(self):
        """(device pointer of the last resolved W*H*3 f32 frame or None, its device id)."""
        return self._mr.frame_ptr()

    def save(self, path):
        """Write a checkpoint (grayshift_amd.checkpoint, format 2): the sums and state words, the
        rounds run, seed, settings, frame size, the gs_camera bytes and the cumulative counters."""
        i = self.info
        ss = self._mr.settings
        sums, state = self.state()
        meta = {"rounds": i.rounds, "seed": i.seed, "width": i.width, "height": i.height,
                "confidence": ss.confidence, "tolerance": ss.tolerance, "batch_size": ss.batch_size,
                "max_samples": ss.max_samples, "camera": bytes(self._mr.cam), "counters": i.counters.as_dict()}
        checkpoint.write_adaptive_checkpoint(path, sums, state, meta)

    @classmethod
    def resume(cls, scene, path, **kw):
        """Continue the checkpoint at `path` on `scene`: **kw as for the constructor (any device
        count or tile plan).  seed defaults to the checkpoint's; the checkpoint is rejected
        (checkpoint.CheckpointError) when its frame size, seed, SampleSettings or gs_camera bytes
        differ from the scene's and the ones given.  Whether `scene` is otherwise the world the
        checkpoint was rendered from is the caller's responsibility."""
        sums, state, meta = checkpoint.read_adaptive_checkpoint(path)
        cam = camera(scene.camera)
        seed = kw.pop("seed", meta["seed"])
        checkpoint.check_adaptive_compatible(meta, cam.image_width, cam.image_height, scene.settings, seed, bytes(cam))
        return cls(scene, seed=seed, _resume=(sums, state, meta), **kw)


class ViewsProgressiveRenderer(_Session):
    """A batch of cameras of one world refined in passes, view by view (gs_multi_views_accum_*):
    every pass adds `samples` more samples per pixel to the f64 sums of a subset of the views and
    returns all V frames resolved so far.

    The contract: after any sequence of passes in which view v received n_v samples, its sums, f32
    frame and rgb8 frame are bit for bit those of a fixed-spp render of cameras[v] with seed
    seeds[v], n_v samples and the same chunk (render_views with that one camera;
    ProgressiveRenderer on it) -- whatever the split into passes, the subset history, the other
    cameras, the GPU count, the tile size or a save() / resume() in between -- and the cumulative
    counters are the sums of those V renders' counters: an unselected view costs no ray.

    cameras: gs_camera_specs of one width and height; seeds: one per camera (default 1 each);
    chunk: the coarse sample chunk c (0 = 16), every pass is 1 to 64 whole chunks.  The scene's own
    camera and SampleSettings are not used."""

    _end = "gs_multi_views_accum_end"

    def __init__(self, scene, cameras, seeds=None, num_gpus=1, chunk=0, tile=64, devices=None, bvh="host",
                 _resume=None):
        self.scene = scene
        self._cams = [camera(c) for c in cameras]
        V = len(self._cams)
        self.seeds = [1] * V if seeds is None else [int(s) for s in seeds]
        if len(self.seeds) != V:
            raise ValueError("one seed per camera")
        self._views = (N.gs_view * max(V, 1))()
        for v in range(V):
            self._views[v].cam = self._cams[v]
            self._views[v].seed = self.seeds[v]
        self._mr = MultiRenderer(scene, num_gpus=num_gpus, tile=tile, plan=False, devices=devices, bvh=bvh)
        self._open = False
        self._passes0 = 0
        self._deltas0 = None
        try:
            if _resume is None:
                N.check(N.lib.gs_multi_views_accum_begin(self._mr.handle, self._views, V, int(chunk)))
            else:
                sums, meta = _resume
                cnt = N.gs_counters(**meta["counters"])
                ns = np.array(meta["samples"], dtype=np.uint32)
                N.check(N.lib.gs_multi_views_accum_upload(self._mr.handle, self._views, V, int(chunk), ns.ctypes.data,
                                                          sums.ctypes.data, C.byref(cnt)))
                self._passes0 = meta.get("passes", 0)
                self._deltas0 = np.array(meta.get("deltas", [0.0] * V), dtype=np.float64)
            self._open = True
            i = self._info()[0]
            self.chunk, self.n_views, self.width, self.height = i.chunk, i.n_views, i.width, i.height
        except Exception:
            self.close()
            raise

    def _info(self):
        i = N.gs_views_accum_info()
        V = len(self._cams)
        ns = np.zeros(max(V, 1), dtype=np.uint32)
        ds = np.zeros(max(V, 1), dtype=np.float64)
        N.check(N.lib.gs_multi_views_accum_info(self._mr.handle, C.byref(i), ns.ctypes.data, ds.ctypes.data))
        if self._deltas0 is not None:  # (after resume(): a view's checkpointed delta until a pass selects it)
            ds = np.where(self._fresh, self._deltas0, ds[:V])
        return i, ns[:V], ds[:V]

    _fresh = True  # (an array of V flags after resume(): views no pass has selected since)

    @property
    def samples(self):
        """[V] u32: the samples per pixel accumulated in each view."""
        return self._info()[1]

    @property
    def deltas(self):
        """[V] f64: per view, the mean |change| of the f64 colour over its W*H*3 values in the last
        pass that selected it (0 before its first)."""
        return self._info()[2]

    @property
    def info(self):
        """width, height (of one view), n_views, chunk, passes, tile_h, the cumulative counters,
        "samples" and "deltas" (lists, per view).  After resume(), passes continues the
        checkpoint's count."""
        i, ns, ds = self._info()
        d = i.as_dict()
        d["passes"] += self._passes0
        d["samples"] = [int(n) for n in ns]
        d["deltas"] = [float(x) for x in ds]
        return d

    def _selection(self, views):
        V = len(self._cams)
        if views is None:
            return None, list(range(V))
        idx = sorted({int(v) for v in views})
        if any(v < 0 or v >= V for v in idx):
            raise ValueError("view index out of range")
        sel = np.zeros(max(V, 1), dtype=np.uint8)
        sel[idx] = 1
        return sel, idx

    def render_pass(self, samples, views=None, rgb=True, rgb8=False):
        """Render `samples` more samples (1 to 64 whole chunks) of every pixel of the views `views`
        (indices; None: all) and resolve all V frames.  Selected views that hold different sample
        counts are rendered count by count, one launch each (the library's pass takes one sample
        base).  Returns a dict: the requested outputs ("rgb" [V,H,W,3] f32, "rgb8"; with none the
        f32 frames stay on the first device, frame_ptr()), this pass's "counters" and "stats" (a
        list when it took several launches), and "info" (info after the pass)."""
        sel, idx = self._selection(views)
        V, W, H = len(self._cams), self.width, self.height
        groups = [sel]
        if sel is not None:
            ns = self.samples
            groups = []
            for n in sorted({int(ns[v]) for v in idx}):
                g = np.zeros(max(V, 1), dtype=np.uint8)
                g[[v for v in idx if int(ns[v]) == n]] = 1
                groups.append(g)
            if not groups:
                groups = [sel]  # (empty: the library reports it)
        elif len({int(n) for n in self.samples}) > 1:
            return self.render_pass(samples, range(V), rgb, rgb8)
        res, stats, counters = {}, [], None
        for k, g in enumerate(groups):
            last = k == len(groups) - 1
            out, res, _ = _outputs(W, V * H, rgb and last, rgb8 and last, False)
            if not last:  # (frames of an intermediate launch stay on the device)
                out = None
            st = N.gs_stats()
            N.check(N.lib.gs_multi_views_accum_pass(self._mr.handle, int(samples), g.ctypes.data if g is not None else None,
                                                    C.byref(out) if out is not None else None, C.byref(st)))
            if self._deltas0 is not None:
                self._fresh = np.where(g[:V] != 0, False, self._fresh) if g is not None else np.zeros(V, dtype=bool)
            c = st.counters.as_dict()
            counters = c if counters is None else {n: counters[n] + c[n] for n in c}
            stats.append({n: v for n, v in st.as_dict().items() if n != "counters"})
        for k in ("rgb", "rgb8"):
            if k in res:
                res[k] = res[k].reshape(V, H, W, 3)
        res["counters"] = counters
        res["stats"] = stats if len(stats) > 1 else stats[0]
        res["info"] = self.info
        return res

    def render_until(self, total_samples=None, seconds=None, min_delta=None, pass_samples=None, on_pass=None):
        """Run passes until the first bound is reached: every view still selected holds
        `total_samples` samples (a multiple of the chunk), or `seconds` of wall time have passed
        since the call.  With `min_delta`, a view leaves the selection once a pass left its delta
        below the threshold, and the loop also ends when no view is left.  pass_samples: samples
        per pass, rounded up to whole chunks and capped at 64 chunks (default: 4 chunks).
        on_pass(info, frames) is called after every pass with info and the resolved [V,H,W,3] f32
        frames.  Returns (info, frames) of the last pass; frames is None when no pass ran."""
        if total_samples is None and seconds is None and min_delta is None:
            raise ValueError("render_until needs a bound: total_samples, seconds or min_delta")
        c = self.chunk
        if total_samples is not None and total_samples % c:
            raise ValueError("total_samples %d is not a multiple of the chunk %d" % (total_samples, c))
        step = 4 * c if pass_samples is None else int(pass_samples)
        step = min(64 * c, max(c, (step + c - 1) // c * c))
        t0 = time.monotonic()
        info, frames = self.info, None
        active = list(range(len(self._cams)))
        while active:
            if total_samples is not None:
                active = [v for v in active if info["samples"][v] < total_samples]
                if not active:
                    break
            if seconds is not None and frames is not None and time.monotonic() - t0 >= seconds:
                break
            # (views short of the budget by less than a step take what remains, in a pass of their own)
            if total_samples is not None:
                n = min(step, min(total_samples - info["samples"][v] for v in active))
                now = [v for v in active if total_samples - info["samples"][v] >= n]
            else:
                n, now = step, active
            res = self.render_pass(n, now)
            info, frames = res["info"], res["rgb"]
            if on_pass is not None:
                on_pass(info, frames)
            if min_delta is not None:
                active = [v for v in active if v not in now or info["deltas"][v] >= min_delta]
        return info, frames

    def sums(self):
        """The running sums, [V, H, W, 3] f64 in image order (a copy on the host)."""
        out = np.zeros((len(self._cams), self.height, self.width, 3), dtype=np.float64)
        N.check(N.lib.gs_multi_views_accum_download(self._mr.handle, out.ctypes.data))
        return out

    def frame_ptr(self):
        """(device pointer of the last resolved [V,H,W,3] f32 frames or None, its device id)."""
        return self._mr.frame_ptr()

    def save(self, path):
        """Write a checkpoint (grayshift_amd.checkpoint, format 3): the sums, the per-view samples,
        seeds and gs_camera bytes, chunk, view size and the cumulative counters."""
        i = self.info
        meta = {k: i[k] for k in ("samples", "chunk", "width", "height", "counters", "passes", "deltas")}
        meta["seeds"] = self.seeds
        meta["cameras"] = [bytes(c) for c in self._cams]
        checkpoint.write_views_checkpoint(path, self.sums(), meta)

    @classmethod
    def resume(cls, scene, path, cameras, seeds=None, **kw):
        """Continue the checkpoint at `path` on `scene` with the batch `cameras`: **kw as for the
        constructor (any device count or tile size).  seeds and chunk default to the checkpoint's;
        the checkpoint is rejected (checkpoint.CheckpointError) when its view count, view size,
        chunk, seeds or gs_camera bytes differ from the batch's and the ones given.  Whether
        `scene` is otherwise the world the checkpoint was rendered from is the caller's
        responsibility."""
        sums, meta = checkpoint.read_views_checkpoint(path)
        cams = [camera(c) for c in cameras]
        seeds = meta["seeds"] if seeds is None else list(seeds)
        chunk = kw.pop("chunk", meta["chunk"]) or 16
        W, H = (cams[0].image_width, cams[0].image_height) if cams else (0, 0)
        checkpoint.check_views_compatible(meta, W, H, chunk, seeds, [bytes(c) for c in cams])
        r = cls(scene, cameras, seeds=seeds, chunk=chunk, _resume=(sums, meta), **kw)
        r._fresh = np.ones(len(cams), dtype=bool)
        return r


class ViewsAdaptiveRenderer(_Session):
    """A batch of cameras of one world under ONE set of adaptive SampleSettings, in passes of batch
    rounds on the tall frame (gs_multi_views_adapt_*): round r renders batch r of every pixel of
    every view that is still active, so a late round's few surviving pixels of all views share one
    launch; every pass returns all V frames resolved so far.

    The contract: whatever the number and order of the views, the other cameras, the split into
    passes, the GPU count, the tile size or a save() / resume() in between, view v's finished frame,
    rgb8 bytes, sample_counts() and error_map() are bit for bit those of AdaptiveRenderer / render()
    of cameras[v] alone with seed seeds[v] and the same settings, and the cumulative counters are
    the sums of those V renders' counters; after k rounds every view shows what AdaptiveRenderer
    shows for it after k rounds.

    cameras: gs_camera_specs of one width and height; seeds: one per camera (default 1 each);
    settings: a gs_sample_settings (default: the scene's own).  The scene's own camera is not used."""

    _end = "gs_multi_views_adapt_end"

    def __init__(self, scene, cameras, seeds=None, settings=None, num_gpus=1, tile=64, devices=None, bvh="host",
                 _resume=None):
        self.scene = scene
        self._cams = [camera(c) for c in cameras]
        V = len(self._cams)
        self.seeds = [1] * V if seeds is None else [int(s) for s in seeds]
        if len(self.seeds) != V:
            raise ValueError("one seed per camera")
        self.settings = scene.settings if settings is None else settings
        self._views = (N.gs_view * max(V, 1))()
        for v in range(V):
            self._views[v].cam = self._cams[v]
            self._views[v].seed = self.seeds[v]
        self._mr = MultiRenderer(scene, num_gpus=num_gpus, tile=tile, plan=False, devices=devices, bvh=bvh)
        self._open = False
        try:
            if _resume is None:
                N.check(N.lib.gs_multi_views_adapt_begin(self._mr.handle, self._views, V, C.byref(self.settings)))
            else:
                sums, state, meta = _resume
                cnt = N.gs_counters(**meta["counters"])
                N.check(N.lib.gs_multi_views_adapt_upload(self._mr.handle, self._views, V, C.byref(self.settings),
                                                          meta["rounds"], sums.ctypes.data, state.ctypes.data,
                                                          C.byref(cnt)))
            self._open = True
            i = self._info()
            self.n_views, self.width, self.height = i.n_views, i.width, i.height
        except Exception:
            self.close()
            raise

    def _info(self, active=None):
        i = N.gs_views_adapt_info()
        N.check(N.lib.gs_multi_views_adapt_info(self._mr.handle, C.byref(i),
                                                active.ctypes.data if active is not None else None))
        return i

    @property
    def finished(self):
        return bool(self._info().finished)

    def info(self):
        """width, height (of one view), n_views, tile_h, batch, rounds, max_rounds, finished,
        active_pixels, samples_total, samples_max (over the batch), the cumulative counters, and
        "active_fractions": per view, the share of its pixels still active (counted on the host
        from the downloaded state: not for a hot loop)."""
        act = np.zeros(max(len(self._cams), 1), dtype=np.uint64)
        d = self._info(act).as_dict()
        d["active_fractions"] = [float(a) / (self.width * self.height) for a in act[:len(self._cams)]]
        return d

    def render_rounds(self, n, rgb=True, rgb8=False):
        """Render the next `n` rounds (clipped to what remains; none once finished) and resolve all
        V frames.  Returns a dict: the requested outputs ("rgb" [V,H,W,3] f32, "rgb8"; with none the
        f32 frames stay on the first device, frame_ptr()), this pass's "counters" and "stats", and
        "info" (the batch totals after the pass, without the per-view fractions)."""
        V, W, H = len(self._cams), self.width, self.height
        out, res, _ = _outputs(W, V * H, rgb, rgb8, False)
        st = N.gs_stats()
        N.check(N.lib.gs_multi_views_adapt_pass(self._mr.handle, int(n), C.byref(out) if out is not None else None,
                                                C.byref(st)))
        res = _result(res, st, views=(V, H, W))
        res["info"] = self._info().as_dict()
        return res

    def render_until(self, rounds=None, seconds=None, active_fraction=None, pass_rounds=1, on_pass=None):
        """Run passes of `pass_rounds` rounds until the first bound is reached: `rounds` rounds have
        run in all, `seconds` of wall time have passed since the call, at most `active_fraction`
        of the batch's pixels are still active -- or, at the latest, the batch is finished.
        on_pass(info, frames) is called after every pass with the batch totals and the resolved
        [V,H,W,3] f32 frames.  Returns (info, frames) of the last pass; frames is None when no pass
        ran."""
        step = max(1, int(pass_rounds))
        t0 = time.monotonic()
        info, frames = self._info().as_dict(), None
        npx = self.width * self.height * len(self._cams)
        while not info["finished"]:
            n = step
            if rounds is not None:
                n = min(n, int(rounds) - info["rounds"])
                if n <= 0:
                    break
            if seconds is not None and frames is not None and time.monotonic() - t0 >= seconds:
                break
            res = self.render_rounds(n)
            info, frames = res["info"], res["rgb"]
            if on_pass is not None:
                on_pass(info, frames)
            if active_fraction is not None and info["active_pixels"] <= active_fraction * npx:
                break
        return info, frames

    def sample_counts(self):
        """[V, H, W] u32: the samples every pixel has taken so far (multiples of the batch size)."""
        out = np.zeros((len(self._cams), self.height, self.width), dtype=np.uint32)
        N.check(N.lib.gs_multi_views_adapt_maps(self._mr.handle, out.ctypes.data, None))
        return out

    def error_map(self):
        """[V, H, W] f32: what the stop test compares with the tolerance (AdaptiveRenderer.error_map)."""
        out = np.zeros((len(self._cams), self.height, self.width), dtype=np.float32)
        N.check(N.lib.gs_multi_views_adapt_maps(self._mr.handle, None, out.ctypes.data))
        return out

    def state(self):
        """(sums [V, H, W, 5] f64: Σr, Σg, Σb, Σlum, Σlum²; state [V, H, W] u32: batches taken, the
        top bit once the pixel has stopped) in image order, copies on the host."""
        V = len(self._cams)
        sums = np.zeros((V, self.height, self.width, 5), dtype=np.float64)
        state = np.zeros((V, self.height, self.width), dtype=np.uint32)
        N.check(N.lib.gs_multi_views_adapt_download(self._mr.handle, sums.ctypes.data, state.ctypes.data))
        return sums, state

    def frame_ptr(self):
        """(device pointer of the last resolved [V,H,W,3] f32 frames or None, its device id)."""
        return self._mr.frame_ptr()

    def save(self, path):
        """Write a checkpoint (grayshift_amd.checkpoint, format 4): the sums and state words, the
        rounds run, the settings, the views' seeds and gs_camera bytes, the view size and the
        cumulative counters."""
        i = self._info()
        ss = self.settings
        sums, state = self.state()
        meta = {"rounds": i.rounds, "seeds": self.seeds, "cameras": [bytes(c) for c in self._cams],
                "width": i.width, "height": i.height, "confidence": ss.confidence, "tolerance": ss.tolerance,
                "batch_size": ss.batch_size, "max_samples": ss.max_samples, "counters": i.counters.as_dict()}
        checkpoint.write_views_adaptive_checkpoint(path, sums, state, meta)

    @classmethod
    def resume(cls, scene, path, cameras, seeds=None, settings=None, **kw):
        """Continue the checkpoint at `path` on `scene` with the batch `cameras`: **kw as for the
        constructor (any device count or tile size).  seeds default to the checkpoint's, settings
        to the scene's; the checkpoint is rejected (checkpoint.CheckpointError) when its view
        count, view size, seeds, SampleSettings or gs_camera bytes differ from the batch's.  Whether
        `scene` is otherwise the world the checkpoint was rendered from is the caller's
        responsibility."""
        sums, state, meta = checkpoint.read_views_adaptive_checkpoint(path)
        cams = [camera(c) for c in cameras]
        seeds = meta["seeds"] if seeds is None else list(seeds)
        settings = scene.settings if settings is None else settings
        W, H = (cams[0].image_width, cams[0].image_height) if cams else (0, 0)
        checkpoint.check_views_adaptive_compatible(meta, W, H, settings, seeds, [bytes(c) for c in cams])
        return cls(scene, cameras, seeds=seeds, settings=settings, _resume=(sums, state, meta), **kw)


def render_views_adaptive(scene, cameras, seeds=None, settings=None, num_gpus=1, tile=64, devices=None, rgb=True,
                          rgb8=False, maps=False, bvh="host"):
    """A batch of cameras under adaptive settings, run to the end in one call
    (ViewsAdaptiveRenderer): upload `scene`, run every round, free it.  Returns a dict: "rgb"
    [V,H,W,3] f32, "rgb8", the cumulative "counters", "info", and with maps=True "samples" and
    "rel_error" ([V,H,W])."""
    with ViewsAdaptiveRenderer(scene, cameras, seeds=seeds, settings=settings, num_gpus=num_gpus, tile=tile,
                               devices=devices, bvh=bvh) as r:
        res = r.render_rounds(r._info().max_rounds, rgb=rgb, rgb8=rgb8)
        res["counters"] = res["info"]["counters"]
        if maps:
            res["samples"], res["rel_error"] = r.sample_counts(), r.error_map()
        return res


def ppm_encode_async(d_rgb8, width, height, d_text, text_capacity, d_len, d_scratch, scratch_bytes, stream=0):
    """Format a device W*H*3 byte frame as the reference's PPM text on the device."""
    N.check(N.lib.gs_ppm_encode_async(C.c_void_p(d_rgb8), width, height, C.c_void_p(d_text), text_capacity,
                                      C.c_void_p(d_len), C.c_void_p(d_scratch), scratch_bytes, C.c_void_p(stream)))


def set_tuning(shade_batch=0, blocks_per_cu=0, leaf_batch=0, sample_chunk=-1):
    """Process-wide launch tuning (see gs_set_tuning in include/grayshift_gpu.h)."""
    N.check(N.lib.gs_set_tuning(shade_batch, blocks_per_cu, leaf_batch, sample_chunk))


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    N.check(N.lib.gs_host_write_ppm(path.encode(), rgb.shape[1], rgb.shape[0], rgb.ctypes.data))


class HostScene:
    """World + BVHNode::from_list + flat arrays, built by the C++ host mirror."""

    BVH = {"host": 0, "device": 1, "host-order": 2}  # ("host-order": the rebuild fed by the host, a test seam)

    def __init__(self, spec, bvh="host", device_min_members=0):
        """bvh: who builds the spec's BVHs (the world and each nested one): "host"
        (construct_tree) or "device" (gs_bvh_build_async on the current device for lists of
        at least device_min_members members, 0 = the measured default; the flat scene is
        byte-identical either way)."""
        if bvh not in self.BVH:
            raise ValueError("bvh must be 'host' or 'device', not %r" % (bvh,))
        self._spec = spec
        h = C.c_void_p()
        opt = N.gs_build_options(bvh=self.BVH[bvh], device_min_members=device_min_members)
        N.check(N.lib.gs_host_scene_from_spec_ex(spec.ptr(), C.byref(opt), C.byref(h)))
        self.handle = h
        self.flat_ptr = N.lib.gs_host_scene_flat(h)
        self.flat = N.gs_flat_scene.from_address(self.flat_ptr)

    def close(self):
        if self.handle:
            N.lib.gs_host_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: the binding may be gone)
            pass

    def build_info(self):
        """gs_build_info of this scene's build: BVHs built on the device / the host, members
        of the device-built ones, and the build's split in ms."""
        info = N.gs_build_info()
        N.check(N.lib.gs_host_scene_build_info(self.handle, C.byref(info)))
        return info.as_dict()

    def stats(self):
        f = self.flat
        return {"nodes": f.n_nodes, "spheres": f.n_spheres, "mspheres": f.n_mspheres, "quads": f.n_quads,
                "triangles": f.n_triangles, "lists": f.n_lists, "instances": f.n_instances,
                "materials": f.n_materials, "textures": f.n_textures, "max_bvh_depth": f.max_bvh_depth}


class Renderer:
    """A scene resident in HBM of the current device, rendered tile-partitioned."""

    def __init__(self, scene, rank=0, world_size=1, tile=64, tile_h=None, plan=False, plan_seed=1, order=None,
                 bvh="host"):
        """plan: cost-balanced tile assignment (gs_plan_tiles: a 1-spp pilot of the whole
        frame on this device) instead of round-robin.  order: a plan computed elsewhere
        (e.g. on rank 0 and broadcast: int32, slots_per_rank * world_size entries, see
        gs_partition.d_tile_order), used as given."""
        self.scene = scene
        self.host = HostScene(scene.spec, bvh=bvh)
        self.cam = camera(scene.camera)
        self.settings = scene.settings
        self.part = N.gs_partition(rank=rank, world_size=world_size, tile_w=tile, tile_h=tile_h or tile)
        self.order = None
        self.d_order = None
        d = C.c_void_p()
        N.check(N.lib.gs_device_scene_create(self.host.flat_ptr, C.byref(d)))
        self.dev = d
        if order is not None:
            self._use_order(np.ascontiguousarray(order, dtype=np.int32))
        elif plan:
            self._plan(plan_seed)
        self.capacity = N.lib.gs_partition_capacity(C.byref(self.cam), C.byref(self.part))
        if self.capacity < 0:
            raise ValueError("bad partition")

    def _plan(self, seed):
        p = self.part
        slots = C.c_int32()
        N.check(N.lib.gs_plan_tiles(self.dev, C.byref(self.cam), seed, p.world_size, p.tile_w, p.tile_h, None, 0,
                                    C.byref(slots)))
        order = np.zeros(slots.value * p.world_size, dtype=np.int32)
        N.check(N.lib.gs_plan_tiles(self.dev, C.byref(self.cam), seed, p.world_size, p.tile_w, p.tile_h,
                                    order.ctypes.data, order.size, C.byref(slots)))
        self._use_order(order)

    def _use_order(self, order):
        p = self.part
        if order.size % p.world_size:
            raise ValueError("tile order of %d entries for %d ranks" % (order.size, p.world_size))
        slots = order.size // p.world_size
        ids = np.sort(order[order >= 0])
        tx = (self.cam.image_width + p.tile_w - 1) // p.tile_w
        ty = (self.cam.image_height + p.tile_h - 1) // p.tile_h
        if not np.array_equal(ids, np.arange(tx * ty)):
            raise ValueError("tile order must hold every tile exactly once")
        d = C.c_void_p()
        N.check(N.lib.gs_device_alloc(order.nbytes, C.byref(d)))
        self.d_order = d
        N.check(N.lib.gs_device_upload(d, order.ctypes.data, order.nbytes))
        self.order = order
        p.d_tile_order = d.value
        p.slots_per_rank = slots

    @property
    def width(self):
        return self.cam.image_width

    @property
    def height(self):
        return self.cam.image_height

    def scene_info(self):
        """gs_device_scene_info as a dict (tree records, LDS mirror prefixes, kernel choices)."""
        i = N.gs_scene_info()
        N.check(N.lib.gs_device_scene_info(self.dev, C.byref(i)))
        return {k: getattr(i, k) for k, _ in N.gs_scene_info._fields_}

    def render_async(self, d_packed, d_counters=0, stream=0, seed=1):
        """d_packed: device pointer to capacity*3 f32; d_counters: device gs_counters or 0."""
        N.check(N.lib.gs_render_tiles_async(self.dev, C.byref(self.cam), C.byref(self.settings), seed,
                                            C.byref(self.part), C.c_void_p(d_packed), C.c_void_p(d_counters),
                                            C.c_void_p(stream)))

    def render_ex_async(self, d_rgb=0, d_rgb8=0, d_counters=0, stream=0, seed=1, d_item_visits=0):
        """Either or both outputs: d_rgb capacity*3 f32, d_rgb8 capacity*3 u8 (write_color bytes)."""
        o = N.gs_render_outputs(d_rgb or None, d_rgb8 or None, d_item_visits or None)
        N.check(N.lib.gs_render_tiles_ex_async(self.dev, C.byref(self.cam), C.byref(self.settings), seed,
                                               C.byref(self.part), C.byref(o), C.c_void_p(d_counters),
                                               C.c_void_p(stream)))

    def render_pass_async(self, samples, sample_base, d_sums, d_rgb=0, d_rgb8=0, d_counters=0, stream=0, seed=1,
                          chunk=0):
        """One progressive pass of this rank's tiles (gs_render_tiles_pass_async): samples
        [sample_base, sample_base + samples) are added to d_sums (device, capacity*3 f64, zeroed by
        the caller before the first pass) and d_sums / (sample_base + samples) is written to d_rgb
        (capacity*3 f32) and / or d_rgb8.  chunk: the coarse chunk, 0 = 16; samples and sample_base
        are multiples of it.  The scene's own SampleSettings are not used."""
        o = N.gs_render_outputs(d_rgb or None, d_rgb8 or None, None)
        N.check(N.lib.gs_render_tiles_pass_async(self.dev, C.byref(self.cam), samples, seed, C.byref(self.part),
                                                 sample_base, chunk, C.c_void_p(d_sums), C.byref(o),
                                                 C.c_void_p(d_counters), C.c_void_p(stream)))

    def round_state_bytes(self):
        """Bytes of the device blob render_rounds_async keeps this rank's round state in."""
        n = N.lib.gs_round_state_bytes(C.byref(self.cam), C.byref(self.part), C.byref(self.settings))
        if n < 0:
            raise ValueError("the scene's settings have no round form (max_samples < batch_size?)")
        return n

    def render_rounds_async(self, first_round, rounds, d_state, state_bytes, d_rgb=0, d_rgb8=0, d_samples=0,
                            d_rel_error=0, d_counters=0, stream=0, seed=1):
        """One progressive adaptive pass of this rank's tiles (gs_render_tiles_rounds_async) with the
        scene's own SampleSettings: rounds [first_round, first_round + rounds) on the round state in
        d_state (device, round_state_bytes(); first_round 0 initialises it), then every packed
        pixel's colour resolved into d_rgb (capacity*3 f32) and / or d_rgb8, and the maps into
        d_samples (capacity u32) / d_rel_error (capacity f32) when given."""
        o = N.gs_round_outputs(d_rgb or None, d_rgb8 or None, d_samples or None, d_rel_error or None)
        N.check(N.lib.gs_render_tiles_rounds_async(self.dev, C.byref(self.cam), C.byref(self.settings), seed,
                                                   C.byref(self.part), first_round, rounds, C.c_void_p(d_state),
                                                   state_bytes, C.byref(o), C.c_void_p(d_counters),
                                                   C.c_void_p(stream)))

    def unpack_u8_async(self, d_gathered, d_frame, world_size, stream=0):
        part = N.gs_partition(0, world_size, self.part.tile_w, self.part.tile_h, self.part.d_tile_order,
                              self.part.slots_per_rank, 0)
        N.check(N.lib.gs_unpack_tiles_part_async(C.byref(self.cam), C.byref(part), self.capacity,
                                                 C.c_void_p(d_gathered), C.c_void_p(d_frame), 3, C.c_void_p(stream)))

    def unpack_async(self, d_gathered, d_frame, world_size, stream=0):
        part = N.gs_partition(0, world_size, self.part.tile_w, self.part.tile_h, self.part.d_tile_order,
                              self.part.slots_per_rank, 0)
        N.check(N.lib.gs_unpack_tiles_part_async(C.byref(self.cam), C.byref(part), self.capacity,
                                                 C.c_void_p(d_gathered), C.c_void_p(d_frame), 12, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "d_order", None):
            N.lib.gs_device_free(self.d_order)
            self.d_order = None
        if getattr(self, "dev", None):
            N.lib.gs_device_scene_destroy(self.dev)
            self.dev = None
        if getattr(self, "host", None):
            self.host.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown: the binding may be gone)
            pass
