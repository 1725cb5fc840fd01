"""Checkpoints of a progressive render: one ``.npz`` holding the frame's running sums and what
they are sums of.  Pure numpy: nothing here loads the native library or touches a device.

A checkpoint holds

* ``sums``     -- [H, W, 3] f64, Σ of the samples' colours per pixel, in image order (so a frame
  saved on N GPUs resumes on M);
* ``samples``, ``seed``, ``chunk``, ``width``, ``height`` -- the samples per pixel in the sums,
  the RNG seed, the coarse sample chunk and the frame size;
* ``camera``   -- the bytes of the ``gs_camera`` the frame is rendered with;
* ``counters`` -- the cumulative work counters, in ``COUNTER_NAMES`` order;
* ``passes``, ``last_delta`` -- how many passes produced it and the last pass's change.

``check_compatible`` compares size, chunk, seed and camera bytes with the scene a caller wants to
resume on.  Scene identity beyond that -- the world's objects, materials, textures, background --
is the caller's responsibility: a checkpoint does not fingerprint the world, and resuming it on
another world with the same camera silently mixes two images.

An adaptive frame in progress (``AdaptiveRenderer``) is format ``ADAPTIVE_FORMAT`` (2):

* ``sums``  -- [H, W, 5] f64: Σr, Σg, Σb, Σlum, Σlum² per pixel, in image order;
* ``state`` -- [H, W] u32: batches taken, the top bit set once the pixel has stopped;
* ``rounds``, ``seed``, ``width``, ``height`` -- the rounds run, the RNG seed, the frame size;
* ``confidence``, ``tolerance``, ``batch_size``, ``max_samples`` -- the SampleSettings;
* ``camera``, ``counters`` -- as above.

``read_checkpoint`` rejects it, and ``read_adaptive_checkpoint`` rejects format 1: neither
renderer can resume the other's file.  A batch of views in progress (``ViewsProgressiveRenderer``)
is format ``VIEWS_FORMAT`` (3), described with its functions below; its reader rejects formats 1
and 2, and their readers reject it.  A batch of views under adaptive settings in progress
(``ViewsAdaptiveRenderer``) is format ``VIEWS_ADAPTIVE_FORMAT`` (4), at the end of this file;
its reader rejects formats 1 to 3, and their readers reject it.
"""
import numpy as np

FORMAT = 1
COUNTER_NAMES = ["rays", "node_visits", "sphere_tests", "msphere_tests", "quad_tests", "tri_tests",
                 "instance_tests", "list_tests", "hits", "image_texels", "hdri_texels", "paths", "pixels",
                 "medium_tests", "noise_evals"]
REQUIRED = ("samples", "seed", "chunk", "width", "height", "camera", "counters")


class CheckpointError(ValueError):
    pass


def write_checkpoint(path, sums, meta):
    """Write `sums` ([H, W, 3] f64) and `meta` to `path` (a file name, used as given, or a file
    object).  meta: samples, seed, chunk, width, height (ints), camera (bytes), counters (a dict
    by COUNTER_NAMES); optional passes (int) and last_delta (float)."""
    for k in REQUIRED:
        if k not in meta:
            raise CheckpointError("checkpoint meta lacks %r" % k)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    h, w = int(meta["height"]), int(meta["width"])
    if sums.shape != (h, w, 3):
        raise CheckpointError("sums of shape %r for a %d x %d frame" % (sums.shape, w, h))
    chunk, samples = int(meta["chunk"]), int(meta["samples"])
    if chunk <= 0 or samples < 0 or samples % chunk:
        raise CheckpointError("samples %d are not whole chunks of %d" % (samples, chunk))
    counters = np.array([int(meta["counters"][n]) for n in COUNTER_NAMES], dtype=np.uint64)
    fields = dict(format=np.int64(FORMAT), sums=sums, samples=np.uint64(samples), seed=np.uint64(int(meta["seed"])),
                  chunk=np.uint32(chunk), width=np.int32(w), height=np.int32(h),
                  camera=np.frombuffer(bytes(meta["camera"]), dtype=np.uint8), counters=counters,
                  passes=np.uint32(int(meta.get("passes", 0))), last_delta=np.float64(meta.get("last_delta", 0.0)))
    if hasattr(path, "write"):
        np.savez(path, **fields)
    else:
        with open(path, "wb") as f:  # (the name as given: numpy would add ".npz" to it)
            np.savez(f, **fields)


def read_checkpoint(path):
    """-> (sums [H, W, 3] f64, meta) as write_checkpoint took them."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != FORMAT:
            raise CheckpointError("not a grayshift checkpoint of format %d" % FORMAT)
        for k in REQUIRED + ("sums",):
            if k not in z.files:
                raise CheckpointError("checkpoint lacks %r" % k)
        sums = np.ascontiguousarray(z["sums"], dtype=np.float64)
        meta = {"samples": int(z["samples"]), "seed": int(z["seed"]), "chunk": int(z["chunk"]),
                "width": int(z["width"]), "height": int(z["height"]), "camera": z["camera"].tobytes(),
                "counters": {n: int(v) for n, v in zip(COUNTER_NAMES, z["counters"])},
                "passes": int(z["passes"]) if "passes" in z.files else 0,
                "last_delta": float(z["last_delta"]) if "last_delta" in z.files else 0.0}
    if sums.shape != (meta["height"], meta["width"], 3):
        raise CheckpointError("sums of shape %r for a %d x %d frame" % (sums.shape, meta["width"], meta["height"]))
    if meta["chunk"] <= 0 or meta["samples"] % meta["chunk"]:
        raise CheckpointError("samples %d are not whole chunks of %d" % (meta["samples"], meta["chunk"]))
    return sums, meta


def check_compatible(meta, width, height, chunk, seed, camera):
    """Raise CheckpointError unless the checkpoint's size, chunk, seed and camera bytes are the
    ones given (the scene's a caller resumes on).  The world itself is not compared."""
    for name, have, want in (("width", meta["width"], int(width)), ("height", meta["height"], int(height)),
                             ("chunk", meta["chunk"], int(chunk)), ("seed", meta["seed"], int(seed))):
        if have != want:
            raise CheckpointError("checkpoint %s %d differs from the scene's %d" % (name, have, want))
    if bytes(meta["camera"]) != bytes(camera):
        raise CheckpointError("checkpoint camera differs from the scene's")


# ------------------------------------------------------------------ adaptive frames (format 2)
ADAPTIVE_FORMAT = 2
STOPPED = 0x80000000
SETTINGS = ("confidence", "tolerance", "batch_size", "max_samples")
ADAPTIVE_REQUIRED = ("rounds", "seed", "width", "height", "camera", "counters") + SETTINGS


def _check_adaptive(sums, state, meta):
    h, w = meta["height"], meta["width"]
    if sums.shape != (h, w, 5):
        raise CheckpointError("sums of shape %r for a %d x %d adaptive frame" % (sums.shape, w, h))
    if state.shape != (h, w):
        raise CheckpointError("state of shape %r for a %d x %d frame" % (state.shape, w, h))
    bs, ms = meta["batch_size"], meta["max_samples"]
    if bs <= 0 or ms < bs:
        raise CheckpointError("settings with batch_size %d, max_samples %d are not adaptive" % (bs, ms))
    if not 0 <= meta["rounds"] <= ms // bs + 1:
        raise CheckpointError("rounds %d outside the settings' %d" % (meta["rounds"], ms // bs + 1))
    taken = state & np.uint32(STOPPED - 1)
    stopped = (state & np.uint32(STOPPED)) != 0
    if np.any(taken[~stopped] != meta["rounds"]) or np.any(taken[stopped] > meta["rounds"]) or \
            np.any(taken[stopped] < 1):
        raise CheckpointError("a pixel's state disagrees with %d rounds" % meta["rounds"])


def write_adaptive_checkpoint(path, sums, state, meta):
    """Write `sums` ([H, W, 5] f64), `state` ([H, W] u32) and `meta` to `path` (a file name, used as
    given, or a file object).  meta: rounds, seed, width, height, batch_size, max_samples (ints),
    confidence, tolerance (floats), camera (bytes), counters (a dict by COUNTER_NAMES)."""
    for k in ADAPTIVE_REQUIRED:
        if k not in meta:
            raise CheckpointError("checkpoint meta lacks %r" % k)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    state = np.ascontiguousarray(state, dtype=np.uint32)
    m = {k: int(meta[k]) for k in ("rounds", "seed", "width", "height", "batch_size", "max_samples")}
    _check_adaptive(sums, state, m)
    counters = np.array([int(meta["counters"][n]) for n in COUNTER_NAMES], dtype=np.uint64)
    fields = dict(format=np.int64(ADAPTIVE_FORMAT), sums=sums, state=state, rounds=np.uint32(m["rounds"]),
                  seed=np.uint64(m["seed"]), width=np.int32(m["width"]), height=np.int32(m["height"]),
                  confidence=np.float64(meta["confidence"]), tolerance=np.float64(meta["tolerance"]),
                  batch_size=np.uint32(m["batch_size"]), max_samples=np.uint32(m["max_samples"]),
                  camera=np.frombuffer(bytes(meta["camera"]), dtype=np.uint8), counters=counters)
    if hasattr(path, "write"):
        np.savez(path, **fields)
    else:
        with open(path, "wb") as f:  # (the name as given: numpy would add ".npz" to it)
            np.savez(f, **fields)


def read_adaptive_checkpoint(path):
    """-> (sums [H, W, 5] f64, state [H, W] u32, meta) as write_adaptive_checkpoint took them."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != ADAPTIVE_FORMAT:
            raise CheckpointError("not a grayshift adaptive checkpoint (format %d)" % ADAPTIVE_FORMAT)
        for k in ADAPTIVE_REQUIRED + ("sums", "state"):
            if k not in z.files:
                raise CheckpointError("checkpoint lacks %r" % k)
        sums = np.ascontiguousarray(z["sums"], dtype=np.float64)
        state = np.ascontiguousarray(z["state"], dtype=np.uint32)
        meta = {"rounds": int(z["rounds"]), "seed": int(z["seed"]), "width": int(z["width"]),
                "height": int(z["height"]), "confidence": float(z["confidence"]), "tolerance": float(z["tolerance"]),
                "batch_size": int(z["batch_size"]), "max_samples": int(z["max_samples"]),
                "camera": z["camera"].tobytes(),
                "counters": {n: int(v) for n, v in zip(COUNTER_NAMES, z["counters"])}}
    _check_adaptive(sums, state, meta)
    return sums, state, meta


def check_adaptive_compatible(meta, width, height, settings, seed, camera):
    """Raise CheckpointError unless the checkpoint's size, seed, camera bytes and the four
    SampleSettings fields are the ones given.  settings: an object with confidence, tolerance,
    batch_size and max_samples (a gs_sample_settings), or a dict of them.  Floats compare by
    value of the f64; the world itself is not compared."""
    def get(k):
        return settings[k] if isinstance(settings, dict) else getattr(settings, k)
    for name, have, want in (("width", meta["width"], int(width)), ("height", meta["height"], int(height)),
                             ("seed", meta["seed"], int(seed)),
                             ("batch_size", meta["batch_size"], int(get("batch_size"))),
                             ("max_samples", meta["max_samples"], int(get("max_samples")))):
        if have != want:
            raise CheckpointError("checkpoint %s %d differs from the scene's %d" % (name, have, want))
    for name in ("confidence", "tolerance"):
        if np.float64(meta[name]).tobytes() != np.float64(get(name)).tobytes():
            raise CheckpointError("checkpoint %s %r differs from the scene's %r" % (name, meta[name], get(name)))
    if bytes(meta["camera"]) != bytes(camera):
        raise CheckpointError("checkpoint camera differs from the scene's")


# ------------------------------------------------------------------ progressive views (format 3)
# A batch of views in progress (``ViewsProgressiveRenderer``):
#
# * ``sums``     -- [V, H, W, 3] f64, Σ of the samples' colours per pixel of every view, image order;
# * ``samples``  -- [V] u32, the samples per pixel in each view's sums (whole chunks; they may differ);
# * ``seeds``    -- [V] u64, the views' RNG seeds;
# * ``cameras``  -- [V, sizeof(gs_camera)] u8, the bytes of each view's ``gs_camera``;
# * ``chunk``, ``width``, ``height`` -- the coarse sample chunk and the size of one view;
# * ``counters`` -- the cumulative work counters, in ``COUNTER_NAMES`` order;
# * ``passes``, ``deltas`` ([V] f64) -- how many passes produced it and each view's last change.
#
# The three readers reject each other's files.
VIEWS_FORMAT = 3
VIEWS_REQUIRED = ("samples", "seeds", "cameras", "chunk", "width", "height", "counters")


def _check_views(sums, meta):
    v, h, w = len(meta["samples"]), meta["height"], meta["width"]
    if v == 0:
        raise CheckpointError("a views checkpoint of 0 views")
    if sums.shape != (v, h, w, 3):
        raise CheckpointError("sums of shape %r for %d views of %d x %d" % (sums.shape, v, w, h))
    if len(meta["seeds"]) != v or len(meta["cameras"]) != v:
        raise CheckpointError("%d sample counts, %d seeds, %d cameras" % (v, len(meta["seeds"]), len(meta["cameras"])))
    if len({len(c) for c in meta["cameras"]}) != 1:
        raise CheckpointError("cameras of different byte lengths")
    if meta["chunk"] <= 0 or any(n < 0 or n % meta["chunk"] for n in meta["samples"]):
        raise CheckpointError("samples %r are not whole chunks of %d" % (list(meta["samples"]), meta["chunk"]))


def write_views_checkpoint(path, sums, meta):
    """Write `sums` ([V, H, W, 3] f64) and `meta` to `path` (a file name, used as given, or a file
    object).  meta: samples, seeds (V ints each), cameras (V byte strings), chunk, width, height
    (ints), counters (a dict by COUNTER_NAMES); optional passes (int) and deltas (V floats)."""
    for k in VIEWS_REQUIRED:
        if k not in meta:
            raise CheckpointError("checkpoint meta lacks %r" % k)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    m = {"samples": [int(n) for n in meta["samples"]], "seeds": [int(s) for s in meta["seeds"]],
         "cameras": [bytes(c) for c in meta["cameras"]], "chunk": int(meta["chunk"]), "width": int(meta["width"]),
         "height": int(meta["height"])}
    _check_views(sums, m)
    v = len(m["samples"])
    deltas = np.array(list(meta.get("deltas", [0.0] * v)), dtype=np.float64)
    if deltas.shape != (v,):
        raise CheckpointError("%d deltas for %d views" % (deltas.size, v))
    counters = np.array([int(meta["counters"][n]) for n in COUNTER_NAMES], dtype=np.uint64)
    fields = dict(format=np.int64(VIEWS_FORMAT), sums=sums, samples=np.array(m["samples"], dtype=np.uint32),
                  seeds=np.array(m["seeds"], dtype=np.uint64),
                  cameras=np.frombuffer(b"".join(m["cameras"]), dtype=np.uint8).reshape(v, -1),
                  chunk=np.uint32(m["chunk"]), width=np.int32(m["width"]), height=np.int32(m["height"]),
                  counters=counters, passes=np.uint32(int(meta.get("passes", 0))), deltas=deltas)
    if hasattr(path, "write"):
        np.savez(path, **fields)
    else:
        with open(path, "wb") as f:  # (the name as given: numpy would add ".npz" to it)
            np.savez(f, **fields)


def read_views_checkpoint(path):
    """-> (sums [V, H, W, 3] f64, meta) as write_views_checkpoint took them."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != VIEWS_FORMAT:
            raise CheckpointError("not a grayshift views checkpoint (format %d)" % VIEWS_FORMAT)
        for k in VIEWS_REQUIRED + ("sums",):
            if k not in z.files:
                raise CheckpointError("checkpoint lacks %r" % k)
        sums = np.ascontiguousarray(z["sums"], dtype=np.float64)
        cams = np.ascontiguousarray(z["cameras"], dtype=np.uint8)
        if cams.ndim != 2:
            raise CheckpointError("cameras of shape %r" % (cams.shape,))
        meta = {"samples": [int(n) for n in z["samples"]], "seeds": [int(s) for s in z["seeds"]],
                "cameras": [c.tobytes() for c in cams], "chunk": int(z["chunk"]), "width": int(z["width"]),
                "height": int(z["height"]), "counters": {n: int(v) for n, v in zip(COUNTER_NAMES, z["counters"])},
                "passes": int(z["passes"]) if "passes" in z.files else 0}
        meta["deltas"] = [float(d) for d in z["deltas"]] if "deltas" in z.files else [0.0] * len(meta["samples"])
    _check_views(sums, meta)
    if len(meta["deltas"]) != len(meta["samples"]):
        raise CheckpointError("%d deltas for %d views" % (len(meta["deltas"]), len(meta["samples"])))
    return sums, meta


def check_views_compatible(meta, width, height, chunk, seeds, cameras, samples=None):
    """Raise CheckpointError unless the checkpoint's view count, size, chunk, seeds and camera bytes
    are the ones given (the batch a caller resumes on) -- and, when `samples` is given, its per-view
    sample vector too.  The world itself is not compared."""
    seeds, cameras = [int(s) for s in seeds], [bytes(c) for c in cameras]
    if len(meta["samples"]) != len(cameras) or len(seeds) != len(cameras):
        raise CheckpointError("checkpoint of %d views, a batch of %d cameras and %d seeds" %
                              (len(meta["samples"]), len(cameras), len(seeds)))
    for name, have, want in (("width", meta["width"], int(width)), ("height", meta["height"], int(height)),
                             ("chunk", meta["chunk"], int(chunk))):
        if have != want:
            raise CheckpointError("checkpoint %s %d differs from the batch's %d" % (name, have, want))
    for v, (have, want) in enumerate(zip(meta["seeds"], seeds)):
        if have != want:
            raise CheckpointError("checkpoint seed %d of view %d differs from the batch's %d" % (have, v, want))
    for v, (have, want) in enumerate(zip(meta["cameras"], cameras)):
        if have != want:
            raise CheckpointError("checkpoint camera of view %d differs from the batch's" % v)
    if samples is not None and [int(n) for n in samples] != list(meta["samples"]):
        raise CheckpointError("checkpoint samples %r differ from %r" % (list(meta["samples"]), [int(n) for n in samples]))


# ------------------------------------------------------------------ adaptive views (format 4)
# A batch of views under adaptive settings in progress (``ViewsAdaptiveRenderer``):
#
# * ``sums``    -- [V, H, W, 5] f64: Σr, Σg, Σb, Σlum, Σlum² per pixel of every view, image order;
# * ``state``   -- [V, H, W] u32: batches taken, the top bit set once the pixel has stopped;
# * ``rounds``  -- the rounds run (one count for the batch: every active pixel takes every round);
# * ``seeds``   -- [V] u64; ``cameras`` -- [V, sizeof(gs_camera)] u8;
# * ``width``, ``height`` -- the size of one view;
# * ``confidence``, ``tolerance``, ``batch_size``, ``max_samples`` -- the batch's one SampleSettings;
# * ``counters`` -- the cumulative work counters, in ``COUNTER_NAMES`` order.
#
# Its reader rejects formats 1 to 3, and their readers reject it.
VIEWS_ADAPTIVE_FORMAT = 4
VIEWS_ADAPTIVE_REQUIRED = ("rounds", "seeds", "cameras", "width", "height", "counters") + SETTINGS


def _check_views_adaptive(sums, state, meta):
    v, h, w = len(meta["seeds"]), meta["height"], meta["width"]
    if v == 0:
        raise CheckpointError("a views checkpoint of 0 views")
    if len(meta["cameras"]) != v:
        raise CheckpointError("%d seeds, %d cameras" % (v, len(meta["cameras"])))
    if len({len(c) for c in meta["cameras"]}) != 1:
        raise CheckpointError("cameras of different byte lengths")
    if sums.shape != (v, h, w, 5) or state.shape != (v, h, w):
        raise CheckpointError("sums of shape %r, state of shape %r for %d adaptive views of %d x %d" %
                              (sums.shape, state.shape, v, w, h))
    # (the per-pixel rules are format 2's, on the tall frame)
    _check_adaptive(sums.reshape(v * h, w, 5), state.reshape(v * h, w), dict(meta, height=v * h))


def write_views_adaptive_checkpoint(path, sums, state, meta):
    """Write `sums` ([V, H, W, 5] f64), `state` ([V, H, W] u32) and `meta` to `path` (a file name,
    used as given, or a file object).  meta: rounds, width, height, batch_size, max_samples (ints),
    confidence, tolerance (floats), seeds (V ints), cameras (V byte strings), counters (a dict by
    COUNTER_NAMES)."""
    for k in VIEWS_ADAPTIVE_REQUIRED:
        if k not in meta:
            raise CheckpointError("checkpoint meta lacks %r" % k)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    state = np.ascontiguousarray(state, dtype=np.uint32)
    m = {k: int(meta[k]) for k in ("rounds", "width", "height", "batch_size", "max_samples")}
    m["seeds"] = [int(s) for s in meta["seeds"]]
    m["cameras"] = [bytes(c) for c in meta["cameras"]]
    _check_views_adaptive(sums, state, m)
    v = len(m["seeds"])
    counters = np.array([int(meta["counters"][n]) for n in COUNTER_NAMES], dtype=np.uint64)
    fields = dict(format=np.int64(VIEWS_ADAPTIVE_FORMAT), sums=sums, state=state, rounds=np.uint32(m["rounds"]),
                  seeds=np.array(m["seeds"], dtype=np.uint64),
                  cameras=np.frombuffer(b"".join(m["cameras"]), dtype=np.uint8).reshape(v, -1),
                  width=np.int32(m["width"]), height=np.int32(m["height"]),
                  confidence=np.float64(meta["confidence"]), tolerance=np.float64(meta["tolerance"]),
                  batch_size=np.uint32(m["batch_size"]), max_samples=np.uint32(m["max_samples"]), counters=counters)
    if hasattr(path, "write"):
        np.savez(path, **fields)
    else:
        with open(path, "wb") as f:  # (the name as given: numpy would add ".npz" to it)
            np.savez(f, **fields)


def read_views_adaptive_checkpoint(path):
    """-> (sums [V, H, W, 5] f64, state [V, H, W] u32, meta) as write_views_adaptive_checkpoint took
    them."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != VIEWS_ADAPTIVE_FORMAT:
            raise CheckpointError("not a grayshift adaptive views checkpoint (format %d)" % VIEWS_ADAPTIVE_FORMAT)
        for k in VIEWS_ADAPTIVE_REQUIRED + ("sums", "state"):
            if k not in z.files:
                raise CheckpointError("checkpoint lacks %r" % k)
        sums = np.ascontiguousarray(z["sums"], dtype=np.float64)
        state = np.ascontiguousarray(z["state"], dtype=np.uint32)
        cams = np.ascontiguousarray(z["cameras"], dtype=np.uint8)
        if cams.ndim != 2:
            raise CheckpointError("cameras of shape %r" % (cams.shape,))
        meta = {"rounds": int(z["rounds"]), "seeds": [int(s) for s in z["seeds"]],
                "cameras": [c.tobytes() for c in cams], "width": int(z["width"]), "height": int(z["height"]),
                "confidence": float(z["confidence"]), "tolerance": float(z["tolerance"]),
                "batch_size": int(z["batch_size"]), "max_samples": int(z["max_samples"]),
                "counters": {n: int(v) for n, v in zip(COUNTER_NAMES, z["counters"])}}
    _check_views_adaptive(sums, state, meta)
    return sums, state, meta


def check_views_adaptive_compatible(meta, width, height, settings, seeds, cameras):
    """Raise CheckpointError unless the checkpoint's view count, view size, seeds, camera bytes and
    the four SampleSettings fields are the ones given (the batch a caller resumes on).  settings: as
    for check_adaptive_compatible.  The world itself is not compared."""
    def get(k):
        return settings[k] if isinstance(settings, dict) else getattr(settings, k)
    seeds, cameras = [int(s) for s in seeds], [bytes(c) for c in cameras]
    if len(meta["seeds"]) != len(cameras) or len(seeds) != len(cameras):
        raise CheckpointError("checkpoint of %d views, a batch of %d cameras and %d seeds" %
                              (len(meta["seeds"]), len(cameras), len(seeds)))
    for name, have, want in (("width", meta["width"], int(width)), ("height", meta["height"], int(height)),
                             ("batch_size", meta["batch_size"], int(get("batch_size"))),
                             ("max_samples", meta["max_samples"], int(get("max_samples")))):
        if have != want:
            raise CheckpointError("checkpoint %s %d differs from the batch's %d" % (name, have, want))
    for name in ("confidence", "tolerance"):
        if np.float64(meta[name]).tobytes() != np.float64(get(name)).tobytes():
            raise CheckpointError("checkpoint %s %r differs from the batch's %r" % (name, meta[name], get(name)))
    for v, (have, want) in enumerate(zip(meta["seeds"], seeds)):
        if have != want:
            raise CheckpointError("checkpoint seed %d of view %d differs from the batch's %d" % (have, v, want))
    for v, (have, want) in enumerate(zip(meta["cameras"], cameras)):
        if have != want:
            raise CheckpointError("checkpoint camera of view %d differs from the batch's" % v)
