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
