"""CPU tests of progressive adaptive passes: gs_render_tiles_rounds_async rejects bad arguments
before any device work, the frame-context calls reject a null context, gs_round_state_bytes
sizes the blob, and adaptive checkpoints (grayshift_amd.checkpoint, format 2, pure numpy)
round-trip exactly and reject every mismatch.  No compute on a device."""
import ctypes as C
import io

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import checkpoint, scenes
from grayshift_amd.scene import sample_settings

P = C.c_void_p
OK = P(0x1000)  # a non-null pointer that must never be followed
BIG = 1 << 40   # state_bytes no blob of these frames needs


@pytest.fixture(scope="module")
def cam():
    return g.camera(scenes.config("C4", width=64, spp=1).camera)


def _ss(batch=8, maxs=64, tol=0.05):
    return sample_settings(0.95, tol, batch, maxs)


def _rounds(cam, ss, first, rounds, scene=OK, part="ok", state=OK, state_bytes=BIG, outs="rgb"):
    part = {"ok": N.gs_partition(0, 1, 64, 64, None, 0, 0), "bad": N.gs_partition(2, 2, 64, 64, None, 0, 0),
            "null": None}[part]
    o = {"rgb": N.gs_round_outputs(0x2000, None, None, None), "rgb8": N.gs_round_outputs(None, 0x2000, None, None),
         "maps": N.gs_round_outputs(None, None, 0x2000, 0x3000), "null": None}[outs]
    return N.lib.gs_render_tiles_rounds_async(scene, C.byref(cam) if cam is not None else None,
                                              C.byref(ss) if ss is not None else None, 1,
                                              C.byref(part) if part is not None else None, first, rounds, state,
                                              state_bytes, C.byref(o) if o is not None else None, None, None)


def _err():
    return N.lib.gs_last_error()


def test_rounds_reject_bad_arguments_before_the_device(cam):
    """Every GS_ERR_ARG rule of gs_render_tiles_rounds_async, with pointers that would fault if
    they were followed and no device in the machine: the checks come before any device work."""
    ss = _ss()  # R = 64 / 8 + 1 = 9
    for kw in ({"scene": None}, {"part": "null"}, {"state": None}, {"outs": "null"}, {"outs": "maps"}):
        assert _rounds(cam, ss, 0, 1, **kw) == N.GS_ERR_ARG, kw
        assert b"null" in _err()
    assert _rounds(None, ss, 0, 1) == N.GS_ERR_ARG
    assert _rounds(cam, None, 0, 1) == N.GS_ERR_ARG
    assert _rounds(cam, ss, 0, 1, part="bad") == N.GS_ERR_ARG
    assert b"partition" in _err()
    assert _rounds(cam, ss, 0, 0) == N.GS_ERR_ARG
    assert b"0 rounds" in _err()
    assert _rounds(cam, _ss(batch=0), 0, 1) == N.GS_ERR_ARG
    assert b"batch_size 0" in _err()
    assert _rounds(cam, _ss(batch=8, maxs=7), 0, 1) == N.GS_ERR_ARG
    assert b"one batch" in _err() and b"gs_render_tiles_pass_async" in _err()
    assert _rounds(cam, _ss(batch=1, maxs=65536), 0, 1) == N.GS_ERR_ARG   # R = 65537
    assert b"65536" in _err()
    assert _rounds(cam, ss, 8, 2) == N.GS_ERR_ARG                         # 8 + 2 > 9
    assert b"first_round" in _err()
    assert _rounds(cam, ss, 9, 1) == N.GS_ERR_ARG
    assert _rounds(cam, ss, 0xFFFFFFFF, 2) == N.GS_ERR_ARG                # (no 32-bit wrap)
    need = N.lib.gs_round_state_bytes(C.byref(cam), C.byref(N.gs_partition(0, 1, 64, 64, None, 0, 0)), C.byref(ss))
    assert need > 0
    assert _rounds(cam, ss, 0, 1, state_bytes=need - 1) == N.GS_ERR_ARG
    assert b"state_bytes" in _err()
    assert _rounds(cam, ss, 0, 1, state_bytes=-1) == N.GS_ERR_ARG
    assert _rounds(cam, ss, 0, 1, outs="rgb8", state_bytes=0) == N.GS_ERR_ARG


def test_rounds_reject_a_batch_beyond_the_partial_budget(cam):
    """One pixel's batch of colours (batch_size * 24 bytes) against gs_debug_set_partial_budget."""
    ss = _ss(batch=8, maxs=64)
    N.check(N.lib.gs_debug_set_partial_budget(8 * 24 - 1))
    try:
        assert _rounds(cam, ss, 0, 1) == N.GS_ERR_ARG
        assert b"budget" in _err()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


def test_round_state_bytes(cam):
    """Monotonic in the capacity, at least 52 bytes per packed pixel (5 f64 sums, the batches
    word, two list entries), -1 for arguments and settings without a round form."""
    ss = _ss()
    sizes = []
    for world in (8, 4, 2, 1):  # rank 0 of 12 tiles of 16 x 16: 2, 3, 6, 12 tiles
        p = N.gs_partition(0, world, 16, 16, None, 0, 0)
        cap = N.lib.gs_partition_capacity(C.byref(cam), C.byref(p))
        n = N.lib.gs_round_state_bytes(C.byref(cam), C.byref(p), C.byref(ss))
        assert n >= 52 * cap
        sizes.append((cap, n))
    sizes.sort()
    assert all(a[1] <= b[1] for a, b in zip(sizes, sizes[1:])) and sizes[0][0] < sizes[-1][0]
    assert sizes[0][1] < sizes[-1][1]
    p = N.gs_partition(0, 1, 64, 64, None, 0, 0)
    more_rounds = N.lib.gs_round_state_bytes(C.byref(cam), C.byref(p), C.byref(_ss(batch=1, maxs=65535)))
    assert more_rounds >= N.lib.gs_round_state_bytes(C.byref(cam), C.byref(p), C.byref(ss))
    assert N.lib.gs_round_state_bytes(None, C.byref(p), C.byref(ss)) == -1
    assert N.lib.gs_round_state_bytes(C.byref(cam), C.byref(N.gs_partition(2, 2, 64, 64, None, 0, 0)), C.byref(ss)) == -1
    assert N.lib.gs_round_state_bytes(C.byref(cam), C.byref(p), C.byref(_ss(batch=8, maxs=7))) == -1
    assert N.lib.gs_round_state_bytes(C.byref(cam), C.byref(p), C.byref(_ss(batch=0))) == -1
    assert N.lib.gs_round_state_bytes(C.byref(cam), C.byref(p), C.byref(_ss(batch=1, maxs=65536))) == -1


def test_adaptation_calls_reject_a_null_context(cam):
    ss = _ss()
    st, info, cnt = N.gs_stats(), N.gs_adapt_info(), N.gs_counters()
    buf = np.zeros(16)
    assert N.lib.gs_multi_adapt_begin(None, C.byref(cam), C.byref(ss), 1) == N.GS_ERR_ARG
    assert N.lib.gs_multi_adapt_pass(None, 1, None, C.byref(st)) == N.GS_ERR_ARG
    assert b"null" in _err()
    assert N.lib.gs_multi_adapt_info(None, C.byref(info)) == N.GS_ERR_ARG
    assert N.lib.gs_multi_adapt_maps(None, buf.ctypes.data, buf.ctypes.data) == N.GS_ERR_ARG
    assert N.lib.gs_multi_adapt_download(None, buf.ctypes.data, buf.ctypes.data) == N.GS_ERR_ARG
    assert N.lib.gs_multi_adapt_upload(None, C.byref(cam), C.byref(ss), 1, 1, buf.ctypes.data, buf.ctypes.data,
                                       C.byref(cnt)) == N.GS_ERR_ARG
    assert N.lib.gs_multi_adapt_end(None) == N.GS_ERR_ARG


def test_struct_layouts_match():
    assert N.lib.gs_host_struct_size(b"gs_adapt_info") == C.sizeof(N.gs_adapt_info)
    assert N.lib.gs_host_struct_size(b"gs_round_outputs") == C.sizeof(N.gs_round_outputs)
    assert N.GS_ADAPT_STOPPED == checkpoint.STOPPED == 0x80000000
    assert N.lib.gs_version() == 11


def test_adaptive_renderer_is_exported():
    assert g.AdaptiveRenderer.__name__ == "AdaptiveRenderer"
    assert hasattr(g.Renderer, "render_rounds_async") and hasattr(g.Renderer, "round_state_bytes")
    for name in ("render_rounds", "render_until", "info", "finished", "sample_counts", "error_map", "state",
                 "frame_ptr", "save", "resume", "close", "__enter__", "__exit__"):
        assert hasattr(g.AdaptiveRenderer, name), name


@pytest.mark.parametrize("name", ["gs_adapt_info", "gs_round_outputs"])
def test_rust_binding_declares_the_adaptation_structs(name):
    """The structs' fields, in the header's order, in bindings/grayshift_gpu.rs and in _native."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "grayshift_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    c_names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
               for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    rs = re.search(r"pub struct %s \{(.*?)\}" % name, open(os.path.join(root, "bindings", "grayshift_gpu.rs")).read(),
                   re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+)\s*:", rs) == c_names
    assert c_names == [n for n, _ in getattr(N, name)._fields_]


# ------------------------------------------------------------------ checkpoints (format 2)
ROUNDS = 3


def _meta(cam, **kw):
    m = {"rounds": ROUNDS, "seed": 2 ** 63 + 5, "width": cam.image_width, "height": cam.image_height,
         "confidence": 0.95, "tolerance": 0.1 + 0.2, "batch_size": 8, "max_samples": 64, "camera": bytes(cam),
         "counters": {n: 2 ** 40 + k for k, n in enumerate(checkpoint.COUNTER_NAMES)}}
    m.update(kw)
    return m


def _state(cam):
    rng = np.random.default_rng(11)
    h, w = cam.image_height, cam.image_width
    sums = rng.standard_normal((h, w, 5)) * 1e3
    sums[0, 0] = [0.0, -0.0, 5e-324, np.nan, np.inf]  # signed zero, a denormal, NaN and inf survive
    sums[1, 1, 4] = -np.inf
    taken = rng.integers(1, ROUNDS + 1, size=(h, w)).astype(np.uint32)
    stopped = rng.random((h, w)) < 0.5
    state = np.where(stopped, taken | np.uint32(checkpoint.STOPPED), np.uint32(ROUNDS)).astype(np.uint32)
    return sums, state


def test_adaptive_checkpoint_round_trip_is_exact(cam, tmp_path):
    sums, state = _state(cam)
    meta = _meta(cam)
    path = str(tmp_path / "frame.ackpt")  # (written under the name as given)
    checkpoint.write_adaptive_checkpoint(path, sums, state, meta)
    s2, st2, m2 = checkpoint.read_adaptive_checkpoint(path)
    assert s2.dtype == np.float64 and s2.tobytes() == sums.tobytes()   # bytes: NaN payloads too
    assert st2.dtype == np.uint32 and np.array_equal(st2, state)
    assert m2 == meta
    ss = sample_settings(0.95, 0.1 + 0.2, 8, 64)
    checkpoint.check_adaptive_compatible(m2, cam.image_width, cam.image_height, ss, 2 ** 63 + 5, bytes(cam))
    f = io.BytesIO()  # a file object works as well
    checkpoint.write_adaptive_checkpoint(f, sums, state, meta)
    f.seek(0)
    assert checkpoint.read_adaptive_checkpoint(f)[0].tobytes() == sums.tobytes()


@pytest.mark.parametrize("field", ["width", "height", "seed", "confidence", "tolerance", "batch_size", "max_samples",
                                   "camera"])
def test_adaptive_checkpoint_mismatch_is_rejected(cam, field):
    meta = _meta(cam)
    want = {"width": cam.image_width, "height": cam.image_height, "seed": 2 ** 63 + 5, "camera": bytes(cam),
            "settings": {"confidence": 0.95, "tolerance": 0.1 + 0.2, "batch_size": 8, "max_samples": 64}}
    checkpoint.check_adaptive_compatible(meta, **want)
    if field == "camera":
        other = g.camera(scenes.config("C4", width=64, spp=1).camera)
        other.center[0] += 1e-9
        want["camera"] = bytes(other)
    elif field in want["settings"]:
        v = want["settings"][field]
        want["settings"][field] = np.nextafter(v, 1.0) if isinstance(v, float) else v + 1
    else:
        want[field] += 1
    with pytest.raises(checkpoint.CheckpointError) as e:
        checkpoint.check_adaptive_compatible(meta, **want)
    assert field in str(e.value)


def test_adaptive_checkpoint_rejects_malformed_input(cam, tmp_path):
    sums, state = _state(cam)
    meta = _meta(cam)
    bad = [(sums[:-1], state, meta), (sums[..., :3], state, meta), (sums, state[:-1], meta),
           (sums, state, _meta(cam, max_samples=7)),          # not adaptive
           (sums, state, _meta(cam, rounds=10)),              # R = 9
           (sums, state, _meta(cam, rounds=2)),               # active pixels have taken 3
           (sums, state, {k: v for k, v in meta.items() if k != "tolerance"})]
    for k, (s, st, m) in enumerate(bad):
        with pytest.raises(checkpoint.CheckpointError):
            checkpoint.write_adaptive_checkpoint(str(tmp_path / ("bad%d" % k)), s, st, m)
    ahead = state.copy()
    ahead[2, 2] = np.uint32(checkpoint.STOPPED | (ROUNDS + 1))  # stopped after a round not yet run
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_adaptive_checkpoint(str(tmp_path / "ahead"), sums, ahead, meta)
    np.savez(str(tmp_path / "d.npz"), sums=sums, state=state)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.read_adaptive_checkpoint(str(tmp_path / "d.npz"))


def test_the_two_formats_reject_each_others_files(cam, tmp_path):
    sums, state = _state(cam)
    a = str(tmp_path / "adaptive")
    checkpoint.write_adaptive_checkpoint(a, sums, state, _meta(cam))
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.read_checkpoint(a)
    f = str(tmp_path / "fixed")
    checkpoint.write_checkpoint(f, np.zeros((cam.image_height, cam.image_width, 3)),
                                {"samples": 16, "seed": 1, "chunk": 16, "width": cam.image_width,
                                 "height": cam.image_height, "camera": bytes(cam),
                                 "counters": {n: 0 for n in checkpoint.COUNTER_NAMES}})
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.read_adaptive_checkpoint(f)
    assert checkpoint.FORMAT == 1 and checkpoint.ADAPTIVE_FORMAT == 2
