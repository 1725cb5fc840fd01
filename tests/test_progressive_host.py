"""CPU tests of progressive rendering: the pass entry points reject bad arguments before any
device work, and checkpoints (grayshift_amd.checkpoint, pure numpy) round-trip exactly and
reject every mismatch.  No compute on a device."""
import ctypes as C
import io

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import checkpoint, scenes

P = C.c_void_p
OK = P(0x1000)  # a non-null pointer that must never be followed


def _pass(cam, samples, base, chunk, scene=OK, part=None, sums=OK, outs="rgb"):
    part = part if part is not None else N.gs_partition(0, 1, 64, 64, None, 0, 0)
    o = {"rgb": N.gs_render_outputs(0x2000, None, None), "none": N.gs_render_outputs(None, None, None),
         "null": None}[outs]
    return N.lib.gs_render_tiles_pass_async(scene, C.byref(cam) if cam is not None else None, samples, 1,
                                            C.byref(part), base, chunk, sums, C.byref(o) if o is not None else None,
                                            None, None)


@pytest.fixture(scope="module")
def cam():
    return g.camera(scenes.config("C4", width=64, spp=1).camera)


def test_pass_rejects_bad_arguments_before_the_device(cam):
    """Every GS_ERR_ARG rule of gs_render_tiles_pass_async, with a scene pointer that would fault
    if it were read and no device in the machine: the checks come before any device work."""
    assert _pass(cam, 0, 0, 4) == N.GS_ERR_ARG
    assert b"0 samples" in N.lib.gs_last_error()
    assert _pass(cam, 6, 0, 4) == N.GS_ERR_ARG          # samples % c
    assert b"multiple" in N.lib.gs_last_error()
    assert _pass(cam, 24, 0, 0) == N.GS_ERR_ARG         # chunk 0 means 16
    assert _pass(cam, 8, 6, 4) == N.GS_ERR_ARG          # sample_base % c
    assert b"sample_base" in N.lib.gs_last_error()
    assert _pass(cam, 65 * 4, 0, 4) == N.GS_ERR_ARG     # samples / c > 64
    assert b"64 chunks" in N.lib.gs_last_error()
    assert _pass(cam, 16, 0xFFFFFFF0, 16) == N.GS_ERR_ARG  # sample_base + samples overflows u32
    assert b"overflows" in N.lib.gs_last_error()
    # null pointers: scene, camera, sums, outputs, both outputs null
    assert _pass(cam, 8, 0, 4, scene=None) == N.GS_ERR_ARG
    assert _pass(None, 8, 0, 4) == N.GS_ERR_ARG
    assert _pass(cam, 8, 0, 4, sums=None) == N.GS_ERR_ARG
    assert _pass(cam, 8, 0, 4, outs="null") == N.GS_ERR_ARG
    assert _pass(cam, 8, 0, 4, outs="none") == N.GS_ERR_ARG
    assert b"null" in N.lib.gs_last_error()
    assert N.lib.gs_render_tiles_pass_async(OK, C.byref(cam), 8, 1, None, 0, 4, OK,
                                            C.byref(N.gs_render_outputs(0x2000, None, None)), None,
                                            None) == N.GS_ERR_ARG
    # a bad partition
    assert _pass(cam, 8, 0, 4, part=N.gs_partition(2, 2, 64, 64, None, 0, 0)) == N.GS_ERR_ARG


def test_pass_rejects_chunk_sums_beyond_the_partial_budget(cam):
    """capacity * (samples / c) * 24 bytes against the budget (gs_debug_set_partial_budget)."""
    cap = N.lib.gs_partition_capacity(C.byref(cam), C.byref(N.gs_partition(0, 1, 64, 64, None, 0, 0)))
    assert cap == 64 * 64
    N.check(N.lib.gs_debug_set_partial_budget(cap * 2 * 24 - 1))
    try:
        assert _pass(cam, 8, 0, 4) == N.GS_ERR_ARG
        assert b"budget" in N.lib.gs_last_error()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


def test_accumulation_calls_reject_a_null_context(cam):
    st = N.gs_stats()
    info = N.gs_accum_info()
    buf = np.zeros(12)
    cnt = N.gs_counters()
    assert N.lib.gs_multi_accum_begin(None, C.byref(cam), 1, 4) == N.GS_ERR_ARG
    assert N.lib.gs_multi_accum_pass(None, 8, None, C.byref(st)) == N.GS_ERR_ARG
    assert b"null" in N.lib.gs_last_error()
    assert N.lib.gs_multi_accum_info(None, C.byref(info)) == N.GS_ERR_ARG
    assert N.lib.gs_multi_accum_download(None, buf.ctypes.data) == N.GS_ERR_ARG
    assert N.lib.gs_multi_accum_upload(None, C.byref(cam), 1, 4, 8, buf.ctypes.data, C.byref(cnt)) == N.GS_ERR_ARG
    assert N.lib.gs_multi_accum_end(None) == N.GS_ERR_ARG


def test_accum_info_layout_matches():
    assert N.lib.gs_host_struct_size(b"gs_accum_info") == C.sizeof(N.gs_accum_info)


def test_progressive_renderer_is_exported():
    assert g.ProgressiveRenderer.__name__ == "ProgressiveRenderer"
    assert hasattr(g.Renderer, "render_pass_async")
    assert g.checkpoint is checkpoint


# ------------------------------------------------------------------ checkpoints
def _meta(cam, **kw):
    m = {"samples": 48, "seed": 2 ** 63 + 5, "chunk": 16, "width": cam.image_width, "height": cam.image_height,
         "camera": bytes(cam), "counters": {n: 2 ** 40 + k for k, n in enumerate(checkpoint.COUNTER_NAMES)},
         "passes": 3, "last_delta": 0.1 + 0.2}
    m.update(kw)
    return m


def _sums(cam):
    rng = np.random.default_rng(7)
    s = rng.standard_normal((cam.image_height, cam.image_width, 3)) * 1e3
    s[0, 0] = [0.0, -0.0, 5e-324]  # signed zero and a denormal survive too
    return s


def test_checkpoint_round_trip_is_exact(cam, tmp_path):
    assert checkpoint.COUNTER_NAMES == N.COUNTER_NAMES
    sums, meta = _sums(cam), _meta(cam)
    path = str(tmp_path / "frame.ckpt")  # (written under the name as given)
    checkpoint.write_checkpoint(path, sums, meta)
    back, m2 = checkpoint.read_checkpoint(path)
    assert back.dtype == np.float64 and back.tobytes() == sums.tobytes()
    assert m2 == meta
    checkpoint.check_compatible(m2, cam.image_width, cam.image_height, 16, 2 ** 63 + 5, bytes(cam))
    f = io.BytesIO()  # a file object works as well
    checkpoint.write_checkpoint(f, sums, meta)
    f.seek(0)
    assert checkpoint.read_checkpoint(f)[0].tobytes() == sums.tobytes()


@pytest.mark.parametrize("field", ["width", "height", "chunk", "seed", "camera"])
def test_checkpoint_mismatch_is_rejected(cam, field):
    meta = _meta(cam)
    want = {"width": cam.image_width, "height": cam.image_height, "chunk": 16, "seed": 2 ** 63 + 5,
            "camera": bytes(cam)}
    checkpoint.check_compatible(meta, **want)
    if field == "camera":
        other = g.camera(scenes.config("C4", width=64, spp=1).camera)
        other.center[0] += 1e-9
        want["camera"] = bytes(other)
    else:
        want[field] += 1
    with pytest.raises(checkpoint.CheckpointError) as e:
        checkpoint.check_compatible(meta, **want)
    assert field in str(e.value)


def test_checkpoint_writer_and_reader_reject_malformed_input(cam, tmp_path):
    sums, meta = _sums(cam), _meta(cam)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_checkpoint(str(tmp_path / "a"), sums[:-1], meta)       # wrong shape
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_checkpoint(str(tmp_path / "b"), sums, _meta(cam, samples=40))  # not whole chunks
    no_seed = {k: v for k, v in meta.items() if k != "seed"}
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_checkpoint(str(tmp_path / "c"), sums, no_seed)
    np.savez(str(tmp_path / "d.npz"), sums=sums)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.read_checkpoint(str(tmp_path / "d.npz"))


def test_rust_binding_declares_the_accumulation_struct():
    """gs_accum_info's fields, in the header's order, in bindings/grayshift_gpu.rs."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "grayshift_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gs_accum_info \{(.*?)\} gs_accum_info;", hdr, re.S).group(1)
    c_names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
               for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    rs = re.search(r"pub struct gs_accum_info \{(.*?)\}", open(os.path.join(root, "bindings", "grayshift_gpu.rs")).read(),
                   re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+)\s*:", rs) == c_names
    assert c_names == [n for n, _ in N.gs_accum_info._fields_]
