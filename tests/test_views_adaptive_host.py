"""CPU tests of adaptive views (a batch of cameras under one set of adaptive settings): every
argument rule of the tile-level pass returns GS_ERR_ARG with its message before any device work --
with a scene pointer that would fault if it were read and no device in the machine -- the frame
context's calls refuse a NULL context, the ctypes and Rust records follow the header, checkpoint
format 4 round-trips and is told apart from formats 1 to 3, and views_round_kernel_for's table
(csrc/device/render.hip, read as text) holds exactly the GS_K / GS_KR feature sets of
tests/test_gpu_kernel_matrix.py's rows, each in the form its macro implies.  No compute on a device.
(The mutual exclusion of the context's open states needs a context, hence a device:
tests/test_gpu_views_adaptive.py::test_open_states_exclude_each_other.)"""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import checkpoint, scenes
from grayshift_amd.scene import sample_settings

from tests import test_gpu_kernel_matrix as M

P = C.c_void_p
OK = P(0x1000)  # a non-null pointer that must never be followed
W, H = 72, 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cam():
    c = g.camera(scenes.config("C4", width=W, spp=1).camera)
    assert (c.image_width, c.image_height) == (W, H)
    return c


def _views(cam, n=3):
    v = (N.gs_view * n)()
    for k in range(n):
        v[k].cam = cam
        v[k].seed = k + 1
    return v


def _call(views, n, ss=(0.95, 0.05, 4, 16), first=0, rounds=1, scene=OK, part="rr", outs="rgb", state=OK,
          state_bytes=1 << 40):
    """gs_render_tiles_views_rounds_async; tile height 20 divides H = 40."""
    part = {"rr": N.gs_partition(0, 1, 64, 20, None, 0, 0), "bad": N.gs_partition(2, 2, 64, 20, None, 0, 0),
            "straddle": N.gs_partition(0, 1, 64, 64, None, 0, 0), "null": None}[part]
    o = {"rgb": N.gs_round_outputs(0x2000, None, None, None), "rgb8": N.gs_round_outputs(None, 0x2000, None, None),
         "none": N.gs_round_outputs(None, None, 0x2000, 0x3000), "null": None}[outs]
    s = sample_settings(*ss) if ss is not None else None
    return N.lib.gs_render_tiles_views_rounds_async(
        scene, views, n, C.byref(s) if s is not None else None, C.byref(part) if part is not None else None, first, rounds,
        state, state_bytes, C.byref(o) if o is not None else None, None, None)


def _err():
    return N.lib.gs_last_error()


# ------------------------------------------------------------ the views rules
def test_rounds_reject_null_pointers_and_empty_batches(cam):
    v = _views(cam)
    assert _call(v, 3, scene=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(None, 3) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, ss=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, part="null") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, state=None) == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, outs="null") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 3, outs="none") == N.GS_ERR_ARG and b"null" in _err()
    assert _call(v, 0) == N.GS_ERR_ARG and b"0 views" in _err()
    assert _call(v, 3, part="bad") == N.GS_ERR_ARG and b"partition" in _err()


def test_rounds_reject_views_of_another_size_or_depth_0(cam):
    v = _views(cam)
    v[2].cam.image_width = W + 1
    assert _call(v, 3) == N.GS_ERR_ARG and b"view 2 differs" in _err()
    v = _views(cam)
    v[1].cam.image_height = H - 1
    assert _call(v, 3) == N.GS_ERR_ARG and b"view 1 differs" in _err()
    v = _views(cam)
    v[1].cam.max_depth = 0
    assert _call(v, 3) == N.GS_ERR_ARG and b"view 1 has max_depth 0" in _err()
    v = _views(cam)
    v[0].cam.image_width = 0
    assert _call(v, 1) == N.GS_ERR_ARG and b"image size" in _err()


def test_rounds_reject_what_does_not_fit_32_bits(cam):
    big = N.gs_camera.from_buffer_copy(cam)
    big.image_width, big.image_height = 65536, 32768
    assert _call(_views(big, 2), 2) == N.GS_ERR_ARG and b"32-bit pixel" in _err()  # V W H = 2^32
    big.image_width, big.image_height = 1, 1 << 30
    assert _call(_views(big, 2), 2) == N.GS_ERR_ARG and b"32-bit pixel" in _err()  # V H = 2^31: no i32 height


def test_rounds_reject_tiles_that_straddle_views(cam):
    assert _call(_views(cam), 3, part="straddle") == N.GS_ERR_ARG and b"straddle" in _err()


# ------------------------------------------------------------ the adaptation rules
def test_rounds_reject_bad_settings_and_round_ranges(cam):
    v = _views(cam)
    assert _call(v, 3, rounds=0) == N.GS_ERR_ARG and b"0 rounds" in _err()
    assert _call(v, 3, ss=(0.95, 0.05, 0, 16)) == N.GS_ERR_ARG and b"batch_size 0" in _err()
    assert _call(v, 3, ss=(0.95, 0.05, 8, 7)) == N.GS_ERR_ARG and b"one batch" in _err()
    assert _call(v, 3, ss=(0.95, 0.05, 1, 65536)) == N.GS_ERR_ARG and b"65536 batches" in _err()  # R = 65537
    assert _call(v, 3, first=3, rounds=3) == N.GS_ERR_ARG and b"exceeds the settings' 5 rounds" in _err()
    assert _call(v, 3, first=5, rounds=1) == N.GS_ERR_ARG and b"5 rounds" in _err()


def test_rounds_reject_a_state_blob_that_is_too_small(cam):
    """The blob is gs_round_state_bytes of the tall frame's camera."""
    tall = N.gs_camera.from_buffer_copy(cam)
    tall.image_height = 3 * H
    part = N.gs_partition(0, 1, 64, 20, None, 0, 0)
    ss = sample_settings(0.95, 0.05, 4, 16)
    need = N.lib.gs_round_state_bytes(C.byref(tall), C.byref(part), C.byref(ss))
    one = N.lib.gs_round_state_bytes(C.byref(cam), C.byref(part), C.byref(ss))
    assert need > one > 0
    v = _views(cam)
    assert _call(v, 3, state_bytes=need - 1) == N.GS_ERR_ARG and b"state_bytes" in _err()
    assert _call(v, 3, state_bytes=one) == N.GS_ERR_ARG and b"state_bytes" in _err()
    assert _call(v, 3, state_bytes=-1) == N.GS_ERR_ARG and b"state_bytes" in _err()


def test_rounds_reject_a_batch_beyond_the_partial_budget(cam):
    N.check(N.lib.gs_debug_set_partial_budget(4 * 24 - 1))  # one pixel's batch of 4 samples: 96 bytes
    try:
        assert _call(_views(cam), 3) == N.GS_ERR_ARG and b"partial budget" in _err()
    finally:
        N.check(N.lib.gs_debug_set_partial_budget(0))


# ------------------------------------------------------------ the frame context's calls
def test_context_calls_reject_a_null_context(cam):
    v = _views(cam)
    ss = sample_settings(0.95, 0.05, 4, 16)
    info = N.gs_views_adapt_info()
    sums = np.zeros((3, H, W, 5))
    state = np.zeros((3, H, W), dtype=np.uint32)
    cnt = N.gs_counters()
    L = N.lib
    assert L.gs_multi_views_adapt_begin(None, v, 3, C.byref(ss)) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_adapt_pass(None, 1, None, None) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_adapt_info(None, C.byref(info), None) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_adapt_maps(None, None, None) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_adapt_download(None, sums.ctypes.data, state.ctypes.data) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_adapt_upload(None, v, 3, C.byref(ss), 0, sums.ctypes.data, state.ctypes.data,
                                         C.byref(cnt)) == N.GS_ERR_ARG and b"null" in _err()
    assert L.gs_multi_views_adapt_end(None) == N.GS_ERR_ARG and b"null" in _err()


def test_open_states_are_excluded_in_both_directions_in_the_source():
    """Without a device no context can be opened; what can be read here: one function of
    multi_gpu.cpp, gs_multi::admit, holds the refusal for each of the four sessions and refuses
    whenever one is open, whichever it is; every one of the four begin paths (the adaptation's
    begin serves the views adaptation too) asks it before anything else, and so does a frame,
    whose checks come before its first stage; every session call of the header goes through it,
    and nothing but a begin opens a session.  (Read by shape, not by exact text: the first call a
    function makes, what follows it, which functions hold what.)"""
    src = open(os.path.join(ROOT, "grayshift_amd", "csrc", "host", "multi_gpu.cpp")).read()

    def body_of(name):  # of the function defined as `gs_status <name>(...) [const] {` at the left margin
        m = re.search(r"^gs_status %s\([^{;]*\{\n" % re.escape(name), src, re.M)
        assert m, name
        return src[m.end():src.index("\n}\n", m.end())]

    def first_call(body):
        return re.search(r"\b(\w+)\s*\(", body).group(1)

    admit = body_of("gs_multi::admit")
    for message in ("an accumulation is open: gs_multi_accum_end first",
                    "a views accumulation is open: gs_multi_views_accum_end first",
                    "an adaptation is open: gs_multi_adapt_end first",
                    "a views adaptation is open: gs_multi_views_adapt_end first"):
        assert admit.count(message) == 1, message
        assert src.count(message) == 1, message  # (nowhere else: no second copy of the rule)
    # a begin (and a one-shot frame) passes only with no session open; the refusal is the open one's
    assert re.search(r"if \(open == Session::None\) return GS_OK;", admit)
    assert re.search(r"refusal\[\(int\)open\]", admit) and re.search(r"return fail\(GS_ERR_ARG, msg\);\s*$", admit)
    begins = ("gs_multi::accum_begin", "gs_multi::views_accum_begin", "gs_multi::adapt_begin")
    for fn in begins:
        body = body_of(fn)
        assert first_call(body) == "admit", fn
        assert re.search(r"\bs = admit\(Call::Begin, [\w:]+\);\s*if \(s != GS_OK\) return s;", body), fn
    render = body_of("gs_multi::render")
    assert first_call(render) == "check_frame"
    assert re.search(r"\bs = check_frame\(f, out\);\s*if \(s != GS_OK\) return s;", render)
    check = body_of("gs_multi::check_frame")
    assert re.search(r"return admit\(Call::Frame, f\.session\);\s*$", check) and "hip" not in check
    # every pass, info, maps, download and end of the header is a session's own call: through in_session,
    # which asks admit under the context's lock before the call's body runs
    header = open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read()
    own = set(re.findall(r"\b(gs_multi_(?:views_)?(?:accum|adapt)_(?:pass|info|maps|download|end))\s*\(", header))
    assert len(own) == 18, sorted(own)
    for fn in sorted(own):
        assert re.match(r"\s*(?:if \([^\n]*\) return fail\(GS_ERR_ARG, \"null argument\"\);\s*)?"  # (a null guard at most)
                        r"return in_session\(m, Session::\w+, Call::(?:Pass|Other),", body_of(fn)), fn
    gate = src[src.index("gs_status in_session("):]
    gate = gate[:gate.index("\n}\n")]
    assert re.search(r"lock_guard.*\n.*m->admit\(call, s\);\s*return st != GS_OK \? st : body\(\);", gate)
    # only a begin opens a session, and the old parallel flags are gone
    opened = re.findall(r"\bopen = (?!Session::None;)", src)
    assert len(opened) == sum(len(re.findall(r"\bopen = (?!Session::None;)", body_of(fn))) for fn in begins) == 3
    for flag in ("acc_open", "va_open", "ad_open", "vd_open", "th_ctx"):
        assert flag not in src, flag


# ------------------------------------------------------------ records
def test_native_struct_sizes_match_the_library():
    assert N.lib.gs_host_struct_size(b"gs_views_adapt_info") == C.sizeof(N.gs_views_adapt_info)
    assert N.lib.gs_version() == 11


def test_info_record_follows_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read(), flags=re.S)
    body = re.search(r"typedef struct gs_views_adapt_info \{(.*?)\} gs_views_adapt_info;", hdr, re.S).group(1)
    c_names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1)
               for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    rs = re.search(r"pub struct gs_views_adapt_info \{(.*?)\}",
                   open(os.path.join(ROOT, "bindings", "grayshift_gpu.rs")).read(), re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+)\s*:", rs) == c_names
    assert [k for k, _ in N.gs_views_adapt_info._fields_] == c_names


def test_the_header_states_what_is_out_of_scope():
    hdr = open(os.path.join(ROOT, "include", "grayshift_gpu.h")).read()
    block = hdr[hdr.index("---- Adaptive views"):]
    block = re.sub(r"\s*\n \*\s*", " ", block[:block.index("gs_status gs_render_tiles_views_rounds_async")])
    for what in ("per-view settings", "per-pass view selection", "a views form of the catch-all kernel",
                 "cost-planned tiles for batches", "PPM text over views", "GS_USE_RSPLIT 0"):
        assert what in block, what
    assert "Fixed spp only (no adaptive settings" not in hdr


# ------------------------------------------------------------ checkpoint format 4
V = 3
R = 5


def _meta(cam, rounds=2):
    cams = []
    for v in range(V):
        c = N.gs_camera.from_buffer_copy(cam)
        c.center[0] += v
        cams.append(bytes(c))
    return {"rounds": rounds, "seeds": [1, 2, 3], "cameras": cams, "width": W, "height": H, "confidence": 0.95,
            "tolerance": 0.05, "batch_size": 4, "max_samples": 16,
            "counters": {n: 7 * k + 1 for k, n in enumerate(checkpoint.COUNTER_NAMES)}}


def _arrays(rounds=2):
    rng = np.random.default_rng(4)
    sums = rng.random((V, H, W, 5))
    state = np.full((V, H, W), rounds, dtype=np.uint32)
    state[1, :, : W // 2] = 1 | checkpoint.STOPPED  # half of view 1 stopped after round 1
    return sums, state


def _file(write, *args):
    f = io.BytesIO()
    write(f, *args)
    f.seek(0)
    return f


def test_views_adaptive_checkpoint_round_trip(cam):
    meta = _meta(cam)
    sums, state = _arrays()
    s2, st2, m = checkpoint.read_views_adaptive_checkpoint(
        _file(checkpoint.write_views_adaptive_checkpoint, sums, state, meta))
    assert s2.dtype == np.float64 and s2.tobytes() == sums.tobytes()
    assert st2.dtype == np.uint32 and st2.tobytes() == state.tobytes()
    assert m == meta
    checkpoint.check_views_adaptive_compatible(m, W, H, sample_settings(0.95, 0.05, 4, 16), [1, 2, 3], meta["cameras"])


def test_views_adaptive_checkpoint_write_rejects_bad_records(cam):
    meta = _meta(cam)
    sums, state = _arrays()
    for bad in ({"seeds": [1, 2]}, {"rounds": R + 1}, {"batch_size": 0}, {"max_samples": 3}, {"rounds": 3}):
        with pytest.raises(checkpoint.CheckpointError):
            checkpoint.write_views_adaptive_checkpoint(io.BytesIO(), sums, state, dict(meta, **bad))
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_views_adaptive_checkpoint(io.BytesIO(), sums[..., :3], state, meta)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_views_adaptive_checkpoint(io.BytesIO(), sums, state[:, :-1], meta)
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_views_adaptive_checkpoint(io.BytesIO(), sums, state,
                                                   {k: v for k, v in meta.items() if k != "cameras"})
    stopped_at_0 = state.copy()
    stopped_at_0[0, 0, 0] = checkpoint.STOPPED
    with pytest.raises(checkpoint.CheckpointError):
        checkpoint.write_views_adaptive_checkpoint(io.BytesIO(), sums, stopped_at_0, meta)


def test_the_four_readers_reject_each_others_files(cam):
    meta = _meta(cam)
    sums, state = _arrays()
    f4 = _file(checkpoint.write_views_adaptive_checkpoint, sums, state, meta)
    m1 = {"samples": 8, "seed": 1, "chunk": 4, "width": W, "height": H, "camera": bytes(cam), "counters": meta["counters"]}
    f1 = _file(checkpoint.write_checkpoint, np.zeros((H, W, 3)), m1)
    m2 = {"rounds": 0, "seed": 1, "width": W, "height": H, "confidence": 0.95, "tolerance": 0.05, "batch_size": 4,
          "max_samples": 16, "camera": bytes(cam), "counters": meta["counters"]}
    f2 = _file(checkpoint.write_adaptive_checkpoint, np.zeros((H, W, 5)), np.zeros((H, W), dtype=np.uint32), m2)
    m3 = {"samples": [8, 24, 0], "seeds": [1, 2, 3], "cameras": meta["cameras"], "chunk": 4, "width": W, "height": H,
          "counters": meta["counters"]}
    f3 = _file(checkpoint.write_views_checkpoint, np.zeros((V, H, W, 3)), m3)
    for f in (f1, f2, f3):
        with pytest.raises(checkpoint.CheckpointError):
            checkpoint.read_views_adaptive_checkpoint(f)
        f.seek(0)
    for read in (checkpoint.read_checkpoint, checkpoint.read_adaptive_checkpoint, checkpoint.read_views_checkpoint):
        with pytest.raises(checkpoint.CheckpointError):
            read(f4)
        f4.seek(0)
    checkpoint.read_checkpoint(f1)
    checkpoint.read_adaptive_checkpoint(f2)
    checkpoint.read_views_checkpoint(f3)
    checkpoint.read_views_adaptive_checkpoint(f4)


def test_views_adaptive_checkpoint_rejects_any_mismatch(cam):
    meta = _meta(cam)
    sums, state = _arrays()
    _, _, m = checkpoint.read_views_adaptive_checkpoint(
        _file(checkpoint.write_views_adaptive_checkpoint, sums, state, meta))
    cams = meta["cameras"]
    other = N.gs_camera.from_buffer_copy(cam)
    other.max_depth += 1
    ss = (0.95, 0.05, 4, 16)
    cases = {
        "seed": (W, H, ss, [1, 9, 3], cams),
        "camera": (W, H, ss, [1, 2, 3], [cams[0], bytes(other), cams[2]]),
        "width": (W + 1, H, ss, [1, 2, 3], cams),
        "height": (W, H + 1, ss, [1, 2, 3], cams),
        "view count": (W, H, ss, [1, 2], cams[:2]),
        "confidence": (W, H, (0.9, 0.05, 4, 16), [1, 2, 3], cams),
        "tolerance": (W, H, (0.95, 0.1, 4, 16), [1, 2, 3], cams),
        "batch_size": (W, H, (0.95, 0.05, 2, 16), [1, 2, 3], cams),
        "max_samples": (W, H, (0.95, 0.05, 4, 17), [1, 2, 3], cams),
    }
    for what, (w, h, s, seeds, cs) in cases.items():
        with pytest.raises(checkpoint.CheckpointError):  # (a changed `what`)
            checkpoint.check_views_adaptive_compatible(m, w, h, sample_settings(*s), seeds, cs)


# ------------------------------------------------------------ the kernel table
def _word(expr):
    bits = 0
    for name in re.findall(r"[A-Z_][A-Z_0-9]*", expr):
        bits |= M.FEAT_BITS[name]
    return bits


def _source():
    return open(os.path.join(ROOT, "grayshift_amd", "csrc", "device", "render.hip")).read()


def _views_round_table():
    """{feature set: macro} from views_round_kernel_for's body."""
    src = _source()
    body = src[src.index("void (*views_round_kernel_for(int feat))(KArgs) {"):]
    body = body[:body.index("#undef GS_VR")]
    body = body[body.index("switch (feat)"):]
    table = {}
    for macro, expr in re.findall(r"^\s*(GS_VR|GS_VL)\(([^)]*)\)\s*$", body, re.M):
        f = _word(expr)
        assert f not in table, "feature set %d twice" % f
        table[f] = macro
    assert "default: return nullptr;" in body  # (no fallback for any other word)
    return table


def test_views_round_table_is_the_matrix_rows_with_a_views_form():
    table = _views_round_table()
    want = {r.feat: {"GS_KR": "GS_VR", "GS_K": "GS_VL"}[r.macro] for r in M.ROWS if r.macro in ("GS_K", "GS_KR")}
    assert len(want) == 26 and 0 in want
    assert table == want
    for f, macro in table.items():
        media_or_nested = bool(f & (M.MEDIA | M.NESTED))
        assert (macro == "GS_VL") == media_or_nested, f  # (has_rsplit: the sample-loop form without either)
        assert not f & (M.GENERAL | M.VISITS | M.FIXED | M.RSPLIT | M.VIEWS), f


def test_views_round_forms_follow_their_macros():
    src = _source()
    m = re.search(r"#define GS_VR\(F\)(.*?)#define GS_VL\(F\)(.*?)switch", src[src.index("views_round_kernel_for(int feat)"):],
                  re.S)
    vr, vl = m.group(1), m.group(2)
    assert "gs_render_kernel<(F) | GS_FEAT_FIXED | GS_FEAT_RSPLIT | GS_FEAT_VIEWS>" in vr
    assert "case (F) | GS_FEAT_FIXED | GS_FEAT_RSPLIT | GS_FEAT_VIEWS:" in vr
    assert "gs_render_kernel<(F) | GS_FEAT_VIEWS>" in vl and "case (F) | GS_FEAT_VIEWS:" in vl
    assert "FIXED" not in vl and "RSPLIT" not in vl
    # the table sits behind kernel_for's, which stays as tests/test_kernel_table_sync.py reads it
    assert src.index("#undef GS_K0") < src.index("void (*views_round_kernel_for(int feat))(KArgs) {")
    # the kernel takes the views' records whatever the form
    assert "constexpr bool kViews = (FEAT & GS_FEAT_VIEWS) != 0;" in src


def test_the_matrix_test_expects_these_forms():
    from tests import test_gpu_views_adaptive_matrix as VM
    table = _views_round_table()
    assert sorted(r.feat for r in VM.ROWS) == sorted(f for f in table if M.BY_FEAT[f].build is not None)
    for r in VM.ROWS:
        bits = VM.form_bits(r)
        assert bits == (M.FIXED | M.RSPLIT | M.VIEWS if table[r.feat] == "GS_VR" else M.VIEWS)
