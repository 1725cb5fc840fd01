"""tests/test_gpu_kernel_matrix.py's rows and kernel_for's table (csrc/device/render.hip), kept in
step without a GPU: the feature sets named on kernel_for's GS_K0 / GS_K / GS_KR lines, plus the
empty set (whose fixed, views and split-round forms are spelled out as cases and whose loop form
is the switch's default), must be exactly the matrix's rows, each with the forms of its macro.
A new instantiation fails here until the matrix has a scene for it (or says why none exists)."""
import os
import re

from tests import test_gpu_kernel_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _word(expr):
    bits = 0
    for name in re.findall(r"[A-Z_0-9]+", expr):
        bits |= M.FEAT_BITS[name]
    return bits


def _table():
    """{feature set: macro} from kernel_for's body."""
    src = open(os.path.join(ROOT, "grayshift_amd", "csrc", "device", "render.hip")).read()
    body = src[src.index("void (*kernel_for(int feat))(KArgs) {"):]
    body = body[:body.index("#undef GS_K0")]
    body = body[body.index("switch (feat)"):]
    table = {}
    for macro, expr in re.findall(r"^\s*(GS_K0|GS_KR|GS_K)\(([^)]*)\)\s*$", body, re.M):
        f = _word(expr)
        assert f not in table, "feature set %d twice" % f
        table[f] = macro
    # the empty set: `case GS_FEAT_FIXED [| ...]:` lines and the default
    plain = {_word(e) for e in re.findall(r"^\s*case (GS_FEAT_FIXED(?: \| GS_FEAT_[A-Z]+)*):", body, re.M)}
    assert "gs_render_kernel<0>" in body
    assert plain == {M.FIXED, M.FIXED | M.VIEWS, M.FIXED | M.RSPLIT}
    table[0] = "GS_KR"
    return table


def test_matrix_rows_are_the_kernel_table():
    table = _table()
    assert len(table) == 27
    assert sorted(r.feat for r in M.ROWS) == sorted(table)
    assert len({r.feat for r in M.ROWS}) == len(M.ROWS)
    for r in M.ROWS:
        assert r.macro == table[r.feat], r.feat
        assert r.forms == M.FORMS[table[r.feat]]


def test_forms_follow_the_macros():
    src = open(os.path.join(ROOT, "grayshift_amd", "csrc", "device", "render.hip")).read()
    k0 = re.search(r"#define GS_K0\(F\)(.*?)#define GS_K\(F\)(.*?)#define GS_KR\(F\)(.*?)switch", src, re.S)
    assert "GS_FEAT_FIXED>" in k0.group(1) and "VIEWS" not in k0.group(1) and "RSPLIT" not in k0.group(1)
    assert "GS_K0(F)" in k0.group(2) and "GS_FEAT_VIEWS" in k0.group(2) and "RSPLIT" not in k0.group(2)
    assert "GS_K(F)" in k0.group(3) and "GS_FEAT_RSPLIT" in k0.group(3)
    assert M.FORMS == {"GS_K0": ("loop", "fixed"), "GS_K": ("loop", "fixed", "views"),
                       "GS_KR": ("loop", "fixed", "rounds", "views")}


def test_feature_bits_are_the_headers():
    hdr = open(os.path.join(ROOT, "grayshift_amd", "csrc", "device", "kernel_abi.hpp")).read()
    for name, v in re.findall(r"^#define (GS_FEAT_[A-Z]+) (\d+)\b", hdr, re.M):
        assert M.FEAT_BITS[name] == int(v), name
    assert re.search(r"#define GS_FEAT_GENERAL_KERNEL \(GS_FEAT_GENERAL \| GS_FEAT_MEDIA \| GS_FEAT_NESTED \| "
                     r"GS_FEAT_LEAFRUN \| GS_FEAT_MIXED\)", hdr)


def test_every_row_has_a_scene_or_a_reason():
    for r in M.ROWS:
        assert (r.build is None) == bool(r.unreachable), r.feat
        if r.build is not None:
            assert r.name != "-"
    # rounds only where the split-round instantiation exists (has_rsplit: no media, no nested BVHs)
    for r in M.ROWS:
        assert ("rounds" in r.forms) == (r.macro == "GS_KR")
        if r.macro == "GS_KR":
            assert not r.feat & (M.MEDIA | M.NESTED | M.GENERAL)
