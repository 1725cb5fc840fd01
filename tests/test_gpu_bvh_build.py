"""The device BVH builder against the host's construct_tree, bit for bit.

gs_bvh_build_async is compared with gs_host_bvh_build (the product's own code path over bare
boxes) by array_equal on the node bytes and on the order, at sizes that straddle T =
gs_bvh_build_lds_members() -- below it one workgroup builds the whole tree in LDS, above it the
global passes split segments until they fit -- and on box lists that put every tie rule to work:
equal keys at every level, signed zeros in the sort and in the fold, equal extents for
longest_axis, infinite bounds.  Then whole scenes through HostScene(bvh="device"): every flat
array equal as bytes, and one frame equal with its counters."""
import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import fixed_spp

from . import bvh_cases as B

pytestmark = pytest.mark.gpu

T = N.lib.gs_bvh_build_lds_members()
CAP = 100000  # (T = 4096: the largest size below, 4 T + 3 = 16 387, stays under the cap)
SIZES = sorted({min(n, CAP) for n in [1, 2, 3, 4, 5, 6, 7, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T + 3]})


def _same(boxes, refs=None, node_base=0, what=""):
    want_nodes, want_order = B.host_build(boxes, node_base)
    if refs is not None:  # the host writes the build-only kind: put the caller's refs in its leaf slots
        for side in ("left", "right"):
            leaf = (want_nodes[side] >> 28) == B.REF_BUILD_MEMBER
            want_nodes[side][leaf] = refs[want_nodes[side][leaf] & 0x0FFFFFFF]
    status, nodes, order = B.device_build(boxes, refs, node_base)
    assert status == N.GS_OK, (what, N.lib.gs_last_error())
    assert np.array_equal(order, want_order), what
    assert np.array_equal(nodes.view(np.uint8), want_nodes.view(np.uint8)), what


@pytest.mark.parametrize("n", SIZES)
def test_device_build_equals_the_host_build(n):
    for name, boxes in B.box_cases(n).items():
        _same(boxes, what="%s n=%d" % (name, n))


@pytest.mark.parametrize("n", SIZES)
def test_refs_and_node_base(n):
    boxes = B.box_cases(n)["random"]
    refs = ((2 + np.arange(n) % 4) << 28 | (np.arange(n) * 7 + 3) % (1 << 28)).astype(np.uint32)
    _same(boxes, refs=refs, node_base=1000, what="refs n=%d" % n)


@pytest.mark.parametrize("n", [5, 2 * T + 1])
def test_nan_is_reported_by_the_status_call(n):
    boxes = B.box_cases(n)["random"]
    boxes[n // 2, 4] = np.nan
    status, _nodes, _order = B.device_build(boxes)
    assert status == N.GS_ERR_ARG
    assert b"NaN" in N.lib.gs_last_error()


def test_two_builds_are_equal_as_bytes():
    boxes = B.box_cases(2 * T + 1)["grid"]
    s1, n1, o1 = B.device_build(boxes)
    s2, n2, o2 = B.device_build(boxes)
    assert s1 == s2 == N.GS_OK
    assert n1.tobytes() == n2.tobytes() and o1.tobytes() == o2.tobytes()


def test_build_only_kind_is_no_scene_kind():
    """A tree built without refs holds GS_REF_BUILD_MEMBER leaves: no scene for the device."""
    sc = scenes.bouncing_spheres(width=64, settings=fixed_spp(1))
    with_host = g.HostScene(sc.spec)
    try:
        flat = N.gs_flat_scene.from_buffer_copy(with_host.flat)
        nodes = np.ctypeslib.as_array((B.C.c_uint8 * (64 * flat.n_nodes)).from_address(flat.nodes)).copy().view(B.NODE)
        leaf = int(np.flatnonzero((nodes["left"] >> 28) != B.REF_NODE)[0])
        nodes["left"][leaf] = (B.REF_BUILD_MEMBER << 28) | 0
        flat.nodes = nodes.ctypes.data
        d = B.C.c_void_p()
        assert N.lib.gs_device_scene_create(B.C.byref(flat), B.C.byref(d)) in (N.GS_ERR_ARG, N.GS_ERR_UNSUPPORTED)
    finally:
        with_host.close()


@pytest.fixture(scope="module")
def specs():
    return B.scene_specs()


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_box", "final_scene", "triangle_grid", "C4"])
def test_device_built_scene_is_byte_identical(specs, name):
    host = g.HostScene(specs[name])
    dev = g.HostScene(specs[name], bvh="device", device_min_members=3)
    try:
        a, b = B.flat_bytes(host.flat), B.flat_bytes(dev.flat)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], k
        info = dev.build_info()
        assert info["bvhs_device"] >= (2 if name == "final_scene" else 1)  # (the world, and the balls)
        assert host.build_info()["bvhs_device"] == 0
    finally:
        host.close()
        dev.close()


def test_one_frame_through_the_device_builder():
    sc = scenes.bouncing_spheres(width=64, settings=fixed_spp(8))
    frames = []
    for kw in ({}, {"bvh": "device", "device_min_members": 3}):
        r = g.MultiRenderer(sc, **kw)
        try:
            assert (r.width, r.height) == (64, 36)
            if kw:
                assert r.host.build_info()["bvhs_device"] >= 1
            res = r.render(seed=5, rgb=True)
            frames.append((res["rgb"], res["counters"]))
        finally:
            r.close()
    assert np.array_equal(frames[0][0], frames[1][0])
    assert frames[0][1] == frames[1][1]
