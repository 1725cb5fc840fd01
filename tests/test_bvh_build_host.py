"""The host half of the device BVH builder, without a GPU: the tree's shape as a function of n,
gs_host_bvh_build (construct_tree over bare boxes) against an independent restatement of the
reference's rule in pure Python, BVHNode::from_order behind gs_host_scene_from_spec_ex fed by
the host's own order (bvh = 2), and gs_bvh_build_async's argument rules."""
import ctypes as C
import struct

import numpy as np
import pytest

from grayshift_amd import _native as N

from . import bvh_cases as B


def test_counts_follow_the_recurrence():
    for n in list(range(1, 65)) + [10002, 1000001]:
        assert N.lib.gs_bvh_node_count(n) == B.nodes_of(n), n
        assert N.lib.gs_bvh_depth(n) == B.depth_of(n), n
    assert (N.lib.gs_bvh_node_count(10002), N.lib.gs_bvh_depth(10002)) == (11811, 14)
    assert (N.lib.gs_bvh_node_count(1000001), N.lib.gs_bvh_depth(1000001)) == (1048575, 20)
    assert N.lib.gs_bvh_node_count(0) == -1
    assert N.lib.gs_bvh_build_work_bytes(0) == -1 and N.lib.gs_bvh_build_work_bytes(1000001) > 0
    assert N.lib.gs_bvh_build_lds_members() >= 3


F64_MAX = struct.unpack("<d", struct.pack("<Q", 0x7FEFFFFFFFFFFFFF))[0]


def restated_build(boxes, node_base=0):
    """BVH.rs:18-65 over bare boxes, restated: the left fold from AABB::EMPTY with
    from_interval_pair's comparisons, longest_axis' comparison chain, Python's stable sorted()
    on min[axis] with -0.0 normalised, the split at n // 2; nodes in pre-order."""
    rows = [tuple(float(x) for x in r) for r in boxes.tolist()]
    nodes, order = [], []

    def leaf(i):
        order.append(i)
        return (B.REF_BUILD_MEMBER << 28) | i

    def pair(a, b):
        return tuple(a[c] if a[c] <= b[c] else b[c] for c in range(3)) + \
            tuple(a[c] if a[c] >= b[c] else b[c] for c in range(3, 6))

    def build(members):
        idx = len(nodes)
        nodes.append(None)
        if len(members) == 1:
            box, left, right = rows[members[0]], leaf(members[0]), 0
        elif len(members) == 2:
            box = pair(rows[members[0]], rows[members[1]])
            left, right = leaf(members[0]), leaf(members[1])
        else:
            box = (F64_MAX,) * 3 + (-F64_MAX,) * 3
            for m in members:
                box = pair(box, rows[m])
            sx, sy, sz = (box[3 + c] - box[c] for c in range(3))
            axis = (0 if sx > sz else 2) if sx > sy else (1 if sy > sz else 2)
            members = sorted(members, key=lambda m: rows[m][axis] + 0.0)
            h = len(members) // 2
            left, right = build(members[:h]), build(members[h:])
        nodes[idx] = (box, left, right)
        return (B.REF_NODE << 28) | (node_base + idx)

    build(list(range(len(rows))))
    out = np.zeros(len(nodes), dtype=B.NODE)
    for k, (box, left, right) in enumerate(nodes):
        out[k]["min"], out[k]["max"], out[k]["left"], out[k]["right"] = box[:3], box[3:], left, right
    return out, np.array(order, dtype=np.uint32)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 64, 65, 300])
def test_host_build_matches_the_restatement(n):
    for name, boxes in B.box_cases(n).items():
        nodes, order = B.host_build(boxes, node_base=7)
        want_nodes, want_order = restated_build(boxes, node_base=7)
        assert np.array_equal(order, want_order), name
        assert nodes.tobytes() == want_nodes.tobytes(), name


def test_host_build_rejects_nan_and_bad_arguments():
    boxes = B.box_cases(5)["random"]
    boxes[3, 4] = np.nan
    nodes = np.zeros(8, dtype=B.NODE)
    order = np.zeros(5, dtype=np.uint32)
    assert N.lib.gs_host_bvh_build(boxes.ctypes.data, 5, 0, nodes.ctypes.data, order.ctypes.data) == N.GS_ERR_ARG
    assert b"NaN" in N.lib.gs_last_error()
    assert N.lib.gs_host_bvh_build(None, 5, 0, nodes.ctypes.data, order.ctypes.data) == N.GS_ERR_ARG
    assert N.lib.gs_host_bvh_build(boxes.ctypes.data, 0, 0, nodes.ctypes.data, order.ctypes.data) == N.GS_ERR_ARG


@pytest.fixture(scope="module")
def specs():
    return B.scene_specs()


def _scene(spec, bvh, min_members=3):
    h = C.c_void_p()
    opt = N.gs_build_options(bvh=bvh, device_min_members=min_members)
    N.check(N.lib.gs_host_scene_from_spec_ex(spec.ptr(), C.byref(opt), C.byref(h)))
    return h


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_box", "final_scene", "triangle_grid", "C4"])
def test_rebuilt_scene_is_byte_identical(specs, name):
    spec = specs[name]
    h0 = C.c_void_p()
    N.check(N.lib.gs_host_scene_from_spec(spec.ptr(), C.byref(h0)))
    h2 = _scene(spec, 2)
    try:
        a = B.flat_bytes(N.gs_flat_scene.from_address(N.lib.gs_host_scene_flat(h0)))
        b = B.flat_bytes(N.gs_flat_scene.from_address(N.lib.gs_host_scene_flat(h2)))
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], k
        info = N.gs_build_info()
        N.check(N.lib.gs_host_scene_build_info(h2, C.byref(info)))
        assert info.bvhs_device >= (2 if name == "final_scene" else 1)  # (the world, and the balls)
        assert info.members_device >= 3
        N.check(N.lib.gs_host_scene_build_info(h0, C.byref(info)))
        assert info.bvhs_device == 0 and info.bvhs_host >= 1
    finally:
        N.lib.gs_host_scene_destroy(h0)
        N.lib.gs_host_scene_destroy(h2)


def test_struct_sizes_and_options():
    assert N.lib.gs_host_struct_size(b"gs_build_options") == C.sizeof(N.gs_build_options) == 16
    assert N.lib.gs_host_struct_size(b"gs_build_info") == C.sizeof(N.gs_build_info) == 40
    spec = B.triangle_grid(2, 2)
    h = C.c_void_p()
    bad = N.gs_build_options(bvh=3)
    assert N.lib.gs_host_scene_from_spec_ex(spec.ptr(), C.byref(bad), C.byref(h)) == N.GS_ERR_ARG
    # below device_min_members the host builds: 8 members < 8192 (the default)
    h = _scene(spec, 2, 0)
    info = N.gs_build_info()
    N.check(N.lib.gs_host_scene_build_info(h, C.byref(info)))
    N.lib.gs_host_scene_destroy(h)
    assert (info.bvhs_device, info.bvhs_host) == (0, 1)


def test_device_build_arguments_are_checked_before_the_device():
    fake = [C.c_void_p(0x1000 * (k + 1)) for k in range(5)]
    boxes, refs, nodes, order, work = fake
    n = 100
    wb = N.lib.gs_bvh_build_work_bytes(n)
    call = N.lib.gs_bvh_build_async
    assert call(None, refs, n, 0, nodes, order, work, wb, None) == N.GS_ERR_ARG
    assert call(boxes, refs, n, 0, None, order, work, wb, None) == N.GS_ERR_ARG
    assert call(boxes, refs, n, 0, nodes, None, work, wb, None) == N.GS_ERR_ARG
    assert call(boxes, refs, n, 0, nodes, order, None, wb, None) == N.GS_ERR_ARG
    assert b"null" in N.lib.gs_last_error()
    assert call(boxes, None, 0, 0, nodes, order, work, wb, None) == N.GS_ERR_ARG
    assert call(boxes, None, 1 << 28, 0, nodes, order, work, 1 << 40, None) == N.GS_ERR_ARG
    assert call(boxes, None, n, (1 << 28) - 100, nodes, order, work, wb, None) == N.GS_ERR_ARG
    assert b"28-bit" in N.lib.gs_last_error()
    assert call(boxes, None, n, 0, nodes, order, work, wb - 1, None) == N.GS_ERR_ARG
    assert b"work buffer" in N.lib.gs_last_error()
    assert N.lib.gs_bvh_build_status(None, None) == N.GS_ERR_ARG


def test_device_builder_without_a_device_is_an_error_not_a_crash(specs):
    h = C.c_void_p()
    opt = N.gs_build_options(bvh=1, device_min_members=3)
    st = N.lib.gs_host_scene_from_spec_ex(specs["cornell_box"].ptr(), C.byref(opt), C.byref(h))
    assert st in (N.GS_OK, N.GS_ERR_NO_DEVICE)
    if st == N.GS_OK:
        N.lib.gs_host_scene_destroy(h)
