"""What tests/test_gpu_traversal.py's cases (d) and (e) rest on, checked with the CPU oracle and the
host library alone (no GPU):

  * the scaling identity: the oracle's frame and every counter of tests/traversal_cases.py's
    five scenes are the same, bit for bit, at focus distance 1.0, 2^-60 and 2^-460;
  * the camera's rays at the two small scales are no cert rays: every component of every
    direction is below 1e-15 (from the gs_camera record), and |d|^2 < 2^-900 at 2^-460;
  * the two 1e15 scenes render finite frames, and the same one: no ray hits the far sphere, and
    one ulp of its centre moves no pixel and no counter;
  * the two test hooks' argument validation and defaults, without a device.
"""
import numpy as np
import pytest

from grayshift_amd import _native as N
from grayshift_amd import renderer
import oracle

from tests import traversal_cases as TC


def _same(a, b):
    return np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and a[1] == b[1]


@pytest.fixture(scope="module")
def base():
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle.render(TC.scale_scene(name, 1.0), seed=TC.SEED)
        return made[name]
    return get


@pytest.mark.parametrize("scale", list(TC.SCALES))
@pytest.mark.parametrize("name", list(TC.SCALE_SCENES))
def test_oracle_scaling_identity(base, name, scale):
    ref = base(name)
    got = oracle.render(TC.scale_scene(name, TC.SCALES[scale]), seed=TC.SEED)
    assert np.isfinite(ref[0]).all() and ref[1]["paths"] == TC.W * TC.W * TC.SPP
    assert ref[1]["hits"] > 0 and ref[1]["rays"] > ref[1]["paths"]  # camera rays hit, and paths bounce
    assert _same(got, ref), {k: (got[1][k], v) for k, v in ref[1].items() if got[1][k] != v}


def test_scale_scenes_reach_their_primitives(base):
    """The quad, the medium and the nested BVH are met (by bounce rays) in the scenes that have them."""
    assert base("spheres")[1]["quad_tests"] == 0 and base("quad")[1]["quad_tests"] > 0
    assert base("spheres")[1]["medium_tests"] == 0 and base("medium")[1]["medium_tests"] > 0
    assert base("spheres")[1]["instance_tests"] == 0 and base("nested")[1]["instance_tests"] > 0
    c = base("all")[1]
    assert c["quad_tests"] > 0 and c["medium_tests"] > 0 and c["instance_tests"] > 0


@pytest.mark.parametrize("scale", list(TC.SCALES))
def test_small_camera_rays_are_no_cert_rays(scale):
    s = TC.SCALES[scale]
    cam = renderer.camera(TC.scale_camera(s))
    one = renderer.camera(TC.scale_camera(1.0))
    assert cam.defocus_angle == 0.0 and list(cam.center) == [0.0, 0.0, 0.0]
    bound = TC.camera_ray_bound(cam)
    assert max(bound) < TC.NONCERT, bound
    # the record is the unit camera's, scaled exactly
    for f in ("starting_pixel_pos", "pixel_delta_u", "pixel_delta_v"):
        assert [x for x in getattr(cam, f)] == [x * s for x in getattr(one, f)], f
    if scale == "2^-460":  # |d|^2 < 2^-900: sphere_root_take's division flavour
        assert sum(b * b for b in bound) < 2.0 ** -900
    else:
        assert sum(b * b for b in bound) > 2.0 ** -900 * 4.0  # (the reciprocal flavour, with non-cert rays)


def test_unit_camera_rays_are_cert_rays_at_the_frame_centre():
    """At focus distance 1.0 the camera's central direction has |1 / d| within [1e-25, 1e15] on the
    two axes it spans (the scaled frames differ from it in the flavour, not only in the scale)."""
    one = renderer.camera(TC.scale_camera(1.0))
    mid = [one.starting_pixel_pos[k] + 15.7 * one.pixel_delta_u[k] + 16.2 * one.pixel_delta_v[k] for k in range(3)]
    assert all(1e-15 < abs(v) < 1e25 for v in mid), mid


def test_big_scenes_are_finite_and_alike():
    a = oracle.render(TC.big_scene("at 1e15"), seed=TC.SEED)
    b = oracle.render(TC.big_scene("one ulp beyond"), seed=TC.SEED)
    assert TC.BIG_X["at 1e15"] + 1.0 == 1e15 and TC.BIG_X["one ulp beyond"] + 1.0 > 1e15
    assert np.isfinite(a[0]).all() and np.isfinite(b[0]).all()
    assert a[1]["paths"] == TC.W * TC.W * TC.SPP and a[1]["hits"] > 0
    assert _same(a, b)


def test_hooks_validate_their_arguments_without_a_device():
    try:
        for bad in (2, -1, 7):
            assert N.lib.gs_debug_set_cert_boxes(bad) == N.GS_ERR_ARG
            assert b"cert boxes" in N.lib.gs_last_error()
        assert N.lib.gs_debug_set_cert_boxes(0) == N.GS_OK
        assert N.lib.gs_debug_set_cert_boxes(1) == N.GS_OK
        for bad in (-2, -(1 << 40)):
            assert N.lib.gs_debug_set_mirror_budget(bad) == N.GS_ERR_ARG
            assert b"mirror budget" in N.lib.gs_last_error()
        for ok in (0, 32, 1 << 40, -1):
            assert N.lib.gs_debug_set_mirror_budget(ok) == N.GS_OK
    finally:  # the library's defaults
        N.lib.gs_debug_set_cert_boxes(1)
        N.lib.gs_debug_set_mirror_budget(-1)
