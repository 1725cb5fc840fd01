"""Scenes and cameras for the traversal's flavours, shared by
tests/test_gpu_traversal.py and tests/test_traversal_cases_host.py.

SCALE_SCENES -- camera rays that are no cert rays, inside scenes whose boxes are certified.
The camera sits at the origin, looks at (0, -0.3, -1), has no defocus, and its focus distance
is s = 2^-60 or 2^-460.  The viewport's size is proportional to the focus distance, so every
camera ray's direction is s times the direction at focus distance 1.0, exactly (s is a power
of two and nothing under- or overflows).  Then every component of d is below 1e-15: 1/d lies
above 1e15, cert_ray_ok rejects the ray, and the node steps of a wave that holds one take the
reference's f64 box test; at 2^-460, |d|^2 < 2^-900 and the sphere roots are divided by a
itself, not through its refined reciprocal.  Scattered rays have unit scale and are cert rays,
so waves hold both kinds and the flavour flips from phase to phase.

Scaling d by a power of two scales every t by its inverse exactly and leaves every hit point's
bits alone, so the frame and every counter equal those of the same camera at focus distance
1.0, provided that

  * nothing lies within the camera's first unit: tmin = 0.001 is a bound on t, so it cuts
    0.001 |d| of the ray, which depends on the scale (every object here is more than 3 away);
  * every primitive that is no sphere stands behind the camera plane, where no camera ray
    goes: a quad's |n.d| < 1e-8 test is not scale-free, so only bounce rays may meet quads.

BIG_SCENES -- the 1e15 rule itself: a libm-free scene with one unit sphere whose box maximum is
exactly 1e15 (cert_boxes stays 1) or one ulp beyond (cert_boxes 0).
"""
import numpy as np

import grayshift_amd as g
from grayshift_amd import scenes
from grayshift_amd.scene import camera_spec, fixed_spp

W = 32
SPP = 8
SEED = 7
SCALES = {"2^-60": 2.0 ** -60, "2^-460": 2.0 ** -460}
NONCERT = 1e-15  # cert_ray_ok (geometry.hpp): a ray is a cert ray only if every |1 / d| <= 1e15


def scale_camera(focus):
    return camera_spec(1.0, W, 12, 50.0, (0.0, 0.0, 0.0), (0.0, -0.3, -1.0), (0.0, 1.0, 0.0), 0.0, focus)


def camera_ray_bound(cam):
    """Per component, a bound on |d| over every camera ray of a gs_camera record without
    defocus: d = starting_pixel_pos + (i + ox) du + (j + oy) dv - center, with i + ox in
    [-0.5, W - 0.5] and j + oy in [-0.5, H - 0.5]."""
    return [abs(cam.starting_pixel_pos[k] - cam.center[k]) + cam.image_width * abs(cam.pixel_delta_u[k]) +
            cam.image_height * abs(cam.pixel_delta_v[k]) for k in range(3)]


def _scale_scene(quad=False, medium=False, nested=False):
    def build():
        b = g.SceneBuilder()
        mats = [b.lambertian((0.7, 0.4, 0.3)), b.metal((0.8, 0.8, 0.9), 0.2), b.dielectric(1.5)]
        white = b.lambertian((0.7, 0.7, 0.7))
        b.background_solid((0.6, 0.7, 0.9))
        b.add(b.sphere((0.0, -1002.0, 0.0), 1000.0, white))  # the ground: its top at y = -2
        for k in range(12):
            b.add(b.sphere((1.1 * (k - 5.5), -1.5, -6.0), 0.5, mats[k % 3]))
        if quad:  # behind the camera plane (p . (0, -0.3, -1) < 0 over the whole quad)
            b.add(b.quad((-6.0, -2.0, 4.0), (12.0, 0.0, 0.0), (0.0, 5.0, 0.0), white))
        if medium:
            b.add(b.medium_isotropic(b.sphere((-2.0, -1.2, -3.5), 0.8, white), 1.5, (0.9, 0.9, 0.9)))
        if nested:
            members = [b.sphere((-0.7, 0.0, 0.0), 0.3, mats[1]), b.sphere((0.0, 0.1, 0.3), 0.3, mats[0]),
                       b.sphere((0.7, 0.0, -0.2), 0.3, mats[2])]
            b.add(b.translate(b.bvh(members), (2.0, -1.3, -3.5)))
        return b
    return build


# name -> () -> SceneBuilder
SCALE_SCENES = {
    "spheres": _scale_scene(),
    "quad": _scale_scene(quad=True),
    "medium": _scale_scene(medium=True),
    "nested": _scale_scene(nested=True),
    "all": _scale_scene(quad=True, medium=True, nested=True),
}

_SPECS = {}


def _spec(kind, name, build):
    if (kind, name) not in _SPECS:
        _SPECS[kind, name] = build().build()
    return _SPECS[kind, name]


def scale_scene(name, focus):
    """SCALE_SCENES[name] under the camera at focus distance `focus`, 8 spp."""
    return scenes.Scene("scale_" + name, _spec("scale", name, SCALE_SCENES[name]), scale_camera(focus),
                        fixed_spp(SPP))


BIG_X = {"at 1e15": 1e15 - 1.0, "one ulp beyond": float(np.nextafter(1e15 - 1.0, np.inf))}
BIG_CERT = {"at 1e15": 1, "one ulp beyond": 0}


def _big_scene(x):
    def build():
        b = g.SceneBuilder()
        mats = [b.metal((0.8, 0.8, 0.9), 0.2), b.dielectric(1.5)]
        b.background_solid((0.6, 0.7, 0.9))
        for k in range(8):
            b.add(b.sphere((1.1 * (k - 3.5), 0.5, 0.0), 0.5, mats[k % 2]))
        b.add(b.sphere((x, 0.0, 0.0), 1.0, mats[0]))  # the unit sphere: its box's max x is x + 1
        return b
    return build


def big_scene(name):
    """Metal and dielectric spheres over a solid background (no libm call on the colour path)
    plus the far unit sphere of BIG_X[name], under the kernel matrix's camera, 8 spp."""
    cam = camera_spec(1.0, W, 12, 50.0, (0.0, 3.0, 9.0), (0.0, 0.3, -1.0), (0.0, 1.0, 0.0), 0.0, 9.0)
    return scenes.Scene("big_" + name.replace(" ", "_"), _spec("big", name, _big_scene(BIG_X[name])), cam,
                        fixed_spp(SPP))
