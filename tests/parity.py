"""The parity bar for whole-frame comparisons with the CPU oracle:
frames are bit-identical to the oracle's except where an ulp of OCML-vs-glibc libm difference
reroutes a sample, and such pixels are rare.

check(gpu, ref, same_association) measures and asserts, per frame:

  max_abs   the largest per-channel |delta|: < 1e-3, the north star's bar, as everywhere;
  far_px    pixels with a channel more than 1 f32 ulp from the oracle's (the distance is taken
            on the ordered int32 view of the bits; +0 and -0 are equal): <= cap, always;
  diff_px   pixels with a channel whose bits differ: <= cap too when the render adds its
            samples in the oracle's order (`same_association`: adaptive renders, and fixed-spp
            renders whose pixel is one chunk -- every fixed render of 16 spp or fewer under the
            auto chunk rule).  A render that adds several chunk sums rounds a differently
            associated f64 sum to f32 once: at most 1 ulp, so it is bound by far_px alone.

cap = max(1, ceil(4e-4 * pixels)): four times the worst whole-frame share of non-identical
pixels the project has recorded (final_scene at 1440^2 x 64 spp: 1e-4).  A reroute needs a
sample within an ulp of a threshold, so the share falls with the sample count and the test
frames (8-16 spp) sit well inside it.  The cap is a condition: it is not tuned to the device's
counts.  `libm_free` scenes -- metal, dielectric and solid-light materials over solid
textures, a solid background, no media: no libm call on the colour path -- take cap = 0.

A NaN in either frame fails.  The three counts are printed per call (pytest -s, or on failure).
"""
import math

import numpy as np

MAX_ABS = 1e-3
CAP_SHARE = 4e-4


def cap_for(pixels, libm_free=False):
    return 0 if libm_free else max(1, int(math.ceil(CAP_SHARE * pixels)))


def _ordered(a):
    """f32 bits as integers ordered like the values (int64, so distances cannot overflow);
    +0 and -0 both map to 0."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def measure(gpu, ref):
    """{'pixels', 'max_abs', 'far_px', 'diff_px', 'nan'} of two [..., 3] f32 frames."""
    gpu = np.ascontiguousarray(gpu, dtype=np.float32)
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    assert gpu.shape == ref.shape and gpu.shape[-1] == 3, (gpu.shape, ref.shape)
    g3, r3 = gpu.reshape(-1, 3), ref.reshape(-1, 3)
    nan = int(np.isnan(g3).sum() + np.isnan(r3).sum())
    with np.errstate(invalid="ignore"):
        max_abs = float(np.abs(g3.astype(np.float64) - r3.astype(np.float64)).max()) if g3.size else 0.0
    ulps = np.abs(_ordered(g3) - _ordered(r3))
    return {"pixels": int(g3.shape[0]), "max_abs": max_abs,
            "far_px": int((ulps > 1).any(axis=1).sum()),
            "diff_px": int((g3.view(np.int32) != r3.view(np.int32)).any(axis=1).sum()),
            "nan": nan}


def check(gpu, ref, same_association, libm_free=False, label=""):
    """Measure, print and assert (module docstring).  Returns measure()'s dict plus 'cap'."""
    m = measure(gpu, ref)
    m["cap"] = cap = cap_for(m["pixels"], libm_free)
    print("parity %s: pixels %d diff_px %d far_px %d max_abs %.3g (cap %d, %s association)" % (
        label, m["pixels"], m["diff_px"], m["far_px"], m["max_abs"], cap,
        "the oracle's" if same_association else "chunked"))
    assert m["nan"] == 0, "%s: %d NaN values" % (label, m["nan"])
    assert m["max_abs"] < MAX_ABS, "%s: max |delta| %g" % (label, m["max_abs"])
    assert m["far_px"] <= cap, "%s: %d pixels more than 1 ulp from the oracle (cap %d)" % (label, m["far_px"], cap)
    if same_association:
        assert m["diff_px"] <= cap, "%s: %d pixels differ from the oracle (cap %d)" % (label, m["diff_px"], cap)
    return m
