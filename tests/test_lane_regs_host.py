"""Host-side facts of the register lane state (no GPU): the block-limit hook's argument check,
and lane_state_in_regs / lane_nd / lane_ni as kernel_abi.hpp writes them -- no LDS lane field
for a fixed-spp sphere-leaf word, the LDS layout for every other."""
import os
import re

from grayshift_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIA, NESTED, VISITS, SPHLEAF, FIXED, GENERAL = 1, 2, 32, 64, 128, 512


def test_max_blocks_hook_arguments():
    try:
        assert N.lib.gs_debug_set_max_blocks(-1) == N.GS_ERR_ARG
        assert N.lib.gs_debug_set_max_blocks(2) == N.GS_OK
    finally:
        assert N.lib.gs_debug_set_max_blocks(0) == N.GS_OK


def test_the_predicate_names_the_fixed_sphere_leaf_kernels():
    hdr = open(os.path.join(ROOT, "grayshift_amd", "csrc", "device", "kernel_abi.hpp")).read()
    body = re.search(r"constexpr bool lane_state_in_regs\(int feat\) \{(.*?)\n\}", hdr, re.S).group(1)
    assert "GS_FEAT_FIXED" in body and "GS_FEAT_SPHLEAF" in body
    for excluded in ("GS_FEAT_MEDIA", "GS_FEAT_NESTED", "GS_FEAT_GENERAL", "GS_FEAT_VISITS"):
        assert excluded in body
    # both layout counts fall to zero under it, so lane_lds_bytes falls to its constant part
    for fn in ("lane_nd", "lane_ni"):
        m = re.search(r"constexpr uint32_t %s\([^)]*\) \{(.*?)\n\}" % fn, hdr, re.S)
        assert "lane_state_in_regs(feat) ? 0u" in m.group(1), fn
    for name, v in (("MEDIA", MEDIA), ("NESTED", NESTED), ("VISITS", VISITS), ("SPHLEAF", SPHLEAF),
                    ("FIXED", FIXED), ("GENERAL", GENERAL)):
        assert re.search(r"#define GS_FEAT_%s %d\b" % (name, v), hdr)
