"""Every instantiation of views_round_kernel_for (csrc/device/render.hip), at bit parity with the
one-shot renders.  For every reachable row of tests/test_gpu_kernel_matrix.py that has a views form
(the GS_K and GS_KR rows), a two-view adaptation of the row's scene runs to the end; the launch must
have passed exactly F | FIXED | RSPLIT | VIEWS (GS_KR rows: the fixed kernel's sample loop over the
round's items) or F | VIEWS (GS_K rows: media / nested BVHs, the loop's kernel with per-sample items)
to the table (gs_debug_last_launch_feat), and each view must equal the adaptive one-shot render of
its camera bit for bit, the counters their sum.  tests/test_views_adaptive_host.py keeps the table
and these rows in step without a GPU."""
import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd.scene import sample_settings

from tests import test_gpu_kernel_matrix as M

pytestmark = pytest.mark.gpu

ROWS = [r for r in M.REACHABLE if "views" in r.forms]
SEEDS = [M.SEED, M.SEED + 4]


def form_bits(row):
    return M.FIXED | M.RSPLIT | M.VIEWS if row.macro == "GS_KR" else M.VIEWS


@pytest.mark.parametrize("row", ROWS, ids=M._ids(ROWS))
def test_views_rounds(row):
    cams = [M._camera(), M._camera((2.5, 2.0, 8.0))]
    sc = M._scene(row, sample_settings(*M.ADAPTIVE))
    with g.ViewsAdaptiveRenderer(sc, cams, seeds=SEEDS, tile=16) as r:
        res = r.render_rounds(M.ADAPTIVE[3] // M.ADAPTIVE[2] + 1, rgb=True)
        feat, info = M._last_feat(r._mr), r.scene_info()
    assert res["info"]["finished"]
    assert feat == M._launched(row, info, form_bits(row))
    one0, c0, _, _ = M._gpu(row, "loop")
    one1, c1, _, _ = M._render(M._scene(row, sample_settings(*M.ADAPTIVE), cams[1]), seed=SEEDS[1])
    assert np.array_equal(res["rgb"][0].view(np.int32), one0.view(np.int32))
    assert np.array_equal(res["rgb"][1].view(np.int32), one1.view(np.int32))
    assert res["info"]["counters"] == {k: c0[k] + c1[k] for k in c0}
