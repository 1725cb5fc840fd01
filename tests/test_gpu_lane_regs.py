"""The fixed-spp sphere-leaf kernels keep their lane state in registers (kernel_abi.hpp,
lane_state_in_regs; render.hip's LD / LI) and the block's LDS goes to the mirror.

One scene: 100 x 60 = 6000 stationary spheres of Lambertian, metal and dielectric -- 6000 leaf and at
least 5999 node records, more than 480 KB, which no LDS holds -- whose word is SPHLEAF | LEAFRUN | MIXED | PLAIN
(340: the flagship's).  Every comparison is exact: frames with np.array_equal, counter dicts with ==.

  test_registers_survive_item_handover   96 x 64 x 40 spp fixed in 16-sample chunks (16, 16 and a
      short 8) on one tile and 1-sample tail items on the other, on 2 blocks
      (gs_debug_set_max_blocks), so each of the 2048 lanes runs many items of all three kinds in
      turn: the oracle's frame and counters.
  test_results_do_not_depend_on_the_cut   the same render under mirror budgets of 24 KiB, the
      LDS layout's maximum (111 KiB) and the block's own: equal frames and counters, and the
      largest mirror lies where the LDS layout could not reach.
  test_views_equal_their_own_renders      two cameras at 64 x 48 in one launch (F | FIXED | VIEWS).
  test_split_rounds_equal_the_loop        adaptive settings in split batch rounds (F | FIXED |
      RSPLIT) against the per-lane loop (F, lane state in LDS).
  test_the_lds_went_to_the_mirror         scene_info's prefixes after a chunked fixed launch: more
      than 150 KiB of a 160-KiB block.

Every hook is set by `_set`, which puts all of them back to the library's defaults on exit.
"""
import numpy as np
import pytest

import grayshift_amd as g
from grayshift_amd import _native as N
from grayshift_amd import scenes
from grayshift_amd.scene import camera_spec, fixed_spp, sample_settings
import oracle

from tests import test_gpu_kernel_matrix as KM

pytestmark = pytest.mark.gpu

FEAT = KM.SPHLEAF | KM.LEAFRUN | KM.MIXED | KM.PLAIN
SEED = 11
SPP = 40
ADAPTIVE = (0.95, 0.05, 4, 16)  # confidence, tolerance, batch, max samples: up to five batches
OLD_MAX = 160 * 1024 - 1024 * (3 * 8 + 6 * 4) - 1024  # the mirror's budget beside the lane state in LDS


class _set:
    """The process-wide hooks for one block; on exit every one goes back to the library's default."""
    def __init__(self, chunk=-1, tail=0, blocks=0, budget=-1, mode=1, items=0):
        self.chunk, self.tail, self.blocks, self.budget, self.mode, self.items = chunk, tail, blocks, budget, mode, items

    def __enter__(self):
        try:
            g.set_tuning(0, 0, 0, self.chunk)
            N.check(N.lib.gs_debug_set_guided_tail(1 if self.tail else 0, self.tail))
            N.check(N.lib.gs_debug_set_max_blocks(self.blocks))
            N.check(N.lib.gs_debug_set_mirror_budget(self.budget))
            N.check(N.lib.gs_set_adaptive_mode(self.mode))
            N.check(N.lib.gs_debug_set_round_items(self.items))
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        g.set_tuning(0, 0, 0, -1)
        N.check(N.lib.gs_debug_set_guided_tail(0, 0))
        N.check(N.lib.gs_debug_set_max_blocks(0))
        N.check(N.lib.gs_debug_set_mirror_budget(-1))
        N.check(N.lib.gs_set_adaptive_mode(1))
        N.check(N.lib.gs_debug_set_round_items(0))


def _camera(width, height, look_from=(0.0, 3.0, 9.0)):
    return camera_spec(width / height, width, 12, 50.0, look_from, (0.0, 0.3, -1.0), (0.0, 1.0, 0.0), 0.0, 9.0)


_SPEC = []


def _spec():
    if not _SPEC:
        b = g.SceneBuilder()
        b.background_solid((0.6, 0.7, 0.9))
        KM._field(b, KM._mats(b, "LMD"), "sphere", nx=100, nz=60)
        _SPEC.append(b.build())
    return _SPEC[0]


def _scene(settings, cam):
    return scenes.Scene("lane_regs", _spec(), cam, settings)


def _render(sc, seed=SEED, views=None, view_seeds=None, **hooks):
    """One render on a fresh one-device context under `hooks` (_set's arguments): (frame, counters,
    the launched feature word, scene_info).  views: cameras for one views launch."""
    with _set(**hooks):
        r = g.MultiRenderer(sc, num_gpus=1, plan=False)
        try:
            out = r.render_views(views, sc.settings.batch_size, view_seeds) if views else r.render(seed=seed, rgb=True)
            return out["rgb"], out["counters"], KM._last_feat(r), r.scene_info()
        finally:
            r.close()


def _mirror_bytes(info):
    return 32 * info["lds_nodes"] + 48 * info["lds_leaves"]


_CACHE = {}


def _fixed_scene():
    return _scene(fixed_spp(SPP), _camera(96, 64))


def _oracle_fixed():
    if "oracle" not in _CACHE:
        _CACHE["oracle"] = oracle.render(_fixed_scene(), seed=SEED)
    return _CACHE["oracle"]


def _handover():
    """The 2-block render in 16-sample chunks with a tail of 1-sample items, once."""
    if "handover" not in _CACHE:
        # (tail 1: 1% of the device's lanes x 16 samples -- one 64 x 64 tile of the frame's two)
        _CACHE["handover"] = _render(_fixed_scene(), chunk=16, tail=1, blocks=2)
    return _CACHE["handover"]


def _diff(label, a, ca, b, cb):
    px = int((a.view(np.int32) != b.view(np.int32)).any(axis=-1).sum()) if a.shape == b.shape else -1
    dc = {k: (ca.get(k), v) for k, v in cb.items() if ca.get(k) != v}
    print("lane_regs %s: diff_px %d diff_counters %s" % (label, px, dc))


def test_registers_survive_item_handover():
    out, gc, feat, info = _handover()
    ref, rc = _oracle_fixed()
    assert info["feat"] == FEAT and feat == FEAT | KM.FIXED
    assert info["node_records"] >= 5999 and info["leaf_records"] == 6000
    assert 32 * info["node_records"] + 48 * info["leaf_records"] > 480000  # (no block's LDS holds the tree)
    assert info["lds_nodes"] < info["node_records"] and info["lds_leaves"] < 6000  # lanes read global memory too
    _diff("2 blocks, chunks 16 + tail vs oracle", out, gc, ref, rc)
    assert gc["paths"] == 96 * 64 * SPP and gc["pixels"] == 96 * 64
    assert np.array_equal(out, ref)
    assert gc == rc


def test_results_do_not_depend_on_the_cut():
    base, bc, _, _ = _handover()
    sizes = []
    for budget in (24 * 1024, OLD_MAX, -1):
        out, gc, feat, info = _render(_fixed_scene(), chunk=16, tail=1, blocks=2, budget=budget)
        assert feat == FEAT | KM.FIXED
        if budget >= 0:
            assert budget - 48 < _mirror_bytes(info) <= budget, (budget, info)
        sizes.append(_mirror_bytes(info))
        _diff("budget %d (mirror %d B)" % (budget, sizes[-1]), out, gc, base, bc)
        assert np.array_equal(out, base) and gc == bc
    assert sizes[0] < sizes[1] < sizes[2]
    assert sizes[2] > OLD_MAX  # the largest cut: out of the LDS layout's reach


def test_views_equal_their_own_renders():
    cams = [_camera(64, 48), _camera(64, 48, (2.5, 2.0, 8.0))]
    seeds = [SEED, SEED + 4]
    sc = _scene(fixed_spp(8), cams[0])
    got, gc, feat, _ = _render(sc, views=cams, view_seeds=seeds)
    assert feat == FEAT | KM.FIXED | KM.VIEWS
    total = {}
    for v in (0, 1):
        one, oc, f1, _ = _render(_scene(fixed_spp(8), cams[v]), seed=seeds[v])
        assert f1 == FEAT | KM.FIXED
        _diff("view %d" % v, got[v], gc, one, gc)
        assert np.array_equal(got[v], one)
        total = {k: total.get(k, 0) + n for k, n in oc.items()}
    assert gc == total


def test_split_rounds_equal_the_loop():
    sc = _scene(sample_settings(*ADAPTIVE), _camera(64, 48))
    loop, lc, lf, _ = _render(sc, mode=0)
    assert lf == FEAT
    out, gc, feat, _ = _render(sc, mode=2, items=0)
    assert feat == FEAT | KM.FIXED | KM.RSPLIT
    _diff("split rounds vs loop", out, gc, loop, lc)
    assert lc["pixels"] == 64 * 48 and lc["paths"] > 4 * 64 * 48  # (some pixels took further batches)
    assert np.array_equal(out, loop) and gc == lc


def test_the_lds_went_to_the_mirror():
    _, _, feat, info = _handover()
    assert feat == FEAT | KM.FIXED
    assert _mirror_bytes(info) > 150 * 1024, info
