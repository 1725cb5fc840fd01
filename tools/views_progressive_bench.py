#!/usr/bin/env python3
"""What progressive views cost and buy: a batch of cameras refined in passes, view by view.

    python tools/views_progressive_bench.py [--config C1] [--views 16] [--spp 64] [--reps 5] [--out FILE.txt]

In one process, on one GPU, for a config, V cameras (an orbit of the config's look_from around its
look_at) and a total of S samples per pixel, three measurements, each against a baseline that is
not the code under test:

 (a) what a pass costs: ViewsProgressiveRenderer running S samples of all V views as 1, 4 and 16
     passes, against one MultiRenderer.render_views call of S samples;
 (b) what the batch buys: the same passes against a loop over V single-camera
     ProgressiveRenderers, each running the same passes;
 (c) what the empty slots cost: one pass of S samples with every other view unselected, against
     one pass of S samples over a batch of only the selected views.

Every form is warmed first and every call is synchronous, so the device is idle before each timed
run.  Each repetition is printed: the host clock around the run and the sum of the library's
device events (gs_stats render_ms_max: parameter, megakernel and combine launches of every
launch), then the min-max of each form and the ratios of the minima.  Before anything is timed the
tool checks that the passes' frames are bit for bit render_views', the loop's sums are the
batch's, and the half-selected pass's frames are the small batch's."""
import argparse
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--spp", type=int, default=64, help="S: total samples per pixel (16 whole chunks or more)")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    a = ap.parse_args()
    import numpy as np
    import grayshift_amd as g
    from grayshift_amd import _native as N, scenes
    from grayshift_amd.codeobj import code_object_hash
    from views_bench import orbit

    sc = scenes.config(a.config, width=a.width, spp=a.spp)
    S, V = a.spp, a.views
    if V < 2 or V % 2:
        raise SystemExit("--views: an even number, 2 or more")
    specs = orbit(sc.camera, V)
    seeds = [a.seed] * V
    half = list(range(0, V, 2))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = g.MultiRenderer(sc, num_gpus=1, plan=False)
    chunk = m.views_chunk(g.camera(specs[0]), S)
    if S % (16 * chunk):
        raise SystemExit("--spp %d is not 16 whole chunks of %d" % (S, chunk))
    batch = g.ViewsProgressiveRenderer(sc, specs, seeds=seeds, chunk=chunk)
    small = g.ViewsProgressiveRenderer(sc, [specs[v] for v in half], seeds=[a.seed] * len(half), chunk=chunk)
    loop = [g.ProgressiveRenderer(dataclasses.replace(sc, camera=s), seed=a.seed, chunk=chunk, plan=False) for s in specs]
    W, H = batch.width, batch.height
    try:
        # ---- the same bits, once, before anything is timed
        want = m.render_views(specs, S, seeds, chunk=chunk, rgb=True)["rgb"]
        for _ in range(3):
            batch.render_pass(S // 4, rgb=False)
        got = batch.render_pass(S // 4, rgb=True)["rgb"]
        same = bool(np.array_equal(got, want))
        bsums = batch.sums()
        for v, p in enumerate(loop):
            p.render_pass(S, rgb=False)
            same = same and p.sums().tobytes() == bsums[v].tobytes()
        small.render_pass(S, rgb=False)
        sel = batch.render_pass(S, half, rgb=True)["rgb"]   # the selected views at 2 S, the others still at S
        sml = small.render_pass(S, rgb=True)["rgb"]
        same = same and all(bool(np.array_equal(sel[v], sml[k])) for k, v in enumerate(half))
        same = same and all(bool(np.array_equal(sel[v], want[v])) for v in range(1, V, 2))
        batch.render_pass(S, list(range(1, V, 2)), rgb=False)  # (even counts again)
        say("%s %dx%d, V = %d, S = %d spp, chunk %d, tile_h %d, code object %s, frames bit-identical %s" % (
            a.config, W, H, V, S, chunk, batch.info["tile_h"], code_object_hash(N.LIB_PATH), same))
        if not same:
            raise SystemExit("progressive views' frames differ from their baselines'")

        def timed(fn):
            t0 = time.perf_counter()
            dev = fn()
            return (time.perf_counter() - t0) * 1e3, dev

        def one_shot():
            return m.render_views(specs, S, seeds, chunk=chunk, rgb=False)["stats"]["render_ms_max"]

        def passes(k):
            return lambda: sum(batch.render_pass(S // k, rgb=False)["stats"]["render_ms_max"] for _ in range(k))

        def loop_passes(k):
            return lambda: sum(p.render_pass(S // k, rgb=False)["stats"]["render_ms_max"] for _ in range(k) for p in loop)

        def half_pass():
            return batch.render_pass(S, half, rgb=False)["stats"]["render_ms_max"]

        def small_pass():
            return small.render_pass(S, rgb=False)["stats"]["render_ms_max"]

        def even_out():  # (untimed, after half_selected: the other views catch up, so a pass is one launch again)
            batch.render_pass(S, list(range(1, V, 2)), rgb=False)

        forms = [("render_views", one_shot, None)]
        forms += [("passes_%d" % k, passes(k), None) for k in (1, 4, 16)]
        forms += [("loop_%d" % k, loop_passes(k), None) for k in (1, 4, 16)]
        forms += [("half_selected", half_pass, even_out), ("half_batch", small_pass, None)]
        for _ in range(a.warmup):
            for _, fn, after in forms:
                fn()
                if after:
                    after()
        res = {name: [] for name, _, _ in forms}
        for k in range(a.reps):
            for name, fn, after in forms:
                ms, dev = timed(fn)
                if after:
                    after()
                res[name].append((ms, dev))
                say("rep %d %-13s host %9.3f ms  device %9.3f ms" % (k, name, ms, dev))
        for name, _, _ in forms:
            for j, what in enumerate(("host", "device")):
                xs = [r[j] for r in res[name]]
                say("%-13s %-6s min %9.3f  max %9.3f ms" % (name, what, min(xs), max(xs)))

        def lo(name, j):
            return min(r[j] for r in res[name])

        for j, what in enumerate(("host", "device")):
            for k in (1, 4, 16):
                say("(a) passes_%d / render_views (%s, min over reps): %.3f" % (k, what, lo("passes_%d" % k, j) / lo("render_views", j)))
            for k in (1, 4, 16):
                say("(b) passes_%d / loop_%d (%s, min over reps): %.3f" % (k, k, what, lo("passes_%d" % k, j) / lo("loop_%d" % k, j)))
            say("(c) half_selected / half_batch (%s, min over reps): %.3f" % (what, lo("half_selected", j) / lo("half_batch", j)))
    finally:
        for r in [m, batch, small] + loop:
            r.close()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
