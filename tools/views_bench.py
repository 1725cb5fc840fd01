#!/usr/bin/env python3
"""What a views call buys: V cameras of one world as V frames in a loop and as one launch.

    python tools/views_bench.py [--config C1] [--views 16] [--reps 5] [--out FILE.txt]

In one process, on one GPU, for a config and a V: V consecutive MultiRenderer.render(rgb=False)
calls (one per camera, the frame left on the device) alternate with one
MultiRenderer.render_views(rgb=False) call over the same V cameras -- an orbit of the config's
look_from around its look_at.  Both are warmed first and the device is idle before each timed
run (every call is synchronous).  Each repetition is printed: the host clock around the run and
the sum of the library's device events (gs_stats render_ms_max: parameter, megakernel and
combine launches; kernel_ms_max: the megakernel alone), then the min-max of both forms and the
ratio per view.  The views call runs with gs_views_chunk's chunk, so its frames are the loop's,
bit for bit; the tool checks that once, outside the timed runs."""
import argparse
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def orbit(spec, n):
    """n camera specs: spec's look_from turned about the vertical through look_at, 360 / n degrees apart."""
    from grayshift_amd import _native as N
    out = []
    for v in range(n):
        c = N.gs_camera_spec.from_buffer_copy(spec)
        t = 2.0 * math.pi * v / n
        dx, dz = spec.look_from[0] - spec.look_at[0], spec.look_from[2] - spec.look_at[2]
        c.look_from[0] = spec.look_at[0] + dx * math.cos(t) + dz * math.sin(t)
        c.look_from[2] = spec.look_at[2] - dx * math.sin(t) + dz * math.cos(t)
        out.append(c)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
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

    sc = scenes.config(a.config, width=a.width, spp=a.spp)
    ss = sc.settings
    if ss.max_samples >= ss.batch_size:
        raise SystemExit("a views call is fixed spp: give --spp for an adaptive config")
    spp, V = int(ss.batch_size), a.views
    specs = orbit(sc.camera, V)
    cams = [g.camera(s) for s in specs]
    W, H = cams[0].image_width, cams[0].image_height
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        chunk = m.views_chunk(cams[0], spp)
        st = N.gs_stats()

        def loop():
            dev = kern = 0.0
            t0 = time.perf_counter()
            for cam in cams:
                m.cam = cam
                m.render_stats(a.seed, st)
                dev += st.render_ms_max
                kern += st.kernel_ms_max
            return (time.perf_counter() - t0) * 1e3, dev, kern

        def views():
            t0 = time.perf_counter()
            r = m.render_views(specs, spp, [a.seed] * V, chunk=chunk, rgb=False)
            ms = (time.perf_counter() - t0) * 1e3
            return ms, r["stats"]["render_ms_max"], r["stats"]["kernel_ms_max"]

        # the same frames: once, outside the timed runs
        got = m.render_views(specs, spp, [a.seed] * V, chunk=chunk, rgb=True)["rgb"]
        same = True
        for v, cam in enumerate(cams):
            m.cam = cam
            same = same and bool(np.array_equal(m.render(seed=a.seed, rgb=True)["rgb"], got[v]))
        for _ in range(a.warmup):
            loop()
            views()
        say("%s %dx%d x %d spp, V = %d, chunk %d, code object %s, frames bit-identical %s" % (
            a.config, W, H, spp, V, chunk, code_object_hash(N.LIB_PATH), same))
        res = {"loop": [], "views": []}
        for k in range(a.reps):
            for name, fn in (("loop", loop), ("views", views)):
                ms, dev, kern = fn()
                res[name].append((ms, dev, kern))
                say("rep %d %-5s host %9.3f ms  device %9.3f ms  kernel %9.3f ms  (%.4f ms a view, host)" % (
                    k, name, ms, dev, kern, ms / V))
        for name in ("loop", "views"):
            for j, what in enumerate(("host", "device", "kernel")):
                xs = [r[j] for r in res[name]]
                say("%-5s %-6s min %9.3f  max %9.3f ms   per view min %.4f  max %.4f ms" % (
                    name, what, min(xs), max(xs), min(xs) / V, max(xs) / V))
        for j, what in enumerate(("host", "device", "kernel")):
            lo = min(r[j] for r in res["loop"])
            vo = min(r[j] for r in res["views"])
            say("views / loop (%s, min over reps): %.3f" % (what, vo / lo))
        if not same:
            raise SystemExit("the views call's frames differ from the loop's")
    finally:
        m.close()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
