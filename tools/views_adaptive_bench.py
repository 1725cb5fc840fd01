#!/usr/bin/env python3
"""What adaptive views buy: a batch of cameras under the scene's adaptive settings, in batch rounds
on the tall frame, against a loop of single adaptive frames.

    python tools/views_adaptive_bench.py [--config A2] [--width 128] [--views 1,4,16] [--reps 3] [--out FILE.txt]

In one process, on one GPU and ONE frame context, for a config (its own adaptive settings) and
V cameras (the config's look_from turned about the vertical through its look_at, spread over an
arc of 40 degrees: a camera path that keeps the scene in view):

  batch  gs_multi_views_adapt_begin, three passes (round 0; rounds 1 .. R-2; round R-1), _end;
  loop   for each camera: gs_multi_adapt_begin, the same three passes, _end -- existing code that
         this feature does not touch, so a fair comparator.

Every form is warmed first and every call is synchronous, so the device is idle before each timed
run.  Each repetition prints the host clock around the whole form (begin to end, state allocation
included) and the library's device events (gs_stats render_ms_max: every parameter, megakernel and
fold launch of the pass, and the resolve) of all passes, of round 0 and of the last round that ran;
then the min-max of each and the ratios of the minima.  Before anything is timed the tool checks
that every view of the batch is bit for bit its single frame."""
import argparse
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="A2")
    ap.add_argument("--width", type=int, default=None, help="frame width (default: the config's own)")
    ap.add_argument("--views", default="1,4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    a = ap.parse_args()
    import numpy as np
    import grayshift_amd as g
    from grayshift_amd import _native as N, scenes
    from grayshift_amd.codeobj import code_object_hash

    def arc(spec, n, degrees=40.0):
        out = []
        for v in range(n):
            c = N.gs_camera_spec.from_buffer_copy(spec)
            t = math.radians(degrees) * (v / (n - 1) - 0.5) if n > 1 else 0.0
            dx, dz = spec.look_from[0] - spec.look_at[0], spec.look_from[2] - spec.look_at[2]
            c.look_from[0] = spec.look_at[0] + dx * math.cos(t) + dz * math.sin(t)
            c.look_from[2] = spec.look_at[2] - dx * math.sin(t) + dz * math.cos(t)
            out.append(c)
        return out

    sc = scenes.config(a.config, width=a.width)
    ss = sc.settings
    if ss.max_samples < ss.batch_size:
        raise SystemExit("config %s has no adaptive settings" % a.config)
    R = ss.max_samples // ss.batch_size + 1
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m = g.MultiRenderer(sc, num_gpus=1, plan=False)
    h, L = m.handle, N.lib

    def passes(call, frames=None):
        """Round 0, the middle rounds, the last round: (device ms of all, of round 0, of the last
        round that ran).  frames: [rows, W, 3] f32 to receive the last pass's frame."""
        st = N.gs_stats()
        out = None
        if frames is not None:
            out = N.gs_multi_outputs()
            out.rgb = frames.ctypes.data
        ms = []
        for n in (1, max(R - 2, 1), 1):
            last = len(ms) == 2
            N.check(call(h, n, C.byref(out) if (out is not None and last) else None, C.byref(st)))
            ms.append(st.render_ms_max)
        return sum(ms), ms[0], ms[2]

    def views_of(specs):
        v = (N.gs_view * len(specs))()
        for k, s in enumerate(specs):
            v[k].cam, v[k].seed = g.camera(s), a.seed
        return v

    def batch(views, frames=None):
        N.check(L.gs_multi_views_adapt_begin(h, views, len(views), C.byref(ss)))
        try:
            return passes(L.gs_multi_views_adapt_pass, frames)
        finally:
            L.gs_multi_views_adapt_end(h)

    def loop(views, frames=None):
        tot = [0.0, 0.0, 0.0]
        for k in range(len(views)):
            N.check(L.gs_multi_adapt_begin(h, C.byref(views[k].cam), C.byref(ss), views[k].seed))
            try:
                r = passes(L.gs_multi_adapt_pass, frames[k] if frames is not None else None)
            finally:
                L.gs_multi_adapt_end(h)
            tot = [x + y for x, y in zip(tot, r)]
        return tuple(tot)

    try:
        for V in [int(v) for v in a.views.split(",")]:
            specs = arc(sc.camera, V)
            views = views_of(specs)
            W, H = views[0].cam.image_width, views[0].cam.image_height
            got = np.zeros((V, H, W, 3), dtype=np.float32)
            want = np.zeros((V, H, W, 3), dtype=np.float32)
            batch(views, got.reshape(V * H, W, 3))
            loop(views, want)
            same = bool(np.array_equal(got.view(np.int32), want.view(np.int32)))
            say("%s %dx%d, V = %d, batch %d, max_samples %d (R = %d), code object %s, frames bit-identical %s" % (
                a.config, W, H, V, ss.batch_size, ss.max_samples, R, code_object_hash(N.LIB_PATH), same))
            if not same:
                raise SystemExit("the batch's frames differ from the single frames'")
            forms = [("batch", batch), ("loop", loop)]
            for _ in range(a.warmup):
                for _, fn in forms:
                    fn(views)
            res = {name: [] for name, _ in forms}
            for k in range(a.reps):
                for name, fn in forms:
                    t0 = time.perf_counter()
                    dev = fn(views)
                    ms = (time.perf_counter() - t0) * 1e3
                    res[name].append((ms,) + dev)
                    say("V %2d rep %d %-5s host %10.3f ms  device %10.3f ms  round 0 %9.3f ms  last round %8.3f ms" % (
                        (V, k, name, ms) + dev))
            cols = ("host", "device", "round 0", "last round")
            for name, _ in forms:
                for j, what in enumerate(cols):
                    xs = [r[j] for r in res[name]]
                    say("V %2d %-5s %-10s min %10.3f  max %10.3f ms" % (V, name, what, min(xs), max(xs)))
            for j, what in enumerate(cols):
                say("V %2d batch / loop (%s, min over reps): %.3f" % (
                    V, what, min(r[j] for r in res["batch"]) / min(r[j] for r in res["loop"])))
    finally:
        m.close()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
