#!/usr/bin/env python3
"""What progressive passes cost: one frame rendered whole and in passes (C4 at 1920x1080, 512 spp,
chunk 16 by default).

    python tools/progressive_bench.py [--config C4] [--spp 512] [--chunk 16] [--out FILE.json]

Four runs of the same frame on one GPU, the frame left on the device:
  * gs_multi_render at --spp (under set_tuning(sample_chunk = --chunk), the passes' association);
  * the pass API as 1 x spp (when spp / chunk <= 64: one pass holds at most 64 chunks),
    spp/64 x 64 and spp/16 x 16 samples.
Each pass is timed with the library's own device events (gs_stats: render_ms_max = parameter,
megakernel and accumulate launches; kernel_ms_max = the megakernel alone) and each run with the
host clock around it.  The four frames must be bit-identical; the result goes to --out
(default profiles/progressive/pass_overhead.json).

    python tools/progressive_bench.py --adaptive [--config A2] [--out FILE.json]

The adaptive mode: a config with its scene's own adaptive settings (A2: cornell_box at 1024 x
1024) rendered by gs_multi_render and by the adaptation API with all rounds in one pass, 4 rounds
a pass and 1 round a pass, timed the same way (render_ms_max: a pass's parameter, round and
resolve launches).  Again the four frames must be bit-identical; the default --out is
profiles/progressive/adaptive_pass_overhead.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2, help="each run this many times; the fastest is reported")
    ap.add_argument("--adaptive", action="store_true", help="passes of batch rounds over the scene's own settings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "progressive",
                             "adaptive_pass_overhead.json" if a.adaptive else "pass_overhead.json")
    if a.adaptive and a.config == "C4":
        a.config = "A2"
    import numpy as np
    import grayshift_amd as g
    from grayshift_amd import _native as N, scenes
    from grayshift_amd.codeobj import code_object_hash

    if not a.adaptive and (a.spp % a.chunk or a.spp // a.chunk > 64):
        raise SystemExit("--spp must be 1 to 64 whole chunks (the 1 x spp run is one pass)")
    sc = scenes.config(a.config, width=a.width, spp=None if a.adaptive else a.spp)
    W, H = sc.width, sc.height
    runs = {}

    def download(ptr):
        out = np.zeros((H, W, 3), dtype=np.float32)
        N.check(N.lib.gs_device_download(out.ctypes.data, C.c_void_p(ptr), out.nbytes))
        return out

    def record(name, fn):
        """fn() -> (frame, per-pass gs_stats dicts, host ms); warm-up once, then the fastest of --reps."""
        fn()
        best = None
        for _ in range(a.reps):
            frame, passes, ms = fn()
            if best is None or ms < best["total_host_ms"]:
                best = {"total_host_ms": ms, "passes": len(passes),
                        "render_ms_sum": sum(p["render_ms_max"] for p in passes),
                        "kernel_ms_sum": sum(p["kernel_ms_max"] for p in passes),
                        "per_pass_render_ms": [round(p["render_ms_max"], 4) for p in passes],
                        "per_pass_kernel_ms": [round(p["kernel_ms_max"], 4) for p in passes]}
        runs[name] = best
        return frame

    if a.adaptive:
        return adaptive(a, sc, record, download, runs)

    # the one-shot frame, with the passes' chunk
    g.set_tuning(0, 0, 0, a.chunk)
    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        def one_shot():
            st = N.gs_stats()
            t0 = time.perf_counter()
            m.render_stats(a.seed, st)
            ms = (time.perf_counter() - t0) * 1e3
            return download(m.frame_ptr()[0]), [st.as_dict()], ms
        ref = record("gs_multi_render", one_shot)
    finally:
        m.close()
        g.set_tuning(0, 0, 0, -1)

    same = {}
    for n in sorted({a.spp, 64, 16}, reverse=True):
        if a.spp % n:
            continue

        def in_passes(n=n):
            with g.ProgressiveRenderer(sc, seed=a.seed, chunk=a.chunk) as p:
                t0 = time.perf_counter()
                stats = [p.render_pass(n, rgb=False)["stats"] for _ in range(a.spp // n)]
                ms = (time.perf_counter() - t0) * 1e3
                return download(p.frame_ptr()[0]), stats, ms
        name = "passes_%dx%d" % (a.spp // n, n)
        same[name] = bool(np.array_equal(record(name, in_passes), ref))

    base = runs["gs_multi_render"]
    for name, r in runs.items():
        r["render_ms_over_one_shot"] = r["render_ms_sum"] - base["render_ms_sum"]
        r["per_pass_overhead_ms"] = r["render_ms_over_one_shot"] / r["passes"]
    out = {"config": a.config, "width": W, "height": H, "spp": a.spp, "chunk": a.chunk, "seed": a.seed,
           "code_object": code_object_hash(N.LIB_PATH), "frames_bit_identical": same, "runs": runs,
           "note": "render_ms: device events around a pass's parameter, megakernel and accumulate launches; "
                   "total_host_ms: the host clock around the run's synchronous calls"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for name, r in runs.items():
        print("%-18s %3d passes  render %9.3f ms  kernel %9.3f ms  (+%.3f ms, %.4f ms a pass)  bit-identical %s" % (
            name, r["passes"], r["render_ms_sum"], r["kernel_ms_sum"], r["render_ms_over_one_shot"],
            r["per_pass_overhead_ms"], same.get(name, "-")))
    if not all(same.values()):
        raise SystemExit("frames differ: %s" % same)
    print("wrote", a.out)


def adaptive(a, sc, record, download, runs):
    import numpy as np
    import grayshift_amd as g
    from grayshift_amd import _native as N
    from grayshift_amd.codeobj import code_object_hash
    ss = sc.settings
    R = ss.max_samples // ss.batch_size + 1
    m = g.MultiRenderer(sc, num_gpus=1)
    try:
        def one_shot():
            st = N.gs_stats()
            t0 = time.perf_counter()
            m.render_stats(a.seed, st)
            ms = (time.perf_counter() - t0) * 1e3
            return download(m.frame_ptr()[0]), [st.as_dict()], ms
        ref = record("gs_multi_render", one_shot)
    finally:
        m.close()

    same, rounds_run = {}, {}
    for n in (R, 4, 1):
        def in_passes(n=n):
            with g.AdaptiveRenderer(sc, seed=a.seed) as p:
                stats = []
                t0 = time.perf_counter()
                while not p.finished:
                    stats.append(p.render_rounds(n, rgb=False)["stats"])
                ms = (time.perf_counter() - t0) * 1e3
                rounds_run[n] = int(p.info.rounds)
                return download(p.frame_ptr[0]), stats, ms
        name = "all_rounds_one_pass" if n == R else "%d_round%s_a_pass" % (n, "s" if n > 1 else "")
        same[name] = bool(np.array_equal(record(name, in_passes), ref))
        runs[name]["rounds_run"] = rounds_run[n]

    base = runs["gs_multi_render"]
    for name, r in runs.items():
        r["render_ms_over_one_shot"] = r["render_ms_sum"] - base["render_ms_sum"]
        r["per_pass_overhead_ms"] = r["render_ms_over_one_shot"] / r["passes"]
        if len(r["per_pass_render_ms"]) > 12:  # (keep the file small: the first and last passes)
            r["per_pass_render_ms"] = r["per_pass_render_ms"][:6] + ["..."] + r["per_pass_render_ms"][-5:]
            r["per_pass_kernel_ms"] = r["per_pass_kernel_ms"][:6] + ["..."] + r["per_pass_kernel_ms"][-5:]
    out = {"config": a.config, "width": sc.width, "height": sc.height, "seed": a.seed,
           "settings": {"confidence": ss.confidence, "tolerance": ss.tolerance, "batch_size": ss.batch_size,
                        "max_samples": ss.max_samples, "max_rounds": R},
           "code_object": code_object_hash(N.LIB_PATH), "frames_bit_identical": same, "runs": runs,
           "note": "render_ms: device events around a pass's parameter, round (parameters, megakernel, fold) and "
                   "resolve launches; the one-shot render enqueues all max_rounds rounds, a pass form stops at the "
                   "first pass that ends with no active pixel; total_host_ms: the host clock around the run"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for name, r in runs.items():
        print("%-22s %3d passes  render %9.3f ms  kernel %9.3f ms  host %9.3f ms  (+%.3f ms, %.4f ms a pass)  "
              "bit-identical %s" % (name, r["passes"], r["render_ms_sum"], r["kernel_ms_sum"], r["total_host_ms"],
                                    r["render_ms_over_one_shot"], r["per_pass_overhead_ms"], same.get(name, "-")))
    if not all(same.values()):
        raise SystemExit("frames differ: %s" % same)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
