#!/usr/bin/env python3
"""Ray-query rates on one GPU (gs_query_rays_async, csrc/device/query.hip), Mrays/s by HIP events:
the minimum of 5 runs after one warm-up, rays and records resident in HBM.

Cases (one process each, so every GPU step has its own time limit; --all runs them in turn and
stops at the first that fails):
  c4_camera      C4's world (bouncing_spheres, grid 50), the pixel-centre rays of its 1920 x 1080 camera
  c4_incoherent  the same world and ray count: random origins on a sphere round the scene, aimed at
                 random interior points
  final_camera   final_scene's world (a nested tree and two media), the pixel-centre rays of its camera
each in both modes (closest, any).  One JSON line per (case, mode): rays, hits, node visits per ray
(a counted run apart from the timed ones), ms and Mrays/s.

The comparison row is C4's traversal rate from the same session's `python bench.py` (its "value":
rays / time).  The query kernel has no LDS mirror, which the megakernel reads at nearly every node
visit; the rows show what that costs.

Usage: python tools/query_bench.py --all [--out FILE]   |   --case NAME [--runs 5]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("c4_camera", "c4_incoherent", "final_camera")
STEP_TIMEOUT = 240  # seconds per case (scene build and upload included)


def case_rays(name):
    import numpy as np
    import grayshift_amd as g
    from grayshift_amd import scenes
    from grayshift_amd.query import camera_rays
    sc = scenes.config("C4") if name.startswith("c4") else scenes.final_scene(width=1440)
    cam = g.camera(sc.camera)
    rays = camera_rays(cam)
    if name == "c4_incoherent":
        n = len(rays)
        rng = np.random.default_rng(1)
        v = rng.normal(size=(n, 3))
        o = 40.0 * v / np.linalg.norm(v, axis=1, keepdims=True) + np.array([0.0, 1.0, 0.0])
        tgt = rng.uniform(-11.0, 11.0, (n, 3))
        tgt[:, 1] = rng.uniform(0.0, 1.5, n)
        rays[:, 0:3], rays[:, 3:6] = o, tgt - o
    return sc, cam, rays


def run_case(name, runs):
    import numpy as np
    import torch
    from grayshift_amd import _native as N
    from grayshift_amd.query import HIT_DTYPE, RayQuery
    sc, cam, rays = case_rays(name)
    n = len(rays)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    with RayQuery(sc) as rq:
        d_rays = torch.from_numpy(rays).to(dev)
        d_hits = torch.zeros(n * HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(n * 8, dtype=torch.int32, device=dev)
        for mode, label in ((N.GS_QUERY_CLOSEST, "closest"), (N.GS_QUERY_ANY, "any")):
            def go(counts):
                N.check(N.lib.gs_query_rays_async(rq.dev, C.c_void_p(d_rays.data_ptr()), n, mode, 1,
                                                  C.c_void_p(d_hits.data_ptr()),
                                                  C.c_void_p(d_cnt.data_ptr()) if counts else None, sp))
            go(True)  # warm-up, and the counted run
            torch.cuda.synchronize()
            hits = d_hits.cpu().numpy().view(HIT_DTYPE)
            visits = d_cnt.cpu().numpy().view(np.uint32).reshape(n, 8)[:, 0]
            ms = []
            for _ in range(runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                go(False)
                e1.record(stream)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            print(json.dumps({"case": name, "mode": label, "rays": n, "image": "%dx%d" % (cam.image_width, cam.image_height),
                              "hits": int((hits["hit"] != 0).sum()),
                              "node_visits_per_ray": round(float(visits.mean()), 2),
                              "ms_min": round(min(ms), 4), "ms_all": [round(x, 4) for x in ms],
                              "Mrays_per_s": round(n / min(ms) / 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="with --all: also append the lines to this file")
    a = ap.parse_args()
    if a.all:
        for name in CASES:  # each GPU step a process of its own under its own time limit; the first failure ends the run
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--runs", str(a.runs)],
                                   stdout=subprocess.PIPE, text=True, timeout=STEP_TIMEOUT)
            except subprocess.TimeoutExpired:
                print("case %s ran past %d s: stopping" % (name, STEP_TIMEOUT), file=sys.stderr)
                return 124
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if a.out:
                with open(a.out, "a") as f:
                    f.write(p.stdout)
            if p.returncode != 0:
                print("case %s failed (status %d): stopping" % (name, p.returncode), file=sys.stderr)
                return p.returncode
        return 0
    if not a.case:
        ap.error("--case NAME or --all")
    run_case(a.case, a.runs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
