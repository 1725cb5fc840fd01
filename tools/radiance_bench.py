#!/usr/bin/env python3
"""Radiance-query rates on one GPU (gs_query_radiance_async, csrc/device/radiance.hip) by HIP events:
the minimum of 5 runs after one warm-up, rays, records and scratch resident in HBM.

Cases (one process each, so every GPU step has its own time limit; --all runs them in turn and
stops at the first that fails), all on C4's world (bouncing_spheres, grid 50) at max_depth 50:
  c4_camera    the pixel-centre rays of its 1920 x 1080 camera
  c4_panorama  an equirectangular camera at the same ray count (1920 x 1080 directions over the full
               sphere) from the camera's centre
each at 1 and at 16 samples per ray (one chunk per ray either way, so no scratch and no combine).
One JSON line per (case, samples): paths, rays (the batch's counters, from a counted run apart from
the timed ones), rays per path, ms, Mpaths/s and Mrays/s.

The yardstick row is C4 from the same session's `python bench.py` (its "value": rays / time).  The
megakernel reads its node visits from an LDS mirror and steps its waves in passes; this kernel walks
one record per step from global memory, so it is expected to be several times slower per ray.

--batches 1,8,24,64 repeats every row for those shade batches (gs_debug_set_radiance_batch: the lanes
of a wave that wait at their walk's end before the wave shades them; 0 = the default).

Usage: python tools/radiance_bench.py --all [--out FILE] [--batches LIST]   |   --case NAME [--runs 5]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("c4_camera", "c4_panorama")
SAMPLES = (1, 16)
MAX_DEPTH = 50
STEP_TIMEOUT = 240  # seconds per case (scene build and upload included)


def case_rays(name):
    import numpy as np
    import grayshift_amd as g
    from grayshift_amd import scenes
    from grayshift_amd.query import camera_rays, panorama_rays
    sc = scenes.config("C4")
    cam = g.camera(sc.camera)
    if name == "c4_camera":
        return sc, cam, camera_rays(cam)
    return sc, cam, panorama_rays(np.array(cam.center[:]), cam.image_width, cam.image_height)


def run_case(name, runs, batches):
    import torch
    from grayshift_amd import _native as N
    from grayshift_amd.query import RADIANCE_DTYPE, RayQuery
    sc, cam, rays = case_rays(name)
    n = len(rays)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    with RayQuery(sc) as rq:
        d_rays = torch.from_numpy(rays).to(dev)
        d_out = torch.zeros(n * RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(16, dtype=torch.int64, device=dev)
        for samples, batch in ((s, b) for s in SAMPLES for b in batches):
            N.check(N.lib.gs_debug_set_radiance_batch(batch))
            assert N.lib.gs_query_radiance_scratch_bytes(n, samples, 0) == 0  # one chunk per ray

            def go(counted):
                N.check(N.lib.gs_query_radiance_async(rq.dev, C.c_void_p(d_rays.data_ptr()), n, samples, 0, MAX_DEPTH, 1,
                                                      None, C.c_void_p(d_out.data_ptr()),
                                                      C.c_void_p(d_cnt.data_ptr()) if counted else None, None, 0, sp))
            d_cnt.zero_()
            go(True)  # warm-up, and the counted run
            torch.cuda.synchronize()
            cnt = dict(zip(N.COUNTER_NAMES, (int(x) for x in d_cnt.cpu().numpy())))
            out = d_out.cpu().numpy().view(RADIANCE_DTYPE)
            ms = []
            for _ in range(runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                go(False)
                e1.record(stream)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            print(json.dumps({"case": name, "samples": samples, "shade_batch": batch, "max_depth": MAX_DEPTH, "rays_in": n,
                              "image": "%dx%d" % (cam.image_width, cam.image_height), "paths": cnt["paths"],
                              "rays": cnt["rays"], "rays_per_path": round(cnt["rays"] / cnt["paths"], 3),
                              "node_visits_per_ray": round(cnt["node_visits"] / cnt["rays"], 2),
                              "mean_rgb": [round(float(x), 4) for x in out["rgb"].mean(axis=0) / samples],
                              "ms_min": round(min(ms), 4), "ms_all": [round(x, 4) for x in ms],
                              "Mpaths_per_s": round(cnt["paths"] / min(ms) / 1e3, 1),
                              "Mrays_per_s": round(cnt["rays"] / min(ms) / 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", default="0", help="comma-separated shade batches, 0 = the default")
    ap.add_argument("--out", default=None, help="with --all: also append the lines to this file")
    a = ap.parse_args()
    if a.all:
        for name in CASES:  # each GPU step a process of its own under its own time limit; the first failure ends the run
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--runs", str(a.runs),
                                    "--batches", a.batches],
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
    run_case(a.case, a.runs, [int(x) for x in a.batches.split(",")])
    return 0


if __name__ == "__main__":
    sys.exit(main())
