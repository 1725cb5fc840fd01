#!/usr/bin/env python3
"""Generated radiance queries (gs_query_radiance_gen_async, csrc/device/raygen.hip) against the two
routes there were before, on one GPU by HIP events: the minimum of 5 runs after one warm-up.

Cases (one process each, so every GPU step has its own time limit; --all runs them in turn and stops
at the first that fails), on C4's world (bouncing_spheres, grid 50) at max_depth 50, 1920 x 1080 items:
  c4_camera    GS_GEN_CAMERA of its camera (jitter, defocus disk, time)
  c4_panorama  GS_GEN_PANORAMA from the camera's centre (jitter, time)
  c4_hemisphere  GS_GEN_HEMISPHERE about 1920 x 1080 points of a grid just above the ground, normals up: a
               light-map bake of the floor (the point reloaded and the basis rebuilt for every sample)
each at 1 and at 16 samples per item, one chunk per item.  One JSON line per (case, samples), three
columns:
  gen        the generated call
  fixed      gs_query_radiance_async on one fixed ray per item (the pixel's or texel's centre; the point's normal) at the same
             sample count: the kernel before the generators, the per-ray ceiling
  uploaded   the route for distinct rays before the generators: n x samples rays and stream states
             (80 B per sample; here the very rays and streams the generated call emits) through
             gs_query_radiance_async at samples = 1 -- the kernel alone, and with the upload from pinned
             host memory in front of it
Each column has its own counted run for its rays (a fixed ray's paths are not a jittered ray's).

Usage: python tools/raygen_bench.py --all [--out FILE]   |   --case NAME [--runs 5]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("c4_camera", "c4_panorama", "c4_hemisphere")
SAMPLES = (1, 16)
MAX_DEPTH = 50
STEP_TIMEOUT = 300  # seconds per case (scene build and upload included)


def run_case(name, runs):
    import numpy as np
    import torch
    import grayshift_amd as g
    from grayshift_amd import _native as N
    from grayshift_amd import scenes
    from grayshift_amd.query import RADIANCE_DTYPE, RayGen, RayQuery, camera_rays, panorama_rays
    sc = scenes.config("C4")
    cam = g.camera(sc.camera)
    w, h = cam.image_width, cam.image_height
    n = w * h
    if name == "c4_camera":
        gen, centre = RayGen.camera(cam), camera_rays(cam)
    elif name == "c4_panorama":
        gen, centre = RayGen.panorama(np.array(cam.center[:]), w, h), panorama_rays(np.array(cam.center[:]), w, h)
    else:  # the ground is a sphere of radius 1000 about (0, -1000, 0): y = 0.01 clears it over the whole grid
        z, x = np.meshgrid(np.linspace(-11.0, 11.0, h), np.linspace(-11.0, 11.0, w), indexing="ij")
        pts = np.column_stack([x.reshape(-1), np.full(n, 0.01), z.reshape(-1)])
        gen = RayGen.hemisphere(pts, np.broadcast_to(np.array([0.0, 1.0, 0.0]), (n, 3)))
        centre = gen.points
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def timed(fn):
        ms = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def counted(fn, d_cnt):
        d_cnt.zero_()
        fn(d_cnt)  # warm-up, and the counted run
        torch.cuda.synchronize()
        return dict(zip(N.COUNTER_NAMES, (int(x) for x in d_cnt.cpu().numpy())))

    def column(cnt, ms):
        return {"rays": cnt["rays"], "rays_per_path": round(cnt["rays"] / cnt["paths"], 3), "ms_min": round(min(ms), 4),
                "ms_all": [round(x, 4) for x in ms], "Mpaths_per_s": round(cnt["paths"] / min(ms) / 1e3, 1),
                "Mrays_per_s": round(cnt["rays"] / min(ms) / 1e3, 1)}

    with RayQuery(sc) as rq:
        d_centre = torch.from_numpy(np.ascontiguousarray(centre)).to(dev)
        d_points = d_centre if gen.points is not None else None
        d_cnt = torch.zeros(16, dtype=torch.int64, device=dev)
        for samples in SAMPLES:
            assert N.lib.gs_query_radiance_scratch_bytes(n, samples, 0) == 0  # one chunk per item
            d_out = torch.zeros(n * RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_rays = torch.zeros(n * samples * 9, dtype=torch.float64, device=dev)
            d_states = torch.zeros(n * samples, dtype=torch.int64, device=dev)

            def go_gen(cnt=None, emit=False):
                N.check(N.lib.gs_query_radiance_gen_async(rq.dev, C.addressof(gen.raw), ptr(d_points), samples, 0, 0, MAX_DEPTH, 1,
                                                          ptr(d_out), ptr(cnt), ptr(d_rays) if emit else None,
                                                          ptr(d_states) if emit else None, None, 0, sp))

            def go_fixed(cnt=None):
                N.check(N.lib.gs_query_radiance_async(rq.dev, ptr(d_centre), n, samples, 0, MAX_DEPTH, 1, None, ptr(d_out),
                                                      ptr(cnt), None, 0, sp))
            c_gen = counted(go_gen, d_cnt)
            out = d_out.cpu().numpy().view(RADIANCE_DTYPE)
            mean_rgb = [round(float(x), 4) for x in out["rgb"].mean(axis=0) / samples]
            ms_gen = timed(go_gen)
            c_fixed = counted(go_fixed, d_cnt)
            ms_fixed = timed(go_fixed)
            # the uploaded route: the generated call's own rays and streams, n * samples of them at one sample each
            go_gen(emit=True)
            torch.cuda.synchronize()
            h_rays = torch.empty(n * samples * 9, dtype=torch.float64).pin_memory()
            h_states = torch.empty(n * samples, dtype=torch.int64).pin_memory()
            h_rays.copy_(d_rays)
            h_states.copy_(d_states)
            d_out1 = torch.zeros(n * samples * RADIANCE_DTYPE.itemsize, dtype=torch.uint8, device=dev)

            def go_uploaded(cnt=None):
                N.check(N.lib.gs_query_radiance_async(rq.dev, ptr(d_rays), n * samples, 1, 0, MAX_DEPTH, 1, ptr(d_states),
                                                      ptr(d_out1), ptr(cnt), None, 0, sp))

            def go_upload_and_trace():
                d_rays.copy_(h_rays, non_blocking=True)
                d_states.copy_(h_states, non_blocking=True)
                go_uploaded()
            c_up = counted(go_uploaded, d_cnt)
            assert c_up == c_gen, (c_up, c_gen)  # the same paths, field for field
            ms_up = timed(go_uploaded)
            ms_up_all = timed(go_upload_and_trace)
            up = column(c_up, ms_up)
            up["with_upload_ms_min"] = round(min(ms_up_all), 4)
            up["with_upload_ms_all"] = [round(x, 4) for x in ms_up_all]
            up["with_upload_Mrays_per_s"] = round(c_up["rays"] / min(ms_up_all) / 1e3, 1)
            up["uploaded_MB"] = round(n * samples * 80 / 1e6, 1)
            print(json.dumps({"case": name, "samples": samples, "max_depth": MAX_DEPTH, "items": n, "image": "%dx%d" % (w, h),
                              "mean_rgb": mean_rgb, "gen": column(c_gen, ms_gen), "fixed": column(c_fixed, ms_fixed),
                              "uploaded": up}), flush=True)
            del d_out, d_rays, d_states, d_out1, h_rays, h_states


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
