#!/usr/bin/env python3
"""Scene set-up with the host and the device BVH builder, side by side.

For the 10^6-sphere world of tests/test_host.py (every sphere its own material) and for C4's
world, the minimum of --runs runs of
  * gs_host_scene_from_spec                  (the host's construct_tree)
  * gs_host_scene_from_spec_ex, bvh = 1      (the device builder; device_min_members = 3)
  * its gs_build_info split
  * gs_bvh_build_async alone, by device events around the call on the null stream
and, for the crossover behind the default device_min_members, the host's construct_tree over
bare boxes (gs_host_bvh_build) against the whole device path over the same boxes (allocation,
upload, build, download: what gs_host_scene_from_spec_ex pays) at a ladder of sizes.

--parent-tree DIR times gs_host_scene_from_spec of another checkout with its library built (the
parent commit's) in a child process in the same session: the baseline the device path is held
against.

    python tools/build_bench.py [--runs 5] [--parent-tree DIR] [--out profiles/bvh_build/bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GS_BENCH_TREE") or ROOT)  # (GS_BENCH_TREE: the --parent-tree child)


def million_sphere_spec(N, n_side=1000):
    """tests/test_host.py's world: n_side^2 small spheres with unique Lambertians, and the ground."""
    n = n_side * n_side
    rng = np.random.default_rng(7)
    objs = np.zeros(n + 1, dtype=np.dtype(N.gs_object))
    objs["kind"] = N.GS_OBJ_SPHERE
    a, b = np.meshgrid(np.arange(n_side) - n_side // 2, np.arange(n_side) - n_side // 2, indexing="ij")
    objs["p"][:n, 0] = a.ravel() + 0.9 * rng.random(n)
    objs["p"][:n, 1] = 0.2
    objs["p"][:n, 2] = b.ravel() + 0.9 * rng.random(n)
    objs["p"][:n, 3] = 0.2
    objs["material"][:n] = np.arange(n)
    objs["p"][n, :4] = (0.0, -1000.0, 0.0, 1000.0)
    objs["material"][n] = n
    mats = np.zeros(n + 1, dtype=np.dtype(N.gs_material_spec))
    mats["kind"] = N.GS_MAT_LAMBERTIAN
    mats["texture"] = np.arange(n + 1)
    mats["texture"][n] = n + 2
    texs = np.zeros(n + 3, dtype=np.dtype(N.gs_texture_spec))
    texs["kind"] = N.GS_TEX_SOLID
    texs["p"][:n] = rng.random((n, 3))
    texs["kind"][n + 2], texs["a"][n + 2], texs["b"][n + 2] = N.GS_TEX_CHECKERED, n, n + 1
    texs["p"][n + 2, 0] = 0.32
    world = np.arange(n + 1, dtype=np.int32)
    s = N.gs_scene_spec()
    s.objects, s.n_objects = C.cast(objs.ctypes.data, C.POINTER(N.gs_object)), n + 1
    s.world, s.n_world = C.cast(world.ctypes.data, C.POINTER(C.c_int32)), n + 1
    s.materials, s.n_materials = C.cast(mats.ctypes.data, C.POINTER(N.gs_material_spec)), n + 1
    s.textures, s.n_textures = C.cast(texs.ctypes.data, C.POINTER(N.gs_texture_spec)), n + 3
    s.background = N.gs_background_spec(kind=N.GS_BG_SOLID)
    return s, (objs, mats, texs, world)


def specs(N):
    from grayshift_amd import scenes
    big, keep = million_sphere_spec(N)
    c4 = scenes.config("C4", width=64, spp=1).spec
    return [("1e6_spheres", C.pointer(big), keep), ("C4_world", c4.ptr(), c4)]


def time_host(N, ptr, runs):
    best = None
    for _ in range(runs):
        h = C.c_void_p()
        t0 = time.perf_counter()
        N.check(N.lib.gs_host_scene_from_spec(ptr, C.byref(h)))
        dt = (time.perf_counter() - t0) * 1e3
        N.lib.gs_host_scene_destroy(h)
        best = dt if best is None else min(best, dt)
    return best


def time_device(N, ptr, runs):
    best, split = None, None
    opt = N.gs_build_options(bvh=1, device_min_members=3)
    for _ in range(runs):
        h = C.c_void_p()
        t0 = time.perf_counter()
        N.check(N.lib.gs_host_scene_from_spec_ex(ptr, C.byref(opt), C.byref(h)))
        dt = (time.perf_counter() - t0) * 1e3
        info = N.gs_build_info()
        N.check(N.lib.gs_host_scene_build_info(h, C.byref(info)))
        N.lib.gs_host_scene_destroy(h)
        if best is None or dt < best:
            best, split = dt, info.as_dict()
    return best, split


class DeviceBoxes:
    """n boxes resident on the device with the builder's outputs and work buffer."""

    def __init__(self, N, boxes):
        self.N, self.n = N, boxes.shape[0]
        self.boxes = np.ascontiguousarray(boxes, dtype=np.float64)
        self.work = N.lib.gs_bvh_build_work_bytes(self.n)
        self.n_nodes = N.lib.gs_bvh_node_count(self.n)
        self.d = [C.c_void_p() for _ in range(4)]
        for p, size in zip(self.d, (self.boxes.nbytes, self.n_nodes * 64, self.n * 4, self.work)):
            N.check(N.lib.gs_device_alloc(size, C.byref(p)))
        N.check(N.lib.gs_device_upload(self.d[0], self.boxes.ctypes.data, self.boxes.nbytes))

    def build(self):
        N, d = self.N, self.d
        N.check(N.lib.gs_bvh_build_async(d[0], None, self.n, 0, d[1], d[2], d[3], self.work, None))

    def status(self):
        self.N.check(self.N.lib.gs_bvh_build_status(self.d[3], None))

    def close(self):
        for p in self.d:
            self.N.lib.gs_device_free(p)


def time_primitive(N, boxes, runs):
    """gs_bvh_build_async alone: device events on the null stream (torch's), else the host clock."""
    db = DeviceBoxes(N, boxes)
    try:
        db.build()
        db.status()  # warm-up: code object load
        try:
            import torch
            events = torch.cuda.is_available()
        except ImportError:
            events = False
        best = None
        for _ in range(runs):
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(torch.cuda.default_stream())
                db.build()
                e1.record(torch.cuda.default_stream())
                db.status()
                e1.synchronize()
                dt = e0.elapsed_time(e1)
            else:
                t0 = time.perf_counter()
                db.build()
                db.status()
                dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return best, "device events" if events else "host clock"
    finally:
        db.close()


def member_boxes(n, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.random((n, 3)) * np.array([1000.0, 1.0, 1000.0])
    return np.concatenate([c - 0.2, c + 0.2], axis=1)


def crossover(N, runs, sizes):
    rows = []
    for n in sizes:
        boxes = member_boxes(n)
        nodes = np.zeros(N.lib.gs_bvh_node_count(n) * 8, dtype=np.float64)
        order = np.zeros(n, dtype=np.uint32)
        host = dev = None
        for _ in range(runs):
            t0 = time.perf_counter()
            N.check(N.lib.gs_host_bvh_build(boxes.ctypes.data, n, 0, nodes.ctypes.data, order.ctypes.data))
            dt = (time.perf_counter() - t0) * 1e3
            host = dt if host is None else min(host, dt)
            t0 = time.perf_counter()
            db = DeviceBoxes(N, boxes)
            db.build()
            db.status()
            N.check(N.lib.gs_device_download(nodes.ctypes.data, db.d[1], db.n_nodes * 64))
            N.check(N.lib.gs_device_download(order.ctypes.data, db.d[2], n * 4))
            db.close()
            dt = (time.perf_counter() - t0) * 1e3
            dev = dt if dev is None else min(dev, dt)
        rows.append((n, host, dev))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--host-only", action="store_true", help="print the host timings as JSON (the --parent-tree child)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bvh_build", "bench.txt"))
    a = ap.parse_args()
    from grayshift_amd import _native as N
    from grayshift_amd.codeobj import code_object_hash
    if a.host_only:
        print(json.dumps({name: time_host(N, ptr, a.runs) for name, ptr, _keep in specs(N)}))
        return
    lines = ["tools/build_bench.py --runs %d: scene set-up, ms, the minimum of %d runs; code object %s"
             % (a.runs, a.runs, code_object_hash(N.LIB_PATH)),
             "T = gs_bvh_build_lds_members() = %d" % N.lib.gs_bvh_build_lds_members(), ""]
    parent = None
    if a.parent_tree:
        tree = os.path.abspath(a.parent_tree)
        parent_lib = os.path.join(tree, "grayshift_amd", "libgrayshift.so")
        env = dict(os.environ, GS_BENCH_TREE=tree)
        env.pop("GS_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-only", "--runs", str(a.runs)],
                             env=env, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
        parent = json.loads(out.strip().splitlines()[-1])
        lines.append("parent: code object %s, timed in a child process of this run" % code_object_hash(parent_lib))
    for name, ptr, _keep in specs(N):
        host = time_host(N, ptr, a.runs)
        dev, split = time_device(N, ptr, a.runs)
        n = int(split["members_device"])
        lines.append("%s (%d members on the device, %d BVHs):" % (name, n, split["bvhs_device"]))
        if parent:
            lines.append("  parent gs_host_scene_from_spec        %10.2f" % parent[name])
        lines.append("  gs_host_scene_from_spec               %10.2f" % host)
        lines.append("  gs_host_scene_from_spec_ex, device    %10.2f   (%.2fx the %s)"
                     % (dev, (parent[name] if parent else host) / dev, "parent" if parent else "host builder"))
        lines.append("    split: objects %.2f  boxes %.2f  device build (alloc, upload, launches, wait) %.2f  "
                     "download %.2f  from_order %.2f  flatten %.2f"
                     % tuple(split[k] for k in ("ms_objects", "ms_boxes", "ms_device_build", "ms_download",
                                                "ms_rebuild", "ms_flatten")))
        prim, how = time_primitive(N, member_boxes(n), a.runs)
        lines.append("  gs_bvh_build_async alone, n = %d     %10.3f   (%s)" % (n, prim, how))
        lines.append("")
    lines.append("crossover: construct_tree over bare boxes (gs_host_bvh_build) against the device path over the")
    lines.append("same boxes (allocation, upload, build, status, download), ms:")
    lines.append("  %9s %12s %12s" % ("members", "host", "device"))
    first = None
    for n, host, dev in crossover(N, a.runs, [256, 512, 1024, 2048, 4096, 8192, 16384, 65536, 262144]):
        lines.append("  %9d %12.3f %12.3f" % (n, host, dev))
        if first is None and dev <= host:
            first = n
    lines.append("smallest size of the ladder at which the device path is not slower: %s" % first)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
