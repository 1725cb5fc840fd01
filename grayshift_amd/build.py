"""Build the in-tree native libraries.

* ``grayshift_amd/libgrayshift.so`` — the product: HIP megakernel for gfx950 plus
  the C++ host mirror, one shared library (hipcc; no torch, no JIT cache), and beside it
  ``libgrayshift_query.so``, the ray-query kernels it loads.
* ``oracle/liboracle.so`` — the CPU checker (test infrastructure; g++ via
  oracle/Makefile).

Both are compiled with ``-ffp-contract=off``: the reference's Rust f64 code
never fuses multiply-add, and neither may we.

Usage: python -m grayshift_amd.build [--force] [--no-oracle]
"""
import argparse
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libgrayshift.so")
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_LIB = os.path.join(ORACLE_DIR, "liboracle.so")

SOURCES = [
    os.path.join(HERE, "csrc", "device", "render.hip"),   # the kernels and their launchers
    os.path.join(HERE, "csrc", "device", "output.hip"),
    os.path.join(HERE, "csrc", "device", "bvh_build.hip"),  # BVHNode::from_list on the device
    os.path.join(HERE, "csrc", "host", "scene.cpp"),      # flat scene -> device scene
    os.path.join(HERE, "csrc", "host", "launch.cpp"),     # device scene -> launches
    os.path.join(HERE, "csrc", "host", "query.cpp"),      # ray queries: checks, the one launch
    os.path.join(HERE, "csrc", "host", "world.cpp"),
    os.path.join(HERE, "csrc", "host", "camera.cpp"),
    os.path.join(HERE, "csrc", "host", "host_capi.cpp"),
    os.path.join(HERE, "csrc", "host", "multi_gpu.cpp"),
]


# The ray-query kernels (world.hit for caller rays) are a translation unit of their own, listed
# beside bvh_build.hip, and are linked into a library of their own next to the product,
# libgrayshift_query.so, which libgrayshift.so needs: the product's .hip_fatbin -- whose hash keys
# the committed PMC and stamps summaries (grayshift_amd/codeobj.py) -- holds the megakernel's code
# objects only, so adding or changing a query kernel leaves every render profile valid.
QUERY_SOURCE = os.path.join(HERE, "csrc", "device", "query.hip")
# ... and the radiance-query kernels (ray_color for caller rays), the same library's second unit
RADIANCE_SOURCE = os.path.join(HERE, "csrc", "device", "radiance.hip")
# ... and the generated radiance queries (a ray drawn on the device for every sample), its third
RAYGEN_SOURCE = os.path.join(HERE, "csrc", "device", "raygen.hip")
QUERY_SOURCES = [QUERY_SOURCE, RADIANCE_SOURCE, RAYGEN_SOURCE]


def query_lib(lib):
    """The ray-query library that goes with a product library: <name>_query.so beside it."""
    return lib[:-3] + "_query.so"


QUERY_LIB = query_lib(LIB)


def _headers():
    """Every header a source may include, and this file (the compiler flags)."""
    return (sorted(glob.glob(os.path.join(HERE, "csrc", "**", "*.hpp"), recursive=True)) +
            sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))) + [os.path.abspath(__file__)])


ARCH = os.environ.get("GS_OFFLOAD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
          "-Wno-unused-parameter", "-Wno-unused-variable"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build_product(force=False, verbose=False, extra=(), out=None):
    """Build libgrayshift.so (or a variant at `out` with extra compiler flags).

    Nothing is done while the library is newer than every source, every header and this file
    (a tree that was copied with its library but without its objects stays as it is).  Else a
    source is compiled only when its object is missing or older than the source, any header
    or this file; `force` (and so every variant build) compiles them all."""
    lib = out or LIB
    headers = _headers()
    qlib = query_lib(lib)
    if not force and not _stale(lib, SOURCES + QUERY_SOURCES + headers) and os.path.exists(qlib):
        return lib
    objs = []
    compiled = False
    tag = "" if out is None else "_" + os.path.basename(out).replace(".so", "")
    for src in SOURCES + QUERY_SOURCES:
        obj = os.path.join(HERE, "csrc", "_obj" + tag, os.path.basename(src) + ".o")
        objs.append(obj)
        if not force and not _stale(obj, [src] + headers):
            continue
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        cmd = [HIPCC] + COMMON + list(extra)
        if src.endswith(".hip"):
            # Machine LICM hoists the f64 polynomial constants of OCML's asin/atan2/acos
            # out of the megakernel's loop, then spills them to per-lane scratch (344 B/lane)
            # and reloads each one with a dependent scratch load: measured on MI355X C4,
            # disabling it removes all scratch and runs +19% (1990 -> 2370 Msamples/s).
            cmd += ["-x", "hip", "--offload-arch=" + ARCH, "-mllvm", "-disable-machine-licm"]
            # A fixed compilation-unit id: clang's default hashes the command line, -o
            # included, into a symbol of the code object, so the same sources built into
            # another directory would hash differently (grayshift_amd/codeobj.py keys the
            # committed PMC summaries by the code objects' hash).
            cmd += ["-cuid=gs_" + os.path.basename(src).replace(".", "_")]
        # (the .cpp files are plain C++ over the HIP runtime API: a HIP translation unit, even
        # one without kernels, would add a bundle to .hip_fatbin and change that hash)
        cmd += ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        compiled = True
    if not compiled and not _stale(lib, objs) and os.path.exists(qlib):
        return lib
    # the query kernels' library first (found beside the product at load time: $ORIGIN), then the product
    qobjs = objs[len(SOURCES):]
    objs = objs[:len(SOURCES)]
    for target, cmd in ((qlib, qobjs + ["-Wl,-soname," + os.path.basename(qlib)]),
                        (lib, objs + [qlib, "-Wl,-rpath,$ORIGIN", "-lpthread", "-ldl"])):
        tmp = target + ".tmp"
        cmd = [HIPCC, "-shared", "--offload-arch=" + ARCH, "-o", tmp] + cmd
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(tmp, target)
    return lib


KAT_SRC = os.path.join(ROOT, "tests", "hip", "kat_device.hip")
KAT_LIB = os.path.join(ROOT, "tests", "hip", "libkat_device.so")


def build_kat(force=False, verbose=False):
    """Test-only HIP harness running the kernel's device functions on test arrays."""
    deps = [KAT_SRC] + _headers()
    if not force and not _stale(KAT_LIB, deps):
        return KAT_LIB
    cmd = [HIPCC] + COMMON + ["-x", "hip", "--offload-arch=" + ARCH, "-shared", "-o", KAT_LIB + ".tmp", KAT_SRC]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(KAT_LIB + ".tmp", KAT_LIB)
    return KAT_LIB


def build_oracle(force=False, verbose=False):
    if force and os.path.exists(ORACLE_LIB):
        os.remove(ORACLE_LIB)
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)
    return ORACLE_LIB


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--variant", action="append", metavar="NAME:FLAGS", default=[],
                    help="also build variants/NAME.so with extra FLAGS (A/B), e.g. --variant 'v4:-DGS_MIN_WAVES=4'")
    ap.add_argument("--resource-usage", action="store_true",
                    help="print per-kernel VGPR/SGPR/LDS/occupancy (hipcc remarks)")
    a = ap.parse_args(argv)
    extra = ["-Rpass-analysis=kernel-resource-usage"] if a.resource_usage else []
    import concurrent.futures as cf

    def variant(spec):
        name, _, flags = spec.partition(":")
        path = os.path.join(HERE, "variants", name + ".so")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        build_product(force=True, verbose=a.verbose, extra=extra + flags.split(), out=path)
        return "variant %s %s" % (path, flags)

    # the product and the variants side by side (each compile is one process; 4 at a time)
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        jobs = [ex.submit(build_product, force=a.force or a.resource_usage, verbose=a.verbose, extra=extra)]
        jobs += [ex.submit(variant, spec) for spec in a.variant]
        for j in jobs[1:]:
            print(j.result())
        jobs[0].result()
    if not a.no_oracle:
        build_oracle(force=a.force, verbose=a.verbose)
        build_kat(force=a.force, verbose=a.verbose)
    print("built", LIB, "" if a.no_oracle else ORACLE_LIB)


if __name__ == "__main__":
    sys.exit(main())
