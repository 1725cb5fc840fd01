#!/bin/bash
# Per-instantiation VGPRs / scratch of render.hip (gfx950, the product's flags + any extra
# flags given): "FEAT vgprs scratch-bytes-per-lane".  usage: bash tools/resource_usage.sh [-DX=1 ...]
# With --query first: the ray-query kernels of query.hip instead (gs_query_kernel<FEAT, ANY>), with
# their SGPRs, LDS and occupancy too.  With --radiance first: the radiance-query kernels of radiance.hip
# (gs_radiance_kernel<FEAT> and the combine), in the same columns.  With --raygen first: the generated
# radiance queries' kernels of raygen.hip (gs_raygen_kernel<FEAT>), in the same columns.
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
SRC=render.hip
if [ "$1" = "--query" ]; then SRC=query.hip; shift; fi
if [ "$1" = "--radiance" ]; then SRC=radiance.hip; shift; fi
if [ "$1" = "--raygen" ]; then SRC=raygen.hip; shift; fi
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -x hip --offload-arch=gfx950 \
    -mllvm -disable-machine-licm -Rpass-analysis=kernel-resource-usage "$@" \
    -c "$R/grayshift_amd/csrc/device/$SRC" -o "$T/r.o" 2> "$T/ru.txt" || { tail -20 "$T/ru.txt"; exit 1; }
python3 - "$T/ru.txt" <<'PY'
import re, sys
cur = None
for l in open(sys.argv[1]):
    m = re.search(r"Function Name: _Z16gs_render_kernelILi(\d+)E", l)
    q = re.search(r"Function Name: _Z15gs_query_kernelILi(\d+)ELb([01])E", l)
    if m: cur = m.group(1); row = [cur]; extra = None; continue
    if q: cur = q.group(1); row = [cur]; extra = {"any": q.group(2)}; continue
    q = re.search(r"Function Name: _Z1[86]gs_(?:radiance|raygen)_kernelILi(\d+)EE", l)
    if q: cur = q.group(1); row = [cur]; extra = {"any": "-"}; continue
    if "Function Name: _Z26gs_radiance_combine_kernel" in l: cur = "sum"; row = [cur]; extra = {"any": "-"}; continue
    if cur is None: continue
    m = re.search(r" VGPRs: (\d+)", l)
    if m: row.append(m.group(1))
    for key, pat in (("sgprs", r"TotalSGPRs: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
        m = re.search(pat, l)
        if m and extra is not None: extra[key] = m.group(1)
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", l)
    if m: row.append(m.group(1))
    if extra is None and len(row) == 3:
        print("feat %-3s vgprs %-4s scratch %s" % tuple(row)); cur = None
    elif extra is not None and "lds" in extra and len(row) == 3:
        print("feat %-3s any %s  vgprs %-4s sgprs %-4s lds %-6s occupancy %s  scratch %s" % (
            row[0], extra["any"], row[1], extra["sgprs"], extra["lds"], extra["occ"], row[2])); cur = None
PY
rm -rf "$T"
