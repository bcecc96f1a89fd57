#!/bin/bash
# scripts/count_resources.sh [extra hipcc flags]: registers, spills, scratch and occupancy of every kernel instantiation of csrc/count.hip,
# read from the compiler's own remarks (-Rpass-analysis=kernel-resource-usage) and from nothing else.  Compiles the device side with the
# Makefile's flags for gfx950; needs no GPU.  One line per kernel, sorted by name:
#   scripts/count_resources.sh > profiles/count_resources_after.txt
set -e -o pipefail
cd "$(dirname "$0")/../gsn_amd/csrc"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
CXXFLAGS=${CXXFLAGS:--O3 -std=c++17 -fPIC -Wall -Wno-unused-function}
$HIPCC --offload-arch=$ARCH $CXXFLAGS --cuda-device-only -Rpass-analysis=kernel-resource-usage "$@" -c count.hip -o /dev/null 2>&1 | python3 -c '
import re, subprocess, sys
rows, cur = {}, None
for line in sys.stdin:
    m = re.search(r"remark: (?:\[[^\]]*\]\s*)?(.*)$", line)
    if not m:
        continue
    t = m.group(1).strip()
    f = re.match(r"Function Name: (\S+)", t)
    if f:
        cur = rows.setdefault(f.group(1), {})
        continue
    kv = re.match(r"([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", t)
    if kv and cur is not None:
        cur[kv.group(1).strip()] = kv.group(2)
names = sorted(rows)
try:
    dem = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")[:len(names)]
except Exception:
    dem = names
for n, d in sorted(zip(names, dem), key=lambda p: p[1]):
    r = rows[n]
    d = re.sub(r"^void |gsn::|\(CountArgs\)$", "", d.replace("gsn::", ""))
    print("%-58s VGPRs %3s  VGPR spills %3s  SGPRs %3s  SGPR spills %3s  scratch %4s B/lane  occupancy %s waves/SIMD" % (
        d, r.get("VGPRs"), r.get("VGPRs Spill"), r.get("TotalSGPRs"), r.get("SGPRs Spill"), r.get("ScratchSize"), r.get("Occupancy")))
'
