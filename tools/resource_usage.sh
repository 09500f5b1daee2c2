#!/bin/bash
# Registers, scratch, LDS and occupancy of the search kernels as the compiler
# allocates them (gfx950 device compiles of the library's translation units with
# build.py's flags): k_im_search and k_search_lds from the C-ABI unit, k_search's
# generic form (DL = 0) from pomcp_search_tu.hip and its depth-specialised forms
# (DL = 1..3) from pomcp_search_dl_tu.hip.  The last template argument of a
# k_search name is its DL.
# usage: tools/resource_usage.sh   (CPU only; prints one line per search kernel)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
C="$R/posggym-baselines_amd/csrc"
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
F="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC -I$R/include -c --cuda-device-only -Rpass-analysis=kernel-resource-usage"
S="-mllvm -amdgpu-sched-strategy=iterative-ilp"
/opt/rocm/bin/hipcc $F "$C/pomcp_capi.hip" -o "$T/capi.o" > "$T/capi.txt" 2>&1 &
/opt/rocm/bin/hipcc $F $S "$C/pomcp_search_tu.hip" -o "$T/search.o" > "$T/dl0.txt" 2>&1 &
for d in 1 2 3; do
  /opt/rocm/bin/hipcc $F $S -DPB_SEARCH_DL=$d "$C/pomcp_search_dl_tu.hip" -o "$T/dl$d.o" > "$T/dl$d.txt" 2>&1 &
done
wait
cat "$T/capi.txt" "$T/dl0.txt" "$T/dl1.txt" "$T/dl2.txt" "$T/dl3.txt" |
python3 -c "
import re, sys
cur, rows = None, {}
for l in sys.stdin:
    m = re.search(r'remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)', l)
    if not m: continue
    k, v = m.groups()
    if k == 'Function Name': cur = v; rows[cur] = {}
    else: rows[cur][k.split()[0]] = v
for f, r in rows.items():
    if 'k_search' in f or 'k_im_search' in f:
        print(f, r)
"
