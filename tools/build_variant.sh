#!/bin/bash
# A variant build of libhelios_hip.so for same-box A/B runs: tools/build_variant.sh NAME [extra compiler flags ...]
# -> ab/NAME.so (objects under ab/obj_NAME/; the in-tree library and its objects are not touched).  Select it at run time
# with HELIOS_HIP_LIB=ab/NAME.so.  The sources are the SRCS of helios_amd/csrc/Makefile.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
C=$R/helios_amd/csrc
O=$R/ab/obj_$NAME
SRCS=$(make --no-print-directory -C $C -pn | sed -n 's/^SRCS := //p')
[ -n "$SRCS" ] || { echo "no SRCS in $C/Makefile" >&2; exit 1; }
mkdir -p $O
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function $*"
pids=()
for f in $SRCS; do
  /opt/rocm/bin/hipcc $FLAGS -c $C/$f -o $O/${f%.hip}.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $R/ab/$NAME.so $O/*.o
echo "built ab/$NAME.so"
