# Build compile-time variants of the native library for tools/abvariant.py:
#   bash tools/build_variants.sh name:-DFLAG[,-DFLAG2] ...
# -> tools/variants/<name>/libingot_gpu.so (parse.hip rebuilt with the flags,
# the other objects taken from the in-tree build).  SRC=read.hip rebuilds that
# source instead (tools/modify_rows_probe.py --read --lib nofast:
#   SRC=read.hip bash tools/build_variants.sh nofast:-DINGOT_READ_ROWS_FAST_SET=0).
set -e
cd "$(dirname "$0")/.."
python -m ingot_amd.build
src=${SRC:-parse.hip}
for v in "$@"; do
    n=${v%%:*}; f=${v#*:}
    mkdir -p tools/build/$n tools/variants/$n
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function \
        -Iinclude ${f//,/ } -c ingot_amd/csrc/$src -o tools/build/$n/${src%.hip}.o
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/variants/$n/libingot_gpu.so \
        tools/build/$n/${src%.hip}.o $(ls ingot_amd/build/*.o | grep -v "/$src.o") -ldl
done
