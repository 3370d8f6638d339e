#!/bin/bash
# One translation unit rebuilt with build.py's flags for it plus extra ones, linked against the other objects of the library:
#   bash tools/build_variant.sh <name> <file.hip> <flags...>   -> evdeblurnerf_amd/lib/variants/libevd_<name>.so   (load with EVD_LIB_PATH)
set -e
name=$1; src=$2; shift 2
cd "$(dirname "$0")/.."
flags=$(python -c "import sys; from evdeblurnerf_amd import build; print(' '.join(build.unit_flags(sys.argv[1])))" "$src")
cd evdeblurnerf_amd
mkdir -p lib/variants
hipcc $flags "$@" -c csrc/$src -o /tmp/variant_$name.o
objs=$(ls lib/*.o | grep -v "/${src%.hip}.o$")
hipcc -shared -fPIC --offload-arch=gfx950 $objs /tmp/variant_$name.o -o lib/variants/libevd_$name.so
echo lib/variants/libevd_$name.so
