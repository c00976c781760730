#!/bin/bash
# Build an experiment variant of the product library with extra -D flags:
#   tools/build_variant.sh NAME -DFOO=1 ...   ->  tools/build/lib_NAME.so
# (objects in tools/build/obj_NAME; the in-tree product library is not touched)
# The sources are the Makefile's SRCS, so a variant exports what the product library does.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
obj=$root/tools/build/obj_$name
mkdir -p "$obj"
cd "$root/aipstack_amd/csrc"
make -s build/source_digest.h
srcs=$(make -s --eval='print-srcs: ; @echo $(SRCS)' print-srcs)
[ -n "$srcs" ]
flags="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-parameter -I../../include -I. $*"
pids=()
for f in $srcs; do
  case $f in
    *.cc) g++ -std=c++17 -O3 -fPIC -c "$f" -o "$obj/$f.o" & ;;
    *)    /opt/rocm/bin/hipcc $flags -c "$f" -o "$obj/$f.o" & ;;
  esac
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
objs=()
for f in $srcs; do objs+=("$obj/$f.o"); done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined -pthread \
  -o "$root/tools/build/lib_$name.so" "${objs[@]}"
echo "built tools/build/lib_$name.so"
