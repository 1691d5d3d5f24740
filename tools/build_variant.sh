#!/bin/bash
# A/B library builds: tools/build_variant.sh <name> [-DFLAG ...]  ->  build_ab/<name>.so (git-ignored, travels to the GPU box)
# The translation units and the code-generation flags are the library's own (pyisingmontecarlo_amd/build.py).
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p build_ab
S=pyisingmontecarlo_amd/csrc
read -r -a flags <<< "$(python3 -c 'from pyisingmontecarlo_amd.build import HIP_CODEGEN_FLAGS as f; print(" ".join(f))')"
read -r -a sources <<< "$(python3 -c 'from pyisingmontecarlo_amd.build import HIP_SOURCES as s; print(" ".join(s))')"
"${HIPCC:-/opt/rocm/bin/hipcc}" "${flags[@]}" -fPIC -shared "$@" -o "build_ab/$name.so" "${sources[@]/#/$S/}"
echo "built build_ab/$name.so"
