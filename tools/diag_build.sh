#!/bin/bash
# Diagnostic variants of the forward MLP kernels (never loaded by the product or the tests): the library rebuilt with
# -DMI_DIAG_SIN=<mode> as libmirender_diag<mode>.so, in the folder csrc/build.py --profile writes to (the script prints each
# library's path).  The macro lives in mi_math.h, so it reaches every unit that includes it: each mode is a variant build of
# csrc/build.py with an object directory of its own.
# Usage: bash tools/diag_build.sh 1 2 3     then on the GPU box: MI_DIAG_LIB=<printed path, relative to the repository> python tools/perf_quick.py
set -e
cd "$(dirname "$0")/.."
for mode in "$@"; do
  python msra-practice-project_amd/csrc/build.py --variant diag$mode --define=-DMI_DIAG_SIN=$mode
  echo "built diag $mode"
done
