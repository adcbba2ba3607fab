#!/bin/bash
# container-side: build the experiment's library variant, morpheus_amd/_build/ab_fbwd.so = the product library with the generated,
# software-pipelined fused field backward (bf16 x 3 form) in place of field_fused_*_kernel<.., true>.
#   tools/experiments/field_bwd_pipeline/build_variant.sh [--fill 6] [-DFB_ASM_MEM=1]
# Run the A/B on the box with tools/gpu/fbwd_ab.py (MORPHEUS_HIP_LIB=.../ab_fbwd.so for the "new" side).
# The patched sources are laid out as a tree of their own and go through the product's recipe (morpheus_amd.build.build_library:
# the same flags per file), objects under morpheus_amd/_build/obj/ab_fbwd/.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$(cd "$HERE/../../.." && pwd)"
FILL=6; EXTRA=""
while [ $# -gt 0 ]; do case "$1" in --fill) FILL=$2; shift 2;; *) EXTRA="$EXTRA $1"; shift;; esac; done
T=$(mktemp -d)
mkdir -p $T/morpheus_amd
cp -rp "$ROOT"/morpheus_amd/csrc $T/morpheus_amd/csrc
cp -rp "$ROOT"/include $T/include
cp "$HERE/field_bwd_b3.h" $T/morpheus_amd/csrc/
python "$HERE/gen_field_bwd.py" --fill $FILL > $T/morpheus_amd/csrc/field_bwd_b3_gen.h
(cd $T/morpheus_amd/csrc && patch -p1 -s < "$HERE/mlp_launch.patch")
cd "$ROOT"
python - "$T" $EXTRA <<'PY'
import sys
from morpheus_amd import build
build.build_library(sys.argv[1], build.OUT_DIR + "/ab_fbwd.so", obj_dir=build.OUT_DIR + "/obj/ab_fbwd", extra_flags=sys.argv[2:])
PY
FLAGS=$(python -c "from morpheus_amd import build; print(' '.join(build.FLAGS))")
/opt/rocm/bin/hipcc $FLAGS $EXTRA --cuda-device-only -S -o morpheus_amd/_build/ab_fbwd.s $T/morpheus_amd/csrc/mlp.hip 2>/dev/null
echo "built morpheus_amd/_build/ab_fbwd.so (+ ab_fbwd.s); spilled registers per generated kernel:"
awk '/\.name:.*field_fused.*b3/{n=$2} n&&/vgpr_spill_count/{print "  " n, $2; n=""}' morpheus_amd/_build/ab_fbwd.s
rm -rf $T
