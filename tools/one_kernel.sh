#!/bin/bash
# Device assembly + resources of ONE kernel of a problem's translation unit, without the shim and the other kernels
# (seconds instead of minutes):   tools/one_kernel.sh <problem> <fd> '<kernel signature>' [extra hipcc flags] > out.s
#   tools/one_kernel.sh synth16x8 1 'k_backward_quad<true, false>(DevPtrs, ilqg_dev_opts_t, int, int, int)' -DILQG_QUAD_WAVES=8
# Prints the .s on stdout, the register / spill summary on stderr.  Needs the problem's build directory (make first).
# The flags are those of the problem's kernel object in csrc/Makefile (STRICT=1: of its FMA-free twin).
R=$(cd "$(dirname "$0")/.." && pwd)
PROB=$1; FD=$2; SIG=$3; shift 3
cd $R/ddp-generator_amd/csrc || exit 1
FLAGS=$(make -s --no-print-directory print-kernel-flags PROBLEM=$PROB FD=$FD VARIANT=${STRICT:+strict}) || exit 1
OUT=$(mktemp /tmp/onek.XXXXXX.s)
hipcc $FLAGS --cuda-device-only -S "-DILQG_ONLY_KERNEL=$SIG" "$@" ilqg_kernels.hip -o $OUT || exit 1
cat $OUT
grep -E "^\s*; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|NumSgprs|VGPR spill|SGPR spill|LDSByteSize)|\.vgpr_spill_count|^\s*\.name:" $OUT | grep -v "^\s*\.name:.*__" >&2
rm -f $OUT
