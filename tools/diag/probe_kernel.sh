#!/bin/bash
# Register pressure of ONE trace-kernel instantiation in a few seconds (no GPU needed):
#   tools/diag/probe_kernel.sh 'trace_pool_kernel<false, 1024, false>' [extra hipcc flags]
#   tools/diag/probe_kernel.sh 'nee_path_kernel<1, 0, 0, 1, 1>'   (the NEE kernel: MODE, BIG, ENV, TEX, GLOSSY[, CAM])
# prints VGPRs / spills / scratch from -Rpass-analysis=kernel-resource-usage and leaves the ISA in /tmp/ff_probe.s
# (a lone instantiation can compile differently from the build's: its callers alone decide what the optimiser propagates)
K=${1:-trace_pool_kernel<false, 1024, false>}; shift
cd "$(dirname "$0")/../../gpupathtracer_amd/csrc" || exit 1
# the unit that holds the kernel and the switch that instantiates it there (the frame kernels are no templates: `make asm` shows them)
case "$K" in nee_path_kernel*) UNIT=ff_kernels.hip; DEF=FF_PROBE_NEE ;; *) UNIT=ff_kernels.hip; DEF=FF_PROBE ;; esac
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-slp-vectorize \
  --cuda-device-only -S -o /tmp/ff_probe.s "$UNIT" "-D$DEF=$K" -Rpass-analysis=kernel-resource-usage "$@" 2>&1 |
  grep -E "VGPRs:|ScratchSize|SGPRs Spill|VGPRs Spill|TotalSGPRs|error" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | head -5 | tr "\n" ";"; echo
