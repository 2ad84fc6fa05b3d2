// macjd_env_scan_pe.hip — the generic-size (J, R) scanning env step on per-env scenario tables.
//
// A translation unit of its own for ONE instantiation of env_step_kernel (macjd_env_step.h) and its PAT form: at the generic
// bound (32 x 32) the optimizer drops `#pragma unroll` on the kernel's radar / jammer loops once they read per-env tables (the unrolled
// body passes its size threshold), the loops stay loops, and the per-lane arrays they index (suppression sums, false-target
// products, SNRs, detection probabilities) go to scratch: 1040 B per lane.  Unrolled by an explicit count — no threshold —
// the kernel keeps them in registers.  The directive is a macro of the header, so every kernel built in macjd_env.hip
// compiles exactly as before.
#define MACJD_ENV_PRAGMA(x) _Pragma(#x)
#define MACJD_ENV_UNROLL_SIZED(N) MACJD_ENV_PRAGMA(unroll N)
#include "macjd_env_step.h"

namespace macjd {

void launch_scan_pe_generic(dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const ScanPeStepIO<macjd_step_io>& io) {
    hipLaunchKernelGGL((env_step_kernel<0, 0, true, false, ScanPeStepIO<macjd_step_io>, false, false, true>), grid, block, 0, stream,
                       dev, io);
}

// the same kernel under a stepped antenna pattern on per-env tables (PAT = true, the level rows loaded where they are used)
void launch_scan_pe_generic(dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const ScanPePatStepIO<macjd_step_io>& io) {
    hipLaunchKernelGGL((env_step_kernel<0, 0, true, false, ScanPePatStepIO<macjd_step_io>, false, false, true, true>), grid, block, 0,
                       stream, dev, io);
}

}  // namespace macjd
