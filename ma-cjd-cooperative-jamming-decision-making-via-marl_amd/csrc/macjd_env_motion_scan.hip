// macjd_env_motion_scan.hip — the env step of a MOVING scenario with SCANNING beams (include/macjd.h, macjd_motion_scan_io).
//
// A translation unit of its own for the MOV && SCAN instantiations of env_step_kernel (macjd_env_step.h, IO =
// MotionScanStepIO<...>), with and without PAT: the scanning step on per-env tables with every table column — the step's
// own rows, the scan rows and the pattern's level rows — chosen by the env's step counter (frame-major tables, one
// contiguous block each per env-step), and both the theta_a columns and the position columns of the env's state row
// rewritten.  The size-bounded loops are unrolled by an explicit count, as in macjd_env_scan_pe.hip: with `#pragma unroll`
// the generic-size kernel keeps them as loops and its per-lane arrays go to scratch.  Every kernel built in the other
// translation units compiles exactly as before.  The host side (validation, span checks) is in macjd_env.hip.
#define MACJD_ENV_PRAGMA(x) _Pragma(#x)
#define MACJD_ENV_UNROLL_SIZED(N) MACJD_ENV_PRAGMA(unroll N)
#include "macjd_env_step.h"

namespace macjd {

template <int JT, int RT, bool FAST, bool PAT, class IO>
static void launch(dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const IO& io) {
    hipLaunchKernelGGL((env_step_kernel<JT, RT, true, FAST, IO, false, false, true, PAT>), grid, block, 0, stream, dev, io);
}

template <bool FAST, bool PAT, class IO>
static bool launch_compiled(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev, const IO& io) {
    if (J == 3 && R == 4) launch<3, 4, FAST, PAT>(grid, block, stream, dev, io);
    else if (J == 6 && R == 8) launch<6, 8, FAST, PAT>(grid, block, stream, dev, io);
    else if (J == 2 && R == 2) launch<2, 2, FAST, PAT>(grid, block, stream, dev, io);
    else return false;
    return true;
}

bool launch_motion_scan_fast(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev,
                             const MotionScanStepIO<ScanPeStepIO<FastStepIO>>& io) {
    return launch_compiled<true, false>(J, R, grid, block, stream, dev, io);
}

void launch_motion_scan_general(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev,
                                const MotionScanStepIO<ScanPeStepIO<macjd_step_io>>& io) {
    if (!launch_compiled<false, false>(J, R, grid, block, stream, dev, io)) launch<0, 0, false, false>(grid, block, stream, dev, io);
}

bool launch_motion_scan_pattern_fast(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev,
                                     const MotionScanStepIO<ScanPePatStepIO<FastStepIO>>& io) {
    return launch_compiled<true, true>(J, R, grid, block, stream, dev, io);
}

void launch_motion_scan_pattern_general(int J, int R, dim3 grid, dim3 block, hipStream_t stream, const DevTables* dev,
                                        const MotionScanStepIO<ScanPePatStepIO<macjd_step_io>>& io) {
    if (!launch_compiled<false, true>(J, R, grid, block, stream, dev, io)) launch<0, 0, false, true>(grid, block, stream, dev, io);
}

}  // namespace macjd
