// macjd_env_motion_scan.hip — the env step of a MOVING scenario with SCANNING beams (include/macjd.h, macjd_motion_scan_io).
//
// A translation unit of its own for the MOV && SCAN instantiations of env_step_kernel (macjd_env_step.h, IO =
// MotionScanStepIO<...>), with and without PAT: the scanning step on per-env tables with every table column — the step's
// own rows, the scan rows and the pattern's level rows — chosen by the env's step counter (frame-major tables, one
// contiguous block each per env-step), and both the theta_a columns and the position columns of the env's state row
// rewritten.  The size-bounded loops are unrolled by an explicit count, as in macjd_env_scan_pe.hip: with `#pragma unroll`
// the generic-size kernel keeps them as loops and its per-lane arrays go to scratch.  Every kernel built in the other
// translation units compiles exactly as before.  The host side (validation, span checks) is in macjd_env.hip:
// launch_step_moving, the one dispatch function of the moving modes.
#define MACJD_ENV_PRAGMA(x) _Pragma(#x)
#define MACJD_ENV_UNROLL_SIZED(N) MACJD_ENV_PRAGMA(unroll N)
#include "macjd_env_step.h"

namespace macjd {

// launch_motion_sized<FAST, SCAN = true, PAT>
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPeStepIO<FastStepIO>>) { return launch_motion_sized<true, true, false>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPeStepIO<macjd_step_io>>) { return launch_motion_sized<false, true, false>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPePatStepIO<FastStepIO>>) { return launch_motion_sized<true, true, true>(J, R, grid, block, stream, dev, io); }
MACJD_LAUNCH_MOTION(MotionScanStepIO<ScanPePatStepIO<macjd_step_io>>) { return launch_motion_sized<false, true, true>(J, R, grid, block, stream, dev, io); }

}  // namespace macjd
