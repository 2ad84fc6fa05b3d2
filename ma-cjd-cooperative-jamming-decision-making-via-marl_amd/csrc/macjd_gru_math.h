// Gate non-linearities of the GRU kernels (forward scan: macjd_nets.hip; reverse-time scan: macjd_gru_bwd.hip).  One
// definition, so that the backward recomputes exactly the gates that produced the stored hidden states.
#pragma once
#include <hip/hip_runtime.h>
namespace macjd {

// v_rcp_f32 / v_exp_f32 directly (1 ulp each): __frcp_rn is the CORRECTLY ROUNDED reciprocal and expands to the full
// div_scale / div_fmas / div_fixup sequence, ~12 instructions per gate on the serial per-step chain
__device__ __forceinline__ float gru_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float gru_tanh(float x) {
    // tanh(x) = 1 - 2 / (exp(2x) + 1); saturates cleanly: exp -> inf gives 1, exp -> 0 gives -1
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f);
}

}  // namespace macjd
