// Shared helpers of the gfx950 kernels behind include/ctcasr.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/ctcasr.h"

#define CTCASR_WAVE 64

typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int ctcasr_launch_status() {
    return hipGetLastError() == hipSuccess ? CTCASR_OK : CTCASR_ERR_LAUNCH;
}

static inline size_t ctcasr_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// splitmix64 finaliser over (seed, counter): the one counter-based generator of the library.
// Dropout takes its top 24 bits as a uniform in [0, 1) (elementwise.hip), the augmentation draws
// take them as an integer (augment.hip; pinned in include/ctcasr.h).
__host__ __device__ __forceinline__ uint64_t splitmix64_mix(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// its top 24 bits
__host__ __device__ __forceinline__ uint32_t splitmix64_r24(uint64_t seed, uint64_t idx) {
    return (uint32_t)(splitmix64_mix(seed, idx) >> 40);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// min(max(v, 0), cutoff) that keeps a NaN: fmaxf(NaN, 0) is 0, which would hand a finite
// activation to the next layer, a finite loss to ctcasr_step_guard, and the step would be applied.
// (-inf -> 0, +inf -> cutoff as before.)
__device__ __forceinline__ float relu_clip(float v, float cutoff) {
    const float c = fminf(fmaxf(v, 0.f), cutoff);
    return v != v ? v : c;
}
// max(v, 0) that keeps a NaN, for the ReLU recurrence cell: fmaxf(NaN, 0) is 0, and a NaN
// pre-activation would become h = 0 (finite layers above, a finite loss, the step applied).
// (-inf -> 0, +inf -> +inf; finite input: fmaxf's result bit for bit.)
__device__ __forceinline__ float relu_keep_nan(float v) {
    return v != v ? v : fmaxf(v, 0.f);
}
// clamp to [-bound, bound] that keeps a NaN (fmaxf(NaN, -bound) is -bound: a NaN input would
// become a finite one, and the step guard would never see it); infinities saturate.  65504 is the
// finite fp16 range; the GEMM operand packs take 60000, which leaves the second piece room.
__device__ __forceinline__ float saturate_f16(float s, float bound = 65504.f) {
    const float c = fminf(fmaxf(s, -bound), bound);
    return s != s ? s : c;
}
// Gate non-linearities on the hardware transcendentals (v_exp_f32 / v_rcp_f32, ~1 ulp each) and
// branch-free: the library expf / tanhf (range reduction, two divergent tanh paths, IEEE division)
// cost ~250 VALU instructions per LSTM cell update inside every time step of the recurrence.
// Absolute error ~1e-7, far inside the 1e-3 parity bar.  (Measured: the gate phase of the
// persistent forward step drops from 0.59 to 0.49 us; the step itself stays barrier-bound.)
__device__ __forceinline__ float sigmoidf_(float x) {
    return __frcp_rn(1.0f + __expf(-x));
}
__device__ __forceinline__ float tanhf_(float x) {
    const float ax = fabsf(x);
    const float e = __expf(-2.0f * ax);                          // in (0, 1]
    const float big = (1.0f - e) * __frcp_rn(1.0f + e);          // fine once 1 - e is not tiny
    const float x2 = ax * ax;                                    // odd series below 0.05
    const float small = ax * (1.0f + x2 * (-0.33333334f + x2 * (0.13333334f - x2 * 0.053968254f)));
    return copysignf(ax < 0.05f ? small : big, x);
}
