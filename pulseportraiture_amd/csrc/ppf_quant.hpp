// psrfits.quantize on the device, shared by k_fake (ppf_fake.hip: the row it
// holds in LDS) and the stand-alone pack kernels (ppf_pack.hip: rows in
// global memory).  Float64 arithmetic, one operation per rounding, FP
// contraction off, round-half-even: the integers are the host's bit for bit.
//     offs = f32((lo + hi) / 2)
//     scl  = f32(max((hi - lo) / 2 / 32767, 1e-30))
//     q    = clip(rint((x - offs) / scl), -32768, 32767)
// lo / hi: the row's minimum / maximum.
#pragma once
#include <hip/hip_runtime.h>

namespace ppf {

__device__ __forceinline__ float quant_offs(double lo, double hi) {
#pragma clang fp contract(off)
    return (float)((lo + hi) / 2.0);
}
__device__ __forceinline__ float quant_scl(double lo, double hi) {
#pragma clang fp contract(off)
    return (float)fmax((hi - lo) / 2.0 / 32767.0, 1e-30);
}
// the sample's two bytes in file order, as the low half of a little-endian word
__device__ __forceinline__ unsigned quant_q(double x, double offs, double scl) {
#pragma clang fp contract(off)
    double q = rint((x - offs) / scl);
    q = fmin(fmax(q, -32768.0), 32767.0);
    return (unsigned)__builtin_bswap16((unsigned short)(short)(int)q);
}
__device__ __forceinline__ unsigned quant_q2(double x, double y, double offs, double scl) {
    return quant_q(x, offs, scl) | (quant_q(y, offs, scl) << 16);
}

}  // namespace ppf
