// Host-side choice of the kernels' template arguments: the launchers name a
// kernel template once and these helpers call them with the instantiation's
// arguments as constants,
//   dispatch_kmax_mx(nharm, mx, [&](auto K, auto MX) {
//       hipLaunchKernelGGL((k_rotate<K(), MX()>), g, b, lds, st, a); });
//   dispatch_log2n_dt<7, 10>(a.log2N, a.dtype, [&](auto L2, auto DT) {
//       hipLaunchKernelGGL((k_noise_w<L2(), DT()>), g, b, lds, st, a, nrows); });
#pragma once
#include <type_traits>
#include <utility>

#include "ppf_device.hpp"

namespace ppf {

// per-thread harmonic slots of the block kernels' KMAX instantiations (1, 2,
// 4, 8, 16): the smallest that holds ceil(N / kBlock)
static inline int kmax_pow2(int N) {
    int q = (N + kBlock - 1) / kBlock, k = 1;
    while (k < q) k <<= 1;
    return k;
}

// f(MX) with MX() == mx (the mixed-radix FFT is compiled in only where the
// transform length is not a power of two; lds_fft_n)
template <class F>
static inline void dispatch_mx(bool mx, F &&f) {
    if (mx) f(std::true_type{});
    else f(std::false_type{});
}

// f(K, MX) with K() == kmax_pow2(nharm) and MX() == mx, then the launch's
// error; hipErrorInvalidValue (f not called) past 16 slots
template <class F>
static inline hipError_t dispatch_kmax_mx(int nharm, bool mx, F &&f) {
    const auto k = [&](auto K) { dispatch_mx(mx, [&](auto MX) { f(K, MX); }); };
    switch (kmax_pow2(nharm)) {
        case 1: k(std::integral_constant<int, 1>{}); break;
        case 2: k(std::integral_constant<int, 2>{}); break;
        case 4: k(std::integral_constant<int, 4>{}); break;
        case 8: k(std::integral_constant<int, 8>{}); break;
        case 16: k(std::integral_constant<int, 16>{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// f(DT) with DT() == 0 (f32 input rows) or 1 (f64), as the kernels' DT
template <class F>
static inline void dispatch_dt(int dtype, F &&f) {
    if (dtype == 0) f(std::integral_constant<int, 0>{});
    else f(std::integral_constant<int, 1>{});
}

// f(L2, DT) with L2() == log2N in [LO, HI] and DT as dispatch_dt, then the
// launch's error; hipErrorInvalidValue (f not called) outside the range
template <int LO, int HI, class F>
static inline hipError_t dispatch_log2n_dt(int log2N, int dtype, F &&f) {
    if constexpr (LO <= HI) {
        if (log2N != LO) return dispatch_log2n_dt<LO + 1, HI>(log2N, dtype, std::forward<F>(f));
        dispatch_dt(dtype, [&](auto DT) { f(std::integral_constant<int, LO>{}, DT); });
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

}  // namespace ppf
