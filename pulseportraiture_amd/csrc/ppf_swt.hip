// Stationary-wavelet denoise-and-score engine (ppf_swt_analyse_batch /
// ppf_swt_score_batch): what pplib.smart_smooth's search over (level,
// threshold factor) needs, the wavelet coefficients computed once per profile
// and every (profile, level, factor) case denoised and scored independently.
//
// The transform is the undecimated db8 transform of a periodic row x of even
// length n (a_0 = x):
//     a_j = a_{j-1} (*) up_{j-1}(dec_lo),   d_j = a_{j-1} (*) up_{j-1}(dec_hi)
// (*) circular convolution, up_j the filter with 2^j - 1 zeros between taps
// (it wraps, several times at small n); synthesis is half the adjoint,
//     a'_{j-1} = (a'_j (x) up_{j-1}(dec_lo) + d'_j (x) up_{j-1}(dec_hi)) / 2
// (x) circular correlation.
//
//   k_swt_analyse  one workgroup per profile: get_noise_PS of the row, then
//                  level by level a_j (ping-ponged in LDS) and d_j, both
//                  stored, and the exact median of the 2n values |a_j| u |d_j|
//                  (np.median's even-count rule) by a radix selection on the
//                  bit patterns, four bits per pass, counted with block sums.
//   k_swt_score    one workgroup per case (profile, L, factor, hard / soft):
//                  a_L thresholded into LDS, L synthesis steps ping-ponged
//                  between two LDS rows with the thresholded d_j read from
//                  global memory, the residual chi^2 against the profile,
//                  then the row's rfft in place: sum_{k >= 1} |S_k|^2 and the
//                  top-quarter noise.
// No atomics anywhere: every sum has a fixed order, results are bitwise
// reproducible.
#include <hip/hip_runtime.h>

#include "ppf_device.hpp"
#include "ppf_internal.hpp"

namespace ppf {

// PyWavelets' db8 rec_lo; dec_lo[k] = rec_lo[15 - k], dec_hi[k] = (-1)^(k+1) rec_lo[k]
__device__ constexpr double kDb8[16] = {
    0.05441584224308161,   0.3128715909144659,     0.6756307362980128,    0.5853546836548691,
    -0.015829105256023893, -0.2840155429624281,    0.00047248457399797254, 0.128747426620186,
    -0.01736930100202211,  -0.04408825393106472,   0.013981027917015516,  0.008746094047015655,
    -0.00487035299301066,  -0.0003917403729959771, 0.0006754494059985568, -0.00011747678400228192};

__device__ __forceinline__ double swt_lo(int k) { return kDb8[15 - k]; }
__device__ __forceinline__ double swt_hi(int k) { return (k & 1) ? kDb8[k] : -kDb8[k]; }

// i + off modulo n, off of either sign; n a power of two (pow2) or |off| < n
__device__ __forceinline__ int swt_wrap(int i, int off, int n, bool pow2) {
    int j = i + off;
    if (pow2) return j & (n - 1);
    if (j < 0) j += n;
    if (j >= n) j -= n;
    return j;
}

__device__ __forceinline__ double swt_thresh(double c, double lam, bool soft) {
    const double m = fabs(c);
    if (soft) return m <= lam ? 0.0 : c * (1.0 - lam / m);
    return m < lam ? 0.0 : c;
}

__device__ __forceinline__ unsigned long long swt_abs_bits(double v) {
    return (unsigned long long)__double_as_longlong(fabs(v));
}

// np.median of the 2n values |ra[i]| (LDS) and |rd[i]| (global, written by
// this thread: thread t owns i = t + 256 q in both rows): the mean of the
// order statistics n - 1 and n.  Non-negative doubles order as their bit
// patterns; the pattern of statistic n - 1 is found 4 bits per pass.
__device__ double swt_median(const double *ra, const double *rd, int n, double *red) {
    unsigned long long prefix = 0;
    double rank = (double)(n - 1);            // rank inside the values matching the prefix so far
    for (int shift = 60; shift >= 0; shift -= 4) {
        const unsigned long long himask = shift == 60 ? 0ull : (~0ull << (shift + 4));
        int cnt[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) cnt[d] = 0;
        for (int i = threadIdx.x; i < n; i += kBlock) {
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const unsigned long long u = swt_abs_bits(w ? rd[i] : ra[i]);
                if (((u ^ prefix) & himask) == 0) {
                    const int dg = (int)((u >> shift) & 15);
#pragma unroll
                    for (int d = 0; d < 16; ++d) cnt[d] += (dg == d) ? 1 : 0;
                }
            }
        }
        double c[16];
#pragma unroll
        for (int d = 0; d < 16; ++d) c[d] = (double)cnt[d];
        block_sum<16>(c, red);
        double below = 0.0;
        int dg = -1;
#pragma unroll
        for (int d = 0; d < 15; ++d) {
            if (dg < 0) {
                if (rank < below + c[d]) dg = d;
                else below += c[d];
            }
        }
        if (dg < 0) dg = 15;
        rank -= below;
        prefix |= (unsigned long long)dg << shift;
    }
    const double v1 = __longlong_as_double((long long)prefix);
    // statistic n: v1 again when more than n values are <= v1, else the smallest above
    double le[1] = {0.0}, mn[1] = {-__builtin_huge_val()};
    for (int i = threadIdx.x; i < n; i += kBlock) {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const double v = fabs(w ? rd[i] : ra[i]);
            if (swt_abs_bits(v) <= prefix) le[0] += 1.0;
            else mn[0] = fmax(mn[0], -v);
        }
    }
    block_sum<1>(le, red);
    block_max<1>(mn, red);
    const double v2 = le[0] >= (double)(n + 1) ? v1 : -mn[0];
    return 0.5 * (v1 + v2);
}

template <bool MX>
__global__ __launch_bounds__(kBlock) void k_swt_analyse(SwtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 16];
    const int n = a.nbin, N = n >> 1, nl = a.nlevel;
    const int64_t p = blockIdx.x;
    double *A = reinterpret_cast<double *>(lds), *B = A + n;
    const double *x = a.prof + p * n;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const double v = x[i];
        A[i] = v;
        B[i] = v;
    }
    __syncthreads();
    // get_noise_PS of the profile (k_noise's rule) on the copy in B
    double2 *Z = reinterpret_cast<double2 *>(B);
    lds_fft_n<MX>(Z, N, a.T, false);
    double acc[1] = {0.0};
    for (int k = threadIdx.x + a.kc; k <= N; k += kBlock) acc[0] += cabs2(rfft_bin(Z, N, a.T2, k));
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) a.noise[p] = sqrt(acc[0] / (double)n / (double)(N + 1 - a.kc));
    for (int j = 1; j <= nl; ++j) {
        const int s = 1 << (j - 1);
        double *ca = a.coef + ((p * nl + (j - 1)) * 2) * n, *cd = ca + n;
        for (int i = threadIdx.x; i < n; i += kBlock) {
            double lo = 0.0, hi = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const double v = A[swt_wrap(i, -k * s, n, a.pow2)];
                lo = fma(swt_lo(k), v, lo);
                hi = fma(swt_hi(k), v, hi);
            }
            B[i] = lo;
            ca[i] = lo;
            cd[i] = hi;
        }
        __syncthreads();
        const double m = swt_median(B, cd, n, red);
        if (threadIdx.x == 0) a.med[p * nl + (j - 1)] = m;
        double *t = A;
        A = B;
        B = t;
    }
}

template <bool MX>
__global__ __launch_bounds__(kBlock) void k_swt_score(SwtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 2];
    const int n = a.nbin, N = n >> 1, nl = a.nlevel;
    const int64_t c = blockIdx.x;
    const int64_t p = a.cases[3 * c];
    const int L = a.cases[3 * c + 1];
    const bool soft = a.cases[3 * c + 2] != 0;
    const double lam = a.fact[c] * (a.med[p * nl + (L - 1)] / 0.6745) * a.sq2ln;
    double *A = reinterpret_cast<double *>(lds), *B = A + n;
    const double *cp = a.coef + p * nl * 2 * n;
    {
        const double *aL = cp + (int64_t)(L - 1) * 2 * n;
        for (int i = threadIdx.x; i < n; i += kBlock) A[i] = swt_thresh(aL[i], lam, soft);
    }
    __syncthreads();
    for (int j = L; j >= 1; --j) {
        const int s = 1 << (j - 1);
        const double *dj = cp + ((int64_t)(j - 1) * 2 + 1) * n;
        for (int i = threadIdx.x; i < n; i += kBlock) {
            double lo = 0.0, hi = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int q = swt_wrap(i, k * s, n, a.pow2);
                lo = fma(swt_lo(k), A[q], lo);
                hi = fma(swt_hi(k), swt_thresh(dj[q], lam, soft), hi);
            }
            B[i] = 0.5 * (lo + hi);
        }
        __syncthreads();
        double *t = A;
        A = B;
        B = t;
    }
    // A: the smoothed row
    const double *x = a.prof + p * n;
    const double sig_x = a.noise[p];
    double *sm = a.smooth ? a.smooth + c * n : nullptr;
    double chi[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const double sv = A[i], r = (x[i] - sv) / sig_x;
        chi[0] = fma(r, r, chi[0]);
        if (sm) sm[i] = sv;
    }
    block_sum<1>(chi, red);
    double2 *Z = reinterpret_cast<double2 *>(A);
    lds_fft_n<MX>(Z, N, a.T, false);
    double acc[2] = {0.0, 0.0};
    for (int k = threadIdx.x + 1; k <= N; k += kBlock) {
        const double pw = cabs2(rfft_bin(Z, N, a.T2, k));
        acc[0] += pw;
        if (k >= a.kc) acc[1] += pw;
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) {
        double *o = a.out + c * 3;
        o[0] = acc[0];
        o[1] = sqrt(acc[1] / (double)n / (double)(N + 1 - a.kc)) * sqrt((double)n / 2.0);
        o[2] = chi[0] / (double)n;
    }
}

namespace {
template <typename K>
hipError_t swt_launch(K kern, unsigned grid, size_t lds, hipStream_t st, const SwtArgs &a) {
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, a);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_swt_analyse(const SwtArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.nbin * 2 * sizeof(double);
    if (is_pow2(a.nbin / 2)) return swt_launch(k_swt_analyse<false>, (unsigned)a.nprof, lds, st, a);
    return swt_launch(k_swt_analyse<true>, (unsigned)a.nprof, lds, st, a);
}

hipError_t launch_swt_score(const SwtArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.nbin * 2 * sizeof(double);
    if (is_pow2(a.nbin / 2)) return swt_launch(k_swt_score<false>, (unsigned)a.ncase, lds, st, a);
    return swt_launch(k_swt_score<true>, (unsigned)a.ncase, lds, st, a);
}

}  // namespace ppf
