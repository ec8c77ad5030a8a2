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
//   k_swt_search   one workgroup per (profile, level): the fmin finish of
//                  scipy.optimize.brute over the factor, a two-point
//                  Nelder-Mead whose every evaluation is the body of
//                  k_swt_score (swt_score_case), started from the best point
//                  of a grid that one k_swt_score launch has scored.
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

// One denoise-and-score case, the body k_swt_score and k_swt_search share:
// profile p, level L, threshold factor fact.  lds0 is the two rows of nbin
// doubles, red kWaves * 2 doubles; sm receives the smoothed row when not
// null.  s = (signal, noise, red_chi2) comes back identical in every thread
// (block_sum's broadcast).  Ends on block_sum's barrier: the LDS rows are
// free again on return.
template <bool MX>
__device__ __forceinline__ void swt_score_case(const SwtArgs &a, int64_t p, int L, bool soft, double fact,
                                               double *lds0, double *red, double *sm, double (&s)[3]) {
    const int n = a.nbin, N = n >> 1, nl = a.nlevel;
    const double lam = fact * (a.med[p * nl + (L - 1)] / 0.6745) * a.sq2ln;
    double *A = lds0, *B = A + n;
    const double *cp = a.coef + p * nl * 2 * n;
    {
        const double *aL = cp + (int64_t)(L - 1) * 2 * n;
        for (int i = threadIdx.x; i < n; i += kBlock) A[i] = swt_thresh(aL[i], lam, soft);
    }
    __syncthreads();
    for (int j = L; j >= 1; --j) {
        const int st = 1 << (j - 1);
        const double *dj = cp + ((int64_t)(j - 1) * 2 + 1) * n;
        for (int i = threadIdx.x; i < n; i += kBlock) {
            double lo = 0.0, hi = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int q = swt_wrap(i, k * st, n, a.pow2);
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
    s[0] = acc[0];
    s[1] = sqrt(acc[1] / (double)n / (double)(N + 1 - a.kc)) * sqrt((double)n / 2.0);
    s[2] = chi[0] / (double)n;
}

template <bool MX>
__global__ __launch_bounds__(kBlock) void k_swt_score(SwtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 2];
    const int64_t c = blockIdx.x;
    const int64_t p = a.cases[3 * c];
    const int L = a.cases[3 * c + 1];
    const bool soft = a.cases[3 * c + 2] != 0;
    double s[3];
    swt_score_case<MX>(a, p, L, soft, a.fact[c], reinterpret_cast<double *>(lds), red,
                       a.smooth ? a.smooth + c * a.nbin : nullptr, s);
    if (threadIdx.x == 0) {
        double *o = a.out + c * 3;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = s[2];
    }
}

// pplib._wavelet_snr of one (signal, noise, red_chi2) triple, IEEE comparisons
__device__ __forceinline__ double swt_objective(const double (&s)[3], double rchi2_tol) {
    double snr = 0.0;
    if (s[0] != 0.0) snr = s[1] != 0.0 ? s[0] / s[1] : __builtin_huge_val();
    if (fabs(s[2] - 1.0) > rchi2_tol) snr = 0.0;
    return -snr;
}

// c * u, c1 * u - c2 * v and u + c * (v - u) as NumPy rounds them: every
// product and difference rounded on its own (a contracted fma gives another
// factor).  The library is built with -ffp-contract=fast, which no pragma
// overrides; a value passed through swt_rounded is opaque to the compiler,
// so the operation that made it cannot fuse with the one that uses it.
__device__ __forceinline__ double swt_rounded(double v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ double swt_mul(double c, double u) { return swt_rounded(c * u); }
__device__ __forceinline__ double swt_lin(double c1, double u, double c2, double v) {
    const double a1 = swt_rounded(c1 * u), a2 = swt_rounded(c2 * v);
    return swt_rounded(a1 - a2);
}
__device__ __forceinline__ double swt_toward(double u, double c, double v) {
    const double d = swt_rounded(v - u);
    const double h = swt_rounded(c * d);
    return swt_rounded(u + h);
}

// The fmin finish of scipy.optimize.brute for one (profile, level): the 1-D
// Nelder-Mead of scipy's _minimize_neldermead (xatol = fatol = 1e-4, at most
// 200 calls) from the first grid point of minimal objective, as a state
// machine around ONE evaluation site: the barriers of swt_score_case stand
// in the loop body alone, and every thread takes every branch from values
// block_sum gave all of them.  (s0, f0) is the better point, (s1, f1) the
// other.
enum { kSwtInit0, kSwtInit1, kSwtReflect, kSwtExpand, kSwtContract, kSwtInside, kSwtShrink };
constexpr int kSwtMaxCalls = 200;
constexpr double kSwtTol = 1e-4;

template <bool MX>
__global__ __launch_bounds__(kBlock) void k_swt_search(SwtArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 2];
    const int nl = a.nlevel;
    const int64_t pl = blockIdx.x;
    const int64_t p = pl / nl;
    const int L = (int)(pl % nl) + 1;
    const bool soft = a.soft != 0;
    // np.argmin over the grid's objectives: the first minimum, a NaN first
    const double *tab = a.table + pl * a.ngrid * 3;
    int g0 = 0;
    double best = 0.0;
    for (int g = 0; g < a.ngrid; ++g) {
        const double sc[3] = {tab[3 * g], tab[3 * g + 1], tab[3 * g + 2]};
        const double f = swt_objective(sc, a.rchi2_tol);
        if (g == 0 || f < best || (f != f && best == best)) {
            best = f;
            g0 = g;
        }
    }
    const double x0 = a.grid[g0];
    double s0 = x0, s1 = x0 != 0.0 ? swt_mul(1.0 + 0.05, x0) : 0.00025;
    double f0 = __builtin_huge_val(), f1 = f0, xr = 0.0, fxr = 0.0, x = s0;
    int calls = 0, st = kSwtInit0;
    while (calls < kSwtMaxCalls) {            // call 201 is not made: the step in progress is abandoned
        double sc[3];
        swt_score_case<MX>(a, p, L, soft, x, reinterpret_cast<double *>(lds), red, nullptr, sc);
        const double fx = swt_objective(sc, a.rchi2_tol);
        ++calls;
        bool stepped = false, shrink = false;
        if (st == kSwtInit0) {
            f0 = fx;
            x = s1;
            st = kSwtInit1;
        } else if (st == kSwtInit1 || st == kSwtShrink) {
            f1 = fx;
            stepped = true;
        } else if (st == kSwtReflect) {
            xr = x;
            fxr = fx;
            if (fxr < f0) {
                x = swt_lin(3.0, s0, 2.0, s1);
                st = kSwtExpand;
            } else if (fxr < f1) {
                x = swt_lin(1.5, s0, 0.5, s1);
                st = kSwtContract;
            } else {
                x = swt_lin(0.5, s0, -0.5, s1);   // 0.5 s0 + 0.5 s1
                st = kSwtInside;
            }
        } else if (st == kSwtExpand) {
            if (fx < fxr) {
                s1 = x;
                f1 = fx;
            } else {
                s1 = xr;
                f1 = fxr;
            }
            stepped = true;
        } else if (st == kSwtContract) {
            if (fx <= fxr) {
                s1 = x;
                f1 = fx;
                stepped = true;
            } else {
                shrink = true;
            }
        } else {                              // kSwtInside
            if (fx < f1) {
                s1 = x;
                f1 = fx;
                stepped = true;
            } else {
                shrink = true;
            }
        }
        if (shrink) {
            s1 = swt_toward(s0, 0.5, s1);     // assigned before its evaluation, as scipy does
            x = s1;
            st = kSwtShrink;
        }
        if (stepped) {
            if (f1 < f0) {
                double t = s0; s0 = s1; s1 = t;
                t = f0; f0 = f1; f1 = t;
            }
            if (fabs(s1 - s0) <= kSwtTol && fabs(f0 - f1) <= kSwtTol) break;
            x = swt_lin(2.0, s0, 1.0, s1);
            st = kSwtReflect;
        }
    }
    if (threadIdx.x == 0) {
        a.fact_min[pl] = s0;
        a.fun_min[pl] = f1 < f0 ? f1 : f0;
        a.nfev[pl] = calls;
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

hipError_t launch_swt_search(const SwtArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.nbin * 2 * sizeof(double);
    const unsigned grid = (unsigned)((int64_t)a.nprof * a.nlevel);
    if (is_pow2(a.nbin / 2)) return swt_launch(k_swt_search<false>, grid, lds, st, a);
    return swt_launch(k_swt_search<true>, grid, lds, st, a);
}

}  // namespace ppf
