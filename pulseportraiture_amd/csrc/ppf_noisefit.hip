// get_noise_fit / find_kc on the device: the noise floor of a row found by
// a brute-grid fit to its log10 power spectrum (pplib.py:2341-2373 calling
// find_kc, pplib.py:1530-1561, whose scipy.optimize.brute evaluates
// find_kc_function, pplib.py:1509-1527, on a 20 x 20 x 20 grid and returns
// the first minimum in C order).
//
// With d_k = log10(pows_k), k < N, the model is dc + b e_k(a): e_k =
// exp(-a k) (exp_dc) or the unit half triangle (k < A ? 1 - k / A : 0),
// A = floor(a) (half_tri, half_triangle_function pplib.py:1496-1506).  The
// grids are brute's np.mgrid[lo:hi:20j]: a over [1/N, 1] or [1, N] (built by the
// host, they depend on N alone), b over [0, max d - min d], dc over
// [min d, max d].  chi^2 = sum_k w_k (d_k - dc - b e_k)^2, w = 1 / errs^2, is
// quadratic in (b, dc), so per a three sums over k suffice and the 8000 grid
// points are scalar work:
//   chi^2 = Sdd - 2 b Sde - 2 c Sd + b^2 See + 2 b c Se + c^2 Sw,
// taken on d' = d - min d and c = dc - min d, both in [0, max d - min d] like
// b: no term is larger than Sw (max d - min d)^2, against a minimum of about
// 0.3 Sw (the variance of the log10 of an exponential deviate), so the
// expansion loses two to three digits of sixteen.
//
// One workgroup per row.  k_noise_fit transforms the row in LDS as k_noise
// does and keeps d beside the spectrum; k_spec_fit reads power spectra from
// global memory (find_kc's input; the long transforms' output) and strides
// over them.  Every reduction is block_sum / block_max in a fixed order: no
// atomics, bitwise reproducible.
#include <hip/hip_runtime.h>

#include "ppf_device.hpp"
#include "ppf_internal.hpp"
#include "ppf_launch.hpp"

namespace ppf {

namespace {

constexpr int kNfChunk = 4;                       // a values per pass over k
constexpr int kNfPts = kNfGrid * kNfGrid * kNfGrid;
constexpr double kInf = __builtin_huge_val();

// element i of brute's grid np.mgrid[lo:hi:20j]: i * step + lo with step =
// (hi - lo) / 19, each operation rounded as NumPy rounds it (FP contraction
// off, as gp_bin_center).  Unlike np.linspace, mgrid does not set the last
// element to hi itself.
__device__ __forceinline__ double nf_grid(double lo, double hi, int i) {
#pragma clang fp contract(off)
    const double step = (hi - lo) / (double)(kNfGrid - 1);
    return (double)i * step + lo;
}

// The grid fit of one row: dk(k) = d_k, wk(k) = w_k, k < N.  Returns the
// a index of the first minimum of chi^2 in C order (a slowest, dc fastest),
// np.argmin's choice: the first NaN where there is one.  A NaN or infinite
// d (a harmonic of zero power: log10 0) makes element 0 of the b or dc grid
// 0 * inf = NaN, and with it chi^2 at index 0: the answer is 0 then.
// Every thread of the workgroup calls it and gets the same value.
// red: kWaves * 3 * kNfChunk doubles, S: 3 * kNfGrid doubles (shared).
template <typename I, typename FD, typename FW>
__device__ __forceinline__ int nf_grid_fit(FD dk, FW wk, I N, int fn, const double *ag, double *red,
                                           double *S) {
    const I tid = (I)threadIdx.x;
    double mm[3] = {-kInf, -kInf, 0.0};           // max d, max -d, any NaN
    for (I k = tid; k < N; k += kBlock) {
        const double d = dk(k);
        mm[0] = fmax(mm[0], d);
        mm[1] = fmax(mm[1], -d);
        if (d != d) mm[2] = 1.0;
    }
    block_max<3>(mm, red);
    const double dmax = mm[0], dmin = -mm[1];
    if (mm[2] != 0.0 || !(fabs(dmax) <= kDblMax) || !(fabs(dmin) <= kDblMax)) return 0;
    double s0[3] = {0.0, 0.0, 0.0};               // Sw, Sd, Sdd
    for (I k = tid; k < N; k += kBlock) {
        const double w = wk(k), d = dk(k) - dmin;
        s0[0] += w;
        s0[1] = fma(w, d, s0[1]);
        s0[2] = fma(w * d, d, s0[2]);
    }
    block_sum<3>(s0, red);
    for (int c = 0; c < kNfGrid; c += kNfChunk) {
        double acc[3 * kNfChunk];                 // Se, See, Sde per a
        double av[kNfChunk];
#pragma unroll
        for (int j = 0; j < kNfChunk; ++j) {
            av[j] = fn ? floor(ag[c + j]) : -ag[c + j];
            acc[3 * j] = acc[3 * j + 1] = acc[3 * j + 2] = 0.0;
        }
        for (I k = tid; k < N; k += kBlock) {
            const double w = wk(k), wd = w * (dk(k) - dmin), x = (double)k;
#pragma unroll
            for (int j = 0; j < kNfChunk; ++j) {
                const double e = fn ? (x < av[j] ? 1.0 - x / av[j] : 0.0) : exp(av[j] * x);
                acc[3 * j] = fma(w, e, acc[3 * j]);
                acc[3 * j + 1] = fma(w * e, e, acc[3 * j + 1]);
                acc[3 * j + 2] = fma(wd, e, acc[3 * j + 2]);
            }
        }
        block_sum<3 * kNfChunk>(acc, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < 3 * kNfChunk; ++j) S[3 * c + j] = acc[j];
        }
    }
    __syncthreads();
    // the 8000 grid points over the threads, each in ascending index order
    double best = 0.0;
    int bidx = -1, nidx = kNfPts;                 // first minimum, first NaN
    for (int p = threadIdx.x; p < kNfPts; p += kBlock) {
        const int ia = p / (kNfGrid * kNfGrid), ib = (p / kNfGrid) % kNfGrid, ic = p % kNfGrid;
        const double b = nf_grid(0.0, dmax - dmin, ib);
        const double dc = nf_grid(dmin, dmax, ic) - dmin;
        const double Se = S[3 * ia], See = S[3 * ia + 1], Sde = S[3 * ia + 2];
        const double chi = s0[2] - 2.0 * b * Sde - 2.0 * dc * s0[1] + b * b * See + 2.0 * b * dc * Se +
                           dc * dc * s0[0];
        if (chi != chi) {
            if (nidx == kNfPts) nidx = p;
        } else if (bidx < 0 || chi < best) {
            best = chi;
            bidx = p;
        }
    }
    // first-index tie-break restored across the threads: the minimum, then
    // the lowest index that holds it (the maxima of the negated values, as
    // gp_build_row takes its first argmax)
    double v[2] = {bidx < 0 ? -kInf : -best, -(double)nidx};
    block_max<2>(v, red);
    int win;
    if (v[1] > -(double)kNfPts) {
        win = (int)(-v[1]);                       // a NaN: np.argmin returns the first one
    } else {
        double vi[1] = {(bidx >= 0 && -best == v[0]) ? -(double)bidx : -(double)kNfPts};
        block_max<1>(vi, red);
        win = (int)(-vi[0]);
    }
    return win / (kNfGrid * kNfGrid);
}

// pplib.py:2359-2363: the first harmonic of the noise tail
__device__ __forceinline__ int64_t nf_tail_start(double fact, int kc, int64_t N) {
    double k_crit = fact * (double)kc;
    if (k_crit >= (double)N) k_crit = fmin((double)(int64_t)(0.99 * (double)N), k_crit);
    return (int64_t)k_crit;
}

}  // namespace

// ===========================================================================
// k_noise_fit: get_noise_fit per row, the row's rFFT in LDS (every length
// k_noise takes).  LDS: [rfft_len] spectrum | [N + 1] d.
// ===========================================================================
template <bool MX>
__global__ __launch_bounds__(kBlock) void k_noise_fit(NoiseFitArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 3 * kNfChunk];
    __shared__ double S[3 * kNfGrid];
    const int N = a.nbin >> 1, nharm = N + 1, NF = rfft_len(a.nbin);
    const int64_t row = blockIdx.x;
    double *d = reinterpret_cast<double *>(lds + NF);
    load_row(lds, a.in, a.dtype, row, a.nbin);
    __syncthreads();
    lds_fft_n<MX>(lds, NF, a.T, false);
    for (int k = threadIdx.x; k < nharm; k += kBlock)
        d[k] = log10(cabs2(rbin(lds, a.nbin, a.T2, k)) / (double)a.nbin);
    __syncthreads();
    const int ia = nf_grid_fit<int>([&](int k) { return d[k]; }, [](int) { return 1.0; }, nharm, a.fn,
                                    a.a_grid, red, S);
    const int kc = a.kc_table[ia];
    const int k0 = (int)nf_tail_start(a.fact, kc, nharm);
    // the tail mean with k_noise's arithmetic
    double acc[1] = {0.0};
    for (int k = threadIdx.x + k0; k <= N; k += kBlock) acc[0] += cabs2(rbin(lds, a.nbin, a.T2, k));
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) {
        a.noise_out[row] = sqrt(acc[0] / (double)a.nbin / (double)(N + 1 - k0));
        a.kc_out[row] = kc;
    }
}

// ===========================================================================
// k_spec_fit: the same fit on power spectra in global memory, any nharm >= 2
// (find_kc; get_noise_fit of rows past the LDS transforms, whose spectra
// k_lf_pows wrote).  noise_out == nullptr: kc alone.
// ===========================================================================
__global__ __launch_bounds__(kBlock) void k_spec_fit(NoiseFitArgs a) {
    __shared__ double red[kWaves * 3 * kNfChunk];
    __shared__ double S[3 * kNfGrid];
    const int64_t row = blockIdx.x, N = a.nharm;
    const double *p = a.pows + row * N;
    const double *er = a.errs;
    const int64_t el = a.errs_len;
    const int ia = nf_grid_fit<int64_t>([&](int64_t k) { return log10(p[k]); },
                                        [&](int64_t k) {
                                            if (!er) return 1.0;
                                            const double e = er[el == 1 ? 0 : k];
                                            return 1.0 / (e * e);
                                        },
                                        N, a.fn, a.a_grid, red, S);
    const int kc = a.kc_table[ia];
    if (a.noise_out) {
        const int64_t k0 = nf_tail_start(a.fact, kc, N);
        double acc[1] = {0.0};
        for (int64_t k = k0 + threadIdx.x; k < N; k += kBlock) acc[0] += p[k];
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) a.noise_out[a.row0 + row] = sqrt(acc[0] / (double)(N - k0));
    }
    if (threadIdx.x == 0) a.kc_out[a.row0 + row] = kc;
}

hipError_t launch_noise_fit(const NoiseFitArgs &a, int64_t nrows, hipStream_t st) {
    const size_t lds = (size_t)rfft_len(a.nbin) * sizeof(double2) + (size_t)(a.nbin / 2 + 1) * sizeof(double);
    hipError_t e = hipSuccess;
    dispatch_mx(!is_pow2(rfft_len(a.nbin)), [&](auto MX) {
        if (lds > 48 * 1024)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_noise_fit<MX()>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) hipLaunchKernelGGL(k_noise_fit<MX()>, dim3((unsigned)nrows), dim3(kBlock), lds, st, a);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_spec_fit(const NoiseFitArgs &a, int64_t nrows, hipStream_t st) {
    hipLaunchKernelGGL(k_spec_fit, dim3((unsigned)nrows), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace ppf
