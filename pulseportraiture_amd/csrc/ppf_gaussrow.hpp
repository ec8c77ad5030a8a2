// One row of pplib.gen_gaussian_portrait (pplib.py:886-963) in a workgroup's
// LDS: the row builder shared by k_gauss_port (model portraits), k_gauss_rows
// (the columns of the Gaussian least-squares problem, ppf_gaussfit.hip) and
// their joined variants (join_ichans: ROT below), so all produce the same
// bits.  Per component: the evolved loc/wid/amp (evolve_parameter pplib.py:1032-1084), the wrapped,
// truncated Gaussian of gaussian_profile (pplib.py:801-856) with its unit-peak
// factor taken at the first argmax (a block reduction), accumulated into the
// LDS row in component order as gen_gaussian_profile does (pplib.py:859-883).
// A non-zero tau then convolves the row with the one-sided exponential
// (rfft * 1/(1 + 2 pi i k tau_n) -> irfft, pplib.py:951-957, 4212-4260).
// FP contraction is off so each product/sum rounds as NumPy's does.
#pragma once
#include "ppf_device.hpp"

namespace ppf {

__device__ __forceinline__ double gp_evolve(double f, double nu_ref, double v, double e, int code) {
#pragma clang fp contract(off)
    if (code == 0) return exp((log(f) - log(nu_ref)) * e + 1.0 * log(v));   // power_law_evolution
    return (f - nu_ref) * e + 1.0 * v;                                    // linear_evolution
}

__device__ __forceinline__ double gp_bin_center(int j, int nbin) {
#pragma clang fp contract(off)
    // np.linspace(1/(2 nbin), 1 - 1/(2 nbin), nbin) (get_bin_centers, pplib.py:694-707)
    const double lo = 1.0 / (double)(nbin * 2), hi = 1.0 - 1.0 / (double)(nbin * 2);
    if (j == nbin - 1) return hi;
    const double step = (hi - lo) / (double)(nbin - 1);
    return (double)j * step + lo;
}

// unnormalised retval of gaussian_profile at bin j (0 outside |z| < 20);
// *xw receives the wrapped bin centre
__device__ __forceinline__ double gp_raw(int j, int nbin, double mean, double sigma, double *xw) {
#pragma clang fp contract(off)
    double x = gp_bin_center(j, nbin);
    if (mean < 0.5) { if (x > mean + 0.5) x = x - 1.0; }
    else if (x < mean - 0.5) x = x + 1.0;
    *xw = x;
    const double z = (x - mean) / sigma;
    if (!(fabs(z) < 20.0)) return 0.0;
    return exp(-0.5 * (z * z)) / (sigma * 2.5066282746310002);   // sqrt(2 pi)
}

// what gp_build_row left in LDS
enum GpRow {
    kGpReal = 0,      // the nbin doubles of the row, final
    kGpPacked = 1,    // even nbin, scattered: nbin / 2 packed points, to scale by 2 / nbin
    kGpPackedOdd = 2  // odd nbin, scattered: (nbin - 1) / 2 packed points (the reference's
                      // nbin - 1-bin irfft), to scale by 1 / (nbin >> 1); the last bin is 0
};

// Builds the row of (prm, tau, alpha) at frequency f into lds (rfft_len(nbin)
// double2, the row as doubles over the same bytes); red: kWaves * 2 doubles.
// PERT: entry pj of prm is read as prm[pj] + dj (pj < 0: none; the
// forward-difference columns of ppf_gauss_lsq_batch); tau and alpha are
// passed already so.
// ROT (even nbin only): the row of an archive of a joined model
// (gen_gaussian_portrait's join_ichans, pplib.py:956-962), rotated by rot
// [rot] as rotate_data does (pplib.py:2447-2512).  The rotation is folded
// into the scattering multiply: harmonic k is multiplied by B_k e^{2 pi i k
// rot} (B_k = 1 when tau == 0) in ONE transform round trip, which a row with
// rot == 0 takes too, so that the rows of a forward difference in a join
// parameter are built alike.  The reference's irfft between the two steps
// drops the imaginary parts of the DC and Nyquist bins BEFORE the phasor:
// they are zeroed here after the B_k multiply, and again after the phasor
// (the final irfft).  Without ROT rot is not read and the function compiles
// to what it was.
// Every thread of the workgroup calls it; LDS is readable on return.
template <int KMAX, bool MX, bool PERT, bool ROT = false>
__device__ __forceinline__ GpRow gp_build_row(double2 *lds, double *red, int nbin, int ngauss, int code0,
                                              int code1, int code2, const double *prm, int pj, double dj,
                                              double tau, double alpha, double f, double nu_ref,
                                              const double2 *T, const double2 *T2, const double2 *Te,
                                              const double2 *T2e, double rot = 0.0) {
#pragma clang fp contract(off)
    double *row = reinterpret_cast<double *>(lds);
    const int N = nbin >> 1;
    auto P = [&](int i) {
        if constexpr (PERT) return i == pj ? prm[i] + dj : prm[i];
        else return prm[i];
    };
    const double dc = P(0);
    for (int j = threadIdx.x; j < nbin; j += kBlock) row[j] = dc;   // zeros + DC
    const double fwhm = 2.0 * sqrt(2.0 * log(2.0));
    for (int g = 0; g < ngauss; ++g) {
        const int c = 2 + 6 * g;
        const double L = gp_evolve(f, nu_ref, P(c), P(c + 1), code0);
        const double W = gp_evolve(f, nu_ref, P(c + 2), P(c + 3), code1);
        const double A = gp_evolve(f, nu_ref, P(c + 4), P(c + 5), code2);
        if (!(W > 0.0)) {   // wid <= 0 (zeroout) or NaN: amp * zeros
            for (int j = threadIdx.x; j < nbin; j += kBlock) row[j] = row[j] + A * 0.0;
            continue;
        }
        const double sigma = W / fwhm;
        double mean = fmod(L, 1.0);                  // Python/NumPy L % 1.0
        if (mean != 0.0 && mean < 0.0) mean += 1.0;
        // first argmax of the unnormalised profile
        double lmax = -1.0, xw;
        int lidx = nbin;
        for (int j = threadIdx.x; j < nbin; j += kBlock) {
            const double r = gp_raw(j, nbin, mean, sigma, &xw);
            if (r > lmax) { lmax = r; lidx = j; }
        }
        double v[1] = {lmax};
        block_max<1>(v, red);
        const double gmax = v[0];
        double vi[1] = {lmax == gmax ? -(double)lidx : -(double)nbin};
        block_max<1>(vi, red);
        const int imax = (int)(-vi[0]);
        double fact = 1.0;                            // all-zero profile: returned as is
        if (gmax != 0.0) {
            double xi;
            (void)gp_raw(imax, nbin, mean, sigma, &xi);
            const double zz = (xi - L) / sigma;
            fact = exp(-0.5 * (zz * zz)) / gmax;
        }
        for (int j = threadIdx.x; j < nbin; j += kBlock) {
            const double r = gp_raw(j, nbin, mean, sigma, &xw);
            row[j] = row[j] + A * (fact * r);
        }
    }
    // (the scattered branch first: with the unscattered return ahead of it
    // k_gauss_port<4, false> takes 130 VGPRs instead of 125, one wave less
    // per SIMD, and 2048-bin portraits build 3-8 % slower)
    if constexpr (ROT) {
        const double tn = tau != 0.0 ? tau / (double)nbin * pow(f / nu_ref, alpha) : 0.0;
        __syncthreads();
        lds_fft_n<MX>(lds, N, T, false);
        double2 Xk[KMAX], Xn[KMAX];
        harm_fwd<KMAX>(lds, nbin, T2, Xk, Xn, [&](double2 X, int k) {
            if (tn != 0.0) X = cmul(X, scat_recip((2.0 * kPi * (double)k) * tn));
            if (k == 0 || k == N) X.y = 0.0;   // the scattering irfft: DC, Nyquist real
            return cmul(X, cexp2pi((double)k * rot));   // (the rotation's irfft: harm_fwd)
        });
        __syncthreads();
        harm_inv<KMAX, MX>(lds, nbin, T, T2, Xk, Xn);
        return kGpPacked;
    }
    if (tau != 0.0) {
        // taus = (tau / nbin) * (freqs / nu_ref)**alpha; B_k = 1 / (1 + 2 pi i k tau_n)
        const double tn = tau / (double)nbin * pow(f / nu_ref, alpha);
        const bool odd = nbin & 1;
        __syncthreads();
        if (odd) {
            // the real row (doubles) -> complex points in place: all reads first
            double v[2 * KMAX];
#pragma unroll
            for (int i = 0; i < 2 * KMAX; ++i) {
                const int j = threadIdx.x + i * kBlock;
                if (j < nbin) v[i] = row[j];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2 * KMAX; ++i) {
                const int j = threadIdx.x + i * kBlock;
                if (j < nbin) lds[j] = cmk(v[i], 0.0);
            }
            __syncthreads();
        }
        lds_fft_n<MX>(lds, rfft_len(nbin), T, false);
        double2 Xk[KMAX], Xn[KMAX];
        harm_fwd<KMAX>(lds, nbin, T2, Xk, Xn, [&](double2 X, int k) {
            return tn != 0.0 ? cmul(X, scat_recip((2.0 * kPi * (double)k) * tn)) : X;
        });
        __syncthreads();
        if (odd) {
            // the reference's irfft takes no length (pplib.py:957): nbin - 1
            // bins, the row's last column zero
            harm_inv_ref<KMAX, MX>(lds, nbin, Te, T2e, Xk, Xn);
            return kGpPackedOdd;
        }
        harm_inv<KMAX, MX>(lds, nbin, T, T2, Xk, Xn);
        return kGpPacked;
    }
    __syncthreads();
    return kGpReal;
}

}  // namespace ppf
