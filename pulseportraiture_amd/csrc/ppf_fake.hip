// Simulated fold-mode archives (ppf_fake_batch): what pplib.make_fake_pulsar
// (pplib.py:3302-3499) puts into each profile of a new archive, built on the
// device and stored as the 2-byte samples a PSRFITS file holds.
//
//   k_fake   one workgroup per output row (sub-int s, polarisation p, channel
//            n).  The template's spectrum M_k is rotated, scattered and scaled
//            in the Fourier domain,
//                X_k = M_k exp(2 pi i k phi) B_k g,  B_k = 1 / (1 + 2 pi i k tau_n)
//            (B_k = 1 for tau_n = 0), DC real; the Nyquist harmonic is
//                X_N = Re(M_N) cos(2 pi N phi) Re(B_N) g:
//            the reference rotates (rotate_data / add_DM_nu) and scatters
//            (irfft(sp_FT * rfft(...))) in two real transforms, each of which
//            drops the Nyquist term's imaginary part, and one complex product
//            would keep the cross term.  The packed inverse real transform
//            runs in LDS (irfft_prebin + lds_fft_n, as k_synth), then every
//            bin gets its normal deviate from k_synth's counter RNG keyed by
//            (seed, first_sub + s, p, n, bin pair): a sub-int's samples do not
//            depend on how a job is split into calls.  A row whose noise level
//            is 0 gets none (the reference's `if noise:`).
//            out_kind PPF_FAKE_F64 stores the float64 row.  PPF_FAKE_I16 takes
//            the block minimum / maximum of that same LDS row and applies
//            psrfits.quantize's arithmetic to it (ppf_quant.hpp: float64,
//            round-half-even, FP contraction off, so the integers are the
//            host's bit for bit):
//                offs = f32((lo + hi) / 2)
//                scl  = f32(max((hi - lo) / 2 / 32767, 1e-30))
//                q    = clip(rint((x - offs) / scl), -32768, 32767)
//            stored as big-endian int16 straight in the SUBINT DATA layout
//            [nsub][npol][nchan][nbin], 16 bytes (8 bins) per lane where the
//            rows are 16-byte aligned (nbin % 8 == 0), else 4 bytes (2 bins);
//            DAT_SCL / DAT_OFFS go to [nsub][npol * nchan] float32.
// No atomics, no workspace: every row is independent and reproducible.
#include <hip/hip_runtime.h>

#include "ppf_device.hpp"
#include "ppf_internal.hpp"
#include "ppf_launch.hpp"
#include "ppf_quant.hpp"

namespace ppf {

// two neighbouring bins of the LDS row -> their four file bytes
__device__ __forceinline__ unsigned quant_q2z(double2 z, double offs, double scl) {
    return quant_q2(z.x, z.y, offs, scl);
}

template <bool MX>
__global__ __launch_bounds__(kBlock) void k_fake(FakeArgs a) {
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    const int N = a.nbin >> 1;
    const int64_t row = blockIdx.x;                       // (s, p, n)
    const int n = (int)(row % a.nchan);
    const int p = (int)((row / a.nchan) % a.npol);
    const int s = (int)(row / ((int64_t)a.nchan * a.npol));
    const int m = min(max(a.model_of[s], 0), a.nmodel - 1);
    const double2 *Mrow = a.Mft + ((int64_t)m * a.nchan + n) * (N + 1);
    const double ph = a.phase[(int64_t)s * a.nchan + n];
    const double tn = a.tau[(int64_t)s * a.nchan + n];
    const double g = a.gain[row];
    const double sig = a.noise[n];

    for (int k = threadIdx.x; k < N; k += kBlock) {
        double2 X1 = cmul(Mrow[k], cexp2pi((double)k * ph));
        double2 X2 = cmul(Mrow[N - k], cexp2pi((double)(N - k) * ph));
        if (tn != 0.0) {
            X1 = cmul(X1, scat_recip((2.0 * kPi * (double)k) * tn));
            X2 = cmul(X2, scat_recip((2.0 * kPi * (double)(N - k)) * tn));
        }
        if (k == 0) {
            // DC real; Nyquist: the product of the real parts (two real
            // transforms in the reference, each dropping the imaginary part)
            X1.y = 0.0;
            const double bn = tn != 0.0 ? scat_recip((2.0 * kPi * (double)N) * tn).x : 1.0;
            X2 = cmk(Mrow[N].x * cexp2pi((double)N * ph).x * bn, 0.0);
        }
        lds[k] = irfft_prebin(cscale(X1, g), cscale(X2, g), a.T2[k]);
    }
    __syncthreads();
    lds_fft_n<MX>(lds, N, a.T, true);

    // lds[j] = (x_2j, x_2j+1) N: scale, add the noise, keep the row in LDS
    const double sc = 1.0 / (double)N;
    const uint64_t grow =
        ((uint64_t)(a.first + s) * (uint64_t)a.npol + (uint64_t)p) * (uint64_t)a.nchan + (uint64_t)n;
    double lo = kDblMax, hi = -kDblMax;
    for (int j = threadIdx.x; j < N; j += kBlock) {
        double2 z = cscale(lds[j], sc);
        if (sig != 0.0) {
            const uint64_t h = splitmix64(a.seed ^ splitmix64(grow * 0x100000001B3ull + (uint64_t)j));
            const double u1 = u01(h), u2 = u01(splitmix64(h));
            const double r = sqrt(-2.0 * log(u1));
            double sn, cs;
            sincospi(2.0 * u2, &sn, &cs);
            z.x += sig * r * cs;
            z.y += sig * r * sn;
        }
        if (a.kind == kFakeF64) {
            reinterpret_cast<double2 *>(a.out)[row * N + j] = z;
        } else {
            lds[j] = z;
            lo = fmin(lo, fmin(z.x, z.y));
            hi = fmax(hi, fmax(z.x, z.y));
        }
    }
    if (a.kind == kFakeF64) return;

    // block minimum / maximum.  The row fills the LDS allocation (64 KB at
    // 8192 bins), so the waves' partial results pass through lds[0 .. kWaves),
    // whose row values the first kWaves threads hold meanwhile.
    lo = wave_reduce(lo, [](double x, double y) { return fmin(x, y); });
    hi = wave_reduce(hi, [](double x, double y) { return fmax(x, y); });
    __syncthreads();
    double2 keep = cmk(0.0, 0.0);
    if (threadIdx.x < kWaves) keep = lds[threadIdx.x];
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = cmk(lo, hi);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const double2 v = lds[w];
        lo = fmin(lo, v.x);
        hi = fmax(hi, v.y);
    }
    __syncthreads();
    if (threadIdx.x < kWaves) lds[threadIdx.x] = keep;
    __syncthreads();

    const float offs_f = quant_offs(lo, hi), scl_f = quant_scl(lo, hi);
    const double offs = (double)offs_f, scl = (double)scl_f;
    if (threadIdx.x == 0) {
        a.scl[row] = scl_f;
        a.offs[row] = offs_f;
    }
    if ((a.nbin & 7) == 0) {
        // 8 bins = 16 bytes per lane; rows start 16-byte aligned
        uint4 *o = reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(a.out) + row * a.nbin);
        for (int j = threadIdx.x; j < (N >> 2); j += kBlock) {
            uint4 w;
            w.x = quant_q2z(lds[4 * j], offs, scl);
            w.y = quant_q2z(lds[4 * j + 1], offs, scl);
            w.z = quant_q2z(lds[4 * j + 2], offs, scl);
            w.w = quant_q2z(lds[4 * j + 3], offs, scl);
            o[j] = w;
        }
    } else {
        unsigned *o = reinterpret_cast<unsigned *>(reinterpret_cast<uint16_t *>(a.out) + row * a.nbin);
        for (int j = threadIdx.x; j < N; j += kBlock) o[j] = quant_q2z(lds[j], offs, scl);
    }
}

hipError_t launch_fake(const FakeArgs &a, hipStream_t st) {
    const size_t lds = (size_t)(a.nbin >> 1) * sizeof(double2);
    const unsigned grid = (unsigned)((int64_t)a.nsub * a.npol * a.nchan);
    dispatch_mx(!is_pow2(a.nbin >> 1),
                [&](auto MX) { hipLaunchKernelGGL(k_fake<MX()>, dim3(grid), dim3(kBlock), lds, st, a); });
    return hipGetLastError();
}

}  // namespace ppf
