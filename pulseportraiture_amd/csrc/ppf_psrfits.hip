// ppf_psrfits.hip -- device side of the PSRCHIVE-free PSRFITS fast path
// (pulseportraiture_amd/psrfits.py): the raw DATA bytes of
// a fold-mode SUBINT table arrive as they sit in the file and are turned
// into the float32 total-intensity rows load_data would hand get_TOAs
// (pplib.py:2749-2915 with pscrunch=True, rm_baseline=True), plus the
// per-profile baseline statistics and S/N.
//
//   k_unpack      WG = (sub-int, block of kUnpackChans channels), thread =
//                 bin pairs: big-endian int16 / uint8 / float32 samples (or
//                 native float32 rows: load_data's statistics pass after
//                 dedispersion / tscrunch, DAT_SCL = 1, DAT_OFFS = 0) ->
//                 DATA * DAT_SCL + DAT_OFFS in float32 arithmetic (two
//                 roundings, no fma: PSRCHIVE's loader) -> total intensity
//                 (npol 1: itself; AA+BB / AABBCRCI: AA + BB; IQUV: I) ->
//                 rows [nsub][nchan][nbin]; the weighted channel sum of the
//                 block (fixed channel order) -> partials [nsub][nblk][nbin]
//   k_base_window WG per sub-int: total profile = sum of the partials in
//                 block order; PSRCHIVE's BaselineWindow: the circular window
//                 of W = rint(0.15 nbin) bins with the smallest sum (first
//                 minimum) -> window start, total profile out
//   k_row_stats   wave per row: off-pulse mean over the window (subtracted
//                 from the row in place when rm_baseline), off-pulse sigma,
//                 S/N = sum over the on-pulse bins / (sigma sqrt(n_on))
// All of it is HBM-streaming integer/byte work (no MFMA): a few bytes per
// sample against the 2 B per sample that crossed PCIe.
#include "ppf_device.hpp"
#include "ppf_internal.hpp"

namespace ppf {

constexpr int kUnpackChans = 16;

__device__ __forceinline__ float sample_f32(const uint8_t *p, int elem, int64_t i) {
    if (elem == 0) {
        const uint16_t u = reinterpret_cast<const uint16_t *>(p)[i];
        return (float)(int16_t)__builtin_bswap16(u);
    }
    if (elem == 1) return (float)p[i];
    if (elem == 3) return reinterpret_cast<const float *>(p)[i];   // native rows
    const uint32_t u = __builtin_bswap32(reinterpret_cast<const uint32_t *>(p)[i]);
    return __uint_as_float(u);
}

__global__ __launch_bounds__(256) void k_unpack(UnpackArgs a) {
    // DATA * DAT_SCL + DAT_OFFS rounds twice, as PSRCHIVE's (and NumPy's)
    // float32 arithmetic does: the product is pinned in a register before
    // the add, so the compiler cannot fuse them (-ffp-contract=fast)
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    const int s = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const uint8_t *raw = a.raw + (int64_t)s * a.sub_stride;
    const float *scl = a.scl + (int64_t)s * a.npol * a.nchan;
    const float *off = a.offs + (int64_t)s * a.npol * a.nchan;
    const int n0 = blk * kUnpackChans, n1 = min(a.nchan, n0 + kUnpackChans);
    const int npol_used = a.pol_mode == 1 ? 2 : 1;
    for (int b = threadIdx.x; b < a.nbin; b += blockDim.x) {
        double part = 0.0;
        for (int n = n0; n < n1; ++n) {
            float v = 0.0f;
            for (int p = 0; p < npol_used; ++p) {
                const int64_t i = ((int64_t)p * a.nchan + n) * a.nbin + b;
                float prod = sample_f32(raw, a.elem, i) * scl[p * a.nchan + n];
                asm volatile("" : "+v"(prod));      // rounded product: no fma
                const float x = prod + off[p * a.nchan + n];
                v = p == 0 ? x : v + x;
            }
            a.out[((int64_t)s * a.nchan + n) * a.nbin + b] = v;
            const double w = a.wts ? (double)a.wts[(int64_t)s * a.nchan + n] : 1.0;
            if (w != 0.0) part += w * (double)v;
        }
        a.part[((int64_t)s * nblk + blk) * a.nbin + b] = part;
    }
}

// The total profile of a sub-int sits in LDS (nbin doubles) while its window
// sums are formed; a profile past kBaseLdsMax bytes (nbin > 18,816) is read
// back from a.total instead (GLOBAL: written by this workgroup just before,
// visible to it after the barrier), so any length runs.
constexpr size_t kBaseLdsMax = 150u * 1024u - 3u * 1024u;   // next to rb / ri

template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_base_window(UnpackArgs a) {
    extern __shared__ double tot_lds[];
    const int s = blockIdx.x;
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    double *tot = GLOBAL ? a.total + (int64_t)s * a.nbin : tot_lds;
    for (int b = threadIdx.x; b < a.nbin; b += blockDim.x) {
        double t = 0.0;
        for (int k = 0; k < nblk; ++k) t += a.part[((int64_t)s * nblk + k) * a.nbin + b];
        tot[b] = t;
        if (!GLOBAL) a.total[(int64_t)s * a.nbin + b] = t;
    }
    __syncthreads();
    // window sums by thread: each thread scans its share of start bins with
    // a direct sum for its first start and a sliding update after that;
    // the per-thread minima are then reduced in start order (first minimum)
    const int W = a.win;
    const int per = (a.nbin + blockDim.x - 1) / blockDim.x;
    const int b0 = threadIdx.x * per, b1 = min(a.nbin, b0 + per);
    double best = INFINITY;
    int bi = a.nbin;
    if (b0 < b1) {
        double w = 0.0;
        for (int j = 0; j < W; ++j) w += tot[(b0 + j) % a.nbin];
        for (int b = b0; b < b1; ++b) {
            if (b > b0) w += tot[(b - 1 + W) % a.nbin] - tot[b - 1];
            if (w < best) { best = w; bi = b; }
        }
    }
    __shared__ double rb[256];
    __shared__ int ri[256];
    rb[threadIdx.x] = best;
    ri[threadIdx.x] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = rb[0];
        int mi = ri[0];
        for (int t = 1; t < (int)blockDim.x; ++t)
            if (rb[t] < m) { m = rb[t]; mi = ri[t]; }
        a.wstart[s] = mi < a.nbin ? mi : 0;
    }
}

__global__ __launch_bounds__(256) void k_row_stats(UnpackArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)a.nsub * a.nchan) return;
    const int s = (int)(row / a.nchan);
    float *x = a.out + row * a.nbin;
    const int w0 = a.wstart[s], W = a.win;
    double sm = 0.0;
    for (int j = lane; j < W; j += 64) sm += (double)x[(w0 + j) % a.nbin];
    const double mean = wave_sum(sm) / (double)W;
    double sq = 0.0;
    for (int j = lane; j < W; j += 64) {
        const double d = (double)x[(w0 + j) % a.nbin] - mean;
        sq += d * d;
    }
    const double var = wave_sum(sq) / (double)W;
    double on = 0.0;
    for (int b = lane; b < a.nbin; b += 64) {
        const int rel = (b - w0 + a.nbin) % a.nbin;
        const double v = (double)x[b] - mean;
        if (rel >= W) on += v;
        if (a.rm_baseline) x[b] = (float)v;
    }
    on = wave_sum(on);
    const int non = a.nbin - W;
    if (lane == 0) {
        double *o = a.stats + row * 3;
        o[0] = mean;
        o[1] = sqrt(var);
        o[2] = (var > 0.0 && non > 0) ? on / (sqrt(var) * sqrt((double)non)) : 0.0;
    }
}

static hipError_t launch_base_window(const UnpackArgs &a, hipStream_t st) {
    hipError_t e;
    const size_t lds = (size_t)a.nbin * sizeof(double);
    if (lds > kBaseLdsMax) {
        hipLaunchKernelGGL(k_base_window<true>, dim3((unsigned)a.nsub), dim3(256), 0, st, a);
    } else {
        if (lds > 48 * 1024) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_base_window<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_base_window<false>, dim3((unsigned)a.nsub), dim3(256), lds, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_unpack(const UnpackArgs &a, hipStream_t st) {
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    hipLaunchKernelGGL(k_unpack, dim3((unsigned)((int64_t)a.nsub * nblk)), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_base_window(a, st)) != hipSuccess) return e;
    const int64_t rows = (int64_t)a.nsub * a.nchan;
    hipLaunchKernelGGL(k_row_stats, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Full polarisation (ppf_unpack_psrfits_pol_batch): all four polarisation
// blocks of every sample, the state converted on the way.
//
//   k_unpack_pol  k_unpack's grid (WG = sub-int x block of kUnpackChans
//                 channels, threads along the bins).  Per sample: the four
//                 DATA * DAT_SCL + DAT_OFFS values (two roundings each, as in
//                 k_unpack), the state conversion `conv` in float32 (sums,
//                 differences and exact scalings by 2 or 1/2: nothing for an
//                 fma to contract), the four rows of the channel, and the
//                 weighted channel-block partial of the total intensity in
//                 k_unpack's layout, so k_base_window runs on it unchanged.
//                 VEC: a lane takes 4 consecutive bins per polarisation with
//                 one 8-byte load (int16; 4-byte uint8, 16-byte float32) and
//                 one 16-byte store; the launch takes it when nbin is a
//                 multiple of 4 and raw, sub_stride, out and the partials are
//                 aligned for it.  Both forms run the same per-sample code:
//                 identical bits.
// k_row_stats then runs over the nsub x 4 nchan rows (its row -> sub-int map
// holds with nchan := 4 nchan).

__device__ __forceinline__ void samples4_f32(const uint8_t *p, int elem, int64_t i, float x[4]) {
    if (elem == 0) {
        const uint2 u = *reinterpret_cast<const uint2 *>(p + i * 2);
        x[0] = (float)(int16_t)__builtin_bswap16((uint16_t)(u.x & 0xffffu));
        x[1] = (float)(int16_t)__builtin_bswap16((uint16_t)(u.x >> 16));
        x[2] = (float)(int16_t)__builtin_bswap16((uint16_t)(u.y & 0xffffu));
        x[3] = (float)(int16_t)__builtin_bswap16((uint16_t)(u.y >> 16));
    } else if (elem == 1) {
        const uint32_t u = *reinterpret_cast<const uint32_t *>(p + i);
        for (int k = 0; k < 4; ++k) x[k] = (float)((u >> (8 * k)) & 0xffu);
    } else if (elem == 3) {
        const float4 f = *reinterpret_cast<const float4 *>(p + i * 4);
        x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
    } else {
        const uint4 u = *reinterpret_cast<const uint4 *>(p + i * 4);
        x[0] = __uint_as_float(__builtin_bswap32(u.x));
        x[1] = __uint_as_float(__builtin_bswap32(u.y));
        x[2] = __uint_as_float(__builtin_bswap32(u.z));
        x[3] = __uint_as_float(__builtin_bswap32(u.w));
    }
}

// v: the four scaled polarisations of one sample as stored -> o: the four of
// the state asked for; returns the total intensity of the sample
__device__ __forceinline__ float convert_state(int conv, const float v[4], float o[4]) {
    switch (conv) {
    case 2:   // AA BB CR CI -> I Q U V, linear feeds
        o[0] = v[0] + v[1]; o[1] = v[0] - v[1]; o[2] = 2.0f * v[2]; o[3] = 2.0f * v[3];
        break;
    case 3:   // ... circular feeds
        o[0] = v[0] + v[1]; o[1] = 2.0f * v[2]; o[2] = 2.0f * v[3]; o[3] = v[0] - v[1];
        break;
    case 4:   // I Q U V -> AA BB CR CI, linear feeds
        o[0] = 0.5f * (v[0] + v[1]); o[1] = 0.5f * (v[0] - v[1]);
        o[2] = 0.5f * v[2]; o[3] = 0.5f * v[3];
        break;
    case 5:   // ... circular feeds
        o[0] = 0.5f * (v[0] + v[3]); o[1] = 0.5f * (v[0] - v[3]);
        o[2] = 0.5f * v[1]; o[3] = 0.5f * v[2];
        break;
    default:  // 0, 1: as stored
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    }
    return (conv == 1 || conv >= 4) ? o[0] + o[1] : o[0];
}

__device__ __forceinline__ float scaled_f32(float x, float scl, float off) {
    float prod = x * scl;
    asm volatile("" : "+v"(prod));      // rounded product: no fma
    return prod + off;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_unpack_pol(UnpackArgs a, int conv) {
    constexpr int NB = VEC ? 4 : 1;     // bins per lane and trip
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    const int s = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const uint8_t *raw = a.raw + (int64_t)s * a.sub_stride;
    const float *scl = a.scl + (int64_t)s * 4 * a.nchan;
    const float *off = a.offs + (int64_t)s * 4 * a.nchan;
    const int n0 = blk * kUnpackChans, n1 = min(a.nchan, n0 + kUnpackChans);
    for (int b = threadIdx.x * NB; b < a.nbin; b += blockDim.x * NB) {
        double part[NB];
        for (int k = 0; k < NB; ++k) part[k] = 0.0;
        for (int n = n0; n < n1; ++n) {
            float x[4][NB];
            for (int p = 0; p < 4; ++p) {
                const int64_t i = ((int64_t)p * a.nchan + n) * a.nbin + b;
                if (VEC) samples4_f32(raw, a.elem, i, x[p]);
                else x[p][0] = sample_f32(raw, a.elem, i);
            }
            float o[4][NB];
            const double w = a.wts ? (double)a.wts[(int64_t)s * a.nchan + n] : 1.0;
            for (int k = 0; k < NB; ++k) {
                float v[4], c[4];
                for (int p = 0; p < 4; ++p)
                    v[p] = scaled_f32(x[p][k], scl[p * a.nchan + n], off[p * a.nchan + n]);
                const float t = convert_state(conv, v, c);
                for (int p = 0; p < 4; ++p) o[p][k] = c[p];
                if (w != 0.0) part[k] = fma(w, (double)t, part[k]);
            }
            for (int p = 0; p < 4; ++p) {
                float *row = a.out + (((int64_t)s * 4 + p) * a.nchan + n) * a.nbin + b;
                if (VEC) *reinterpret_cast<float4 *>(row) = make_float4(o[p][0], o[p][1], o[p][2], o[p][3]);
                else row[0] = o[p][0];
            }
        }
        double *pt = a.part + ((int64_t)s * nblk + blk) * a.nbin + b;
        if (VEC) {
            reinterpret_cast<double2 *>(pt)[0] = make_double2(part[0], part[1]);
            reinterpret_cast<double2 *>(pt)[1] = make_double2(part[2], part[3]);
        } else {
            pt[0] = part[0];
        }
    }
}

hipError_t launch_unpack_pol(const UnpackArgs &a, int conv, hipStream_t st) {
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    const int64_t esize = a.elem == 0 ? 2 : (a.elem == 1 ? 1 : 4);
    const bool vec = a.nbin % 4 == 0 && a.sub_stride % (4 * esize) == 0 &&
                     (uintptr_t)a.raw % (uintptr_t)(4 * esize) == 0 && (uintptr_t)a.out % 16 == 0 &&
                     (uintptr_t)a.part % 16 == 0;
    const dim3 grid((unsigned)((int64_t)a.nsub * nblk));
    if (vec) hipLaunchKernelGGL(k_unpack_pol<true>, grid, dim3(256), 0, st, a, conv);
    else hipLaunchKernelGGL(k_unpack_pol<false>, grid, dim3(256), 0, st, a, conv);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_base_window(a, st)) != hipSuccess) return e;
    // the statistics of all nsub x 4 x nchan rows, each with its sub-int's window
    UnpackArgs r = a;
    r.nchan = 4 * a.nchan;
    const int64_t rows = (int64_t)r.nsub * r.nchan;
    hipLaunchKernelGGL(k_row_stats, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, r);
    return hipGetLastError();
}

// Device-side copy out of page-locked host memory (zero-copy reads over
// PCIe by the CUs): the fit inputs' staging buffer reaches HBM without a
// copy-engine transfer, so it never queues behind an archive upload.
__global__ __launch_bounds__(256) void k_copy_host(const uint4 *__restrict__ src,
                                                   uint4 *__restrict__ dst, int64_t n16) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
        dst[i] = src[i];
}

__global__ __launch_bounds__(64) void k_copy_host_tail(const uint8_t *__restrict__ src,
                                                       uint8_t *__restrict__ dst, int64_t n) {
    const int64_t i = threadIdx.x;
    if (i < n) dst[i] = src[i];
}

hipError_t launch_copy_host(const void *src_dev, void *dst, int64_t nbytes, hipStream_t st) {
    const int64_t n16 = nbytes / 16, tail = nbytes - n16 * 16;
    if (n16 > 0) {
        const int64_t want = (n16 + 255) / 256;
        const unsigned grid = (unsigned)(want < 1024 ? want : 1024);
        hipLaunchKernelGGL(k_copy_host, dim3(grid), dim3(256), 0, st, (const uint4 *)src_dev,
                           (uint4 *)dst, n16);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (tail > 0) {
        hipLaunchKernelGGL(k_copy_host_tail, dim3(1), dim3(64), 0, st,
                           (const uint8_t *)src_dev + n16 * 16, (uint8_t *)dst + n16 * 16, tail);
        return hipGetLastError();
    }
    return hipSuccess;
}

size_t unpack_partials(int nsub, int nchan, int nbin) {
    return (size_t)nsub * ((nchan + kUnpackChans - 1) / kUnpackChans) * nbin;
}

}  // namespace ppf
