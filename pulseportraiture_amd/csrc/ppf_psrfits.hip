// ppf_psrfits.hip -- device side of the PSRCHIVE-free PSRFITS fast path
// (pulseportraiture_amd/psrfits.py): the raw DATA bytes of
// a fold-mode SUBINT table arrive as they sit in the file and are turned
// into the float32 rows load_data would hand get_TOAs (pplib.py:2749-2915):
// total intensity (pscrunch=True) or all four polarisations in the state
// asked for, plus the per-profile baseline statistics and S/N.
//
//   k_unpack      WG = (sub-int, block of kUnpackChans channels), threads
//                 along the bins.  Per sample: big-endian int16 / uint8 /
//                 float32 (or native float32 rows: load_data's statistics
//                 pass after dedispersion / tscrunch, DAT_SCL = 1, DAT_OFFS =
//                 0) -> DATA * DAT_SCL + DAT_OFFS in float32 arithmetic (two
//                 roundings, no fma: PSRCHIVE's loader) of the NPR
//                 polarisation blocks the instantiation reads, then
//                   NPR 1  total intensity = the block itself (npol 1, IQUV's I)
//                   NPR 2  total intensity = AA + BB (AA+BB / AABBCRCI)
//                   NPR 4  the state conversion `conv` in float32 (sums,
//                          differences and exact scalings by 2 or 1/2:
//                          nothing for an fma to contract)
//                 -> rows [nsub][nchan][nbin] (NPR 1, 2) or [nsub][4][nchan]
//                 [nbin] (NPR 4); the weighted channel sum of the block's
//                 total intensity (fixed channel order) -> partials
//                 [nsub][nblk][nbin].  Blocks past NPR are never touched.
//                 VEC: a lane takes 4 consecutive bins per polarisation with
//                 one 8-byte load (int16; 4-byte uint8, 16-byte float32) and
//                 one 16-byte store; the launch takes it when nbin is a
//                 multiple of 4 and raw, sub_stride, out and the partials are
//                 aligned for it.  Both forms run the same per-sample code:
//                 identical bits.
//   k_base_window WG per sub-int: total profile = sum of the partials in
//                 block order; PSRCHIVE's BaselineWindow: the circular window
//                 of W = rint(0.15 nbin) bins with the smallest sum (first
//                 minimum) -> window start, total profile out
//   k_row_stats   wave per row (nsub x npol_out * nchan of them, each with
//                 its sub-int's window): off-pulse mean over the window
//                 (subtracted from the row in place when rm_baseline),
//                 off-pulse sigma, S/N = sum over the on-pulse bins /
//                 (sigma sqrt(n_on))
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

// DATA * DAT_SCL + DAT_OFFS rounds twice, as PSRCHIVE's (and NumPy's) float32
// arithmetic does: the product is pinned in a register before the add, so
// the compiler cannot fuse them (-ffp-contract=fast)
__device__ __forceinline__ float scaled_f32(float x, float scl, float off) {
    float prod = x * scl;
    asm volatile("" : "+v"(prod));      // rounded product: no fma
    return prod + off;
}

// NPR: polarisation blocks read (1, 2 or 4); POL: four rows per channel are
// written (NPR 4), else the one of the total intensity
template <int NPR, bool POL, bool VEC>
__global__ __launch_bounds__(256) void k_unpack(UnpackArgs a) {
    static_assert(POL ? NPR == 4 : NPR <= 2, "intensity reads 1 or 2 blocks, full polarisation 4");
    constexpr int NB = VEC ? 4 : 1;     // bins per lane and trip
    constexpr int NPO = POL ? 4 : 1;    // rows written per channel
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    const int s = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const uint8_t *raw = a.raw + (int64_t)s * a.sub_stride;
    const float *scl = a.scl + (int64_t)s * a.npol * a.nchan;
    const float *off = a.offs + (int64_t)s * a.npol * a.nchan;
    const int n0 = blk * kUnpackChans, n1 = min(a.nchan, n0 + kUnpackChans);
    for (int b = threadIdx.x * NB; b < a.nbin; b += blockDim.x * NB) {
        double part[NB];
        for (int k = 0; k < NB; ++k) part[k] = 0.0;
        for (int n = n0; n < n1; ++n) {
            float x[NPR][NB];
            for (int p = 0; p < NPR; ++p) {
                const int64_t i = ((int64_t)p * a.nchan + n) * a.nbin + b;
                if (VEC) samples4_f32(raw, a.elem, i, x[p]);
                else x[p][0] = sample_f32(raw, a.elem, i);
            }
            float o[NPO][NB];
            const double w = a.wts ? (double)a.wts[(int64_t)s * a.nchan + n] : 1.0;
            for (int k = 0; k < NB; ++k) {
                float v[NPR], t;
                for (int p = 0; p < NPR; ++p)
                    v[p] = scaled_f32(x[p][k], scl[p * a.nchan + n], off[p * a.nchan + n]);
                if constexpr (POL) {
                    float c[4];
                    t = convert_state(a.conv, v, c);
                    for (int p = 0; p < 4; ++p) o[p][k] = c[p];
                } else {
                    if constexpr (NPR == 1) t = v[0];
                    else t = v[0] + v[1];
                    o[0][k] = t;
                }
                if (w != 0.0) part[k] = fma(w, (double)t, part[k]);
            }
            for (int p = 0; p < NPO; ++p) {
                float *row = a.out + (((int64_t)s * NPO + p) * a.nchan + n) * a.nbin + b;
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

template <int NPR, bool POL>
static void launch_k_unpack(const UnpackArgs &a, bool vec, hipStream_t st) {
    const int nblk = (a.nchan + kUnpackChans - 1) / kUnpackChans;
    const dim3 grid((unsigned)((int64_t)a.nsub * nblk));
    if (vec) hipLaunchKernelGGL((k_unpack<NPR, POL, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_unpack<NPR, POL, false>), grid, dim3(256), 0, st, a);
}

hipError_t launch_unpack(const UnpackArgs &a, hipStream_t st) {
    const int64_t esize = a.elem == 0 ? 2 : (a.elem == 1 ? 1 : 4);
    const bool vec = a.nbin % 4 == 0 && a.sub_stride % (4 * esize) == 0 &&
                     (uintptr_t)a.raw % (uintptr_t)(4 * esize) == 0 && (uintptr_t)a.out % 16 == 0 &&
                     (uintptr_t)a.part % 16 == 0;
    if (a.npol_out == 4) launch_k_unpack<4, true>(a, vec, st);
    else if (a.pol_mode == 1) launch_k_unpack<2, false>(a, vec, st);
    else launch_k_unpack<1, false>(a, vec, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_base_window(a, st)) != hipSuccess) return e;
    // the statistics of all nsub x npol_out x nchan rows, each with its
    // sub-int's window (k_row_stats' row -> sub-int map, nchan := npol_out nchan)
    UnpackArgs r = a;
    r.nchan = a.npol_out * a.nchan;
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
