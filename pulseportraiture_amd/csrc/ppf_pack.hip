// ppf_pack.hip -- the inverse of the PSRFITS unpack (ppf_psrfits.hip): float
// rows that are already on the device (an aligned portrait, a model portrait,
// a rotated or smoothed archive) become the DATA bytes of a fold-mode SUBINT
// table, so only those bytes cross PCIe on the way to the file
// (ppf_pack_psrfits_batch; pplib.write_archive / unload_new_archive).
//
// elem 0, big-endian int16: psrfits.quantize per row (ppf_quant.hpp, the
// arithmetic k_fake applies to the row it holds in LDS).  A row is read twice
// from global memory, once for its minimum / maximum and once to be
// digitised; the second read hits the cache.  Nothing is staged in LDS, so a
// row may have any length.
//   k_pack_wave   rows up to kPackWaveBins bins (a portrait is nchan rows of
//                 64..2048 bins): one WAVE per row, kWaves rows per
//                 workgroup, the minimum / maximum on the DPP network, no
//                 barrier; a workgroup strides over the row groups
//   k_pack_block  longer rows: one workgroup per row, the waves' partial
//                 minima / maxima through 2 kWaves doubles of LDS; a
//                 workgroup strides over the rows
// Both take VEC: rows whose bytes start 16-byte aligned on both sides (nbin %
// 8 == 0 and 16-byte aligned base pointers) are read as 8 bins per lane (two
// float4 or four double2 loads) and stored as one uint4; every other shape
// (odd nbin: a row starts on a 2-byte boundary only) takes one bin per lane
// and 2-byte stores, which are still contiguous across the wave.
//
// elem 2, big-endian float32: the sample is (float)x with its bytes swapped,
// DAT_SCL = 1, DAT_OFFS = 0; rows do not matter, so k_pack_f32 runs over the
// flat array, 4 samples (one uint4) per lane where both base pointers are
// 16-byte aligned, the tail (or everything) one sample per lane.
//
// No atomics; every output byte is written by exactly one lane from one
// row's data: the result is bitwise reproducible.  Row and element counts are
// 64-bit and every launch strides, so the grid never overflows.  A row with a
// NaN or an Inf gives unspecified bytes but no fault: the clip in quant_q
// maps every double to an int16, and nothing is indexed by data.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ppf_device.hpp"
#include "ppf_internal.hpp"
#include "ppf_quant.hpp"

namespace ppf {

constexpr int kPackWaveBins = 2048;      // longest row a single wave takes
constexpr int kPackMaxGrid = 8192;       // workgroups per launch; the rest by stride

__device__ __forceinline__ void load8(const float *x, double (&v)[8]) {
    const float4 a = reinterpret_cast<const float4 *>(x)[0];
    const float4 b = reinterpret_cast<const float4 *>(x)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const double *x, double (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double2 z = reinterpret_cast<const double2 *>(x)[i];
        v[2 * i] = z.x;
        v[2 * i + 1] = z.y;
    }
}

// minimum / maximum of the bins THREADS threads share, into this thread's lo / hi
template <typename T, bool VEC, int THREADS>
__device__ __forceinline__ void row_range(const T *x, int nbin, int t, double &lo, double &hi) {
    lo = kDblMax;
    hi = -kDblMax;
    if (VEC) {
        for (int j = t; j < (nbin >> 3); j += THREADS) {
            double v[8];
            load8(x + 8 * (int64_t)j, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                lo = fmin(lo, v[i]);
                hi = fmax(hi, v[i]);
            }
        }
    } else {
        for (int b = t; b < nbin; b += THREADS) {
            const double v = (double)x[b];
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
    }
}

// the row digitised with (offs, scl) into its nbin * 2 bytes at o
template <typename T, bool VEC, int THREADS>
__device__ __forceinline__ void row_store(const T *x, int nbin, int t, double offs, double scl,
                                          uint8_t *o) {
    if (VEC) {
        uint4 *o16 = reinterpret_cast<uint4 *>(o);
        for (int j = t; j < (nbin >> 3); j += THREADS) {
            double v[8];
            load8(x + 8 * (int64_t)j, v);
            uint4 w;
            w.x = quant_q2(v[0], v[1], offs, scl);
            w.y = quant_q2(v[2], v[3], offs, scl);
            w.z = quant_q2(v[4], v[5], offs, scl);
            w.w = quant_q2(v[6], v[7], offs, scl);
            o16[j] = w;
        }
    } else {
        uint16_t *o2 = reinterpret_cast<uint16_t *>(o);
        for (int b = t; b < nbin; b += THREADS)
            o2[b] = (uint16_t)quant_q((double)x[b], offs, scl);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_pack_wave(PackArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    // the row is the same in every lane of a wave: the loop is wave-uniform,
    // so all 64 lanes reach the DPP reductions
    for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < a.nrow;
         row += stride) {
        const T *x = reinterpret_cast<const T *>(a.rows) + row * a.nbin;
        double lo, hi;
        row_range<T, VEC, 64>(x, a.nbin, lane, lo, hi);
        lo = wave_reduce(lo, [](double p, double q) { return fmin(p, q); });
        hi = wave_reduce(hi, [](double p, double q) { return fmax(p, q); });
        const float offs_f = quant_offs(lo, hi), scl_f = quant_scl(lo, hi);
        if (lane == 0) {
            a.scl[row] = scl_f;
            a.offs[row] = offs_f;
        }
        row_store<T, VEC, 64>(x, a.nbin, lane, (double)offs_f, (double)scl_f,
                              a.raw + row * a.nbin * 2);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_pack_block(PackArgs a) {
    __shared__ double red[2 * kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // blockIdx-only loop bounds: every thread of the workgroup takes the same
    // trips and reaches both barriers
    for (int64_t row = blockIdx.x; row < a.nrow; row += gridDim.x) {
        const T *x = reinterpret_cast<const T *>(a.rows) + row * a.nbin;
        double lo, hi;
        row_range<T, VEC, kBlock>(x, a.nbin, (int)threadIdx.x, lo, hi);
        lo = wave_reduce(lo, [](double p, double q) { return fmin(p, q); });
        hi = wave_reduce(hi, [](double p, double q) { return fmax(p, q); });
        if (lane == 0) {
            red[wave] = lo;
            red[kWaves + wave] = hi;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            lo = fmin(lo, red[w]);
            hi = fmax(hi, red[kWaves + w]);
        }
        __syncthreads();                 // red is rewritten for the next row
        const float offs_f = quant_offs(lo, hi), scl_f = quant_scl(lo, hi);
        if (threadIdx.x == 0) {
            a.scl[row] = scl_f;
            a.offs[row] = offs_f;
        }
        row_store<T, VEC, kBlock>(x, a.nbin, (int)threadIdx.x, (double)offs_f, (double)scl_f,
                                  a.raw + row * a.nbin * 2);
    }
}

__device__ __forceinline__ uint32_t be_f32(float v) {
    return __builtin_bswap32(__float_as_uint(v));
}

// four samples from a 16-byte aligned address, rounded to float32
__device__ __forceinline__ float4 load4(const float *x) {
    return *reinterpret_cast<const float4 *>(x);
}
__device__ __forceinline__ float4 load4(const double *x) {
    const double2 p = reinterpret_cast<const double2 *>(x)[0];
    const double2 q = reinterpret_cast<const double2 *>(x)[1];
    return make_float4((float)p.x, (float)p.y, (float)q.x, (float)q.y);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_pack_f32(PackArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n = a.nrow * a.nbin;
    const T *x = reinterpret_cast<const T *>(a.rows);
    for (int64_t r = t; r < a.nrow; r += stride) {
        a.scl[r] = 1.0f;
        a.offs[r] = 0.0f;
    }
    const int64_t n4 = VEC ? n >> 2 : 0;
    uint4 *o16 = reinterpret_cast<uint4 *>(a.raw);
    for (int64_t j = t; j < n4; j += stride) {
        const float4 v = load4(x + 4 * j);
        uint4 w;
        w.x = be_f32(v.x);
        w.y = be_f32(v.y);
        w.z = be_f32(v.z);
        w.w = be_f32(v.w);
        o16[j] = w;
    }
    uint32_t *o4 = reinterpret_cast<uint32_t *>(a.raw);
    for (int64_t i = 4 * n4 + t; i < n; i += stride) o4[i] = be_f32((float)x[i]);
}

template <typename T, bool VEC>
static void launch_pack_t(const PackArgs &a, hipStream_t st) {
    if (a.elem == 2) {
        const int64_t per = VEC ? 4 : 1;
        const int64_t want = (a.nrow * a.nbin + per * kBlock - 1) / (per * kBlock);
        const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(want, 1), kPackMaxGrid);
        hipLaunchKernelGGL((k_pack_f32<T, VEC>), dim3(grid), dim3(kBlock), 0, st, a);
    } else if (a.nbin <= kPackWaveBins) {
        const int64_t want = (a.nrow + kWaves - 1) / kWaves;
        const unsigned grid = (unsigned)std::min<int64_t>(want, kPackMaxGrid);
        hipLaunchKernelGGL((k_pack_wave<T, VEC>), dim3(grid), dim3(kBlock), 0, st, a);
    } else {
        const unsigned grid = (unsigned)std::min<int64_t>(a.nrow, kPackMaxGrid);
        hipLaunchKernelGGL((k_pack_block<T, VEC>), dim3(grid), dim3(kBlock), 0, st, a);
    }
}

hipError_t launch_pack(const PackArgs &a, hipStream_t st) {
    // wide accesses only where every one of them is 16-byte aligned: the
    // base pointers, and for int16 every row start on both sides
    const bool base16 = (((uintptr_t)a.rows | (uintptr_t)a.raw) & 15) == 0;
    const bool vec = base16 && (a.elem == 2 || (a.nbin & 7) == 0);
    if (a.f32in) {
        if (vec) launch_pack_t<float, true>(a, st);
        else launch_pack_t<float, false>(a, st);
    } else {
        if (vec) launch_pack_t<double, true>(a, st);
        else launch_pack_t<double, false>(a, st);
    }
    return hipGetLastError();
}

}  // namespace ppf
