// Normal equations of the Gaussian-component portrait model
// (ppf_gauss_lsq_batch): what a Levenberg-Marquardt fit of
// pplib.fit_gaussian_portrait needs per iteration, from one call.
//
//   k_gauss_rows   one workgroup per (fit, channel, column): the model row
//                  m(p + delta_j e_j) (column j < nfree) or m(p) (column
//                  nfree) by gp_build_row, the row builder of k_gauss_port,
//                  so m(p) carries the bits of ppf_gauss_portrait_batch.
//                  rows: [nfit][nchan][nfree + 1][nbin].
//   k_gauss_gram   the columns c_j = ((m_j - m) / delta_j) * w and
//                  c_nfree = (data - m) * w are formed on load (contraction
//                  off, in that order) and contracted with the f64 MFMA
//                  (v_mfma_f64_16x16x4f64): nfree + 1 padded to 16-row tiles,
//                  upper-triangle tile pairs only.  A workgroup takes one
//                  tile pair over one chunk of the K = nchan nbin axis (a
//                  channel's kGramSeg bins), a wave every fourth 64-bin block
//                  of it; the four wave tiles are summed in wave order and
//                  written as the chunk's partial tile.
//   k_gauss_gram_fin  sums the partial tiles in chunk order and writes both
//                  triangles.  No atomics: the result is bitwise reproducible.
//
// The joined model (ppf_gauss_portrait_join_batch, ppf_gauss_lsq_join_batch:
// several archives, each rotated by a phase and a DM of its own):
// k_gauss_port_join, k_gauss_rows_join and k_gauss_gram_join take the join
// arguments (GaussJoin) as a second kernel argument and build an archive's
// rows with gp_build_row<..., ROT>; the kernels above are as they were.
#include <hip/hip_runtime.h>

#include "ppf_device.hpp"
#include "ppf_gaussrow.hpp"
#include "ppf_internal.hpp"
#include "ppf_launch.hpp"

namespace ppf {

// the rotation of a row of archive id (>= 0) at frequency f, rotate_data's
// order of operations (pplib.py:2478-2504); jp: the fit's join parameters,
// entry pq (an index into them, < 0: none) read as jp[pq] + dj
__device__ __forceinline__ double join_rot(const double *jp, int id, int pq, double dj, double P, double f,
                                           double nu_ref) {
#pragma clang fp contract(off)
    const double phi = pq == 2 * id ? jp[2 * id] + dj : jp[2 * id];
    const double DM = pq == 2 * id + 1 ? jp[2 * id + 1] + dj : jp[2 * id + 1];
    const double D = kDconst * DM / P;
    const double fterm = pow(f, -2.0) - pow(nu_ref, -2.0);
    return phi + D * fterm;
}

// lds as gp_build_row left it (even nbin) to the row o of nbin doubles
__device__ __forceinline__ void gauss_store_even(double2 *o, const double2 *lds, int N, GpRow kind) {
    if (kind == kGpPacked) {
        store_packed(o, lds, N, 1.0 / (double)N);
        return;
    }
    for (int j = threadIdx.x; j < N; j += kBlock) o[j] = lds[j];
}

// k_gauss_rows and, JOIN, k_gauss_rows_join (even nbin): free_idx then
// indexes [params, join params, scattering index].  A column that perturbs a
// join parameter of another archive than the row's equals m(p): its
// workgroup builds nothing, and k_gauss_gram_join reads no row there.  A row
// of no archive (join_id < 0) is built by the unrotated code.
template <int KMAX, bool MX, bool JOIN>
__device__ __forceinline__ void gauss_rows_body(const GaussLsqArgs &a, const GaussJoin &jn) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 2];
    const int nbin = a.nbin, N = nbin >> 1, ncol = a.nfree + 1;
    const int col = blockIdx.x % ncol;
    const int n = (blockIdx.x / ncol) % a.nchan, fit = blockIdx.x / (ncol * a.nchan);
    int id = -1, next = a.npar;   // the row's archive; the scattering index's entry
    if constexpr (JOIN) {
        id = jn.join_id[(int64_t)fit * a.nchan + n];
        next = a.npar + 2 * jn.njoin;
    }
    int pj = -1;
    double dj = 0.0;
    if (col < a.nfree) {
        pj = a.free_idx[col];
        dj = a.delta[(int64_t)fit * a.nfree + col];
    }
    const int pq = pj >= a.npar && pj < next ? pj - a.npar : -1;
    if (pq >= 0 && (pq >> 1) != id) return;   // (block-uniform)
    const double *prm = a.params + (int64_t)fit * a.npar;
    const double f = a.freqs[(int64_t)fit * a.nchan + n], nu_ref = a.nu_ref[fit];
    const double tau = pj == 1 ? prm[1] + dj : prm[1];
    const double alpha = pj == next ? a.scat_index[fit] + dj : a.scat_index[fit];
    GpRow kind;
    if (JOIN && id >= 0) {
        const double rot = join_rot(jn.join_params + (int64_t)fit * 2 * jn.njoin, id, pq, dj, jn.P[fit], f, nu_ref);
        kind = gp_build_row<KMAX, MX, true, JOIN>(lds, red, nbin, a.ngauss, a.code[0], a.code[1], a.code[2], prm, pj,
                                                  dj, tau, alpha, f, nu_ref, a.T, a.T2, a.T, a.T2, rot);
    } else {
        kind = gp_build_row<KMAX, MX, true>(lds, red, nbin, a.ngauss, a.code[0], a.code[1], a.code[2], prm, pj, dj,
                                            tau, alpha, f, nu_ref, a.T, a.T2, a.T, a.T2);
    }
    gauss_store_even(reinterpret_cast<double2 *>(a.rows) + (int64_t)blockIdx.x * N, lds, N, kind);
}

template <int KMAX, bool MX>
__global__ __launch_bounds__(kBlock) void k_gauss_rows(GaussLsqArgs a) {
    gauss_rows_body<KMAX, MX, false>(a, GaussJoin{});
}

template <int KMAX, bool MX>
__global__ __launch_bounds__(kBlock) void k_gauss_rows_join(GaussLsqArgs a, GaussJoin jn) {
    gauss_rows_body<KMAX, MX, true>(a, jn);
}

// k_gauss_port of the joined model (even nbin within the LDS transforms): a
// row of no archive (join_id < 0) is built by the unrotated code
template <int KMAX, bool MX>
__global__ __launch_bounds__(kBlock) void k_gauss_port_join(GaussArgs a, GaussJoin jn) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double2 lds[];
    __shared__ double red[kWaves * 2];
    const int nbin = a.nbin, N = nbin >> 1;
    const int p = blockIdx.x / a.nchan, n = blockIdx.x % a.nchan;
    const double *prm = a.params + (int64_t)p * a.npar;
    const double f = a.freqs[(int64_t)p * a.nchan + n], nu_ref = a.nu_ref[p];
    const int id = jn.join_id[blockIdx.x];
    GpRow kind;
    if (id >= 0) {
        const double rot = join_rot(jn.join_params + (int64_t)p * 2 * jn.njoin, id, -1, 0.0, jn.P[p], f, nu_ref);
        kind = gp_build_row<KMAX, MX, false, true>(lds, red, nbin, a.ngauss, a.code[0], a.code[1], a.code[2], prm, -1,
                                                   0.0, prm[1], a.scat_index[p], f, nu_ref, a.T, a.T2, a.Te, a.T2e,
                                                   rot);
    } else {
        kind = gp_build_row<KMAX, MX, false>(lds, red, nbin, a.ngauss, a.code[0], a.code[1], a.code[2], prm, -1, 0.0,
                                             prm[1], a.scat_index[p], f, nu_ref, a.T, a.T2, a.Te, a.T2e);
    }
    gauss_store_even(reinterpret_cast<double2 *>(a.out) + (int64_t)blockIdx.x * N, lds, N, kind);
}

// tile pair index -> (ti <= tj), row-major over the upper triangle
__device__ __forceinline__ void gram_pair(int pair, int ntile, int &ti, int &tj) {
    ti = 0;
    int left = ntile;
    while (pair >= left) { pair -= left; --left; ++ti; }
    tj = ti + pair;
}

// JOIN: a column that perturbs a join parameter of another archive than the
// channel's is exact zeros over the channel (k_gauss_rows_join built no row
// there: none is read)
template <bool JOIN>
__device__ __forceinline__ void gauss_gram_body(const GaussLsqArgs &a, const GaussJoin &jn) {
#pragma clang fp contract(off)
    __shared__ double sh[kWaves][256];
    const int nbin = a.nbin, nfree = a.nfree, ncol = nfree + 1;
    const int chunk = blockIdx.x, pair = blockIdx.y, fit = blockIdx.z;
    const int n = chunk / a.nseg, seg = chunk % a.nseg;
    int ti, tj;
    gram_pair(pair, a.ntile, ti, tj);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int ia = ti * 16 + c, ib = tj * 16 + c;
    const int64_t rowch = (int64_t)fit * a.nchan + n;
    const double *R = a.rows + rowch * ncol * nbin;
    const double *mb = R + (int64_t)nfree * nbin;
    const double *ma = R + (int64_t)min(ia, nfree) * nbin;
    const double *mc = R + (int64_t)min(ib, nfree) * nbin;
    const double *w = a.inv_errs + rowch * nbin;
    const float *d32 = reinterpret_cast<const float *>(a.data) + rowch * nbin;
    const double *d64 = reinterpret_cast<const double *>(a.data) + rowch * nbin;
    const double da = ia < nfree ? a.delta[(int64_t)fit * nfree + ia] : 1.0;
    const double db = ib < nfree ? a.delta[(int64_t)fit * nfree + ib] : 1.0;
    const bool needd = ia == nfree || ib == nfree;
    bool za = false, zb = false;   // the column is zero over this channel
    if constexpr (JOIN) {
        const int id = jn.join_id[rowch], next = a.npar + 2 * jn.njoin;
        if (ia < nfree) {
            const int pa = a.free_idx[ia];
            za = pa >= a.npar && pa < next && ((pa - a.npar) >> 1) != id;
        }
        if (ib < nfree) {
            const int pb = a.free_idx[ib];
            zb = pb >= a.npar && pb < next && ((pb - a.npar) >> 1) != id;
        }
    }
    const int kend = min(nbin, (seg + 1) * kGramSeg);
    typedef double d4 __attribute__((ext_vector_type(4)));
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int b0 = seg * kGramSeg + wave * 64; b0 < kend; b0 += kWaves * 64) {   // (wave-uniform)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k0 = b0 + h * 32 + q * 8;
            double va[8], vb[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int k = k0 + s;
                const bool in = k < kend;
                const double m0 = in ? mb[k] : 0.0, wk = in ? w[k] : 0.0;
                double xa, xb;
                if constexpr (JOIN) {
                    xa = in && !za ? ma[k] : 0.0;
                    xb = in && !zb ? mc[k] : 0.0;
                } else {
                    xa = in ? ma[k] : 0.0;
                    xb = in ? mc[k] : 0.0;
                }
                double dk = 0.0;
                if (in && needd) dk = a.dtype == 0 ? (double)d32[k] : d64[k];
                double ca = 0.0, cb = 0.0;
                if (in) {
                    if (ia < nfree) ca = ((xa - m0) / da) * wk;
                    else if (ia == nfree) ca = (dk - m0) * wk;
                    if (ib < nfree) cb = ((xb - m0) / db) * wk;
                    else if (ib == nfree) cb = (dk - m0) * wk;
                    if constexpr (JOIN) {
                        if (za) ca = 0.0;
                        if (zb) cb = 0.0;
                    }
                }
                va[s] = ca;
                vb[s] = cb;
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[s], vb[s], acc, 0, 0, 0);
        }
    }
    // D[row][col]: col = lane & 15 (B's column), row = (lane >> 4) + 4 r (A's)
#pragma unroll
    for (int r = 0; r < 4; ++r) sh[wave][(q + 4 * r) * 16 + c] = acc[r];
    __syncthreads();
    const int t = threadIdx.x;
    const double s = ((sh[0][t] + sh[1][t]) + sh[2][t]) + sh[3][t];
    a.part[(((int64_t)fit * gridDim.x + chunk) * a.npair + pair) * 256 + t] = s;
}

__global__ __launch_bounds__(kBlock) void k_gauss_gram(GaussLsqArgs a) {
    gauss_gram_body<false>(a, GaussJoin{});
}

__global__ __launch_bounds__(kBlock) void k_gauss_gram_join(GaussLsqArgs a, GaussJoin jn) {
    gauss_gram_body<true>(a, jn);
}

__global__ __launch_bounds__(kBlock) void k_gauss_gram_fin(GaussLsqArgs a, int nchunk) {
#pragma clang fp contract(off)
    const int pair = blockIdx.x, fit = blockIdx.y, t = threadIdx.x;
    const int ncol = a.nfree + 1;
    int ti, tj;
    gram_pair(pair, a.ntile, ti, tj);
    const double *p = a.part + (((int64_t)fit * nchunk) * a.npair + pair) * 256 + t;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s = s + p[(int64_t)ch * a.npair * 256];
    const int i = ti * 16 + (t >> 4), j = tj * 16 + (t & 15);
    if (i >= ncol || j >= ncol) return;
    double *G = a.gram + (int64_t)fit * ncol * ncol;
    G[(int64_t)i * ncol + j] = s;
    if (ti != tj) G[(int64_t)j * ncol + i] = s;   // a diagonal tile holds both triangles itself
}

hipError_t launch_gauss_lsq(const GaussLsqArgs &a, hipStream_t st) {
    const size_t lds = (size_t)(a.nbin / 2) * sizeof(double2);
    const int ncol = a.nfree + 1;
    dim3 g((unsigned)((int64_t)a.nfit * a.nchan * ncol)), b(kBlock);
    hipError_t e = dispatch_kmax_mx(a.nbin / 2, !is_pow2(a.nbin / 2), [&](auto K, auto MX) {
        hipLaunchKernelGGL((k_gauss_rows<K(), MX()>), g, b, lds, st, a);
    });
    if (e != hipSuccess) return e;
    const int nchunk = a.nchan * a.nseg;
    hipLaunchKernelGGL(k_gauss_gram, dim3((unsigned)nchunk, (unsigned)a.npair, (unsigned)a.nfit), b, 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_gauss_gram_fin, dim3((unsigned)a.npair, (unsigned)a.nfit), b, 0, st, a, nchunk);
    return hipGetLastError();
}

hipError_t launch_gauss_lsq_join(const GaussLsqArgs &a, const GaussJoin &j, hipStream_t st) {
    const size_t lds = (size_t)(a.nbin / 2) * sizeof(double2);
    const int ncol = a.nfree + 1;
    dim3 g((unsigned)((int64_t)a.nfit * a.nchan * ncol)), b(kBlock);
    hipError_t e = dispatch_kmax_mx(a.nbin / 2, !is_pow2(a.nbin / 2), [&](auto K, auto MX) {
        hipLaunchKernelGGL((k_gauss_rows_join<K(), MX()>), g, b, lds, st, a, j);
    });
    if (e != hipSuccess) return e;
    const int nchunk = a.nchan * a.nseg;
    hipLaunchKernelGGL(k_gauss_gram_join, dim3((unsigned)nchunk, (unsigned)a.npair, (unsigned)a.nfit), b, 0, st, a,
                       j);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_gauss_gram_fin, dim3((unsigned)a.npair, (unsigned)a.nfit), b, 0, st, a, nchunk);
    return hipGetLastError();
}

// even nbin within the LDS transforms (checked by the caller)
hipError_t launch_gauss_port_join(const GaussArgs &a, const GaussJoin &j, hipStream_t st) {
    const size_t lds = (size_t)(a.nbin / 2) * sizeof(double2);
    dim3 g((unsigned)((int64_t)a.nport * a.nchan)), b(kBlock);
    return dispatch_kmax_mx(a.nbin / 2, !is_pow2(a.nbin / 2), [&](auto K, auto MX) {
        hipLaunchKernelGGL((k_gauss_port_join<K(), MX()>), g, b, lds, st, a, j);
    });
}

}  // namespace ppf
