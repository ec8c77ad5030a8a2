// ppf_eval.hip -- the portrait likelihood evaluated at many parameter points.
//
// chi'^2(theta) = -sum_n C_n^2 / S_n (pptoaslib.py:564-581), its gradient
// (584-614) and Hessian (617-684) at npoint vectors theta = (phi, DM, GM, tau,
// alpha) per problem, one problem being one (data_FT, model_FT) pair as the
// reference's functions take them: channel-major [nchan][nharm] complex128.
//
// k_eval: one workgroup per (problem, block of kEvalPointBlock points,
// channel).  The workgroup forms X_k = D_k conj(M_k) and |M_k|^2 of its
// channel ONCE, in tiles of kEvalTile harmonics held in LDS, and every point
// of the block is summed from that tile: the spectra's global traffic does not
// grow with the points of a block.  Lanes run along harmonics -- the input's
// contiguous axis, so the loads coalesce with no transposed copy and a single
// point (K = 1, the reference's one-point signatures) still fills a wave; a
// wave owns kEvalPPW points of the block.  Lane l of a point takes harmonics
// tile0 + l + 64 j: its phasor is seeded exactly, cexp2pi((tile0 + l) phi_n),
// at every tile and stepped by exp(2 pi i 64 phi_n) (64 phi_n is exact), at
// most kEvalTile / 64 = 16 steps from a seed.  The nine raw harmonic sums of
// k_pass (ppf_solve.hip: a0 a1 a2 q1 q1p q2 s0 t1 t2, in u = 2 pi k tau_n) are
// kept per lane across tiles, folded over the wave on the DPP network in a
// fixed order, and lane 0 turns them into the channel's C, S and their
// derivatives (the closed forms of chan_derivs) and into the channel's
// contribution to f, g and H, stored to the workspace.
//
// k_eval_reduce: one wave per (problem, point); lane q < 21 adds component q
// over the channels in channel order, skipping masked channels (their slots
// are never written nor read).  No atomics anywhere: results are bitwise
// reproducible, do not depend on how the points are blocked (a K-point call
// equals K one-point calls bit for bit), and a masked channel changes no bit
// against the same problem with the channel deleted.
#include "ppf_device.hpp"
#include "ppf_internal.hpp"

namespace ppf {

namespace {

constexpr int kEvalPPW = kEvalPointBlock / kWaves;   // points per wave
static_assert(kEvalPPW * kWaves == kEvalPointBlock, "point block = waves x points per wave");
static_assert(kEvalTile % 64 == 0 && kEvalTile / 64 <= 64, "phasor recurrence <= 64 steps");

// components of the (f, g[5], upper H[15]) vector an order needs
__host__ __device__ constexpr int eval_ncomp(int order) { return order == 0 ? 1 : (order == 1 ? 6 : 21); }
__device__ __forceinline__ int upper_idx(int i, int j) { return i * 5 - i * (i - 1) / 2 + (j - i); }

// nu^-2 and nu^-4 rounded once, as the correctly rounded powers NumPy hands
// the reference: k phi_n multiplies every rounding of phi_n, and the runtime's
// pow() may be an ulp or two off.  nu^2 (nu^4) is formed exactly as hi + lo and
// the quotient corrected by its residual.  An infinite reference frequency
// gives 0.
__device__ __forceinline__ double inv_hilo(double hi, double lo) {
#pragma clang fp contract(off)
    const double q = 1.0 / hi;
    const double r = fma(-q, hi, 1.0) - q * lo;
    return fma(q, r, q);
}
__device__ __forceinline__ double inv_pow2(double nu) {
#pragma clang fp contract(off)
    if (!(fabs(nu) <= kDblMax)) return nu == nu ? 0.0 : nu;
    const double hi = nu * nu;
    return inv_hilo(hi, fma(nu, nu, -hi));
}
__device__ __forceinline__ double inv_pow4(double nu) {
#pragma clang fp contract(off)
    if (!(fabs(nu) <= kDblMax)) return nu == nu ? 0.0 : nu;
    const double hi = nu * nu, lo = fma(nu, nu, -hi);
    const double h2 = hi * hi;
    return inv_hilo(h2, fma(hi, hi, -h2) + 2.0 * hi * lo);
}

struct RawSums {
    double a0, a1, a2, q1, q1p, q2, s0, t1, t2;
};

template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_eval(EvalArgs a) {
    // no contraction of a * b + c beyond the fma()s written out: a point's
    // bits must not depend on which of the unrolled point slots computes it
#pragma clang fp contract(off)
    __shared__ double2 xs[kEvalTile];
    __shared__ double ps[kEvalTile];
    const int npb = (a.npoint + kEvalPointBlock - 1) / kEvalPointBlock;
    const int n = (int)(blockIdx.x % (unsigned)a.nchan);
    const int pb = (int)((blockIdx.x / (unsigned)a.nchan) % (unsigned)npb);
    const int s = (int)(blockIdx.x / (unsigned)a.nchan / (unsigned)npb);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t sn = (int64_t)s * a.nchan + n;
    const int p_blk = pb * kEvalPointBlock;
    if (a.mask && !a.mask[sn]) {
        // a masked channel: exact zeros in the per-channel terms, nothing
        // loaded (its data may be NaN), no workspace slot written
        if (a.terms) {
            const int np = min(kEvalPointBlock, a.npoint - p_blk);
            for (int i = threadIdx.x; i < np * kEvalTerms; i += kBlock) {
                const int p = p_blk + i / kEvalTerms, q = i % kEvalTerms;
                a.terms[(((int64_t)s * a.npoint + p) * kEvalTerms + q) * a.nchan + n] = 0.0;
            }
        }
        return;
    }
    const int mi = a.model_index ? a.model_index[s] : (a.nmodel > 1 ? s : 0);
    const double2 *D = a.D + sn * a.nharm;
    const double2 *M = a.M + ((int64_t)mi * a.nchan + n) * a.nharm;
    const double nu = a.freqs[sn], P = a.P[s];
    const double nu_DM = a.nus[s * 3 + 0], nu_GM = a.nus[s * 3 + 1], nu_tau = a.nus[s * 3 + 2];
    const double err = a.errs[sn], e2 = err * err;
    // phase_shifts / phase_shifts_deriv (pptoaslib.py:195-242), the
    // reference's order of operations: k phi_n amplifies every rounding here
    const double f2 = inv_pow2(nu) - inv_pow2(nu_DM), f4 = inv_pow4(nu) - inv_pow4(nu_GM);
    double phin[kEvalPPW], aa[kEvalPPW], tau_lin[kEvalPPW];
    double2 W64[kEvalPPW];
    bool live[kEvalPPW];
    RawSums r[kEvalPPW];
#pragma unroll
    for (int u = 0; u < kEvalPPW; ++u) {
        const int p = p_blk + wave * kEvalPPW + u;
        live[u] = p < a.npoint;
        const double *th = a.theta + ((int64_t)s * a.npoint + (live[u] ? p : a.npoint - 1)) * 5;
        phin[u] = th[0] + kDconst * th[1] * f2 / P + kDconst * kDconst * th[2] * f4 / P;
        tau_lin[u] = a.log10_tau ? pow(10.0, th[3]) : th[3];
        aa[u] = kTwoPi * (tau_lin[u] * pow(nu / nu_tau, th[4]));
        W64[u] = cexp2pi(64.0 * phin[u]);
        r[u] = RawSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    }
    for (int tile0 = 0; tile0 < a.nharm; tile0 += kEvalTile) {
        if (tile0) __syncthreads();
        const int tl = min(kEvalTile, a.nharm - tile0);
        const int tl64 = (tl + 63) & ~63;            // whole 64-harmonic groups, zero-filled
        for (int t = threadIdx.x; t < tl64; t += kBlock) {
            double2 x = cmk(0.0, 0.0);
            double pk = 0.0;
            if (t < tl) {
                const double2 d = ld_stream(D + tile0 + t), m = M[tile0 + t];
                x = cmulc(d, m);
                pk = cabs2(m);
            }
            xs[t] = x;
            ps[t] = pk;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kEvalPPW; ++u) {
            if (!live[u]) continue;                  // wave-uniform
            double2 E = cexp2pi((double)(tile0 + lane) * phin[u]);
            const double2 W = W64[u];
            const double au = aa[u];
            RawSums q = r[u];
            for (int j = 0; j < tl64; j += 64) {
                const double kk = (double)(tile0 + j + lane);
                const double2 y = cmul(xs[j + lane], E);
                const double pk = ps[j + lane];
                // the scattering terms in closed form, as k_pass (ppf_solve.hip):
                // u = 2 pi k tau_n, d = 1 / (1 + u^2), conj(B) = d (1 + i u)
                const double uu = au * kk, u2 = uu * uu, den = 1.0 + u2;
                double d = __builtin_amdgcn_rcp(den);
                d = fma(d, fma(-den, d, 1.0), d);
                d = fma(d, fma(-den, d, 1.0), d);
                const double ud = uu * d;
                const double2 z1 = cmk(fma(y.x, d, -y.y * ud), fma(y.y, d, y.x * ud));
                q.a0 += z1.x;
                q.s0 = fma(d, pk, q.s0);
                if constexpr (ORDER >= 1) {
                    const double2 z2 = cmk(fma(z1.x, d, -z1.y * ud), fma(z1.y, d, z1.x * ud));
                    const double tp = u2 * d * d * pk;
                    q.a1 = fma(kk, z1.y, q.a1);
                    q.q1 = fma(-uu, z2.y, q.q1);
                    q.t1 += tp;
                    if constexpr (ORDER >= 2) {
                        const double z3 = fma(z2.x, d, -z2.y * ud);
                        q.a2 = fma(kk * kk, z1.x, q.a2);
                        q.q1p = fma(kk * uu, z2.x, q.q1p);
                        q.q2 = fma(-u2, z3, q.q2);
                        q.t2 = fma(tp * d, 1.0 - u2, q.t2);
                    }
                }
                E = cmul(E, W);
            }
            r[u] = q;
        }
    }
    double fl[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) fl[i] = a.flags ? a.flags[i] : 1.0;
    constexpr int NC = eval_ncomp(ORDER);
#pragma unroll
    for (int u = 0; u < kEvalPPW; ++u) {
        if (!live[u]) continue;
        const int p = p_blk + wave * kEvalPPW + u;
        // lanes -> wave, fixed order; every lane holds the totals
        const double C = wave_sum(r[u].a0) / e2, S = wave_sum(r[u].s0) / e2;
        double Cp = 0.0, Cpp = 0.0, Q1 = 0.0, Q1p = 0.0, Q2 = 0.0, S1 = 0.0, S2a = 0.0, S2b = 0.0;
        if constexpr (ORDER >= 1) {
            Cp = -kTwoPi * wave_sum(r[u].a1) / e2;
            Q1 = wave_sum(r[u].q1) / e2;
            const double t1 = wave_sum(r[u].t1) / e2;
            S1 = -2.0 * t1;
            S2a = 2.0 * t1;
        }
        if constexpr (ORDER >= 2) {
            Cpp = -kTwoPi * kTwoPi * wave_sum(r[u].a2) / e2;
            Q1p = -kTwoPi * wave_sum(r[u].q1p) / e2;
            Q2 = wave_sum(r[u].q2) / e2;
            S2b = -2.0 * wave_sum(r[u].t2) / e2;
        }
        if (lane == 0) {
            // (d tau_n / d theta_j) / tau_n and (d2 tau_n / d theta_i d theta_j) /
            // tau_n for j = tau, alpha (pptoaslib.py:266-299); tau = 0: the
            // reference's taus.sum() branches, every tau / alpha derivative 0
            const double dphi[3] = {1.0, kDconst * f2 / P, kDconst * kDconst * f4 / P};
            const double lnf = log(nu / nu_tau);
            double t[2] = {0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
            if (tau_lin[u] != 0.0) {
                t[1] = lnf;
                w[2] = lnf * lnf;
                if (a.log10_tau) {
                    t[0] = kLn10;
                    w[0] = kLn10 * kLn10;
                    w[1] = kLn10 * lnf;
                } else {
                    t[0] = 1.0 / tau_lin[u];
                    w[1] = lnf / tau_lin[u];
                }
            }
            double dC[5], dS[5], d2C[5][5], d2S[5][5];
    #pragma unroll
            for (int i = 0; i < 5; ++i) {
                dC[i] = dS[i] = 0.0;
    #pragma unroll
                for (int j = 0; j < 5; ++j) d2C[i][j] = d2S[i][j] = 0.0;
            }
            if constexpr (ORDER >= 1) {
    #pragma unroll
                for (int i = 0; i < 3; ++i) dC[i] = Cp * dphi[i];
    #pragma unroll
                for (int j = 0; j < 2; ++j) { dC[3 + j] = Q1 * t[j]; dS[3 + j] = S1 * t[j]; }
            }
            if constexpr (ORDER >= 2) {
    #pragma unroll
                for (int i = 0; i < 3; ++i) {
    #pragma unroll
                    for (int j = 0; j < 3; ++j) d2C[i][j] = Cpp * dphi[i] * dphi[j];
    #pragma unroll
                    for (int j = 0; j < 2; ++j) d2C[i][3 + j] = d2C[3 + j][i] = dphi[i] * t[j] * Q1p;
                }
    #pragma unroll
                for (int i = 0; i < 2; ++i)
    #pragma unroll
                    for (int j = i; j < 2; ++j) {
                        const double tt = t[i] * t[j], ww = w[i + j];
                        d2C[3 + i][3 + j] = d2C[3 + j][3 + i] = 2.0 * tt * Q2 + ww * Q1;
                        d2S[3 + i][3 + j] = d2S[3 + j][3 + i] = tt * S2a + 2.0 * tt * S2b + ww * S1;
                    }
            }
            if (a.terms) {
                double *o = a.terms + ((int64_t)s * a.npoint + p) * kEvalTerms * a.nchan + n;
                const int64_t st = a.nchan;
                o[0] = C;
                o[st] = S;
    #pragma unroll
                for (int i = 0; i < 5; ++i) {
                    o[(2 + i) * st] = dC[i];
                    o[(7 + i) * st] = dS[i];
    #pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        o[(12 + i * 5 + j) * st] = d2C[i][j];
                        o[(37 + i * 5 + j) * st] = d2S[i][j];
                    }
                }
            }
            // the channel's share of f, g, H (pptoaslib.py:580, 612, 665-671 with
            // no division by C, as k_pass)
            double acc[NC];
            const double iS = 1.0 / S, iS2 = iS * iS, iS3 = iS2 * iS, C2 = C * C;
            acc[0] = -C2 * iS;
            if constexpr (ORDER >= 1) {
    #pragma unroll
                for (int i = 0; i < 5; ++i) acc[1 + i] = -(2.0 * C * dC[i] * iS - C2 * dS[i] * iS2) * fl[i];
            }
            if constexpr (ORDER >= 2) {
    #pragma unroll
                for (int i = 0; i < 5; ++i)
    #pragma unroll
                    for (int j = i; j < 5; ++j)
                        acc[6 + upper_idx(i, j)] =
                            -2.0 * (C * d2C[i][j] * iS - 0.5 * C2 * d2S[i][j] * iS2 + dC[i] * dC[j] * iS +
                                    C2 * dS[i] * dS[j] * iS3 - C * (dC[i] * dS[j] + dS[i] * dC[j]) * iS2) *
                            fl[i] * fl[j];
            }
            double *dst = a.part + (((int64_t)s * a.npoint + p) * a.nchan + n) * NC;
    #pragma unroll
            for (int i = 0; i < NC; ++i) dst[i] = acc[i];
        }
    }
}

// one wave per (problem, point): lane q adds component q over the channels,
// in channel order
template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_eval_reduce(EvalArgs a) {
    constexpr int NC = eval_ncomp(ORDER);
    const int64_t sp = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int q = threadIdx.x & 63;
    if (sp >= (int64_t)a.nprob * a.npoint || q >= NC) return;
    const int s = (int)(sp / a.npoint);
    const uint8_t *mask = a.mask ? a.mask + (int64_t)s * a.nchan : nullptr;
    const double *src = a.part + sp * a.nchan * NC + q;
    double v = 0.0;
    for (int n = 0; n < a.nchan; ++n)
        if (!mask || mask[n]) v += src[(int64_t)n * NC];
    if (q == 0) {
        a.f[sp] = v;
    } else if (q < 6) {
        a.g[sp * 5 + (q - 1)] = v;
    } else {
        int i = 0, e = q - 6;
        while (e >= 5 - i) { e -= 5 - i; ++i; }
        const int j = i + e;
        a.H[sp * 25 + i * 5 + j] = v;
        a.H[sp * 25 + j * 5 + i] = v;
    }
}

template <int ORDER>
hipError_t launch_eval_t(const EvalArgs &a, hipStream_t st) {
    const int64_t npb = (a.npoint + kEvalPointBlock - 1) / kEvalPointBlock;
    const int64_t nblk = (int64_t)a.nprob * npb * a.nchan;
    hipLaunchKernelGGL(k_eval<ORDER>, dim3((unsigned)nblk), dim3(kBlock), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t nsp = (int64_t)a.nprob * a.npoint;
    hipLaunchKernelGGL(k_eval_reduce<ORDER>, dim3((unsigned)((nsp + kWaves - 1) / kWaves)), dim3(kBlock), 0,
                       st, a);
    return hipGetLastError();
}

}  // namespace

int64_t eval_partials(int64_t nprob, int64_t nchan, int64_t npoint, int order) {
    return nprob * nchan * npoint * eval_ncomp(order);
}

hipError_t launch_eval(const EvalArgs &a, hipStream_t st) {
    switch (a.order) {
        case 0: return launch_eval_t<0>(a, st);
        case 1: return launch_eval_t<1>(a, st);
        default: return launch_eval_t<2>(a, st);
    }
}

}  // namespace ppf
