// ppf_api.cpp -- C ABI of libppfit (include/ppfit.h): validation, workspace
// carving, twiddle-table cache and kernel sequencing.  No compute here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ppfit.h"
#include "ppf_internal.hpp"
#include "ppf_device.hpp"

struct ppf_ctx {
    int device;
    std::string err;               // last error message, guarded by err_mu
    mutable std::mutex err_mu;
    std::map<int, double2 *> tw;   // nbin -> [T (N) | T2 (N)]
    std::map<std::pair<int, int>, double2 *> cz;   // (Ns, Kmax) -> chirp z-transform tables
    std::mutex tw_mu;              // guards tw and cz (calls from several host threads)
    bool prof = false;
    static constexpr int kRing = 256;
    // [0..4]: stage boundaries; [5, 6]: the first moment pass (k_xmom_g,
    // FULL); [7, 8]: the guess-profile pass (k_dsum_w)
    static constexpr int kEv = 9;
    hipEvent_t ring[kRing][kEv] = {};
    bool ran[kRing][6] = {};
    // every streaming pass (k_pass) of a call: its (start, end) event pairs,
    // the pool grown on demand and reused by the ring slot
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pass_ev[kRing];
    int npass[kRing] = {};
    // the solver kernels of a call (kind 0 k_tr_mom, 1 k_tr_step (+ gates),
    // 2 k_postfit): (start, end) pairs, as pass_ev
    std::vector<std::pair<hipEvent_t, hipEvent_t>> solv_ev[kRing];
    std::vector<int> solv_kind[kRing];
    int nsolv[kRing] = {};
    long ncalls = 0;
    unsigned *host_active = nullptr;   // pinned, for the iteration loop
    // device scratch of the long-row FFTFIT (ppf_phase_shift_batch past the
    // LDS transforms; grown on demand, held for the whole synchronous call)
    void *lscr = nullptr;
    size_t lscr_bytes = 0;
    std::mutex lscr_mu;
};

namespace {

int fail(ppf_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx->err_mu);
        ctx->err = buf;
    }
    return code;
}

int hip_fail(ppf_ctx *ctx, hipError_t e, const char *where) {
    return fail(ctx, PPF_EHIP, "%s: %s", where, hipGetErrorString(e));
}

bool pow2_in_range(int nbin) {
    return nbin >= 32 && nbin <= 8192 && (nbin & (nbin - 1)) == 0;
}

// nbin the FFT kernels take: even 32..8192 and odd 33..4095 (power-of-two
// nbin on the register / radix-4 paths, the others on the mixed-radix LDS
// FFT, whose generic-radix stage takes prime factors above 7; odd nbin as a
// full-length complex transform of the row, ppf::rfft_len)
bool nbin_supported(int nbin) {
    return nbin >= 32 && nbin <= 8192 && ppf::fft_len_supported(ppf::rfft_len(nbin));
}

// log2 of a power-of-two FFT length, 0 otherwise (the kernels' "not a power
// of two" marker: no wave-FFT path, mixed-radix LDS FFT)
int fft_log2(int n) {
    if (n < 1 || (n & (n - 1))) return 0;
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

// fft_log2 of the real-row transform: 0 (mixed-radix LDS FFT) for odd nbin
int rfft_log2(int nbin) { return (nbin & 1) ? 0 : fft_log2(nbin / 2); }

int ilog2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

// get_noise_PS cut: int((1 - frac**-1) * nharm)  (pplib.py:2330)
int noise_kc(int nharm, int frac) {
    return (int)((1.0 - std::pow((double)frac, -1.0)) * (double)nharm);
}

int twiddles(ppf_ctx *ctx, int nbin, hipStream_t st, const double2 **T, const double2 **T2) {
    std::lock_guard<std::mutex> lock(ctx->tw_mu);
    auto it = ctx->tw.find(nbin);
    if (it == ctx->tw.end()) {
        const int N = ppf::rfft_len(nbin);
        double2 *p = nullptr;
        hipError_t e = hipMalloc(&p, sizeof(double2) * 2 * (size_t)N);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(twiddles)");
        e = ppf::launch_twiddles(N, p, p + N, st);
        if (e != hipSuccess) return hip_fail(ctx, e, "k_twiddles");
        // the table is cached for calls on ANY stream: finish it before it
        // is published (one-time cost per nbin)
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize(twiddles)");
        it = ctx->tw.emplace(nbin, p).first;
    }
    *T = it->second;
    *T2 = it->second + ppf::rfft_len(nbin);
    return PPF_OK;
}

// A small device -> pinned-host read-back the iteration loop waits on (round
// 6).  hipStreamSynchronize wakes the host 30-70 us after the copy lands
// (C4's kernel trace: the gaps before the re-centring k_xmom_g and before
// k_postfit); with PPF_OPT_SPIN_WAIT the words are instead preset to a
// sentinel no count takes and polled until the copy has overwritten them,
// with the stream synchronisation as the fallback after 2 s.  Opt-in: on
// GetTOAs' threaded host pipeline the polling cost 20 % of the PSRFITS rate
// even yielding the core (profiles/r06/ab_gtspin_status.txt).
constexpr unsigned kUnset = 0xFFFFFFFFu;
int read_back(ppf_ctx *ctx, unsigned *host, const unsigned *dev, int n, hipStream_t st, bool spin) {
    volatile unsigned *h = host;
    for (int i = 0; i < n; ++i) h[i] = kUnset;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    hipError_t e = hipMemcpyAsync(host, dev, n * sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpyAsync");
    if (spin) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            bool done = true;
            for (int i = 0; i < n; ++i) done = done && h[i] != kUnset;
            if (done) {
                std::atomic_thread_fence(std::memory_order_seq_cst);
                return PPF_OK;
            }
            const auto dt = std::chrono::steady_clock::now() - t0;
            if (dt > std::chrono::seconds(2)) break;
            // past the first 50 us the core is offered to other host threads
            // between polls (GetTOAs' readers and stagers share the CPUs)
            if (dt > std::chrono::microseconds(50)) std::this_thread::yield();
            else __builtin_ia32_pause();
        }
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
    return PPF_OK;
}

// The guess's brute grid of a whole turn with Ns >= 512 points (ppalign:
// Ns = nbin) as a chirp z-transform (k_guess, round 6): the plan and its
// cached kernel tables.  Returns false (direct sums) where it does not apply.
// (Round 6, first build: P was taken >= 2K - 1 = 1025, i.e. 2048, which
// cz_fft refuses, so the A/B of ab_czc4_status.txt ran the direct sums on
// both sides.)
bool cz_plan(int Ns, int K, ppf::CzPlan &c) {
    if (Ns < 2 * ppf::kBlock || K < 2) return false;
    // P >= K + J - 1 with chunks of J >= 256 outputs (nbin 1024: K = 513,
    // P = 1024, two chunks of 512)
    int P = 64;
    while (P < K + 255) P *= 2;
    if (P < 512 || P > 2048) return false;       // k_guess's instantiations (nbin 512-2048)
    c.Ns = Ns; c.K = K; c.P = P; c.J = P - K + 1; c.Q = (Ns + c.J - 1) / c.J;
    return true;
}
int cz_tables(ppf_ctx *ctx, const ppf::CzPlan &c, hipStream_t st, const double2 **B, const double2 **T) {
    const double2 *T2;
    int rc = twiddles(ctx, 2 * c.P, st, T, &T2);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(ctx->tw_mu);
    const auto key = std::make_pair(c.Ns, c.K);
    auto it = ctx->cz.find(key);
    if (it == ctx->cz.end()) {
        double2 *p = nullptr;
        hipError_t e = hipMalloc(&p, sizeof(double2) * (size_t)c.Q * c.P);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(cz)");
        e = ppf::launch_cz_table(c, p, *T, st);
        if (e != hipSuccess) return hip_fail(ctx, e, "k_cz_table");
        // cached for calls on any stream (as the twiddles)
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize(cz)");
        it = ctx->cz.emplace(key, p).first;
    }
    *B = it->second;
    return PPF_OK;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace regions in the order they are taken, each a multiple of 256
// bytes (an empty one takes none)
struct Carver {
    size_t o = 0;
    size_t operator()(size_t bytes) {
        const size_t at = o;
        o += align256(bytes);
        return at;
    }
};

// ---- the long (four-step / Bluestein) transforms: what their callers share --
// The transform of rows of n complex points (packed: two real samples each):
// M >= n points (a plain power of two) or >= 2 n - 1 (Bluestein), M = M1 M2
// for the four-step passes.  False past 2^24 points.
bool long_len(int64_t nbin, int64_t n, bool packed, bool bluestein, ppf::LongNoiseArgs &a) {
    a = ppf::LongNoiseArgs{};
    a.nbin = nbin; a.n = n; a.packed = packed ? 1 : 0; a.bluestein = bluestein ? 1 : 0;
    int64_t M = 64;
    while (M < (bluestein ? 2 * n - 1 : n)) M *= 2;
    int m = 0;
    while (((int64_t)1 << m) < M) ++m;
    if (m > 24) return false;             // M1, M2 <= 4096 (the block LDS FFT)
    a.M = M; a.log2M = m; a.log2M1 = (m + 1) / 2;
    a.M1 = (int64_t)1 << a.log2M1; a.M2 = M / a.M1;
    return true;
}
bool bluestein_plan(int64_t nbin, int64_t n, bool packed, ppf::LongNoiseArgs &a) {
    return long_len(nbin, n, packed, true, a);
}

// rows per chunk: at most 256 MB of complex work rows (A and Y together), at
// least one row, no more than the call has
int64_t long_chunk_rows(int64_t nrows, size_t row_b) {
    int64_t rc = (int64_t)((size_t)(256u << 20) / (2 * row_b));
    if (rc < 1) rc = 1;
    return nrows < rc ? (nrows > 0 ? nrows : 1) : rc;
}

// A long transform's work area in a workspace: the chirp table (two rows;
// chirp_b: the inverse plan's, ppf_rotate_long), the chunk's work rows A and
// Y, and the rows per chunk
struct LongWork {
    size_t chirp, chirp_b, A, Y;
    int64_t rows;
};
LongWork long_work(Carver &take, int64_t nrows, size_t row_b, size_t chirp_bytes, size_t chirp_b_bytes = 0) {
    LongWork w;
    w.rows = long_chunk_rows(nrows, row_b);
    w.chirp = take(chirp_bytes);
    w.chirp_b = take(chirp_b_bytes);
    w.A = take((size_t)w.rows * row_b);
    w.Y = take((size_t)w.rows * row_b);
    return w;
}

// a plan's twiddle pair (of 2 M1 and 2 M2) and its chirp table at B,
// launched where `chirp` asks for it
struct LongTables {
    const double2 *T1, *T2;
    double2 *B;
};
int long_tables(ppf_ctx *ctx, const ppf::LongNoiseArgs &f, double2 *B, bool chirp, hipStream_t st,
                LongTables &t) {
    const double2 *unused;
    int rc;
    if ((rc = twiddles(ctx, (int)(2 * f.M1), st, &t.T1, &unused))) return rc;
    if ((rc = twiddles(ctx, (int)(2 * f.M2), st, &t.T2, &unused))) return rc;
    t.B = B;
    hipError_t e;
    if (chirp && (e = ppf::launch_chirp_ft(f, B, B + f.M, t.T1, t.T2, st)) != hipSuccess)
        return hip_fail(ctx, e, "k_lf_chirp");
    return PPF_OK;
}

// body(r0, nr) for each chunk of at most rows_c rows, until one fails
template <class F>
int for_chunks(int64_t nrows, int64_t rows_c, F &&body) {
    for (int64_t r0 = 0; r0 < nrows; r0 += rows_c)
        if (int rc = body(r0, nrows - r0 < rows_c ? nrows - r0 : rows_c)) return rc;
    return PPF_OK;
}

struct FitLayout {
    size_t M, X, chan, stats, x0, gP, gw, nuref, Msum, gpart, gwx, gflag, state, partials, active, mom, dphi,
        mres, hcen, Mpow, MP, KC, needx, xslot, xtile, cls, rec, hmlist, nglist, rclist, Bt, total;
    // rows past the LDS transforms (round 6): their rFFTs (data spectra,
    // the long transform's work area)
    int lng;
    size_t spec, gprof, gspec, gsh;
    LongWork lw;
    int nblk, cb, cbd, nblkd;
    int cbx, nblkx;   // the spectrum pass's own channel block (ppf::xspec_own_cb), else cb, nblk
    int fused;    // phase+DM fits on the fused moment pass (k_xmom_g), X only for scattering fits
    int momx;     // wave shapes, PPF_OPT_MOM_X: every fit's moments from X (k_xspec_w + k_moments)
    int xcap;     // X slots
    int tiled;    // momx at 2048 bins: the moment-mode sub-ints' slots are tiled (ppf::xspec_tiled)
    int xnh;      // harmonics per channel of an X slot
};

// 16 moments about each wave's band centre where the moments come from a
// stored X and that was measured to pay (ab_m16_status.txt): the wave
// shapes' MOM_X path and the non-power-of-two nbin, whose moments always
// come from X (round 5's PPF_MOM16_BLOCK: nbin 1000 278-280k -> 293-294k,
// 1536 178-179k -> 183k fits/s in one call).
// Power-of-two nbin off the wave shapes (32-128, 4096, 8192) and block sizes
// the wave kernels refuse keep 32 moments about the global centre (radius
// 4.5 instead of 0.73, so fewer re-centring passes).
static bool mom16_layout(const FitLayout &L, int nbin) {
    return L.momx || (!L.fused && !ppf::is_pow2(ppf::rfft_len(nbin)));
}

// the long-transform plan of the rFFT of real rows of nbin samples (even
// nbin: two samples per complex point)
bool long_row_plan(int64_t nbin, ppf::LongNoiseArgs &f) {
    return bluestein_plan(nbin, (nbin & 1) ? nbin : nbin / 2, !(nbin & 1), f);
}

// fits at nbin past the LDS transforms (even > 8192, odd > 4095): the rows'
// rFFTs on the long transforms, then the X-based fit.  With the GetTOAs
// guess the profile's spectrum (N + 1 harmonics) sits in one workgroup's
// LDS (nbin up to ~19,000); its brute grid too where it fits, else in
// global memory (grid_gsh: ppalign's Ns = nbin)
//
// grid_gsh: whether the FFTFIT brute grid of Ns points leaves the LDS for
// global memory ([rows][Ns + 8] doubles): the spectrum (N + 2 bins), the
// rFFT buffer of the LDS transforms (none for long rows, whose spectra come
// from the long transforms) and the grid past 150 KB.  ppalign at nbin 8192
// (Ns = nbin: 197 KB) and past.
bool grid_gsh(int nbin, int Ns, bool lng) {
    const size_t fb = lng ? 0 : (size_t)ppf::rfft_len(nbin) * sizeof(double2);
    return fb + ((size_t)nbin / 2 + 2) * sizeof(double2) + (size_t)(Ns + 8) * sizeof(double) > 150u * 1024u;
}
bool long_fit_ok(const ppf_fit_desc *d) {
    ppf::LongNoiseArgs f;
    if (d->guess && ((size_t)d->nbin / 2 + 2) * sizeof(double2) > 150u * 1024u) return false;
    return !nbin_supported(d->nbin) && d->nbin > 4095 && long_row_plan(d->nbin, f);
}

FitLayout fit_layout(const ppf_fit_desc *d) {
    FitLayout L{};
    const size_t nharm = (size_t)d->nbin / 2 + 1;
    const size_t nsub = (size_t)d->nsub, nchan = (size_t)d->nchan;
    const size_t nmodel = (size_t)(d->nmodel > 0 ? d->nmodel : 1);
    L.cb = d->nchan < 32 ? d->nchan : 32;
    L.nblk = (d->nchan + L.cb - 1) / L.cb;
    L.fused = ppf::xspec_wave_supported(rfft_log2(d->nbin), L.cb) ? 1 : 0;
    L.cbx = L.cb;
    if (L.fused && ppf::xspec_own_cb(rfft_log2(d->nbin)) > 0) L.cbx = ppf::xspec_own_cb(rfft_log2(d->nbin));
    L.nblkx = (d->nchan + L.cbx - 1) / L.cbx;
    // moments from X: on request, or by default where the GetTOAs guess is
    // fused into the spectrum pass (1024-point rows): there the X pass
    // replaces both the guess pass (k_dsum) and k_xmom_g's re-FFT
    const bool mom_auto = d->guess && rfft_log2(d->nbin) == 10;
    L.momx = (L.fused && !(d->options & PPF_OPT_FUSED_MOM) &&
              ((d->options & PPF_OPT_MOM_X) || mom_auto)) ? 1 : 0;
    L.xcap = (L.fused && d->x_subints > 0 && d->x_subints < d->nsub) ? d->x_subints : d->nsub;
    if (L.fused && (d->options & PPF_OPT_NO_X)) L.xcap = 0;
    if (L.momx) L.xcap = d->nsub;
    L.cbd = d->nchan < 128 ? d->nchan : 128;          // k_dsum channel block
    L.nblkd = (d->nchan + L.cbd - 1) / L.cbd;
    Carver take;
    L.M = take(sizeof(double2) * nmodel * nchan * nharm);
    // tiled slots hold whole tiles of 8 harmonics per channel (1032 at 2048
    // bins); the harmonic-major slots of the same call keep that stride
    L.tiled = (L.momx && ppf::xspec_tiled(rfft_log2(d->nbin))) ? 1 : 0;
    L.xnh = L.tiled ? (int)ppf::xtile_harm((int64_t)nharm) : (int)nharm;
    L.X = take(sizeof(double2) * (size_t)L.xcap * nchan * (size_t)L.xnh);
    L.chan = take(sizeof(double) * nsub * nchan * 4);
    L.stats = take(sizeof(double) * nsub * 2 * nchan * 10);
    L.x0 = take(sizeof(double) * nsub * 8);
    L.state = take(ppf::tr_state_bytes() * nsub);
    L.partials = take(sizeof(double) * nsub * (size_t)ppf::pass_blocks(d->nchan) * 21);
    L.active = take(256);
    L.mom = take(sizeof(double2) * nsub * 2 * nchan * (size_t)ppf::kMoments);
    L.dphi = take(sizeof(double) * nsub * nchan * 2);
    L.mres = take(sizeof(double) * nsub * 2 * nchan);
    L.hcen = take(mom16_layout(L, d->nbin) ? sizeof(double) * nsub * 2 * nchan : 0);
    L.Mpow = take(sizeof(double) * nmodel * nchan);
    L.MP = take(sizeof(double) * nmodel * nchan * nharm);
    L.KC = take(sizeof(int32_t) * nmodel * nchan);
    L.needx = take(nsub);
    L.xslot = take(sizeof(int32_t) * nsub);
    L.xtile = take(L.tiled ? nsub : 0);
    L.cls = take(sizeof(int32_t) * nsub);
    L.rec = take(sizeof(double) * nsub * ppf::kRecN);
    L.hmlist = take(sizeof(int32_t) * nsub);
    L.nglist = take(sizeof(int32_t) * nsub);
    L.rclist = take(sizeof(int32_t) * nsub);
    L.Bt = take(sizeof(double) * (nharm - 1) / 2 * 16);
    if (d->guess) {
        L.gP = take(sizeof(double) * nsub * (size_t)L.nblkd * (size_t)d->nbin);
        L.gw = take(sizeof(double) * nsub * (size_t)L.nblkd * 2);
        L.nuref = take(sizeof(double) * nsub);
        L.Msum = take(sizeof(double2) * nmodel * nharm);
        if (L.fused) {   // guess spectrum fused into k_xspec_w2 (k_classify: gflag)
            const size_t ng = (size_t)ppf::guess_slots(rfft_log2(d->nbin));
            L.gpart = take(sizeof(double2) * nsub * (size_t)L.nblkx * ng);
            L.gwx = take(sizeof(double) * nsub * (size_t)L.nblkx * 3);
            L.gflag = take(nsub);
        }
    }
    L.lng = long_fit_ok(d) ? 1 : 0;
    if (L.lng) {
        ppf::LongNoiseArgs f;
        long_row_plan(d->nbin, f);
        const size_t row_b = (size_t)f.M * sizeof(double2);
        L.spec = take(sizeof(double2) * nsub * nchan * nharm);
        if (d->guess) {
            L.gprof = take(sizeof(double) * nsub * (size_t)d->nbin);
            L.gspec = take(sizeof(double2) * nsub * nharm);
        }
        L.lw = long_work(take, (int64_t)(nsub > nmodel ? nsub : nmodel) * (int64_t)nchan, row_b, 2 * row_b);
    }
    if (d->guess && grid_gsh(d->nbin, d->guess_Ns, L.lng))
        L.gsh = take(sizeof(double) * nsub * ((size_t)d->guess_Ns + 8));
    L.total = take.o;
    return L;
}

// the rFFTs of nrows real rows of nbin samples on the long transforms into
// out[row][k], k <= nbin / 2 (Bluestein; the chirp table once per call)
int long_rfft_rows(ppf_ctx *ctx, const LongWork &w, char *ws, int64_t nbin, int64_t nrows, int dtype,
                   const void *in, double2 *out, bool chirp_ready, hipStream_t st) {
    ppf::LongNoiseArgs f;
    if (!long_row_plan(nbin, f)) return fail(ctx, PPF_EUNSUP, "nbin=%lld", (long long)nbin);
    LongTables t;
    if (int rc = long_tables(ctx, f, (double2 *)(ws + w.chirp), !chirp_ready, st, t)) return rc;
    f.in_dtype = dtype;
    f.in = in;
    return for_chunks(nrows, w.rows, [&](int64_t r0, int64_t nr) {
        f.row0 = r0;
        const hipError_t e = ppf::launch_rfft_long(f, nr, (double2 *)(ws + w.A), (double2 *)(ws + w.Y), t.B, out,
                                                   t.T1, t.T2, st);
        return e == hipSuccess ? PPF_OK : hip_fail(ctx, e, "k_lr_spec");
    });
}

int check_fit_desc(ppf_ctx *ctx, const ppf_fit_desc *d) {
    if (!d) return fail(ctx, PPF_EINVAL, "null descriptor");
    if (d->nsub < 1 || d->nchan < 1) return fail(ctx, PPF_EINVAL, "nsub=%d nchan=%d", d->nsub, d->nchan);
    if (!nbin_supported(d->nbin) && !long_fit_ok(d))
        return fail(ctx, PPF_EUNSUP,
                    "nbin=%d: must be even in [32, 8192] or odd in [33, 4095], or longer without the "
                    "GetTOAs guess (up to 2^23 transform points)", d->nbin);
    if (d->data_dtype != PPF_F32 && d->data_dtype != PPF_F64)
        return fail(ctx, PPF_EINVAL, "data_dtype=%d", d->data_dtype);
    if (d->nmodel < 1) return fail(ctx, PPF_EINVAL, "nmodel=%d", d->nmodel);
    if (!d->data || !d->model || !d->freqs || !d->P || !d->init || !d->fit_flags || !d->nu_fits ||
        !d->nu_outs || !d->results || !d->scales || !d->scale_errs || !d->channel_snrs ||
        !d->covariance)
        return fail(ctx, PPF_EINVAL, "required pointer is NULL");
    if (d->mode != PPF_MODE_FULL && d->mode != PPF_MODE_LEGACY2)
        return fail(ctx, PPF_EINVAL, "mode=%d", d->mode);
    if (d->guess) {
        if (!d->guess_weights || !d->guess_DM) return fail(ctx, PPF_EINVAL, "guess needs weights and DM");
        if (d->guess_Ns < 1 || d->guess_Ns > 65536) return fail(ctx, PPF_EINVAL, "guess_Ns=%d", d->guess_Ns);
    }
    if (!d->workspace) return fail(ctx, PPF_EINVAL, "workspace is NULL");
    FitLayout L = fit_layout(d);
    if (d->workspace_bytes < L.total)
        return fail(ctx, PPF_ENOMEM, "workspace %zu < %zu bytes", d->workspace_bytes, L.total);
    return PPF_OK;
}

// ---- profiling plumbing ----------------------------------------------------
using EvPair = std::pair<hipEvent_t, hipEvent_t>;

// (start, end) pair i of a pool, created on demand; null, with the error in
// *e, where an event cannot be created
EvPair *event_pair(std::vector<EvPair> &v, int i, hipError_t *e) {
    if ((int)v.size() <= i) {
        EvPair pr{};
        if ((*e = hipEventCreate(&pr.first)) != hipSuccess) return nullptr;
        if ((*e = hipEventCreate(&pr.second)) != hipSuccess) {
            (void)hipEventDestroy(pr.first);
            return nullptr;
        }
        v.push_back(pr);
    }
    return &v[i];
}

// ms between two recorded events of one stream, once the later one has passed
int event_ms(ppf_ctx *ctx, hipEvent_t a, hipEvent_t b, double *ms) {
    hipError_t e = hipEventSynchronize(b);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipEventSynchronize");
    float t = 0.f;
    if ((e = hipEventElapsedTime(&t, a, b)) != hipSuccess) return hip_fail(ctx, e, "hipEventElapsedTime");
    *ms = (double)t;
    return PPF_OK;
}

// The ms-history getters' common part: checks the arguments, clamps n to the
// profiled calls the ring still holds and calls entry(c, slot) for history
// entry c = 0..n-1 (oldest first, in ring slot `slot`).  Returns n or an error.
template <class F>
int for_history(ppf_ctx *ctx, int n, const double *ms, F &&entry) {
    if (!ctx || !ms || n < 0) return PPF_EINVAL;
    if (!ctx->prof) return fail(ctx, PPF_EINVAL, "profiling is off");
    const long avail = ctx->ncalls < ppf_ctx::kRing ? ctx->ncalls : ppf_ctx::kRing;
    if (n > avail) n = (int)avail;
    for (int c = 0; c < n; ++c)
        if (int rc = entry(c, (int)((ctx->ncalls - n + c) % ppf_ctx::kRing))) return rc;
    return n;
}

// ---- ppf_fit_batch: what the stages of one call share, then the stages -----
struct FitCall {
    ppf_ctx *ctx;
    const ppf_fit_desc *d;
    hipStream_t st;
    FitLayout L;
    char *ws;
    const double2 *T, *T2;       // twiddles of nbin (long rows: null, no LDS transform runs)
    double2 *Mft;                // [nmodel][nchan][nharm] model spectra
    double *Mpow;
    int nharm, kc;               // harmonics per row, get_noise_PS cut
    int slot;                    // profiling ring slot of the call
    // fused moment pass (k_xmom) only on the wave-FFT shapes; elsewhere the
    // moments are taken from X (k_moments)
    bool fused;
    // the caller expects no streaming fit (C2's pipeline): the launches
    // whose sub-ints are then few or none stride over k_classify's lists
    bool bounded;
    // moment-mode sub-ints (no scattering) on the fused path never need the
    // cross spectrum in HBM: k_xmom_g re-FFTs their rows; k_classify marks
    // the others and gives each an X slot
    uint8_t *needx;
    int32_t *xslot;
    uint8_t *xtile;              // null: no tiled slot
    // fused guess: the sub-ints of k_xspec_w2 whose mean-model cutoff
    // fits its guess harmonics accumulate the guess spectrum there
    uint8_t *gflag;              // null: no fused guess (then gpart, gwx too)
    double2 *gpart;
    double *gwx;
    // the words behind active: [4], [5] k_tr_init's kind counts, [8]
    // k_classify's arrival ticket, [9], [10] its list counts
    unsigned *kinds;
    int32_t *cls;
    double *rec;
    int pf_skip;                 // solve(): the post-fit kernels with nothing to do (ppf::kPfSkip*)

    template <class U>
    U *at(size_t off) const { return (U *)(ws + off); }
    const int32_t *KC() const { return at<const int32_t>(L.KC); }
    unsigned *counts() const { return kinds + 4; }
    void mark(int i) const { if (ctx->prof) (void)hipEventRecord(ctx->ring[slot][i], st); }
    // events around one solver launch (profiling only; where a pair cannot
    // be created the launch goes untimed)
    EvPair *solv_begin(int kind) const {
        hipError_t e;
        EvPair *pe = ctx->prof ? event_pair(ctx->solv_ev[slot], ctx->nsolv[slot], &e) : nullptr;
        if (!pe) return nullptr;
        ctx->solv_kind[slot].resize(ctx->solv_ev[slot].size());
        ctx->solv_kind[slot][ctx->nsolv[slot]++] = kind;
        (void)hipEventRecord(pe->first, st);
        return pe;
    }
    void solv_end(EvPair *pe) const { if (pe) (void)hipEventRecord(pe->second, st); }

    int begin();
    int models(), spectra(), guess();     // stages 0, 1, 2 of ppf_stage_ms_history
    ppf::SolveArgs solve_args() const;
    ppf::XmomArgs xmom_args(const ppf::SolveArgs &sa) const;
    int round(const ppf::SolveArgs &sa, const ppf::XmomArgs &ma, bool any_pass, bool any_mom, bool first);
    int solve(const ppf::SolveArgs &sa), postfit(const ppf::SolveArgs &sa);   // stage 3
};

// the call's layout, twiddles and workspace pointers (ctx, d, st are set);
// opens its profiling slot
int FitCall::begin() {
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    L = fit_layout(d);
    int rc;
    if (!L.lng && (rc = twiddles(ctx, d->nbin, st, &T, &T2))) return rc;
    ws = (char *)d->workspace;
    Mft = at<double2>(L.M); Mpow = at<double>(L.Mpow);
    nharm = d->nbin / 2 + 1; kc = noise_kc(nharm, 4);
    fused = L.fused && !L.momx;
    bounded = (d->options & PPF_OPT_NO_X) != 0;
    needx = at<uint8_t>(L.needx); xslot = at<int32_t>(L.xslot);
    xtile = L.tiled ? at<uint8_t>(L.xtile) : nullptr;
    if (d->guess && L.fused && ppf::xspec_guess_fused_n(rfft_log2(d->nbin))) {
        gflag = at<uint8_t>(L.gflag); gpart = at<double2>(L.gpart); gwx = at<double>(L.gwx);
    }
    kinds = at<unsigned>(L.active + 16); cls = at<int32_t>(L.cls); rec = at<double>(L.rec);
    slot = (int)(ctx->ncalls % ppf_ctx::kRing);
    for (int i = 0; i < 4; ++i) ctx->ran[slot][i] = true;
    ctx->npass[slot] = ctx->nsolv[slot] = 0;
    ctx->ran[slot][2] = d->guess != 0;
    ctx->ran[slot][4] = ctx->ran[slot][5] = false;
    return PPF_OK;
}

// stage 0: model spectra, their power and harmonic cutoffs; k_classify
int FitCall::models() {
    hipError_t e;
    if (L.lng) {
        if (int rc = long_rfft_rows(ctx, L.lw, ws, d->nbin, (int64_t)d->nmodel * d->nchan, PPF_F64, d->model, Mft,
                                    false, st))
            return rc;
    } else {
        ppf::RfftArgs ra{d->nbin, rfft_log2(d->nbin), PPF_F64, d->model, T, T2, Mft};
        if ((e = ppf::launch_rfft_rows(ra, (int64_t)d->nmodel * d->nchan, st)) != hipSuccess)
            return hip_fail(ctx, e, "k_rfft_rows");
    }
    if ((e = ppf::launch_model_pow_t(Mft, d->nchan, nharm, d->nmodel, at<double>(L.MP), st)) != hipSuccess)
        return hip_fail(ctx, e, "k_model_pow_t");
    if ((e = ppf::launch_model_cut(at<const double>(L.MP), d->nchan, nharm, d->nmodel,
                                   (d->options & PPF_OPT_NO_HCUT) != 0, at<int32_t>(L.KC), st)) != hipSuccess)
        return hip_fail(ctx, e, "k_model_cut");
    if ((e = ppf::launch_model_pow(Mft, d->nchan, nharm, d->nmodel, Mpow, st)) != hipSuccess)
        return hip_fail(ctx, e, "k_model_pow");
    if ((e = hipMemsetAsync(kinds, 0, 8 * sizeof(unsigned), st)) != hipSuccess)
        return hip_fail(ctx, e, "hipMemsetAsync");
    ppf::ClassifyArgs ca{};
    ca.nsub = d->nsub; ca.nchan = d->nchan; ca.log10_tau = d->log10_tau;
    ca.fused = fused ? 1 : 0; ca.xcap = L.xcap;
    ca.fit_flags = d->fit_flags; ca.init = d->init; ca.freqs = d->freqs; ca.P = d->P;
    ca.nu_fits = d->nu_fits; ca.mask = d->chan_mask; ca.model_index = d->model_index;
    ca.KC = KC(); ca.klim = gflag ? 64 * ppf::guess_npl(rfft_log2(d->nbin)) : -1;
    ca.guess_DM = d->guess ? d->guess_DM : nullptr; ca.guess_ref = d->guess ? d->guess_ref : 0;
    ca.needx = needx; ca.xslot = xslot; ca.xtile = xtile; ca.gflag = gflag; ca.cls = cls; ca.rec = rec;
    ca.hm_list = at<int32_t>(L.hmlist); ca.ng_list = at<int32_t>(L.nglist); ca.counts = counts();
    if ((e = ppf::launch_classify(ca, st)) != hipSuccess) return hip_fail(ctx, e, "k_classify");
    return PPF_OK;
}

// stage 1: the spectrum pass (wave, long-row or block FFT): the per-channel
// terms and the cross spectra of the sub-ints that need them
int FitCall::spectra() {
    hipError_t e;
    ppf::XspecArgs xa{};
    xa.nsub = d->nsub; xa.nchan = d->nchan; xa.nbin = d->nbin; xa.log2N = rfft_log2(d->nbin);
    xa.kc = kc; xa.nblk = L.nblkx; xa.cb = L.cbx; xa.dtype = d->data_dtype;
    // k_xspec_w: channel-block-major (mode 2) when the model spectra
    // outgrow the L2s, sub-int-major otherwise; k_xmom_g stages its model
    // row in LDS per workgroup and keeps mode 1 (xmom_args)
    constexpr long long kOrder2Bytes = 32ll << 20;
    const long long model_bytes = (long long)d->nchan * (d->nbin / 2 + 1) * 16;
    const int xcdx = (L.nblkx % 8 == 0) ? 1 : 0;
    xa.xcd_swizzle = (xcdx && model_bytes > kOrder2Bytes) ? 2 : xcdx;
    xa.data = d->data; xa.Mft = Mft; xa.model_index = d->model_index; xa.mask = d->chan_mask;
    xa.errs = d->errs; xa.freqs = d->freqs; xa.P = d->P; xa.T = T; xa.T2 = T2;
    xa.X = at<double2>(L.X); xa.chan = at<double>(L.chan);
    xa.Mpow = Mpow; xa.xslot = xslot; xa.xtile = xtile; xa.xnh = L.xnh;
    xa.gflag = gflag; xa.cls = cls; xa.rec = rec;
    if (bounded && xtile) {
        xa.list = at<int32_t>(L.hmlist);
        xa.nlist = counts() + 1;
    }
    if (gflag) {
        xa.gpart = gpart; xa.gw = gwx; xa.guess_weights = d->guess_weights;
        xa.guess_DM = d->guess_DM; xa.nu_fits = d->nu_fits; xa.guess_ref = d->guess_ref;
    }
    const bool wave = L.fused != 0;
    xa.needx = (fused || L.momx) ? needx : nullptr;
    // fused: only k_pass reads X, and only below its channels' cutoffs;
    // momx: k_moments reads it below the same cutoffs
    // block-FFT path: only k_xspec_wm (the smooth non-power-of-two lengths)
    // uses it, writing X below the same cutoffs its readers stop at
    xa.KC = (fused || L.momx || !wave) ? KC() : nullptr;
    if (wave) {
        // (nothing to do when the caller has ruled out X: every sub-int is
        // fitted from k_xmom_g's moments)
        if (!(fused && L.xcap == 0) && (e = ppf::launch_xspec_wave(xa, st)) != hipSuccess)
            return hip_fail(ctx, e, "k_xspec_w");
    } else if (L.lng) {
        double2 *spec = at<double2>(L.spec);
        if (int rc = long_rfft_rows(ctx, L.lw, ws, d->nbin, (int64_t)d->nsub * d->nchan, d->data_dtype, d->data,
                                    spec, true, st))
            return rc;
        xa.spec = spec;
        if ((e = ppf::launch_xspec_spec(xa, st)) != hipSuccess) return hip_fail(ctx, e, "k_xspec_spec");
    } else {
        if ((e = ppf::launch_xspec(xa, st)) != hipSuccess) return hip_fail(ctx, e, "k_xspec");
    }
    return PPF_OK;
}

// stage 2: the GetTOAs guess.  Guess profile: time-domain dedispersion
// (k_dsum), then FFTFIT against the mean model (k_guess)
int FitCall::guess() {
    hipError_t e;
    int rc;
    ppf::DsumArgs da{};
    da.nsub = d->nsub; da.nchan = d->nchan; da.nbin = d->nbin; da.dtype = d->data_dtype;
    da.cbd = L.cbd; da.nblkd = L.nblkd; da.data = d->data; da.mask = d->chan_mask;
    da.freqs = d->freqs; da.P = d->P; da.guess_DM = d->guess_DM; da.guess_weights = d->guess_weights;
    da.guess_ref = d->guess_ref; da.nu_fits = d->nu_fits;
    da.gP = at<double>(L.gP); da.gw = at<double>(L.gw); da.nuref = at<double>(L.nuref);
    da.gflag = gflag;
    if (bounded && gflag) {
        da.list = at<int32_t>(L.nglist);
        da.nlist = counts() + 2;
    }
    mark(7);
    if ((e = ppf::launch_dsum(da, st)) != hipSuccess) return hip_fail(ctx, e, "k_dsum");
    mark(8);
    ctx->ran[slot][5] = true;
    double2 *msum = at<double2>(L.Msum);
    if ((e = ppf::launch_model_sum(Mft, d->nchan, nharm, d->nmodel, msum, st)) != hipSuccess)
        return hip_fail(ctx, e, "k_model_sum");
    ppf::GuessArgs ga{};
    ga.nsub = d->nsub; ga.nchan = d->nchan; ga.nbin = d->nbin; ga.log2N = rfft_log2(d->nbin);
    ga.kc = kc; ga.nblkd = L.nblkd; ga.Ns = d->guess_Ns; ga.mask = d->chan_mask; ga.guess_ref = d->guess_ref;
    ga.freqs = d->freqs; ga.P = d->P; ga.guess_DM = d->guess_DM; ga.guess_tau = d->guess_tau;
    ga.nu_fits = d->nu_fits; ga.gP = da.gP; ga.gw = da.gw; ga.T = T; ga.T2 = T2;
    ga.KC = KC(); ga.x0 = at<double>(L.x0); ga.Msum = msum; ga.Mft = Mft; ga.model_index = d->model_index;
    ga.gflag = gflag; ga.gpart = gpart; ga.gwx = gwx; ga.nblk = L.nblkx;
    if (L.lng) {
        // the profiles' rFFTs on the long transforms (same plan as the rows)
        double *prof = at<double>(L.gprof);
        double2 *gspec = at<double2>(L.gspec);
        if ((e = ppf::launch_gsum(d->nsub, L.nblkd, d->nbin, da.gP, prof, st)) != hipSuccess)
            return hip_fail(ctx, e, "k_gsum");
        if ((rc = long_rfft_rows(ctx, L.lw, ws, d->nbin, d->nsub, PPF_F64, prof, gspec, true, st))) return rc;
        ga.gspec = gspec;
    }
    if (grid_gsh(d->nbin, ga.Ns, L.lng)) ga.gsh = at<double>(L.gsh);
    ppf::CzPlan cz{};
    if (cz_plan(ga.Ns, d->nbin / 2 + 1, cz)) {
        if ((rc = cz_tables(ctx, cz, st, &ga.czB, &ga.czT))) return rc;
        ga.czP = cz.P; ga.czJ = cz.J; ga.czQ = cz.Q; ga.czK = cz.K;
    }
    if ((e = ppf::launch_guess(ga, st)) != hipSuccess) return hip_fail(ctx, e, "k_guess");
    return PPF_OK;
}

// the solver kernels' argument block (k_tr_init .. k_postfit)
ppf::SolveArgs FitCall::solve_args() const {
    ppf::SolveArgs sa{};
    sa.nsub = d->nsub; sa.nchan = d->nchan; sa.nbin = d->nbin;
    sa.X = at<double2>(L.X); sa.Mft = Mft; sa.model_index = d->model_index; sa.chan = at<double>(L.chan);
    sa.MP = at<const double>(L.MP); sa.KC = KC();
    sa.freqs = d->freqs; sa.P = d->P; sa.mask = d->chan_mask; sa.init = d->init;
    sa.fit_flags = d->fit_flags; sa.nu_fits = d->nu_fits; sa.nu_outs = d->nu_outs; sa.bounds = d->bounds;
    sa.log10_tau = d->log10_tau; sa.option = d->option; sa.is_toa = d->is_toa; sa.mode = d->mode;
    sa.max_iter = d->max_iter; sa.guess = d->guess; sa.x0 = at<double>(L.x0);
    sa.newton = (d->options & PPF_OPT_SCIPY_TR) ? 0 : 1;
    sa.stats = at<double>(L.stats); sa.results = d->results; sa.scales = d->scales;
    sa.scale_errs = d->scale_errs; sa.channel_snrs = d->channel_snrs; sa.covariance = d->covariance;
    sa.state = at<ppf::TRState>(L.state); sa.partials = at<double>(L.partials);
    sa.active = at<unsigned>(L.active);
    sa.rc_count = sa.active + 1;             // reset together with active
    sa.rc_list = at<int32_t>(L.rclist); sa.kinds = kinds; sa.rec = rec;
    sa.mom = at<double2>(L.mom); sa.dphi = at<double>(L.dphi); sa.mres = at<double>(L.mres);
    // 16 moments about each wave's band centre (mom16_layout)
    const bool m16 = mom16_layout(L, d->nbin);
    sa.mom16 = m16;
    sa.hcen = m16 ? at<double>(L.hcen) : nullptr;
    sa.xslot = xslot; sa.xtile = xtile; sa.xnh = L.xnh;
    return sa;
}

// the fused moment pass's argument block (k_xmom_g: its model row staged in
// LDS per workgroup, so sub-int-major order whatever the model size)
ppf::XmomArgs FitCall::xmom_args(const ppf::SolveArgs &sa) const {
    ppf::XmomArgs ma{};
    ma.nsub = d->nsub; ma.nchan = d->nchan; ma.nbin = d->nbin; ma.log2N = rfft_log2(d->nbin);
    ma.nblk = L.nblk; ma.cb = L.cb; ma.dtype = d->data_dtype; ma.xcd_swizzle = (L.nblk % 8 == 0) ? 1 : 0;
    ma.data = d->data; ma.Mft = Mft; ma.model_index = d->model_index; ma.mask = d->chan_mask;
    ma.chan = at<double>(L.chan); ma.dphi = sa.dphi; ma.T = T; ma.T2 = T2; ma.state = sa.state;
    ma.mom = (double *)sa.mom; ma.Bt = at<const double>(L.Bt);
    ma.kc = kc; ma.errs = d->errs; ma.Mpow = Mpow; ma.mres = sa.mres; ma.nmodel = d->nmodel;
    ma.rc_count = sa.rc_count; ma.rc_list = sa.rc_list; ma.KC = KC();
    return ma;
}

// re-centring passes: usually few sub-ints, so 8-channel blocks (4x the
// workgroups, a quarter of the rounds each) keep more CUs busy; a channel's
// moments do not depend on its block
ppf::XmomArgs recentre_args(ppf::XmomArgs mr) {
    if (mr.cb > 8) {
        mr.cb = 8;
        mr.nblk = (mr.nchan + 7) / 8;
        mr.xcd_swizzle = (mr.nblk % 8 == 0) ? 1 : 0;
    }
    return mr;
}

// One round of the iteration loop: for the streaming fits (any_pass) k_pass
// and k_tr_step, for the moment fits (any_mom) the (re)centring moment pass
// and k_tr_mom.  first: the call's first round, whose moment pass is the
// full one.
int FitCall::round(const ppf::SolveArgs &sa, const ppf::XmomArgs &ma, bool any_pass, bool any_mom, bool first) {
    hipError_t e;
    if (any_pass) {
        EvPair *pe = nullptr;
        if (ctx->prof) {
            if (!(pe = event_pair(ctx->pass_ev[slot], ctx->npass[slot], &e)))
                return hip_fail(ctx, e, "hipEventCreate");
            ++ctx->npass[slot];
            (void)hipEventRecord(pe->first, st);
        }
        if ((e = ppf::launch_pass(sa, st)) != hipSuccess) return hip_fail(ctx, e, "k_pass");
        if (pe) (void)hipEventRecord(pe->second, st);
    }
    if (any_mom) {
        if (first) mark(5);
        if (!fused) e = ppf::launch_moments(sa, st);
        else e = first ? ppf::launch_xmom(ma, true, st) : ppf::launch_xmom(recentre_args(ma), false, st);
        if (e != hipSuccess) return hip_fail(ctx, e, fused ? "k_xmom" : "k_moments");
        if (first) {
            mark(6);
            ctx->ran[slot][4] = true;
        }
    }
    if ((e = hipMemsetAsync(sa.active, 0, 2 * sizeof(unsigned), st)) != hipSuccess)
        return hip_fail(ctx, e, "hipMemsetAsync");
    if (any_pass) {
        EvPair *pe = solv_begin(1);
        if ((e = ppf::launch_tr_step(sa, st)) != hipSuccess) return hip_fail(ctx, e, "k_tr_step");
        solv_end(pe);
    }
    if (any_mom) {
        EvPair *pe = solv_begin(0);
        if ((e = ppf::launch_tr_mom(sa, st)) != hipSuccess) return hip_fail(ctx, e, "k_tr_mom");
        solv_end(pe);
    }
    return PPF_OK;
}

// stage 3: k_tr_init and the trust-region iterations
int FitCall::solve(const ppf::SolveArgs &sa) {
    hipError_t e;
    int rc;
    if (!ctx->host_active && (e = hipHostMalloc((void **)&ctx->host_active, 4 * sizeof(unsigned))) != hipSuccess)
        return hip_fail(ctx, e, "hipHostMalloc");
    if ((e = ppf::launch_tr_init(sa, st)) != hipSuccess) return hip_fail(ctx, e, "k_tr_init");
    // how many fits iterate on the moments and how many on streaming passes:
    // the iteration loop launches only the kernels some fit needs.  Where
    // PPF_OPT_NO_X took effect (fit_layout: the fused path without moments
    // from X, xcap == 0) no X slot exists, a sub-int that would stream has
    // ended with PPF_ST_NOSPACE in k_tr_init and every other fit is a
    // moment fit, so the answer is known without the read-back and its
    // stream synchronisation (round 6: one host round trip less per call, a
    // few percent of a ppalign iteration); the moment kernels of a batch
    // with nothing left to fit exit at once.  Everywhere else (block-FFT and
    // long rows, moments from X) the option reserves nothing less and every
    // streaming sub-int holds a valid slot, so the counts decide.  Without
    // the option they are read here.  With it (the C2 pipeline: moments from
    // X at 2048 bins) the caller expects no streaming fit, and the counts
    // ride along with the first read-back of the iteration loop instead
    // (kinds_late): no round trip of their own, and a streaming sub-int that
    // is there after all gets its k_pass from the second group on -- a
    // sub-int's iterations do not depend on the round they start in
    const bool spin = (d->options & PPF_OPT_SPIN_WAIT) != 0;
    const bool no_stream = L.fused && L.xcap == 0;
    bool kinds_late = !no_stream && bounded;
    bool any_mom = true, any_pass = false;
    if (!no_stream && !kinds_late) {
        if ((rc = read_back(ctx, ctx->host_active + 1, sa.kinds, 2, st, spin))) return rc;
        any_mom = ctx->host_active[1] != 0;
        any_pass = ctx->host_active[2] != 0;
    }
    const ppf::XmomArgs ma = xmom_args(sa);
    if (fused && (e = ppf::launch_btab(d->nbin / 2, at<double>(L.Bt), st)) != hipSuccess)
        return hip_fail(ctx, e, "k_btab");
    // trust-region iterations.  Scattering fits: each iteration = one
    // streaming pass (k_pass) + one step (k_tr_step).  Other fits: k_moments
    // (re)centres the moment sets of the sub-ints that asked, k_tr_mom runs
    // iterations until the fit stops or leaves the expansion radius.  Groups
    // of rounds are queued without host synchronisation; the count of
    // sub-ints still needing work is read back between groups.
    const int maxiter = d->max_iter > 0 ? d->max_iter : 200 * 5;
    int iter = 0;
    // Moment-only batches read the counter after the first round: most
    // phase+DM fits finish inside it (C2: 1.0 data passes per fit), so the
    // empty re-centring launches that a longer first group would queue
    // are not worth the one synchronisation they save.
    for (int group = any_pass ? 3 : 1; any_mom || any_pass; group = 2) {
        for (int g = 0; g < group; ++g)
            if ((rc = round(sa, ma, any_pass, any_mom, iter == 0 && g == 0))) return rc;
        iter += group;
        // (the same stream, in order: the counts have landed when the
        // read-back behind them has)
        if (kinds_late && (e = hipMemcpyAsync(ctx->host_active + 1, sa.kinds, 2 * sizeof(unsigned),
                                              hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(ctx, e, "hipMemcpyAsync");
        if ((rc = read_back(ctx, ctx->host_active, sa.active, 1, st, spin))) return rc;
        if (kinds_late) {
            kinds_late = false;
            if (ctx->host_active[2] != 0) {
                any_pass = true;      // fits still in PH_INIT: not counted in active yet
                continue;
            }
        }
        if (*ctx->host_active == 0 || iter > maxiter + 2) break;
    }
    // the post-fit kernels to launch: without a streaming fit every fitted
    // sub-int is a moment fit (k_postfit_mom alone); without a moment fit,
    // where the counts say so, k_postfit alone
    pf_skip = !any_pass ? ppf::kPfSkipFull : (!any_mom ? ppf::kPfSkipMom : 0);
    return PPF_OK;
}

// stage 3's end: the output transform, covariances, scales and chi2
int FitCall::postfit(const ppf::SolveArgs &sa) {
    EvPair *pe = solv_begin(2);
    ppf::SolveArgs pa = sa;
    pa.pf_skip = pf_skip;
    const hipError_t e = ppf::launch_postfit(pa, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "k_postfit");
    solv_end(pe);
    return PPF_OK;
}

}  // namespace

extern "C" {

int ppf_abi_version(void) { return PPF_ABI_VERSION; }
size_t ppf_sizeof_fit_desc(void) { return sizeof(ppf_fit_desc); }
size_t ppf_sizeof_result(void) { return sizeof(ppf_result); }

int ppf_create(int device, ppf_ctx **out) {
    if (!out) return PPF_EINVAL;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return PPF_EHIP;
    if (device < 0 || device >= n) return PPF_EINVAL;
    ppf_ctx *c = new ppf_ctx();
    c->device = device;
    *out = c;
    return PPF_OK;
}

void ppf_destroy(ppf_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (auto &kv : ctx->tw) (void)hipFree(kv.second);
    for (auto &kv : ctx->cz) (void)hipFree(kv.second);
    for (auto &set : ctx->ring)
        for (auto &e : set)
            if (e) (void)hipEventDestroy(e);
    for (auto &v : ctx->pass_ev)
        for (auto &pr : v) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (auto &v : ctx->solv_ev)
        for (auto &pr : v) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    if (ctx->host_active) (void)hipHostFree(ctx->host_active);
    if (ctx->lscr) (void)hipFree(ctx->lscr);
    delete ctx;
}

int ppf_set_profiling(ppf_ctx *ctx, int enable) {
    if (!ctx) return PPF_EINVAL;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    if (enable && !ctx->ring[0][0])
        for (auto &set : ctx->ring)
            for (auto &ev : set)
                if ((e = hipEventCreate(&ev)) != hipSuccess) return hip_fail(ctx, e, "hipEventCreate");
    ctx->prof = enable != 0;
    ctx->ncalls = 0;
    return PPF_OK;
}

int ppf_stage_ms_history(ppf_ctx *ctx, int n, double *ms) {
    return for_history(ctx, n, ms, [&](int c, int slot) -> int {
        for (int i = 0; i < 4; ++i) {
            ms[c * 4 + i] = 0.0;
            if (!ctx->ran[slot][i]) continue;
            if (int rc = event_ms(ctx, ctx->ring[slot][i], ctx->ring[slot][i + 1], &ms[c * 4 + i])) return rc;
        }
        return PPF_OK;
    });
}

int ppf_kernel_ms_history(ppf_ctx *ctx, int n, double *ms) {
    return for_history(ctx, n, ms, [&](int c, int slot) -> int {
        for (int i = 0; i < 2; ++i) {
            ms[c * 2 + i] = 0.0;
            if (!ctx->ran[slot][4 + i]) continue;
            if (int rc = event_ms(ctx, ctx->ring[slot][5 + 2 * i], ctx->ring[slot][6 + 2 * i], &ms[c * 2 + i]))
                return rc;
        }
        return PPF_OK;
    });
}

int ppf_pass_ms_history(ppf_ctx *ctx, int n, double *ms) {
    return for_history(ctx, n, ms, [&](int c, int slot) -> int {
        double tot = 0.0, t;
        for (int i = 0; i < ctx->npass[slot]; ++i) {
            const EvPair &pr = ctx->pass_ev[slot][i];
            if (int rc = event_ms(ctx, pr.first, pr.second, &t)) return rc;
            tot += t;
        }
        ms[c * 2 + 0] = tot;
        ms[c * 2 + 1] = (double)ctx->npass[slot];
        return PPF_OK;
    });
}

int ppf_solver_ms_history(ppf_ctx *ctx, int n, double *ms) {
    return for_history(ctx, n, ms, [&](int c, int slot) -> int {
        double *o = ms + c * 6, t;
        for (int i = 0; i < 6; ++i) o[i] = 0.0;
        for (int i = 0; i < ctx->nsolv[slot]; ++i) {
            const EvPair &pr = ctx->solv_ev[slot][i];
            if (int rc = event_ms(ctx, pr.first, pr.second, &t)) return rc;
            const int k = ctx->solv_kind[slot][i];
            o[2 * k] += t;
            o[2 * k + 1] += 1.0;
        }
        return PPF_OK;
    });
}

int ppf_last_stage_ms(ppf_ctx *ctx, double *ms4) {
    int n = ppf_stage_ms_history(ctx, 1, ms4);
    if (n < 0) return n;
    return n == 1 ? PPF_OK : fail(ctx, PPF_EINVAL, "no profiled call yet");
}

const char *ppf_last_error(const ppf_ctx *ctx) {
    if (!ctx) return "null context";
    // a copy per calling thread: another thread's failure cannot rewrite the
    // buffer this pointer refers to
    thread_local std::string copy;
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    copy = ctx->err;
    return copy.c_str();
}

size_t ppf_fit_workspace_bytes(const ppf_fit_desc *desc) {
    if (!desc || desc->nsub < 1 || desc->nchan < 1 || (!nbin_supported(desc->nbin) && !long_fit_ok(desc)))
        return 0;
    return fit_layout(desc).total;
}

int ppf_fit_batch(ppf_ctx *ctx, const ppf_fit_desc *d, void *stream) {
    if (!ctx) return PPF_EINVAL;
    int rc = check_fit_desc(ctx, d);
    if (rc) return rc;
    FitCall c{};
    c.ctx = ctx; c.d = d; c.st = (hipStream_t)stream;
    if ((rc = c.begin())) return rc;
    c.mark(0);
    if ((rc = c.models())) return rc;
    c.mark(1);
    if ((rc = c.spectra())) return rc;
    c.mark(2);
    if (d->guess && (rc = c.guess())) return rc;
    c.mark(3);
    const ppf::SolveArgs sa = c.solve_args();
    if ((rc = c.solve(sa))) return rc;
    if ((rc = c.postfit(sa))) return rc;
    c.mark(4);
    if (ctx->prof) ++ctx->ncalls;
    return PPF_OK;
}

int ppf_fit2_batch(ppf_ctx *ctx, const ppf_fit_desc *desc, void *stream) {
    if (!desc) return fail(ctx, PPF_EINVAL, "null descriptor");
    ppf_fit_desc d = *desc;
    d.mode = PPF_MODE_LEGACY2;
    return ppf_fit_batch(ctx, &d, stream);
}

static int rotate_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype, const void *in,
                        const double *phases, double *out, void *stream, bool ref_len) {
    if (!ctx) return PPF_EINVAL;
    if (!nbin_supported(nbin)) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nrows < 0 || (nrows > 0 && (!in || !phases || !out)))
        return fail(ctx, PPF_EINVAL, "bad rotate arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    if (nrows == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    ppf::RotateArgs a{nbin, rfft_log2(nbin), in_dtype, in, phases, T, T2, out, 0, T, T2};
    if (ref_len && (nbin & 1)) {
        a.ref_len = 1;
        if ((rc = twiddles(ctx, nbin - 1, st, &a.Te, &a.T2e))) return rc;
    }
    if ((e = ppf::launch_rotate(a, nrows, st)) != hipSuccess) return hip_fail(ctx, e, "k_rotate");
    return PPF_OK;
}

int ppf_rotate_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype, const void *in,
                     const double *phases, double *out, void *stream) {
    return rotate_batch(ctx, nrows, nbin, in_dtype, in, phases, out, stream, false);
}

int ppf_rotate_batch_ref(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype, const void *in,
                         const double *phases, double *out, void *stream) {
    return rotate_batch(ctx, nrows, nbin, in_dtype, in, phases, out, stream, true);
}

int ppf_inst_response_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, const double *src,
                            const int32_t *src_row, const double *table, const double *widths,
                            double *out, void *stream) {
    if (!ctx) return PPF_EINVAL;
    // the block LDS transform of even rows only: odd nbin (the reference's
    // length-less irfft gives nbin - 1 bins there) and long rows are refused
    if ((nbin & 1) || !nbin_supported(nbin))
        return fail(ctx, PPF_EUNSUP, "instrumental response: nbin=%d unsupported (even, 32..8192)", nbin);
    if (nrows < 0 || nrows > 0x7fffffff || (nrows > 0 && (!src || !src_row || !widths || !out)))
        return fail(ctx, PPF_EINVAL, "bad instrumental response arguments");
    if (nrows == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    ppf::InstRespArgs a{nbin, src, src_row, table, widths, T, T2, out};
    if ((e = ppf::launch_inst_resp(a, nrows, st)) != hipSuccess) return hip_fail(ctx, e, "k_inst_resp");
    return PPF_OK;
}

size_t ppf_align_workspace_bytes(int32_t nsub, int32_t nchan, int32_t nbin) {
    if (nsub <= 0 || nchan <= 0 || nbin <= 0) return 0;
    const size_t g = (size_t)ppf::align_groups(nsub, nchan);
    return align256(g * nchan * (size_t)(nbin / 2 + 1) * sizeof(double2)) +
           align256(g * nchan * sizeof(double));
}

int ppf_align_phases(ppf_ctx *ctx, int32_t nsub, int32_t nchan, const double *results, const double *freqs,
                     const double *P, const uint8_t *mask, const double *scales, const double *errs,
                     double *phases, double *weights, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nsub < 0 || nchan <= 0) return fail(ctx, PPF_EINVAL, "bad align shape");
    if (nsub == 0) return PPF_OK;
    if (!results || !freqs || !P || !scales || !errs || !phases || !weights)
        return fail(ctx, PPF_EINVAL, "null align_phases argument");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    if ((e = ppf::launch_align_phases(nsub, nchan, results, freqs, P, mask, scales, errs, phases, weights,
                                      (hipStream_t)stream)) != hipSuccess)
        return hip_fail(ctx, e, "k_align_phases");
    return PPF_OK;
}

int ppf_align_accum(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nbin, int32_t in_dtype,
                    const void *in, const double *phases, const double *weights, double *out,
                    double *wsum, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (!nbin_supported(nbin)) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nsub < 0 || nchan <= 0) return fail(ctx, PPF_EINVAL, "bad align shape");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    if (nsub == 0) return PPF_OK;
    if (!in || !phases || !weights || !out || !wsum || !workspace)
        return fail(ctx, PPF_EINVAL, "null align argument");
    const size_t need = ppf_align_workspace_bytes(nsub, nchan, nbin);
    if (workspace_bytes < need)
        return fail(ctx, PPF_ENOMEM, "align workspace %zu < %zu bytes", workspace_bytes, need);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    ppf::AlignArgs a{};
    a.nsub = nsub; a.nchan = nchan; a.nbin = nbin; a.log2N = rfft_log2(nbin); a.dtype = in_dtype;
    a.ngroup = ppf::align_groups(nsub, nchan);
    a.in = in; a.phases = phases; a.weights = weights; a.T = T; a.T2 = T2;
    char *ws = (char *)workspace;
    a.part = (double2 *)ws;
    a.wpart = (double *)(ws + align256((size_t)a.ngroup * nchan * (size_t)(nbin / 2 + 1) *
                                        sizeof(double2)));
    a.out = out; a.wsum = wsum;
    if ((e = ppf::launch_align(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_align");
    return PPF_OK;
}

int ppf_resid_chi2_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype,
                         const void *in, const double *phases, const double *model,
                         const int32_t *model_row, const double *scales, const double *errs,
                         double dof, double *out, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (!nbin_supported(nbin)) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nrows < 0 || (nrows > 0 && (!in || !phases || !model || !model_row || !scales || !errs ||
                                    !out)))
        return fail(ctx, PPF_EINVAL, "bad resid_chi2 arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    if (nrows == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    ppf::ResidArgs a{nbin, rfft_log2(nbin), in_dtype, in, phases, model, model_row, scales, errs,
                     dof, T, T2, out};
    if ((e = ppf::launch_resid_chi2(a, nrows, st)) != hipSuccess) return hip_fail(ctx, e, "k_resid_chi2");
    return PPF_OK;
}

int ppf_noise_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype, const void *in,
                    int32_t frac, double *out, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (!nbin_supported(nbin)) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nrows < 0 || frac < 1 || (nrows > 0 && (!in || !out)))
        return fail(ctx, PPF_EINVAL, "bad noise arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    if (nrows == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    ppf::NoiseArgs a{nbin, rfft_log2(nbin), in_dtype, noise_kc(nbin / 2 + 1, frac), in, T, T2, out};
    if (ppf::noise_wave_supported(a.log2N)) {
        if ((e = ppf::launch_noise_wave(a, nrows, st)) != hipSuccess) return hip_fail(ctx, e, "k_noise_w");
    } else if ((e = ppf::launch_noise(a, nrows, st)) != hipSuccess) {
        return hip_fail(ctx, e, "k_noise");
    }
    return PPF_OK;
}

// ppf_noise_long's plan and workspace (ppf_longfft.hip): rows in chunks of
// at most 256 MB of complex work buffers
namespace {
struct LongPlan {
    ppf::LongNoiseArgs a;
    LongWork w;
    size_t off_part, bytes;
};
bool long_plan(int64_t nrows, int64_t nbin, int frac, LongPlan &p) {
    if (nrows < 0 || nbin < 1 || frac < 1) return false;
    ppf::LongNoiseArgs &a = p.a;
    const bool packed = nbin % 2 == 0;
    const int64_t n = packed ? nbin / 2 : nbin;
    const bool pow2 = (n & (n - 1)) == 0;
    if (!long_len(nbin, n, packed, !(pow2 && n >= 64), a)) return false;
    a.nharm = nbin / 2 + 1;
    a.kc = (int64_t)((1.0 - std::pow((double)frac, -1.0)) * (double)a.nharm);
    const size_t row_b = (size_t)a.M * sizeof(double2);
    Carver take;
    p.w = long_work(take, nrows, row_b, a.bluestein ? 2 * row_b : 0);
    p.off_part = take((size_t)p.w.rows * 256 * sizeof(double));
    p.bytes = take.o;
    return true;
}
}  // namespace

size_t ppf_noise_long_workspace_bytes(int64_t nrows, int64_t nbin) {
    LongPlan p;
    return long_plan(nrows, nbin, 4, p) ? p.bytes : 0;
}

int ppf_noise_long(ppf_ctx *ctx, int64_t nrows, int64_t nbin, int32_t in_dtype, const void *in,
                   int32_t frac, double *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nrows < 0 || nbin < 1 || frac < 1 || (nrows > 0 && (!in || !out)))
        return fail(ctx, PPF_EINVAL, "bad noise arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    LongPlan p;
    if (!long_plan(nrows, nbin, frac, p))
        return fail(ctx, PPF_EUNSUP, "nbin=%lld: transform longer than 2^24 points", (long long)nbin);
    if (nrows == 0) return PPF_OK;
    if (!workspace || workspace_bytes < p.bytes)
        return fail(ctx, PPF_EINVAL, "workspace %zu < %zu bytes", workspace_bytes, p.bytes);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    LongTables t;
    if (int rc = long_tables(ctx, p.a, (double2 *)(ws + p.w.chirp), p.a.bluestein, st, t)) return rc;
    p.a.in_dtype = in_dtype;
    p.a.in = in;
    return for_chunks(nrows, p.w.rows, [&](int64_t r0, int64_t nr) {
        p.a.row0 = r0;
        const hipError_t el = ppf::launch_noise_long(p.a, nr, (double2 *)(ws + p.w.A), (double2 *)(ws + p.w.Y), t.B,
                                                     (double *)(ws + p.off_part), out, t.T1, t.T2, st);
        return el == hipSuccess ? PPF_OK : hip_fail(ctx, el, "k_lf");
    });
}

// get_noise_fit / find_kc (ppf_noisefit.hip)
namespace {
// the checks the three entries share, and the tables into the launch's args
int noise_fit_args(ppf_ctx *ctx, int32_t fn, const double *a_grid, const int32_t *kc_table,
                   ppf::NoiseFitArgs &a) {
    if (fn != 0 && fn != 1) return fail(ctx, PPF_EINVAL, "fn=%d: 0 (exp_dc) or 1 (half_tri)", fn);
    if (!a_grid || !kc_table) return fail(ctx, PPF_EINVAL, "a_grid / kc_table is NULL");
    a = ppf::NoiseFitArgs{};
    a.fn = fn;
    for (int i = 0; i < ppf::kNfGrid; ++i) {
        if (kc_table[i] < 0) return fail(ctx, PPF_EINVAL, "kc_table[%d] = %d < 0", i, kc_table[i]);
        a.a_grid[i] = a_grid[i];
        a.kc_table[i] = kc_table[i];
    }
    return PPF_OK;
}
bool fact_ok(double fact) { return fact > 0.0 && fact <= ppf::kDblMax; }
size_t fit_long_pows_bytes(const LongPlan &p) {
    return align256((size_t)p.w.rows * (size_t)p.a.nharm * sizeof(double));
}
}  // namespace

int ppf_noise_fit_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype, const void *in,
                        double fact, const double *a_grid, const int32_t *kc_table, double *noise_out,
                        int32_t *kc_out, void *stream) {
    // every argument check on the host, before the context or any launch
    if (!nbin_supported(nbin)) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nrows < 0 || !fact_ok(fact) || (nrows > 0 && (!in || !noise_out || !kc_out)))
        return fail(ctx, PPF_EINVAL, "bad noise_fit arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    ppf::NoiseFitArgs a;
    int rc = noise_fit_args(ctx, 0, a_grid, kc_table, a);
    if (rc) return rc;
    if (!ctx) return PPF_EINVAL;
    if (nrows == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = twiddles(ctx, nbin, st, &a.T, &a.T2))) return rc;
    a.nbin = nbin; a.dtype = in_dtype; a.in = in; a.nharm = nbin / 2 + 1; a.fact = fact;
    a.noise_out = noise_out; a.kc_out = kc_out;
    if ((e = ppf::launch_noise_fit(a, nrows, st)) != hipSuccess) return hip_fail(ctx, e, "k_noise_fit");
    return PPF_OK;
}

size_t ppf_noise_fit_long_workspace_bytes(int64_t nrows, int64_t nbin) {
    LongPlan p;
    if (nbin < 3 || !long_plan(nrows, nbin, 4, p)) return 0;
    return p.bytes + fit_long_pows_bytes(p);
}

int ppf_noise_fit_long(ppf_ctx *ctx, int64_t nrows, int64_t nbin, int32_t in_dtype, const void *in,
                       double fact, const double *a_grid, const int32_t *kc_table, double *noise_out,
                       int32_t *kc_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (nrows < 0 || nbin < 1 || !fact_ok(fact) || (nrows > 0 && (!in || !noise_out || !kc_out)))
        return fail(ctx, PPF_EINVAL, "bad noise_fit arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    ppf::NoiseFitArgs f;
    int rc = noise_fit_args(ctx, 0, a_grid, kc_table, f);
    if (rc) return rc;
    LongPlan p;
    if (nbin < 3 || !long_plan(nrows, nbin, 4, p))
        return fail(ctx, PPF_EUNSUP, "nbin=%lld: fewer than 2 harmonics, or a transform longer than 2^24 points",
                    (long long)nbin);
    if (!ctx) return PPF_EINVAL;
    if (nrows == 0) return PPF_OK;
    const size_t need = p.bytes + fit_long_pows_bytes(p);
    if (!workspace || workspace_bytes < need)
        return fail(ctx, PPF_EINVAL, "workspace %zu < %zu bytes", workspace_bytes, need);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    LongTables t;
    if ((rc = long_tables(ctx, p.a, (double2 *)(ws + p.w.chirp), p.a.bluestein, st, t))) return rc;
    p.a.in_dtype = in_dtype;
    p.a.in = in;
    double *pows = (double *)(ws + p.bytes);
    f.nharm = p.a.nharm; f.pows = pows; f.fact = fact; f.noise_out = noise_out; f.kc_out = kc_out;
    return for_chunks(nrows, p.w.rows, [&](int64_t r0, int64_t nr) {
        p.a.row0 = r0;
        f.row0 = r0;
        hipError_t el = ppf::launch_pows_long(p.a, nr, (double2 *)(ws + p.w.A), (double2 *)(ws + p.w.Y), t.B, pows,
                                              t.T1, t.T2, st);
        if (el != hipSuccess) return hip_fail(ctx, el, "k_lf");
        if ((el = ppf::launch_spec_fit(f, nr, st)) != hipSuccess) return hip_fail(ctx, el, "k_spec_fit");
        return (int)PPF_OK;
    });
}

int ppf_find_kc_batch(ppf_ctx *ctx, int64_t nrows, int64_t nharm, const double *pows, const double *errs,
                      int64_t errs_len, int32_t fn, const double *a_grid, const int32_t *kc_table,
                      int32_t *kc_out, void *stream) {
    if (nrows < 0 || nharm < 2 || nharm > ((int64_t)1 << 30) || (nrows > 0 && (!pows || !kc_out)))
        return fail(ctx, PPF_EINVAL, "bad find_kc arguments");
    if (errs && errs_len != 1 && errs_len != nharm)
        return fail(ctx, PPF_EINVAL, "errs_len=%lld: 1 or nharm=%lld", (long long)errs_len, (long long)nharm);
    ppf::NoiseFitArgs a;
    int rc = noise_fit_args(ctx, fn, a_grid, kc_table, a);
    if (rc) return rc;
    if (!ctx) return PPF_EINVAL;
    if (nrows == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    a.nharm = nharm; a.pows = pows; a.errs = errs; a.errs_len = errs_len; a.kc_out = kc_out;
    if ((e = ppf::launch_spec_fit(a, nrows, (hipStream_t)stream)) != hipSuccess)
        return hip_fail(ctx, e, "k_spec_fit");
    return PPF_OK;
}

// ppf_rotate_long's plans and workspace: Bluestein transforms both ways
namespace {
struct RotPlan {
    ppf::LongRotArgs r;
    LongWork w;
    size_t bytes;
};
bool rot_plan(int64_t nrows, int64_t nbin, bool ref_len, RotPlan &p) {
    if (nrows < 0 || nbin < 2) return false;
    const bool odd = nbin & 1;
    if (!bluestein_plan(nbin, odd ? nbin : nbin / 2, !odd, p.r.f)) return false;
    const bool out_even = !odd || ref_len;
    const int64_t nout = odd && ref_len ? nbin - 1 : nbin;
    if (!bluestein_plan(nbin, out_even ? nout / 2 : nout, false, p.r.b)) return false;
    p.r.out_even = out_even ? 1 : 0;
    p.r.nout = nout;
    const size_t row_b = (size_t)p.r.f.M * sizeof(double2);     // b.M <= f.M
    Carver take;
    p.w = long_work(take, nrows, row_b, 2 * row_b, 2 * (size_t)p.r.b.M * sizeof(double2));
    p.bytes = take.o;
    return true;
}
}  // namespace

size_t ppf_rotate_long_workspace_bytes(int64_t nrows, int64_t nbin, int32_t ref_len) {
    RotPlan p;
    return rot_plan(nrows, nbin, ref_len != 0, p) ? p.bytes : 0;
}

static int rotate_long_run(ppf_ctx *ctx, RotPlan &p, int64_t nrows, int32_t in_dtype, const void *in,
                           const double *phases, const double *taus, double *out, char *ws, hipStream_t st);

int ppf_rotate_long(ppf_ctx *ctx, int64_t nrows, int64_t nbin, int32_t in_dtype, const void *in,
                    const double *phases, double *out, int32_t ref_len, void *workspace, size_t workspace_bytes,
                    void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nrows < 0 || nbin < 2 || (nrows > 0 && (!in || !phases || !out)))
        return fail(ctx, PPF_EINVAL, "bad rotate arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    RotPlan p;
    if (!rot_plan(nrows, nbin, ref_len != 0, p))
        return fail(ctx, PPF_EUNSUP, "nbin=%lld: transform longer than 2^24 points", (long long)nbin);
    if (nrows == 0) return PPF_OK;
    if (!workspace || workspace_bytes < p.bytes)
        return fail(ctx, PPF_EINVAL, "workspace %zu < %zu bytes", workspace_bytes, p.bytes);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    return rotate_long_run(ctx, p, nrows, in_dtype, in, phases, nullptr, out, (char *)workspace,
                           (hipStream_t)stream);
}

// the long rotation / scattering convolution of nrows rows on a plan whose
// workspace is `ws` (in may be out: each chunk's rows are read before
// they are written)
static int rotate_long_run(ppf_ctx *ctx, RotPlan &p, int64_t nrows, int32_t in_dtype, const void *in,
                           const double *phases, const double *taus, double *out, char *ws, hipStream_t st) {
    LongTables tf, tb;
    int rc;
    if ((rc = long_tables(ctx, p.r.f, (double2 *)(ws + p.w.chirp), true, st, tf))) return rc;
    if ((rc = long_tables(ctx, p.r.b, (double2 *)(ws + p.w.chirp_b), true, st, tb))) return rc;
    p.r.f.in_dtype = in_dtype;
    p.r.f.in = in;
    p.r.phases = phases;
    p.r.taus = taus;
    p.r.out = out;
    return for_chunks(nrows, p.w.rows, [&](int64_t r0, int64_t nr) {
        p.r.f.row0 = p.r.b.row0 = r0;
        const hipError_t e = ppf::launch_rotate_long(p.r, nr, (double2 *)(ws + p.w.A), (double2 *)(ws + p.w.Y), tf.B,
                                                     tb.B, tf.T1, tf.T2, tb.T1, tb.T2, st);
        return e == hipSuccess ? PPF_OK : hip_fail(ctx, e, "k_lr");
    });
}

int ppf_scales_batch(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nharm, const double *D,
                     const double *M, const int32_t *model_index, const double *errs_FT,
                     const double *params, const double *P, const double *freqs, const double *nus,
                     int32_t log10_tau, double *out, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nsub < 0 || nchan < 1 || nharm < 1 ||
        (nsub > 0 && (!D || !M || !params || !P || !freqs || !nus || !out)))
        return fail(ctx, PPF_EINVAL, "bad scales arguments");
    if (nsub == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    ppf::ScalesArgs a{nsub, nchan, nharm, log10_tau != 0, (const double2 *)D, (const double2 *)M,
                      model_index, errs_FT, params, P, freqs, nus, out};
    if ((e = ppf::launch_scales(a, (hipStream_t)stream)) != hipSuccess) return hip_fail(ctx, e, "k_scales");
    return PPF_OK;
}

int ppf_eval_point_block(void) { return ppf::kEvalPointBlock; }
int ppf_eval_harm_tile(void) { return ppf::kEvalTile; }

size_t ppf_eval_workspace_bytes(int32_t nprob, int32_t nchan, int32_t npoint, int32_t order) {
    if (nprob < 1 || nchan < 1 || npoint < 1 || order < 0 || order > 2) return 0;
    return (size_t)ppf::eval_partials(nprob, nchan, npoint, order) * sizeof(double) + 256;
}

int ppf_eval_batch(ppf_ctx *ctx, int32_t nprob, int32_t nchan, int32_t nharm, int32_t npoint,
                   const double *data_FT, const double *model_FT, int32_t nmodel,
                   const int32_t *model_index, const double *errs_FT, const double *P,
                   const double *freqs, const double *nus, const uint8_t *mask, const double *theta,
                   const double *fit_flags, int32_t log10_tau, int32_t order, double *f, double *grad,
                   double *hess, double *terms, void *workspace, size_t workspace_bytes, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nprob < 0 || nchan < 1 || nharm < 2 || npoint < 1 || nmodel < 1)
        return fail(ctx, PPF_EINVAL, "bad eval shape: nprob %d nchan %d nharm %d npoint %d nmodel %d", nprob,
                    nchan, nharm, npoint, nmodel);
    if (order < 0 || order > 2) return fail(ctx, PPF_EINVAL, "eval order %d not 0, 1 or 2", order);
    if (!model_index && nmodel != 1 && nmodel != nprob)
        return fail(ctx, PPF_EINVAL, "eval: %d models for %d problems need a model_index", nmodel, nprob);
    if (nprob == 0) return PPF_OK;
    if (!data_FT || !model_FT || !errs_FT || !P || !freqs || !nus || !theta || !f || (order >= 1 && !grad) ||
        (order >= 2 && !hess) || !workspace)
        return fail(ctx, PPF_EINVAL, "null eval pointer");
    const int64_t npb = ((int64_t)npoint + ppf::kEvalPointBlock - 1) / ppf::kEvalPointBlock;
    if ((int64_t)nprob * npb > INT32_MAX / (int64_t)nchan || (int64_t)nprob * npoint > INT32_MAX)
        return fail(ctx, PPF_EINVAL, "eval: more than 2^31 - 1 workgroups; split the points over calls");
    if (workspace_bytes < ppf_eval_workspace_bytes(nprob, nchan, npoint, order))
        return fail(ctx, PPF_ENOMEM, "eval workspace %zu < %zu", workspace_bytes,
                    ppf_eval_workspace_bytes(nprob, nchan, npoint, order));
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    ppf::EvalArgs a{};
    a.nprob = nprob; a.nchan = nchan; a.nharm = nharm; a.npoint = npoint; a.nmodel = nmodel;
    a.order = order; a.log10_tau = log10_tau ? 1 : 0;
    a.D = (const double2 *)data_FT; a.M = (const double2 *)model_FT; a.model_index = model_index;
    a.errs = errs_FT; a.P = P; a.freqs = freqs; a.nus = nus; a.mask = mask; a.theta = theta;
    a.flags = fit_flags; a.part = (double *)workspace; a.f = f; a.g = grad; a.H = hess; a.terms = terms;
    if ((e = ppf::launch_eval(a, (hipStream_t)stream)) != hipSuccess) return hip_fail(ctx, e, "k_eval");
    return PPF_OK;
}

size_t ppf_unpack_workspace_bytes(int32_t nsub, int32_t nchan, int32_t nbin) {
    if (nsub < 0 || nchan < 1 || nbin < 2) return 0;
    return ppf::unpack_partials(nsub, nchan, nbin) * sizeof(double) + 256;
}

static int64_t unpack_esize(int32_t elem) { return elem == 0 ? 2 : (elem == 1 ? 1 : 4); }

// The two unpack entries past their own checks (mode, sub_stride against the
// blocks they read): npol_out 1 with pol_mode, or npol_out 4 with conv
static int unpack_batch(ppf_ctx *ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                        int32_t elem, const void *raw, int64_t sub_stride, const float *scl,
                        const float *offs, const float *wts, int32_t npol_out, int32_t pol_mode,
                        int32_t conv, int32_t rm_baseline, float *out, double *stats,
                        double *total, int32_t *wstart, void *workspace, size_t workspace_bytes,
                        void *stream) {
    const int64_t esize = unpack_esize(elem);
    // the kernel loads whole elements: every sub-int block starts on one
    if (sub_stride % esize || (uintptr_t)raw % (uintptr_t)esize)
        return fail(ctx, PPF_EINVAL, "raw and sub_stride must be multiples of the %lld-byte element",
                    (long long)esize);
    if (nsub == 0) return PPF_OK;
    if (!raw || !scl || !offs || !out || !stats || !total || !wstart || !workspace)
        return fail(ctx, PPF_EINVAL, "null unpack pointer");
    if (workspace_bytes < ppf_unpack_workspace_bytes(nsub, nchan, nbin))
        return fail(ctx, PPF_ENOMEM, "unpack workspace %zu < %zu", workspace_bytes,
                    ppf_unpack_workspace_bytes(nsub, nchan, nbin));
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    ppf::UnpackArgs a{};
    a.nsub = nsub; a.npol = npol; a.nchan = nchan; a.nbin = nbin; a.elem = elem;
    a.npol_out = npol_out; a.pol_mode = pol_mode; a.conv = conv;
    a.rm_baseline = rm_baseline ? 1 : 0;
    a.win = std::min(nbin - 1, std::max(1, (int)std::lrint(0.15 * nbin)));
    a.raw = (const uint8_t *)raw; a.sub_stride = sub_stride;
    a.scl = scl; a.offs = offs; a.wts = wts; a.out = out;
    a.part = (double *)workspace; a.total = total; a.wstart = wstart; a.stats = stats;
    if ((e = ppf::launch_unpack(a, (hipStream_t)stream)) != hipSuccess) return hip_fail(ctx, e, "k_unpack");
    return PPF_OK;
}

int ppf_unpack_psrfits_batch(ppf_ctx *ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                             int32_t elem, const void *raw, int64_t sub_stride, const float *scl,
                             const float *offs, const float *wts, int32_t pol_mode,
                             int32_t rm_baseline, float *out, double *stats, double *total,
                             int32_t *wstart, void *workspace, size_t workspace_bytes,
                             void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nsub < 0 || npol < 1 || nchan < 1 || nbin < 2 || elem < 0 || elem > 3 || pol_mode < 0 ||
        pol_mode > 1 || (pol_mode == 1 && npol < 2))
        return fail(ctx, PPF_EINVAL, "bad unpack arguments (npol=%d nchan=%d nbin=%d elem=%d "
                    "pol_mode=%d)", npol, nchan, nbin, elem, pol_mode);
    if (sub_stride < (int64_t)(pol_mode == 1 ? 2 : 1) * nchan * nbin * unpack_esize(elem))
        return fail(ctx, PPF_EINVAL, "sub_stride %lld < one sub-int's DATA", (long long)sub_stride);
    return unpack_batch(ctx, nsub, npol, nchan, nbin, elem, raw, sub_stride, scl, offs, wts, 1,
                        pol_mode, 0, rm_baseline, out, stats, total, wstart, workspace,
                        workspace_bytes, stream);
}

int ppf_unpack_psrfits_pol_batch(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                                 int32_t elem, const void *raw, int64_t sub_stride,
                                 const float *scl, const float *offs, const float *wts,
                                 int32_t conv, int32_t rm_baseline, float *out, double *stats,
                                 double *total, int32_t *wstart, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nsub < 0 || nchan < 1 || nbin < 2 || elem < 0 || elem > 3 || conv < 0 || conv > 5)
        return fail(ctx, PPF_EINVAL, "bad unpack arguments (nchan=%d nbin=%d elem=%d conv=%d)",
                    nchan, nbin, elem, conv);
    if (sub_stride < (int64_t)4 * nchan * nbin * unpack_esize(elem))
        return fail(ctx, PPF_EINVAL, "sub_stride %lld < the four polarisation blocks of a sub-int",
                    (long long)sub_stride);
    return unpack_batch(ctx, nsub, 4, nchan, nbin, elem, raw, sub_stride, scl, offs, wts, 4, 0,
                        conv, rm_baseline, out, stats, total, wstart, workspace, workspace_bytes,
                        stream);
}

int ppf_pack_psrfits_batch(ppf_ctx *ctx, int64_t nrow, int32_t nbin, int32_t in_dtype,
                           const void *rows, int32_t elem, void *raw, float *scl, float *offs,
                           void *stream) {
    if (nrow < 0 || nbin < 1 || (elem != 0 && elem != 2) ||
        (in_dtype != PPF_F32 && in_dtype != PPF_F64))
        return fail(ctx, PPF_EINVAL, "bad pack arguments (nrow=%lld nbin=%d in_dtype=%d elem=%d)",
                    (long long)nrow, nbin, in_dtype, elem);
    // the byte counts stay inside int64
    if (nrow > INT64_MAX / ((int64_t)nbin * 8))
        return fail(ctx, PPF_EINVAL, "pack: nrow=%lld x nbin=%d overflows", (long long)nrow, nbin);
    if (nrow == 0) return PPF_OK;      // nothing to launch: nothing else is looked at
    if (!ctx) return PPF_EINVAL;
    if (!rows || !raw || !scl || !offs) return fail(ctx, PPF_EINVAL, "null pack pointer");
    // whole elements are loaded and stored
    if ((uintptr_t)rows % (in_dtype == PPF_F32 ? 4 : 8) || (uintptr_t)raw % (elem == 0 ? 2 : 4))
        return fail(ctx, PPF_EINVAL, "pack: rows / raw must be aligned to their element size");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    ppf::PackArgs a{nrow, nbin, in_dtype == PPF_F32, elem, rows, (uint8_t *)raw, scl, offs};
    if ((e = ppf::launch_pack(a, (hipStream_t)stream)) != hipSuccess) return hip_fail(ctx, e, "k_pack");
    return PPF_OK;
}

int ppf_copy_from_pinned(ppf_ctx *ctx, void *dst, const void *src, int64_t nbytes, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (nbytes < 0 || (nbytes > 0 && (!dst || !src)))
        return fail(ctx, PPF_EINVAL, "bad copy arguments");
    if (((uintptr_t)dst | (uintptr_t)src) % 16)
        return fail(ctx, PPF_EINVAL, "copy buffers must be 16-byte aligned");
    if (nbytes == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    void *src_dev = nullptr;
    if ((e = hipHostGetDevicePointer(&src_dev, const_cast<void *>(src), 0)) != hipSuccess || !src_dev) {
        (void)hipGetLastError();   // not sticky: the next launch must not see it
        return hip_fail(ctx, e != hipSuccess ? e : hipErrorInvalidValue,
                        "hipHostGetDevicePointer (src must be page-locked host memory)");
    }
    if ((e = ppf::launch_copy_host(src_dev, dst, nbytes, (hipStream_t)stream)) != hipSuccess)
        return hip_fail(ctx, e, "k_copy_host");
    return PPF_OK;
}

// grows the context's scratch to at least `bytes` (lscr_mu held)
static int lscr_reserve(ppf_ctx *ctx, size_t bytes) {
    if (ctx->lscr_bytes >= bytes) return PPF_OK;
    hipError_t e;
    if (ctx->lscr) {
        if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(ctx, e, "hipDeviceSynchronize");
        (void)hipFree(ctx->lscr);
        ctx->lscr = nullptr;
        ctx->lscr_bytes = 0;
    }
    if ((e = hipMalloc(&ctx->lscr, bytes)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc(scratch)");
    ctx->lscr_bytes = bytes;
    return PPF_OK;
}

int ppf_phase_shift_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t in_dtype,
                          const void *data, const double *model, const int32_t *model_index,
                          const double *noise, int32_t Ns, double lo, double hi, double *out,
                          void *stream) {
    if (!ctx) return PPF_EINVAL;
    // rows past the LDS transforms (round 6): their rFFTs on the long
    // transforms first, the FFTFIT on the stored bins (a synchronous call)
    const bool lng = !nbin_supported(nbin) && nbin > 4095;
    if (!nbin_supported(nbin) && !lng) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nprof < 0 || Ns < 1 || Ns > 65536 || (nprof > 0 && (!data || !model || !out)))
        return fail(ctx, PPF_EINVAL, "bad phase-shift arguments");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    if (lng && (size_t)(nbin / 2 + 2) * sizeof(double2) > 150u * 1024u)
        return fail(ctx, PPF_EUNSUP, "nbin=%d: the spectrum exceeds one workgroup's LDS", nbin);
    if (nprof == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T = nullptr, *T2 = nullptr;
    int rc;
    if (!lng && (rc = twiddles(ctx, nbin, st, &T, &T2))) return rc;
    ppf::PhaseShiftArgs a{};
    a.nbin = nbin; a.log2N = rfft_log2(nbin); a.dtype = in_dtype; a.kc = noise_kc(nbin / 2 + 1, 4);
    a.Ns = Ns; a.lo = lo; a.hi = hi; a.data = data; a.model = model; a.model_index = model_index;
    a.noise = noise; a.T = T; a.T2 = T2; a.out = out;
    if (!lng && !grid_gsh(nbin, Ns, false)) {
        if ((e = ppf::launch_phase_shift(a, nprof, st)) != hipSuccess) return hip_fail(ctx, e, "k_phase_shift");
        return PPF_OK;
    }
    if (!lng) {
        // the brute grid past the LDS (Ns = nbin at 8192): in the context's
        // scratch, held for the whole (synchronous) call
        std::lock_guard<std::mutex> lk(ctx->lscr_mu);
        if ((rc = lscr_reserve(ctx, align256(sizeof(double) * (size_t)nprof * ((size_t)Ns + 8))))) return rc;
        a.gsh = (double *)ctx->lscr;
        if ((e = ppf::launch_phase_shift(a, nprof, st)) != hipSuccess) return hip_fail(ctx, e, "k_phase_shift");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
        return PPF_OK;
    }
    // model rows in use: 1 + the largest model_index
    int nmodel = 1;
    if (model_index) {
        std::vector<int32_t> mi(nprof);
        if ((e = hipMemcpyAsync(mi.data(), model_index, nprof * sizeof(int32_t), hipMemcpyDeviceToHost, st)) !=
                hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(ctx, e, "hipMemcpyAsync(model_index)");
        for (int i = 0; i < nprof; ++i) {
            if (mi[i] < 0) return fail(ctx, PPF_EINVAL, "model_index[%d] = %d", i, mi[i]);
            nmodel = std::max(nmodel, mi[i] + 1);
        }
    }
    ppf::LongNoiseArgs f;
    if (!long_row_plan(nbin, f)) return fail(ctx, PPF_EUNSUP, "nbin=%d", nbin);
    const size_t nharm = (size_t)nbin / 2 + 1, row_b = (size_t)f.M * sizeof(double2);
    Carver take;
    const size_t oD = take(sizeof(double2) * (size_t)nprof * nharm);
    const size_t oM = take(sizeof(double2) * (size_t)nmodel * nharm);
    const LongWork L = long_work(take, std::max<int64_t>(nprof, nmodel), row_b, 2 * row_b);
    const bool gs = grid_gsh(nbin, Ns, true);
    const size_t oG = take(gs ? sizeof(double) * (size_t)nprof * ((size_t)Ns + 8) : 0);
    std::lock_guard<std::mutex> lk(ctx->lscr_mu);
    if ((rc = lscr_reserve(ctx, take.o))) return rc;
    char *ws = (char *)ctx->lscr;
    if ((rc = long_rfft_rows(ctx, L, ws, nbin, nmodel, PPF_F64, model, (double2 *)(ws + oM), false, st))) return rc;
    if ((rc = long_rfft_rows(ctx, L, ws, nbin, nprof, in_dtype, data, (double2 *)(ws + oD), true, st))) return rc;
    a.Mspec = (const double2 *)(ws + oM);
    a.Dspec = (const double2 *)(ws + oD);
    if (gs) a.gsh = (double *)(ws + oG);
    if ((e = ppf::launch_phase_shift(a, nprof, st)) != hipSuccess) return hip_fail(ctx, e, "k_phase_shift");
    // the scratch is reused by the next call (any stream): finish here
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
    return PPF_OK;
}

namespace {
// the three digits of a Gaussian model's evolution code into code[3]: PPF_OK
// or the error set
int parse_model_code(ppf_ctx *ctx, const char *model_code, int code[3]) {
    if (!model_code) return fail(ctx, PPF_EINVAL, "model_code is NULL");
    for (int i = 0; i < 3; ++i) {
        const char c = model_code[i];
        if (c != '0' && c != '1')   // evolve_parameter's KeyError (pplib.py:1082-1084)
            return fail(ctx, PPF_EINVAL, "model_code '%.3s': digit %d must be '0' or '1'", model_code, i);
        code[i] = c - '0';
    }
    return PPF_OK;
}

// the join arguments of the joined Gaussian entry points, checked on the
// host: PPF_OK or the error set
int check_join(ppf_ctx *ctx, int64_t nrow, int32_t njoin, const int32_t *join_id, const double *join_params,
               const double *P) {
    if (njoin < 0) return fail(ctx, PPF_EINVAL, "njoin=%d", njoin);
    if (nrow > 0 && (!join_id || !P || (njoin > 0 && !join_params)))
        return fail(ctx, PPF_EINVAL, "join_id / join_params / P is NULL");
    for (int64_t i = 0; i < nrow; ++i)
        if (join_id[i] < -1 || join_id[i] >= njoin)
            return fail(ctx, PPF_EINVAL, "join_id[%lld] = %d: -1 or an archive in [0, %d)", (long long)i,
                        join_id[i], njoin);
    return PPF_OK;
}

// j.join_id: the device copy of join_id (nrow entries) in the context's
// scratch.  The call is synchronous: the caller holds ctx->lscr_mu until its
// stream is done.
int join_id_to_scratch(ppf_ctx *ctx, const int32_t *join_id, int64_t nrow, hipStream_t st, ppf::GaussJoin &j) {
    const size_t jb = sizeof(int32_t) * (size_t)nrow;
    int rc;
    if ((rc = lscr_reserve(ctx, align256(jb)))) return rc;
    hipError_t e = hipMemcpyAsync(ctx->lscr, join_id, jb, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpyAsync(join_id)");
    j.join_id = (const int32_t *)ctx->lscr;
    return PPF_OK;
}

// ppf_gauss_portrait_batch (jn == nullptr) and ppf_gauss_portrait_join_batch.
// Each keeps its order of checks: the plain call looks at the context first,
// the joined one after its own length, shape and join checks.
int gauss_portrait_run(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin, int32_t ngauss,
                       const char *model_code, const double *params, const double *scattering_index,
                       const double *freqs, const double *nu_ref, const ppf::GaussJoin *jn,
                       const int32_t *join_id, double *out, void *stream) {
    const bool bad = nport < 0 || nchan < 1 || ngauss < 0 ||
                     (nport > 0 && (!params || !scattering_index || !freqs || !nu_ref || !out));
    int rc;
    if (jn) {
        // the rotation needs the even-length LDS transforms (the reference's
        // irfft returns nbin - 1 bins at odd nbin: it cannot rotate those either)
        if ((nbin & 1) || nbin < 32 || nbin > 8192 || !nbin_supported(nbin))
            return fail(ctx, PPF_EUNSUP, "nbin=%d: even lengths in [32, 8192] (the LDS row transforms)", nbin);
        if (bad) return fail(ctx, PPF_EINVAL, "bad gauss_portrait arguments");
        if ((rc = check_join(ctx, (int64_t)(nport > 0 ? nport : 0) * nchan, jn->njoin, join_id, jn->join_params,
                             jn->P)))
            return rc;
        if (jn->njoin == 0 || nport == 0) jn = nullptr;   // the plain model
    }
    if (!ctx) return PPF_EINVAL;
    // rows past the LDS transforms (round 6): the Gaussians are evaluated
    // per bin in LDS (nbin doubles); the scattering convolution of even rows
    // then runs on the long transforms (ppf_rotate_long's pipeline with the
    // 1 / (1 + 2 pi i k tau_n) factor in place of the phasor; a synchronous
    // call with the context's scratch); scattered odd rows are refused
    const bool lng = !nbin_supported(nbin);
    if (lng && (nbin <= 4095 || (size_t)nbin * sizeof(double) > 150u * 1024u))
        return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (bad) return fail(ctx, PPF_EINVAL, "bad gauss_portrait arguments");
    ppf::GaussArgs a{};
    if ((rc = parse_model_code(ctx, model_code, a.code))) return rc;
    if (nport == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T = nullptr, *T2 = nullptr;
    bool lscat = false;
    if (lng) {
        // the models' tau (params[p][1]) on the host: a scattered one at
        // this length is refused, not half-built (a one-off small copy)
        std::vector<double> prm((size_t)nport * (2 + 6 * ngauss));
        if ((e = hipMemcpyAsync(prm.data(), params, prm.size() * sizeof(double), hipMemcpyDeviceToHost, st)) !=
                hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return hip_fail(ctx, e, "hipMemcpyAsync(params)");
        for (int p = 0; p < nport; ++p)
            if (prm[(size_t)p * (2 + 6 * ngauss) + 1] != 0.0) lscat = true;
        if (lscat && (nbin & 1))
            return fail(ctx, PPF_EUNSUP, "scattered model (TAU != 0) at odd nbin=%d past 4095 (the reference's "
                        "nbin - 1-bin irfft rows)", nbin);
    } else if ((rc = twiddles(ctx, nbin, st, &T, &T2))) {
        return rc;
    }
    a.nport = nport; a.nchan = nchan; a.nbin = nbin; a.log2N = rfft_log2(nbin);
    a.ngauss = ngauss; a.npar = 2 + 6 * ngauss;
    a.params = params; a.scat_index = scattering_index; a.freqs = freqs; a.nu_ref = nu_ref;
    a.T = T; a.T2 = T2; a.out = out;
    a.Te = T; a.T2e = T2;
    if (!lng && (nbin & 1) && (rc = twiddles(ctx, nbin - 1, st, &a.Te, &a.T2e))) return rc;
    if (jn) {
        std::lock_guard<std::mutex> lk(ctx->lscr_mu);
        ppf::GaussJoin j = *jn;
        if ((rc = join_id_to_scratch(ctx, join_id, (int64_t)nport * nchan, st, j))) return rc;
        if ((e = ppf::launch_gauss_port_join(a, j, st)) != hipSuccess) return hip_fail(ctx, e, "k_gauss_port_join");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
        return PPF_OK;
    }
    if (!lscat) {
        if ((e = ppf::launch_gauss_port(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_gauss_port");
        return PPF_OK;
    }
    const int64_t nrows = (int64_t)nport * nchan;
    RotPlan rp;
    if (!rot_plan(nrows, nbin, false, rp)) return fail(ctx, PPF_EUNSUP, "nbin=%d", nbin);
    const size_t oT = align256(rp.bytes);
    std::lock_guard<std::mutex> lk(ctx->lscr_mu);
    if ((rc = lscr_reserve(ctx, oT + align256(sizeof(double) * (size_t)nrows)))) return rc;
    char *ws = (char *)ctx->lscr;
    a.taus_out = (double *)(ws + oT);
    if ((e = ppf::launch_gauss_port(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_gauss_port");
    if ((rc = rotate_long_run(ctx, rp, nrows, PPF_F64, out, nullptr, a.taus_out, out, ws, st))) return rc;
    // the scratch is reused by the next call (any stream): finish here
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
    return PPF_OK;
}
}  // namespace

int ppf_gauss_portrait_batch(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin,
                             int32_t ngauss, const char *model_code, const double *params,
                             const double *scattering_index, const double *freqs,
                             const double *nu_ref, double *out, void *stream) {
    return gauss_portrait_run(ctx, nport, nchan, nbin, ngauss, model_code, params, scattering_index, freqs, nu_ref,
                              nullptr, nullptr, out, stream);
}

int ppf_gauss_portrait_join_batch(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin,
                                  int32_t ngauss, const char *model_code, const double *params,
                                  const double *scattering_index, const double *freqs,
                                  const double *nu_ref, int32_t njoin, const int32_t *join_id,
                                  const double *join_params, const double *P, double *out,
                                  void *stream) {
    ppf::GaussJoin j{};
    j.njoin = njoin; j.join_params = join_params; j.P = P;
    return gauss_portrait_run(ctx, nport, nchan, nbin, ngauss, model_code, params, scattering_index, freqs, nu_ref,
                              &j, join_id, out, stream);
}

namespace {
// workspace of ppf_gauss_lsq_batch: the model rows, the partial tiles and the
// device copies of free_idx / delta
struct GaussLsqLayout {
    int ntile, npair, nseg;
    size_t rows, part, fidx, delta, bytes;
};
bool gauss_lsq_layout(int64_t nfit, int64_t nchan, int64_t nbin, int64_t nfree, GaussLsqLayout &L) {
    if (nfit < 0 || nchan < 1 || nfree < 0 || nfree + 1 > ppf::kGramMaxCol) return false;
    if ((nbin & 1) || !nbin_supported((int)nbin) || nbin > 8192) return false;
    L.ntile = (int)((nfree + 1 + 15) / 16);
    L.npair = L.ntile * (L.ntile + 1) / 2;
    L.nseg = (int)((nbin + ppf::kGramSeg - 1) / ppf::kGramSeg);
    // one workgroup per row, one grid dimension per fit
    if (nfit > 65535 || nfit * nchan * (nfree + 1) > 0x7fffffffLL || nchan * L.nseg > 0x7fffffffLL) return false;
    size_t o = 0;
    L.rows = o;  o += align256(sizeof(double) * (size_t)nfit * nchan * (nfree + 1) * nbin);
    L.part = o;  o += align256(sizeof(double) * (size_t)nfit * nchan * L.nseg * L.npair * 256);
    L.fidx = o;  o += align256(sizeof(int32_t) * (size_t)(nfree > 0 ? nfree : 1));
    L.delta = o; o += align256(sizeof(double) * (size_t)(nfit * nfree > 0 ? nfit * nfree : 1));
    L.bytes = o;
    return true;
}
}  // namespace

size_t ppf_gauss_lsq_workspace_bytes(int32_t nfit, int32_t nchan, int32_t nbin, int32_t nfree) {
    GaussLsqLayout L;
    return gauss_lsq_layout(nfit, nchan, nbin, nfree, L) ? L.bytes : 0;
}

namespace {
// ppf_gauss_lsq_batch (jn == nullptr) and ppf_gauss_lsq_join_batch
int gauss_lsq_run(ppf_ctx *ctx, int32_t nfit, int32_t nchan, int32_t nbin, int32_t ngauss,
                  const char *model_code, const double *params, const double *scattering_index,
                  const double *freqs, const double *nu_ref, const ppf::GaussJoin *jn,
                  const int32_t *join_id, int32_t nfree,
                  const int32_t *free_idx, const double *delta, int32_t in_dtype,
                  const void *data, const double *inv_errs, double *gram, void *workspace,
                  size_t workspace_bytes, void *stream) {
    // every argument check on the host, before the context or any launch
    if ((nbin & 1) || nbin < 32 || nbin > 8192 || !nbin_supported(nbin))
        return fail(ctx, PPF_EUNSUP, "nbin=%d: even lengths in [32, 8192] (the LDS row transforms)", nbin);
    if (nfree >= ppf::kGramMaxCol)
        return fail(ctx, PPF_EUNSUP, "nfree=%d: at most %d free parameters", nfree, ppf::kGramMaxCol - 1);
    if (nfit < 0 || nchan < 1 || ngauss < 0 || nfree < 0)
        return fail(ctx, PPF_EINVAL, "bad gauss_lsq shape");
    if (in_dtype != PPF_F32 && in_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "in_dtype");
    ppf::GaussLsqArgs a{};
    int rc;
    if ((rc = parse_model_code(ctx, model_code, a.code))) return rc;
    const int npar = 2 + 6 * ngauss;
    const int njoin = jn ? jn->njoin : 0, next = npar + 2 * njoin;   // the scattering index's entry
    if (jn && (rc = check_join(ctx, (int64_t)(nfit > 0 ? nfit : 0) * nchan, njoin, join_id, jn->join_params, jn->P)))
        return rc;
    if (nfree > 0 && (!free_idx || (nfit > 0 && !delta))) return fail(ctx, PPF_EINVAL, "free_idx / delta is NULL");
    for (int j = 0; j < nfree; ++j) {
        if (free_idx[j] < 0 || free_idx[j] > next || (j > 0 && free_idx[j] <= free_idx[j - 1]))
            return fail(ctx, PPF_EINVAL, "free_idx[%d] = %d: strictly increasing in [0, %d]", j, free_idx[j], next);
        for (int f = 0; f < nfit; ++f) {
            const double d = delta[(size_t)f * nfree + j];
            if (!(d != 0.0) || !std::isfinite(d))
                return fail(ctx, PPF_EINVAL, "delta[%d][%d] = %g: a finite non-zero step", f, j, d);
        }
    }
    GaussLsqLayout L;
    if (!gauss_lsq_layout(nfit, nchan, nbin, nfree, L)) return fail(ctx, PPF_EUNSUP, "gauss_lsq shape too large");
    if (nfit > 0 && (!workspace || workspace_bytes < L.bytes))
        return fail(ctx, PPF_EINVAL, "workspace: %zu bytes given, %zu needed", workspace_bytes, L.bytes);
    if (nfit > 0 && (!params || !scattering_index || !freqs || !nu_ref || !data || !inv_errs || !gram))
        return fail(ctx, PPF_EINVAL, "null gauss_lsq argument");
    if (!ctx) return PPF_EINVAL;
    if (nfit == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = twiddles(ctx, nbin, st, &a.T, &a.T2))) return rc;
    char *ws = (char *)workspace;
    if (nfree > 0) {
        if ((e = hipMemcpyAsync(ws + L.fidx, free_idx, sizeof(int32_t) * nfree, hipMemcpyHostToDevice, st)) !=
                hipSuccess ||
            (e = hipMemcpyAsync(ws + L.delta, delta, sizeof(double) * (size_t)nfit * nfree,
                                hipMemcpyHostToDevice, st)) != hipSuccess)
            return hip_fail(ctx, e, "hipMemcpyAsync(free_idx, delta)");
    }
    a.nfit = nfit; a.nchan = nchan; a.nbin = nbin; a.ngauss = ngauss; a.npar = npar; a.nfree = nfree;
    a.dtype = in_dtype; a.ntile = L.ntile; a.npair = L.npair; a.nseg = L.nseg;
    a.params = params; a.scat_index = scattering_index; a.freqs = freqs; a.nu_ref = nu_ref;
    a.free_idx = (const int32_t *)(ws + L.fidx); a.delta = (const double *)(ws + L.delta);
    a.data = data; a.inv_errs = inv_errs;
    a.rows = (double *)(ws + L.rows); a.part = (double *)(ws + L.part); a.gram = gram;
    if (njoin > 0) {
        std::lock_guard<std::mutex> lk(ctx->lscr_mu);
        ppf::GaussJoin j = *jn;
        if ((rc = join_id_to_scratch(ctx, join_id, (int64_t)nfit * nchan, st, j))) return rc;
        if ((e = ppf::launch_gauss_lsq_join(a, j, st)) != hipSuccess)
            return hip_fail(ctx, e, "k_gauss_rows_join / k_gauss_gram_join");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
        return PPF_OK;
    }
    if ((e = ppf::launch_gauss_lsq(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_gauss_rows / k_gauss_gram");
    return PPF_OK;
}
}  // namespace

int ppf_gauss_lsq_batch(ppf_ctx *ctx, int32_t nfit, int32_t nchan, int32_t nbin, int32_t ngauss,
                        const char *model_code, const double *params, const double *scattering_index,
                        const double *freqs, const double *nu_ref, int32_t nfree,
                        const int32_t *free_idx, const double *delta, int32_t in_dtype,
                        const void *data, const double *inv_errs, double *gram, void *workspace,
                        size_t workspace_bytes, void *stream) {
    return gauss_lsq_run(ctx, nfit, nchan, nbin, ngauss, model_code, params, scattering_index, freqs, nu_ref,
                         nullptr, nullptr, nfree, free_idx, delta, in_dtype, data, inv_errs, gram, workspace,
                         workspace_bytes, stream);
}

int ppf_gauss_lsq_join_batch(ppf_ctx *ctx, int32_t nfit, int32_t nchan, int32_t nbin, int32_t ngauss,
                             const char *model_code, const double *params, const double *scattering_index,
                             const double *freqs, const double *nu_ref, int32_t njoin,
                             const int32_t *join_id, const double *join_params, const double *P,
                             int32_t nfree, const int32_t *free_idx, const double *delta,
                             int32_t in_dtype, const void *data, const double *inv_errs, double *gram,
                             void *workspace, size_t workspace_bytes, void *stream) {
    ppf::GaussJoin j{};
    j.njoin = njoin; j.join_params = join_params; j.P = P;
    return gauss_lsq_run(ctx, nfit, nchan, nbin, ngauss, model_code, params, scattering_index, freqs, nu_ref, &j,
                         join_id, nfree, free_idx, delta, in_dtype, data, inv_errs, gram, workspace,
                         workspace_bytes, stream);
}

namespace {
// workspace of the ppf_swt_* calls: the coefficient rows and the device
// copies of the case lists
struct SwtLayout {
    size_t coef, cases, fact, bytes;
};
// PPF_OK, or the error code of an unsupported / invalid transform shape
int swt_shape(int64_t nprof, int64_t nbin, int64_t nlevel, int64_t max_ncase, SwtLayout &L) {
    if ((nbin & 1) || nbin < 32 || nbin > 8192 || !nbin_supported((int)nbin)) return PPF_EUNSUP;
    if (nprof < 0 || nlevel < 1 || max_ncase < 0) return PPF_EINVAL;
    const bool pow2 = (nbin & (nbin - 1)) == 0;
    if (pow2 ? ((int64_t)1 << nlevel) > nbin : nlevel > 1) return PPF_EUNSUP;
    if (nprof > 0x7fffffffLL || max_ncase > 0x7fffffffLL) return PPF_EUNSUP;   // one workgroup each
    size_t o = 0;
    L.coef = o;  o += align256(sizeof(double) * (size_t)(nprof > 0 ? nprof : 1) * nlevel * 2 * nbin);
    L.cases = o; o += align256(sizeof(int32_t) * 3 * (size_t)(max_ncase > 0 ? max_ncase : 1));
    L.fact = o;  o += align256(sizeof(double) * (size_t)(max_ncase > 0 ? max_ncase : 1));
    L.bytes = o;
    return PPF_OK;
}
int swt_fail(ppf_ctx *ctx, int rc, int nbin, int nlevel) {
    return fail(ctx, rc, "swt: nbin=%d nlevel=%d: nbin even in [32, 8192], 1 <= nlevel <= log2(nbin) for a "
                         "power of two, nlevel = 1 otherwise", nbin, nlevel);
}
}  // namespace

size_t ppf_swt_workspace_bytes(int32_t nprof, int32_t nbin, int32_t nlevel, int32_t max_ncase) {
    SwtLayout L;
    return swt_shape(nprof, nbin, nlevel, max_ncase, L) == PPF_OK ? L.bytes : 0;
}

int ppf_swt_analyse_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t nlevel, const double *prof,
                          double *medians, double *noise, void *workspace, size_t workspace_bytes,
                          void *stream) {
    // every argument check on the host, before the context or any launch
    SwtLayout L;
    int rc = swt_shape(nprof, nbin, nlevel, 0, L);
    if (rc) return swt_fail(ctx, rc, nbin, nlevel);
    if (nprof > 0 && (!prof || !medians || !noise)) return fail(ctx, PPF_EINVAL, "null swt argument");
    if (nprof > 0 && (!workspace || workspace_bytes < L.bytes))
        return fail(ctx, PPF_EINVAL, "workspace: %zu bytes given, %zu needed", workspace_bytes, L.bytes);
    if (!ctx) return PPF_EINVAL;
    if (nprof == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    ppf::SwtArgs a{};
    if ((rc = twiddles(ctx, nbin, st, &a.T, &a.T2))) return rc;
    a.nprof = nprof; a.nbin = nbin; a.nlevel = nlevel; a.kc = noise_kc(nbin / 2 + 1, 4);
    a.pow2 = (nbin & (nbin - 1)) == 0;
    a.sq2ln = std::sqrt(2.0 * std::log((double)nbin));
    a.prof = prof; a.coef = (double *)((char *)workspace + L.coef); a.med = medians; a.noise = noise;
    if ((e = ppf::launch_swt_analyse(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_swt_analyse");
    return PPF_OK;
}

int ppf_swt_score_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t nlevel, const double *prof,
                        const double *medians, const double *noise, int32_t ncase, const int32_t *cases,
                        const double *fact, double *out, double *smooth, void *workspace,
                        size_t workspace_bytes, void *stream) {
    SwtLayout L;
    int rc = swt_shape(nprof, nbin, nlevel, ncase, L);
    if (rc) return swt_fail(ctx, rc, nbin, nlevel);
    if (ncase > 0 && (!cases || !fact || !out || !prof || !medians || !noise))
        return fail(ctx, PPF_EINVAL, "null swt argument");
    for (int c = 0; c < ncase; ++c) {
        const int32_t *k = cases + 3 * (size_t)c;
        if (k[0] < 0 || k[0] >= nprof)
            return fail(ctx, PPF_EINVAL, "case %d: profile %d outside [0, %d)", c, k[0], nprof);
        if (k[1] < 1 || k[1] > nlevel)
            return fail(ctx, PPF_EINVAL, "case %d: level %d outside [1, %d]", c, k[1], nlevel);
        if (k[2] != 0 && k[2] != 1) return fail(ctx, PPF_EINVAL, "case %d: threshold type %d", c, k[2]);
        if (!std::isfinite(fact[c])) return fail(ctx, PPF_EINVAL, "case %d: factor %g", c, fact[c]);
    }
    if (ncase > 0 && (!workspace || workspace_bytes < L.bytes))
        return fail(ctx, PPF_EINVAL, "workspace: %zu bytes given, %zu needed", workspace_bytes, L.bytes);
    if (!ctx) return PPF_EINVAL;
    if (ncase == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    ppf::SwtArgs a{};
    if ((rc = twiddles(ctx, nbin, st, &a.T, &a.T2))) return rc;
    char *ws = (char *)workspace;
    if ((e = hipMemcpyAsync(ws + L.cases, cases, sizeof(int32_t) * 3 * (size_t)ncase, hipMemcpyHostToDevice,
                            st)) != hipSuccess ||
        (e = hipMemcpyAsync(ws + L.fact, fact, sizeof(double) * (size_t)ncase, hipMemcpyHostToDevice, st)) !=
            hipSuccess)
        return hip_fail(ctx, e, "hipMemcpyAsync(cases, fact)");
    a.nprof = nprof; a.nbin = nbin; a.nlevel = nlevel; a.kc = noise_kc(nbin / 2 + 1, 4); a.ncase = ncase;
    a.pow2 = (nbin & (nbin - 1)) == 0;
    a.sq2ln = std::sqrt(2.0 * std::log((double)nbin));
    a.prof = prof; a.coef = (double *)(ws + L.coef);
    a.med = const_cast<double *>(medians); a.noise = const_cast<double *>(noise);
    a.cases = (const int32_t *)(ws + L.cases); a.fact = (const double *)(ws + L.fact);
    a.out = out; a.smooth = smooth;
    if ((e = ppf::launch_swt_score(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_swt_score");
    return PPF_OK;
}

int ppf_swt_search_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t nlevel, const double *prof,
                         const double *medians, const double *noise, int32_t soft, double rchi2_tol,
                         int32_t ngrid, const double *grid, const double *table, double *fact_min,
                         double *fun_min, int32_t *nfev, void *workspace, size_t workspace_bytes,
                         void *stream) {
    SwtLayout L;
    // the grid takes the factor slot of a score call of ngrid cases
    int rc = swt_shape(nprof, nbin, nlevel, ngrid, L);
    if (rc) return swt_fail(ctx, rc, nbin, nlevel);
    if ((int64_t)nprof * nlevel > 0x7fffffffLL) return swt_fail(ctx, PPF_EUNSUP, nbin, nlevel);   // one workgroup each
    if (ngrid < 1) return fail(ctx, PPF_EINVAL, "swt search: ngrid = %d", ngrid);
    if (soft != 0 && soft != 1) return fail(ctx, PPF_EINVAL, "swt search: threshold type %d", soft);
    if (!std::isfinite(rchi2_tol)) return fail(ctx, PPF_EINVAL, "swt search: rchi2_tol %g", rchi2_tol);
    if (!grid || (nprof > 0 && (!prof || !medians || !noise || !table || !fact_min || !fun_min || !nfev)))
        return fail(ctx, PPF_EINVAL, "null swt argument");
    for (int g = 0; g < ngrid; ++g)
        if (!std::isfinite(grid[g])) return fail(ctx, PPF_EINVAL, "swt search: grid[%d] = %g", g, grid[g]);
    if (nprof > 0 && (!workspace || workspace_bytes < L.bytes))
        return fail(ctx, PPF_EINVAL, "workspace: %zu bytes given, %zu needed", workspace_bytes, L.bytes);
    if (!ctx) return PPF_EINVAL;
    if (nprof == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    ppf::SwtArgs a{};
    if ((rc = twiddles(ctx, nbin, st, &a.T, &a.T2))) return rc;
    char *ws = (char *)workspace;
    if ((e = hipMemcpyAsync(ws + L.fact, grid, sizeof(double) * (size_t)ngrid, hipMemcpyHostToDevice, st)) !=
        hipSuccess)
        return hip_fail(ctx, e, "hipMemcpyAsync(grid)");
    a.nprof = nprof; a.nbin = nbin; a.nlevel = nlevel; a.kc = noise_kc(nbin / 2 + 1, 4);
    a.pow2 = (nbin & (nbin - 1)) == 0;
    a.sq2ln = std::sqrt(2.0 * std::log((double)nbin));
    a.prof = prof; a.coef = (double *)(ws + L.coef);
    a.med = const_cast<double *>(medians); a.noise = const_cast<double *>(noise);
    a.ngrid = ngrid; a.soft = soft; a.rchi2_tol = rchi2_tol;
    a.grid = (const double *)(ws + L.fact); a.table = table;
    a.fact_min = fact_min; a.fun_min = fun_min; a.nfev = nfev;
    if ((e = ppf::launch_swt_search(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_swt_search");
    return PPF_OK;
}

int ppf_spline_portrait_batch(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin_model,
                              int32_t nbin, int32_t ncomp, int32_t nknots, int32_t degree,
                              const double *mean_prof, const double *eigvec, const double *knots,
                              const double *coefs, const double *freqs, double *out, void *stream) {
    if (!ctx) return PPF_EINVAL;
    // the model's own length: no transform (any nbin); resampled: two even
    // lengths the LDS transforms take (scipy.signal.resample's Nyquist
    // split as restated in k_spline_port assumes even lengths)
    const bool same = nbin == nbin_model;
    if (same ? nbin < 2
             : !(nbin % 2 == 0 && nbin_model % 2 == 0 && nbin_supported(nbin) && nbin_supported(nbin_model)))
        return fail(ctx, PPF_EUNSUP,
                    "nbin=%d nbin_model=%d: the model's own length, or both even in [32, 8192]", nbin,
                    nbin_model);
    if (nport < 0 || nchan < 1 || ncomp < 0 || ncomp > ppf::kSplineMaxComp || degree < 0 ||
        degree > ppf::kSplineMaxDeg || (ncomp > 0 && nknots < 2 * degree + 2))
        return fail(ctx, PPF_EINVAL, "bad spline model (ncomp=%d nknots=%d degree=%d)", ncomp, nknots,
                    degree);
    if (nport == 0) return PPF_OK;
    if (!mean_prof || !freqs || !out || (ncomp > 0 && (!eigvec || !knots || !coefs)))
        return fail(ctx, PPF_EINVAL, "null spline argument");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    ppf::SplineArgs a{};
    a.nport = nport; a.nchan = nchan; a.nbin_model = nbin_model; a.nbin = nbin; a.ncomp = ncomp;
    a.nknots = nknots; a.degree = degree;
    a.log2N0 = fft_log2(nbin_model / 2); a.log2N1 = rfft_log2(nbin);
    a.mean_prof = mean_prof; a.eigvec = eigvec; a.knots = knots; a.coefs = coefs; a.freqs = freqs;
    a.out = out;
    int rc;
    if (nbin != nbin_model) {
        if ((rc = twiddles(ctx, nbin_model, st, &a.T0, &a.T20))) return rc;
        if ((rc = twiddles(ctx, nbin, st, &a.T1, &a.T21))) return rc;
    }
    if ((e = ppf::launch_spline_port(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_spline_port");
    return PPF_OK;
}

int ppf_synth_batch(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nbin, const double *model,
                    const double *freqs, const double *phi, const double *DM, const double *P,
                    double nu_ref, double noise, uint64_t seed, int64_t first_sub,
                    int32_t out_dtype, void *out, void *stream) {
    if (!ctx) return PPF_EINVAL;
    if (!nbin_supported(nbin)) return fail(ctx, PPF_EUNSUP, "nbin=%d unsupported", nbin);
    if (nsub < 0 || nchan < 1 || (nsub > 0 && (!model || !freqs || !phi || !DM || !P || !out)))
        return fail(ctx, PPF_EINVAL, "bad synth arguments");
    if (out_dtype != PPF_F32 && out_dtype != PPF_F64) return fail(ctx, PPF_EINVAL, "out_dtype");
    if (nsub == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    // model spectra into a temporary buffer owned by this call
    double2 *Mft = nullptr;
    const size_t nharm = (size_t)nbin / 2 + 1;
    e = hipMallocAsync((void **)&Mft, sizeof(double2) * nchan * nharm, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMallocAsync(synth)");
    ppf::RfftArgs ra{nbin, rfft_log2(nbin), PPF_F64, model, T, T2, Mft};
    if ((e = ppf::launch_rfft_rows(ra, nchan, st)) != hipSuccess) return hip_fail(ctx, e, "k_rfft_rows");
    ppf::SynthArgs a{};
    a.nsub = nsub; a.nchan = nchan; a.nbin = nbin; a.log2N = rfft_log2(nbin); a.dtype = out_dtype;
    a.Mft = Mft; a.freqs = freqs; a.phi = phi; a.DM = DM; a.P = P; a.nu_ref = nu_ref;
    a.noise = noise; a.seed = seed; a.first = first_sub; a.T = T; a.T2 = T2; a.out = out;
    if ((e = ppf::launch_synth(a, st)) != hipSuccess) return hip_fail(ctx, e, "k_synth");
    (void)hipFreeAsync(Mft, st);
    return PPF_OK;
}

int ppf_fake_batch(ppf_ctx *ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin, int32_t nmodel,
                   const double *model, const int32_t *model_of, const double *phase,
                   const double *tau_n, const double *gain, const double *noise, uint64_t seed,
                   int64_t first_sub, int32_t out_kind, void *out, float *dat_scl, float *dat_offs,
                   void *stream) {
    // every argument check on the host, before the context or any launch
    if ((nbin & 1) || nbin < 32 || nbin > 8192 || !nbin_supported(nbin))
        return fail(ctx, PPF_EUNSUP, "nbin=%d: even nbin in [32, 8192] (the LDS row transforms)", nbin);
    if (nsub < 0 || npol < 1 || nchan < 1 || nmodel < 1 || first_sub < 0)
        return fail(ctx, PPF_EINVAL, "bad fake shape (nsub=%d npol=%d nchan=%d nmodel=%d first_sub=%lld)",
                    nsub, npol, nchan, nmodel, (long long)first_sub);
    if (out_kind != PPF_FAKE_I16 && out_kind != PPF_FAKE_F64) return fail(ctx, PPF_EINVAL, "out_kind");
    if ((int64_t)nsub * npol * nchan > 0x7fffffffLL)   // one workgroup per row
        return fail(ctx, PPF_EUNSUP, "nsub * npol * nchan = %lld rows: at most 2^31 - 1 per call",
                    (long long)((int64_t)nsub * npol * nchan));
    if (nsub > 0 && (!model || !model_of || !phase || !tau_n || !gain || !noise || !out ||
                     (out_kind == PPF_FAKE_I16 && (!dat_scl || !dat_offs))))
        return fail(ctx, PPF_EINVAL, "null fake argument");
    if (((uintptr_t)out & 15) || ((uintptr_t)dat_scl & 3) || ((uintptr_t)dat_offs & 3))
        return fail(ctx, PPF_EINVAL, "out must be 16-byte aligned, dat_scl / dat_offs 4-byte aligned");
    if (!ctx) return PPF_EINVAL;
    if (nsub == 0) return PPF_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const double2 *T, *T2;
    int rc = twiddles(ctx, nbin, st, &T, &T2);
    if (rc) return rc;
    // the templates' spectra in a buffer owned by this call (as ppf_synth_batch)
    double2 *Mft = nullptr;
    const size_t nharm = (size_t)nbin / 2 + 1;
    e = hipMallocAsync((void **)&Mft, sizeof(double2) * (size_t)nmodel * nchan * nharm, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipMallocAsync(fake)");
    ppf::RfftArgs ra{nbin, rfft_log2(nbin), PPF_F64, model, T, T2, Mft};
    if ((e = ppf::launch_rfft_rows(ra, (int64_t)nmodel * nchan, st)) != hipSuccess) {
        (void)hipFreeAsync(Mft, st);
        return hip_fail(ctx, e, "k_rfft_rows");
    }
    ppf::FakeArgs a{};
    a.nsub = nsub; a.npol = npol; a.nchan = nchan; a.nbin = nbin; a.nmodel = nmodel; a.kind = out_kind;
    a.Mft = Mft; a.model_of = model_of; a.phase = phase; a.tau = tau_n; a.gain = gain; a.noise = noise;
    a.seed = seed; a.first = first_sub; a.T = T; a.T2 = T2; a.out = out; a.scl = dat_scl; a.offs = dat_offs;
    e = ppf::launch_fake(a, st);
    (void)hipFreeAsync(Mft, st);
    if (e != hipSuccess) return hip_fail(ctx, e, "k_fake");
    return PPF_OK;
}

int ppf_poly_real_roots_host(const double *coeffs, int deg, double *out) {
    if (!coeffs || !out || deg < 0 || deg > 8) return -2;
    return ppf::poly_real_roots(coeffs, deg, out);
}

int ppf_tr_subproblem_host(const double *H, const double *g, int n, double R, double *p) {
    if (!H || !g || !p || n < 1 || n > 5 || !(R > 0.0)) return -1;
    double A[5][5];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) A[i][j] = H[i * n + j];
    bool hb = false;
    switch (n) {
        case 1: hb = ppf::tr_exact<1>(A, g, R, p); break;
        case 2: hb = ppf::tr_exact<2>(A, g, R, p); break;
        case 3: hb = ppf::tr_exact<3>(A, g, R, p); break;
        case 4: hb = ppf::tr_exact<4>(A, g, R, p); break;
        default: hb = ppf::tr_exact<5>(A, g, R, p); break;
    }
    return hb ? 1 : 0;
}

}  // extern "C"
