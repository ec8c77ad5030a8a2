// ppf_internal.hpp -- kernel argument blocks and launchers (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ppfit.h"

namespace ppf {

struct RfftArgs {
    int nbin, log2N, dtype;
    const void *in;
    const double2 *T, *T2;
    double2 *out;      // [rows][N+1]
};

struct XspecArgs {
    int nsub, nchan, nbin, log2N, kc, nblk, cb, dtype, xcd_swizzle;
    const void *data;
    const double2 *Mft;          // [nmodel][nchan][N+1]
    const int32_t *model_index;
    const uint8_t *mask;
    const double *errs;          // [nsub][nchan] or null
    const double *freqs, *P;
    const double2 *T, *T2;
    double2 *X;                  // [slot][xnh][nchan] (harmonic-major; tiled slots: xtile below)
    double *chan;                // [nsub][nchan][4]
    const double2 *spec;         // k_xspec_spec: the rows' rFFTs [nsub][nchan][N+1] (long rows)
    // wave path: model row power sum_{k>=1} |M_nk|^2 ([nmodel][nchan]) and
    // the per-sub-int "write X" flag (null: every sub-int).  Sub-ints whose
    // fit runs on moments (k_xmom) are skipped.
    const double *Mpow;
    const uint8_t *needx;        // [nsub]
    const int32_t *KC;           // [nmodel][nchan] harmonic cutoff (k_model_cut) or null: X is
                                 // written only below the cutoff of each 64-channel group
    const int32_t *xslot;        // [nsub] X slot of each sub-int (k_classify), or null: slot = s
    // tiled slots (k_xspec_w2 -> k_moments, xspec_tiled()): xtile[s] set = the
    // sub-int's slot is X[k/8][n][k%8] (one channel's 8 consecutive harmonics
    // in one 128-byte line) instead of harmonic-major; null: no tiled slot.
    // xnh: harmonics per channel of a slot, tiled or not (xtile_harm(N + 1)
    // where slots are tiled, else N + 1)
    const uint8_t *xtile;        // [nsub] or null
    int xnh;
    // GetTOAs guess spectrum fused into the wave pass (gflag[s] set, see
    // k_classify): sum_n w_n D_nk exp(2 pi i k dphi_n(DM_guess)) of the block's
    // rows for the harmonics guess_pairs() covers, per (sub-int, block)
    const uint8_t *gflag;        // [nsub] or null (no fused guess)
    double2 *gpart;              // [nsub][nblk][guess_slots(log2N)]
    double *gw;                  // [nsub][nblk][3] (sum w, count, sum w^2 errs_FT^2)
    const double *guess_weights, *guess_DM, *nu_fits;
    int guess_ref;
    // k_xspec_w2: what k_classify formed once per sub-int, read instead of
    // the byte flags and of a frequency reduction per workgroup
    const int32_t *cls;          // [nsub] kCls* bits
    const double *rec;           // [nsub][kRecN] (kRec*)
    // bounded launch of the harmonic-major instantiation (PPF_OPT_NO_X): the
    // workgroups stride over list entries x blocks; null: the full grid
    const int32_t *list;         // [*nlist] sub-ints with a harmonic-major slot
    const unsigned *nlist;
};

// k_classify's per-sub-int class bits and record
constexpr int kClsNeedX = 1, kClsTile = 2, kClsGflag = 4;
// nu_ref^-2 of the guess, Dconst DM_guess / P, usable channels, their mean frequency
constexpr int kRecNuRefM2 = 0, kRecDg = 1, kRecCnt = 2, kRecNuMean = 3, kRecN = 4;

// Fused guess harmonics of an N = 2^log2N point wave FFT: k < 64 guess_npl
// (the FFTFIT sums stop at the mean model's cutoff; a sub-int whose cutoff
// is higher takes the time-domain pass, k_dsum)
__host__ __device__ constexpr int guess_npl(int log2N) { return log2N >= 10 ? 7 : (log2N == 9 ? 3 : (log2N == 8 ? 2 : 1)); }
__host__ __device__ constexpr int guess_slots(int log2N) { return 64 * guess_npl(log2N); }

// k_dsum: GetTOAs guess profile, time-domain dedispersion (pptoas.py:461-464)
struct DsumArgs {
    int nsub, nchan, nbin, dtype, cbd, nblkd;
    int guess_ref;               // 1: dedisperse at nu_fits[s][0] (ppalign), 0: at the mean freq
    const double *nu_fits;       // [nsub][3]
    const void *data;
    const uint8_t *mask;
    const double *freqs, *P, *guess_DM, *guess_weights;
    double *gP;                  // [nsub][nblkd][nbin] partial profiles
    double *gw;                  // [nsub][nblkd][2] (sum w, count)
    const uint8_t *gflag;        // [nsub]: 1 = fused into k_xspec_w2 (skip), or null
    double *nuref;               // [nsub] nu_ref^-2 per sub-int (k_nu_ref), or null:
                                 // every workgroup reduces the frequencies itself
    // bounded launch of k_dsum_w (fused guess with PPF_OPT_NO_X): the
    // workgroups stride over list entries x blocks; null: the full grid
    const int32_t *list;         // [*nlist] sub-ints without gflag
    const unsigned *nlist;
};

// k_xmom: fused re-FFT + cross spectrum + Taylor moments (no X in HBM)
struct XmomArgs {
    int nsub, nchan, nbin, log2N, nblk, cb, dtype, xcd_swizzle, nmodel;
    const void *data;
    const double2 *Mft;
    const int32_t *model_index;
    const uint8_t *mask;
    double *chan;                // [nsub][nchan][4] (written: noise, Sd, S)
    const double *dphi;          // [nsub][nchan][2]
    const double2 *T, *T2;
    const void *state;           // TRState[nsub]
    double *mom;                 // [nsub][2][nchan][kMoments] (double2)
    const double *Bt;            // [N/2][16] folded-moment B tile (k_btab)
    int kc;                      // get_noise_PS cut
    const double *errs;          // [nsub][nchan] or null
    const double *Mpow;          // [nmodel][nchan]
    double *mres;                // [nsub][2][nchan] centre residual phi_c,n - s_n/nbin
    const int32_t *KC;           // [nchan] harmonic cutoff of the (single) model, or null
    // re-centring launches (FULL = false): the sub-ints of rc_list[0..*rc_count)
    // packed eight to a workgroup; null: every sub-int whose need_mom is set
    const unsigned *rc_count;
    const int32_t *rc_list;
};

struct GuessArgs {
    int nsub, nchan, nbin, log2N, kc, nblkd, Ns;
    int guess_ref;               // 1: the profile is already at nu_fit (no phase_transform)
    const uint8_t *mask;
    const double *freqs, *P, *guess_DM, *guess_tau, *nu_fits;
    const double *gP;            // [nsub][nblkd][nbin] (k_dsum)
    const double *gw;            // [nsub][nblkd][2]
    const double2 *T, *T2;
    double *x0;                  // [nsub][8]
    // mean model = (Msum - masked rows) / count
    const double2 *Msum;         // [nmodel][N+1]
    const double2 *Mft;
    const int32_t *model_index;
    const int32_t *KC;           // [nmodel][nchan] harmonic cutoff (k_model_cut) or null
    // fused guess spectrum (k_xspec_w2) for the sub-ints with gflag set
    const uint8_t *gflag;        // [nsub] or null
    const double2 *gpart;        // [nsub][nblk][guess_slots(log2N)]
    const double *gwx;           // [nsub][nblk][3]
    int nblk;
    // brute grid of a whole turn (Ns >= 512, ppalign's Ns = nbin) as a
    // chirp z-transform (round 6): czB = FFT_P of the chirp kernel of each of
    // the czQ output chunks of czJ points (scaled by 1/P), czT its P-point
    // twiddles; null: the direct sums
    const double2 *czB, *czT;
    int czP, czJ, czQ, czK;
    // long rows (round 6): the guess profiles' rFFTs [nsub][N+1], taken on
    // the long transforms, replace the LDS transform of the profile
    const double2 *gspec;
    // long rows whose brute grid does not fit next to the spectrum in LDS
    // (ppalign: Ns = nbin): the grid in global memory, [nsub][Ns + 8]
    double *gsh;
};

// chirp z-transform plan of a whole-turn brute grid (k_guess): Kmax
// harmonics, Ns points over [lo, lo + 1], outputs in Q chunks of J points,
// P-point transforms (P = pow2 >= Kmax + 255, J = P - Kmax + 1)
struct CzPlan {
    int Ns, K, P, J, Q;
};
hipError_t launch_cz_table(const CzPlan &c, double2 *B, const double2 *T, hipStream_t st);

struct TRState;

struct SolveArgs {
    int nsub, nchan, nbin;
    const double2 *X, *Mft;
    const double *MP;            // [nmodel][N+1][nchan] |M_nk|^2 (k = 0: 0)
    const int32_t *KC;           // [nmodel][nchan] harmonics that matter (k_model_cut)
    const int32_t *model_index;
    const double *chan;
    const double *freqs, *P;
    const uint8_t *mask;
    const double *init;
    const int32_t *fit_flags;
    const double *nu_fits, *nu_outs;
    const double *bounds;        // [nsub][5][2] (NaN: none) or null
    int log10_tau, option, is_toa, mode, max_iter, guess;
    int newton;                  // 1: scattering fits use the Newton trust region (not PPF_OPT_SCIPY_TR)
    const double *x0;
    double *stats;               // [nsub][2][nchan][10]
    ppf_result *results;
    double *scales, *scale_errs, *channel_snrs, *covariance;
    TRState *state;              // [nsub]
    double *partials;            // [nsub][pass_blocks(nchan)][21]
    unsigned *active;            // sub-ints still iterating (k_tr_step)
    unsigned *kinds;             // k_tr_init: [0] moment-mode fits, [1] streaming-pass fits
    // moment-expansion solver for fits without scattering (ppf_moments)
    double2 *mom;                // [nsub][2][nchan][kMoments]
    double *dphi;                // [nsub][nchan][2]: d phi_n / d(DM, GM)
    double *mres;                // [nsub][2][nchan]: moment-centre residual per channel
    // PPF_OPT_MOM_X: 16 moments per channel, expanded in u = (k - h_n) / h_n
    // about the centre h_n of the wave's harmonic band [0, cutoff)
    int mom16;
    double *hcen;                // [nsub][2][nchan]: h_n of each moment set (mom16)
    const int32_t *xslot;        // [nsub] X slot (k_classify; -1 none, -2 no room) or null
    const uint8_t *xtile;        // [nsub] tiled X slot (XspecArgs::xtile) or null
    int xnh;                     // harmonics per channel of an X slot (XspecArgs::xnh)
    unsigned *rc_count;          // sub-ints k_tr_mom sent back for a new moment centre
    int32_t *rc_list;            // [nsub] their indices (slot order of the atomic)
    const double *rec;           // [nsub][kRecN] (k_classify): usable channels, mean frequency
    // launch_postfit: the post-fit kernels the batch has no sub-int for
    // (kPfSkip*, from k_tr_init's kind counts; 0: both run)
    int pf_skip;
};
// k_postfit_mom takes the sub-ints without scattering and the unfitted ones,
// k_postfit the scattering fits (and everything where k_postfit_mom is skipped)
enum { kPfSkipMom = 1, kPfSkipFull = 2 };

struct RotateArgs {
    int nbin, log2N, dtype;
    const void *in;
    const double *phases;
    const double2 *T, *T2;
    double *out;
    // ref_len (odd nbin only): the reference's length-less irfft
    // (pplib.py:2466, 2508-2512, 2550, 2652): nbin - 1 samples per row from
    // X_0..X_{nbin/2}, the last as the Nyquist term; out rows of nbin - 1;
    // Te / T2e the twiddles of nbin - 1
    int ref_len;
    const double2 *Te, *T2e;
};

// Instrumental response on template rows (pptoaslib.py:124-192):
// out_r = irfft(rfft(src[src_row_r]) * table_k * sinc(k widths_r)), even nbin
struct InstRespArgs {
    int nbin;
    const double *src;           // [nsrc][nbin]
    const int32_t *src_row;      // [nrows] source row of each output row
    const double *table;         // [nbin / 2 + 1] constant-width factors, or null (ones)
    const double *widths;        // [nrows] rect width of the row [rot]; 0: factor 1
    const double2 *T, *T2;
    double *out;                 // [nrows][nbin]
};

// ppalign accumulation (ppalign.py:236-247): per channel, sum_s w_sn *
// rotate(x_sn, phase_sn), done in the frequency domain
struct AlignArgs {
    int nsub, nchan, nbin, log2N, dtype, ngroup;
    const void *in;              // [nsub][nchan][nbin]
    const double *phases;        // [nsub][nchan]
    const double *weights;       // [nsub][nchan]
    const double2 *T, *T2;
    double2 *part;               // [ngroup][nchan][N+1] partial spectra
    double *wpart;               // [ngroup][nchan] partial weight sums
    double *out;                 // [nchan][nbin] (accumulated into)
    double *wsum;                // [nchan]      (accumulated into)
};
int align_groups(int nsub, int nchan);
hipError_t launch_align(const AlignArgs &a, hipStream_t st);
bool align_wave_supported(int log2N);                                   // nbin 256..2048
hipError_t launch_align_part_w(const AlignArgs &a, hipStream_t st);
hipError_t launch_align_phases(int nsub, int nchan, const double *results, const double *freqs, const double *P,
                               const uint8_t *mask, const double *scales, const double *errs, double *phases,
                               double *weights, hipStream_t st);     // wave-per-row partials

// per-row reduced chi^2 of (rotated data - scale * model) (the channel test
// of pptoas.get_channels_to_zap, pptoas.py:1266-1343 via show_fit 1375-1480)
struct ResidArgs {
    int nbin, log2N, dtype;
    const void *in;              // [nrows][nbin]
    const double *phases;        // [nrows]
    const double *model;         // [nmodelrows][nbin]
    const int32_t *model_row;    // [nrows]
    const double *scales, *errs; // [nrows]
    double dof;
    const double2 *T, *T2;
    double *out;                 // [nrows]
};
hipError_t launch_resid_chi2(const ResidArgs &a, int64_t nrows, hipStream_t st);

struct NoiseArgs {
    int nbin, log2N, dtype, kc;
    const void *in;
    const double2 *T, *T2;
    double *out;
};

// get_noise_fit / find_kc (ppf_noisefit.hip): the brute-grid fit of the
// noise floor to the log10 power spectrum of each row
constexpr int kNfGrid = 20;     // scipy.optimize.brute's Ns (pplib.py:1550)
struct NoiseFitArgs {
    int nbin, dtype;            // k_noise_fit: the rows and their length
    const void *in;
    const double2 *T, *T2;
    int64_t nharm;              // k_spec_fit: power spectra [rows][nharm] f64
    const double *pows;
    const double *errs;         // nullptr: errs = 1; else [errs_len], errs_len 1 or nharm
    int64_t errs_len;
    int fn;                     // 0 exp_dc, 1 half_tri
    double fact;                // get_noise_fit's factor on kc
    double a_grid[kNfGrid];     // the width grid and the kc of each of its values
    int32_t kc_table[kNfGrid];
    double *noise_out;          // [rows] or nullptr (find_kc)
    int32_t *kc_out;            // [rows]
    int64_t row0;               // first output row of this launch
};

// get_noise_PS of long rows (ppf_longfft.hip): the plan of one call
struct LongNoiseArgs {
    int64_t nbin;               // real samples per row
    int64_t n;                  // complex transform length (rfft_len)
    int64_t M, M1, M2;          // four-step size M = M1 M2 (powers of two)
    int log2M, log2M1;
    int packed;                 // even nbin: two samples per complex point
    int bluestein;              // n not a power of two >= 64: chirp z-transform
    int64_t nharm, kc;          // rfft bins nbin / 2 + 1, noise cut
    int in_dtype;
    const void *in;
    int64_t row0;               // first row of this launch
};
// ppf_rotate_long: the forward (f: nbin) and inverse (b: output) Bluestein
// plans of one call
struct LongRotArgs {
    LongNoiseArgs f, b;
    int out_even;               // output of even length 2 b.n (packed inverse)
    int64_t nout;               // output samples per row
    const double *phases;       // [nrows], or null: no rotation
    // [nrows] scattering tau_n (rotations per harmonic): the spectrum times
    // 1 / (1 + 2 pi i k tau_n) (the long rows' scattered Gaussian
    // portraits); null: none
    const double *taus;
    double *out;                // [nrows][nout]
};
struct LongPassArgs {
    int64_t nbatch;
    int len, log2len;
    int64_t in_stride, in_bstride, out_stride, out_bstride, row_elems, M;
    int twiddle, inverse;
    const double2 *in;
    double2 *out;
    const double2 *T;
};

struct PhaseShiftArgs {
    int nbin, log2N, dtype, kc, Ns;
    double lo, hi;
    const void *data;
    const double *model;
    const int32_t *model_index;
    const double *noise;
    const double2 *T, *T2;
    double *out;
    // long rows (round 6): the profiles' and model rows' rFFTs ([nprof] /
    // [nmodel][N+1]) taken beforehand on the long transforms; null: LDS FFTs
    const double2 *Dspec, *Mspec;
    // their brute grid in global memory ([nprof][Ns + 8]) when it does not
    // fit next to the spectrum in LDS; null: in LDS
    double *gsh;
};

struct SynthArgs {
    int nsub, nchan, nbin, log2N, dtype;
    const double2 *Mft;          // [nchan][N+1]
    const double *freqs, *phi, *DM, *P;
    double nu_ref, noise;
    uint64_t seed;
    int64_t first;
    const double2 *T, *T2;
    void *out;
};

// ppf_fake_batch (ppf_fake.hip): simulated archive rows, quantised on the device
constexpr int kFakeI16 = 0, kFakeF64 = 1;   // PPF_FAKE_I16 / PPF_FAKE_F64
struct FakeArgs {
    int nsub, npol, nchan, nbin, nmodel, kind;
    const double2 *Mft;          // [nmodel][nchan][N+1]
    const int32_t *model_of;     // [nsub]
    const double *phase, *tau;   // [nsub][nchan]: rotation [rot], scattering time [rot]
    const double *gain;          // [nsub][npol][nchan]
    const double *noise;         // [nchan]
    uint64_t seed;
    int64_t first;
    const double2 *T, *T2;
    void *out;                   // [nsub][npol][nchan][nbin] big-endian int16 or f64
    float *scl, *offs;           // [nsub][npol * nchan] (kFakeI16)
};
hipError_t launch_fake(const FakeArgs &a, hipStream_t st);

// pptoaslib.get_scales_full (pptoaslib.py:953-971) per (sub-int, channel) row
struct ScalesArgs {
    int nsub, nchan, nharm, log10_tau;
    const double2 *D;            // [nsub][nchan][nharm] data spectra
    const double2 *M;            // [nmodel][nchan][nharm] model spectra
    const int32_t *model_index;  // [nsub] or null (model 0)
    const double *errs_FT;       // [nsub][nchan] or null (no division)
    const double *params;        // [nsub][5]
    const double *P;             // [nsub]
    const double *freqs;         // [nsub][nchan]
    const double *nus;           // [nsub][3] nu_DM, nu_GM, nu_tau
    double *out;                 // [nsub][nchan]
};
hipError_t launch_scales(const ScalesArgs &a, hipStream_t st);

// The likelihood at many parameter points (ppf_eval.hip): f, gradient,
// Hessian and the per-channel terms of ppf_eval_batch
constexpr int kEvalPointBlock = 8;   // points that share one load of a channel's spectra
constexpr int kEvalTile = 1024;      // harmonics staged in LDS at a time
constexpr int kEvalTerms = 62;       // C, S, dC[5], dS[5], d2C[5][5], d2S[5][5]
struct EvalArgs {
    int nprob, nchan, nharm, npoint, nmodel, order, log10_tau;
    const double2 *D;            // [nprob][nchan][nharm] data spectra
    const double2 *M;            // [nmodel][nchan][nharm] model spectra
    const int32_t *model_index;  // [nprob] or null (model s, or model 0 when nmodel == 1)
    const double *errs;          // [nprob][nchan] errs_FT
    const double *P;             // [nprob]
    const double *freqs;         // [nprob][nchan]
    const double *nus;           // [nprob][3] nu_DM, nu_GM, nu_tau
    const uint8_t *mask;         // [nprob][nchan] or null
    const double *theta;         // [nprob][npoint][5]
    const double *flags;         // [5] or null (all 1)
    double *part;                // workspace: [nprob][npoint][nchan][1 | 6 | 21]
    double *f, *g, *H;           // [nprob][npoint] ([5], [5][5]); g / H unused below their order
    double *terms;               // [nprob][npoint][kEvalTerms][nchan] or null
};
int64_t eval_partials(int64_t nprob, int64_t nchan, int64_t npoint, int order);   // doubles in part
hipError_t launch_eval(const EvalArgs &a, hipStream_t st);

// PSRFITS fast path (ppf_psrfits.hip): raw SUBINT DATA bytes -> float32
// rows (total intensity, or all four polarisations), baseline window,
// per-row statistics
struct UnpackArgs {
    int nsub, npol, nchan, nbin;
    int elem;                    // 0 big-endian int16, 1 uint8, 2 big-endian float32
    int npol_out;                // 1: total intensity; 4: full polarisation (npol = 4)
    int pol_mode;                // npol_out 1.  0: pol 0 (npol 1, IQUV); 1: AA + BB
    int conv;                    // npol_out 4.  0..5 (include/ppfit.h)
    int rm_baseline, win;        // subtract the off-pulse mean; window bins
    const uint8_t *raw;          // [nsub] blocks of sub_stride bytes
    int64_t sub_stride;
    const float *scl, *offs;     // [nsub][npol * nchan]
    const float *wts;            // [nsub][nchan] or null
    float *out;                  // [nsub][npol_out][nchan][nbin]
    double *part;                // [nsub][nblk][nbin] workspace
    double *total;               // [nsub][nbin]
    int32_t *wstart;             // [nsub]
    double *stats;               // [nsub][npol_out][nchan][3]: off mean, off sigma, S/N
};
hipError_t launch_unpack(const UnpackArgs &a, hipStream_t st);
hipError_t launch_copy_host(const void *src_dev, void *dst, int64_t nbytes, hipStream_t st);
size_t unpack_partials(int nsub, int nchan, int nbin);

// ppf_pack_psrfits_batch (ppf_pack.hip): float rows -> SUBINT DATA bytes
struct PackArgs {
    int64_t nrow;
    int nbin;
    int f32in;                   // rows are float32 (else float64)
    int elem;                    // 0 big-endian int16, 2 big-endian float32
    const void *rows;            // [nrow][nbin]
    uint8_t *raw;                // [nrow][nbin * esize]
    float *scl, *offs;           // [nrow]
};
hipError_t launch_pack(const PackArgs &a, hipStream_t st);

// pplib.gen_gaussian_portrait (pplib.py:886-963) per (portrait, channel) row
struct GaussArgs {
    int nport, nchan, nbin, log2N, ngauss, npar;
    int code[3];                 // evolution code per (loc, wid, amp): 0 power law, 1 linear
    const double *params;        // [nport][npar]: dc, tau [bin], ngauss x (loc, mloc, wid, mwid, amp, mamp)
    const double *scat_index;    // [nport]
    const double *freqs;         // [nport][nchan]
    const double *nu_ref;        // [nport]
    const double2 *T, *T2;
    const double2 *Te, *T2e;     // odd nbin: the twiddles of nbin - 1 (the scattered rows' irfft)
    double *out;                 // [nport][nchan][nbin] (odd nbin, tau != 0: nbin - 1 bins, then 0)
    // long rows: the unscattered rows, and each row's tau_n here for the
    // convolution on the long transforms (0: unscattered); null: in LDS
    double *taus_out;
};
hipError_t launch_gauss_port(const GaussArgs &a, hipStream_t st);

// ppf_gauss_lsq_batch (ppf_gaussfit.hip): the Gram matrix of the
// forward-difference Jacobian columns and the residual of the Gaussian
// portrait model
constexpr int kGramSeg = 1024;   // bins of one channel per Gram workgroup (one K chunk)
constexpr int kGramMaxCol = 128; // nfree + 1 <= 8 tiles of 16
struct GaussLsqArgs {
    int nfit, nchan, nbin, ngauss, npar, nfree, dtype;
    int ntile, npair, nseg;      // 16-row tiles of nfree + 1, upper-triangle pairs, chunks per channel
    int code[3];
    const double *params;        // [nfit][npar]
    const double *scat_index;    // [nfit]
    const double *freqs;         // [nfit][nchan]
    const double *nu_ref;        // [nfit]
    const int32_t *free_idx;     // [nfree] (device copy)
    const double *delta;         // [nfit][nfree] (device copy)
    const void *data;            // [nfit][nchan][nbin] in dtype
    const double *inv_errs;      // [nfit][nchan][nbin]
    const double2 *T, *T2;
    double *rows;                // [nfit][nchan][nfree + 1][nbin]: m(p + delta_j e_j), last m(p)
    double *part;                // [nfit][nchan * nseg][npair][256] partial tiles
    double *gram;                // [nfit][nfree + 1][nfree + 1]
};
hipError_t launch_gauss_lsq(const GaussLsqArgs &a, hipStream_t st);

// The joined model (gen_gaussian_portrait's join_ichans, pplib.py:956-962):
// the rows of archive a = join_id[row] are rotated by phi_a + Dconst DM_a /
// P (nu^-2 - nu_ref^-2).  A second kernel argument of the joined kernels
// (ppf_gaussfit.hip), so GaussArgs / GaussLsqArgs and the unjoined kernels
// stay as they are.  The extended parameter vector of the joined fit is
// [params (npar), join_params (2 njoin), scattering index].
struct GaussJoin {
    int njoin;
    const int32_t *join_id;      // [nport | nfit][nchan] (device copy): archive, -1 = not rotated
    const double *join_params;   // [nport | nfit][2 njoin]: phase [rot], DM per archive
    const double *P;             // [nport | nfit] period [s]
};
hipError_t launch_gauss_port_join(const GaussArgs &a, const GaussJoin &j, hipStream_t st);
hipError_t launch_gauss_lsq_join(const GaussLsqArgs &a, const GaussJoin &j, hipStream_t st);

// ppf_swt_analyse_batch / ppf_swt_score_batch (ppf_swt.hip): the stationary
// db8 wavelet transform of profiles and the denoise-and-score cases of
// pplib.smart_smooth
struct SwtArgs {
    int nprof, nbin, nlevel, kc, ncase;
    bool pow2;                   // nbin a power of two (else nlevel == 1)
    double sq2ln;                // sqrt(2 ln nbin)
    const double *prof;          // [nprof][nbin]
    double *coef;                // [nprof][nlevel][2][nbin]: a_j, d_j
    double *med;                 // [nprof][nlevel]: median(|a_j| u |d_j|)
    double *noise;               // [nprof]: get_noise_PS of the profile
    const int32_t *cases;        // [ncase][3] (device copy): profile, level, soft
    const double *fact;          // [ncase] (device copy)
    double *out;                 // [ncase][3]: signal, noise, red_chi2
    double *smooth;              // [ncase][nbin] or null
    const double2 *T, *T2;
    // k_swt_search only
    int ngrid, soft;
    double rchi2_tol;
    const double *grid;          // [ngrid] (device copy)
    const double *table;         // [nprof][nlevel][ngrid][3]: k_swt_score's out at the grid points
    double *fact_min, *fun_min;  // [nprof][nlevel]
    int32_t *nfev;               // [nprof][nlevel]
};
hipError_t launch_swt_analyse(const SwtArgs &a, hipStream_t st);
hipError_t launch_swt_score(const SwtArgs &a, hipStream_t st);
hipError_t launch_swt_search(const SwtArgs &a, hipStream_t st);

// pplib.gen_spline_portrait (pplib.py:966-990): per (portrait, channel) row,
// splev of the B-spline curve tck at the channel frequency (FITPACK splev /
// fpbspl, ext = 0), the eigenvector expansion plus the mean profile, and
// (nbin != nbin_model) scipy.signal.resample to nbin followed by the
// half-bin rotate_portrait of the reference
struct SplineArgs {
    int nport, nchan, nbin_model, nbin, ncomp, nknots, degree;
    int log2N0, log2N1;          // log2 of the half lengths (model, output)
    const double *mean_prof;     // [nbin_model]
    const double *eigvec;        // [nbin_model][ncomp]
    const double *knots;         // [nknots]
    const double *coefs;         // [ncomp][nknots]  (splprep c, zero-padded)
    const double *freqs;         // [nport][nchan]
    const double2 *T0, *T20;     // twiddles of nbin_model
    const double2 *T1, *T21;     // twiddles of nbin
    double *out;                 // [nport][nchan][nbin]
};
constexpr int kSplineMaxComp = 64;
constexpr int kSplineMaxDeg = 5;
hipError_t launch_spline_port(const SplineArgs &a, hipStream_t st);

hipError_t launch_twiddles(int N, double2 *T, double2 *T2, hipStream_t st);
hipError_t launch_rfft_rows(const RfftArgs &a, int64_t nrows, hipStream_t st);
hipError_t launch_xspec(const XspecArgs &a, hipStream_t st);
hipError_t launch_guess(const GuessArgs &a, hipStream_t st);
hipError_t launch_dsum(const DsumArgs &a, hipStream_t st);
bool xspec_wave_supported(int log2N, int cb);
// channels per workgroup of the spectrum pass where it has a block size of
// its own (k_xspec_w2: 64), else 0: the layout's
int xspec_own_cb(int log2N);
// wave-per-row mixed-radix spectrum pass (k_xspec_wm): nbin / 2 not a power
// of two, <= 1024 (prime factors above 7 on the generic-radix stage)
bool xspec_wm_supported(int nbin);
// the spectrum pass accumulates the GetTOAs guess at this FFT size (k_classify: gflag)
bool xspec_guess_fused_n(int log2N);
hipError_t launch_xspec_wm(const XspecArgs &a, hipStream_t st);
hipError_t launch_xspec_wave(const XspecArgs &a, hipStream_t st);
hipError_t launch_xmom(const XmomArgs &a, bool full, hipStream_t st);
hipError_t launch_btab(int N, double *Bt, hipStream_t st);
// k_classify: per sub-int, which stream the cross spectrum and in which slot,
// whether the guess rides in the spectrum pass, and the scalars every later
// kernel would otherwise reduce from the frequency list again
struct ClassifyArgs {
    int nsub, nchan, log10_tau, fused, xcap;
    const int32_t *fit_flags;
    const double *init, *freqs, *P, *nu_fits;
    const uint8_t *mask;
    const int32_t *model_index;
    const int32_t *KC;           // [nmodel][nchan]
    int klim;                    // gflag: max_n KC <= klim; < 0: no fused guess (gflag null)
    const double *guess_DM;      // or null (no guess)
    int guess_ref;
    uint8_t *needx;              // [nsub]
    int32_t *xslot;              // [nsub]
    uint8_t *xtile;              // [nsub] or null: 1 = tiled slot (moment mode), 0 = k_pass streams it
    uint8_t *gflag;              // [nsub] or null
    int32_t *cls;                // [nsub] kCls* bits
    double *rec;                 // [nsub][kRecN]
    // the sub-ints with a harmonic-major slot (needx, not tiled) and those
    // without gflag, in sub-int order, with their counts
    int32_t *hm_list, *ng_list;
    unsigned *counts;            // [0] arrival ticket (zero on entry), [1] hm, [2] ng
};
hipError_t launch_classify(const ClassifyArgs &a, hipStream_t st);
// k_xspec_w2 writes the moment-mode sub-ints' X tiled (X[k/8][n][k%8]) for
// k_moments at this FFT size (1024-point rows)
bool xspec_tiled(int log2N);
// harmonics per channel of a tiled slot: whole tiles of 8
constexpr int kXTile = 8;
inline int64_t xtile_harm(int64_t nharm) { return (nharm + kXTile - 1) / kXTile * kXTile; }
hipError_t launch_model_pow(const double2 *Mft, int nchan, int nharm, int nmodel, double *out,
                            hipStream_t st);
hipError_t launch_model_sum(const double2 *Mft, int nchan, int nharm, int nmodel, double2 *out,
                            hipStream_t st);
hipError_t launch_tr_init(const SolveArgs &a, hipStream_t st);
hipError_t launch_pass(const SolveArgs &a, hipStream_t st);
hipError_t launch_tr_step(const SolveArgs &a, hipStream_t st);
hipError_t launch_moments(const SolveArgs &a, hipStream_t st);
hipError_t launch_tr_mom(const SolveArgs &a, hipStream_t st);
constexpr int kMoments = 32;     // Taylor moments per channel
// Newton trust region of the scattering fits (ppf_solve.hip tr_update_newton):
// initial radius in Jacobi-scaled units (~sigma), and the predicted reduction
// of the objective (chi^2 units) below which the fit has converged
constexpr double kNewtonR0 = 10.0;
constexpr double kNewtonTol = 1e-12;
// its warm start on a channel subset (every sub-th group of 64 channels;
// scattering fits with >= 256 channels): leave it for every channel once an
// interior step predicts less than kSubsetSwitch (chi^2 units of the subset)
constexpr double kSubsetSwitch = 1.0;
constexpr int kSubsetMaxStride = 16;
hipError_t launch_postfit(const SolveArgs &a, hipStream_t st);
size_t tr_state_bytes();
int pass_blocks(int nchan);
hipError_t launch_rotate(const RotateArgs &a, int64_t nrows, hipStream_t st);
hipError_t launch_inst_resp(const InstRespArgs &a, int64_t nrows, hipStream_t st);
hipError_t launch_noise(const NoiseArgs &a, int64_t nrows, hipStream_t st);
int lf_pow_blocks(const LongNoiseArgs &a);
hipError_t launch_chirp_ft(const LongNoiseArgs &a, double2 *Bf, double2 *Bs, const double2 *T1,
                           const double2 *T2, hipStream_t st);
hipError_t launch_rfft_long(const LongNoiseArgs &f, int64_t nrows, double2 *A, double2 *Y, const double2 *Bf,
                            double2 *out, const double2 *T1, const double2 *T2, hipStream_t st);
hipError_t launch_xspec_spec(const XspecArgs &a, hipStream_t st);
hipError_t launch_gsum(int nsub, int nblkd, int nbin, const double *gP, double *prof, hipStream_t st);
hipError_t launch_rotate_long(const LongRotArgs &r, int64_t nrows, double2 *A, double2 *Y, const double2 *Bff,
                              const double2 *Bfb, const double2 *T1f, const double2 *T2f, const double2 *T1b,
                              const double2 *T2b, hipStream_t st);
hipError_t launch_noise_long(const LongNoiseArgs &a, int64_t nrows, double2 *A, double2 *Y,
                             const double2 *Bf, double *part, double *out, const double2 *T1,
                             const double2 *T2, hipStream_t st);
// the power spectra |F_k|^2 / nbin, k < nharm, of the rows launch_noise_long
// would reduce -> pows [nrows][nharm] (ppf_noise_fit_long)
hipError_t launch_pows_long(const LongNoiseArgs &a, int64_t nrows, double2 *A, double2 *Y,
                            const double2 *Bf, double *pows, const double2 *T1, const double2 *T2,
                            hipStream_t st);
// get_noise_fit per row in LDS (k_noise_fit) / from power spectra (k_spec_fit)
hipError_t launch_noise_fit(const NoiseFitArgs &a, int64_t nrows, hipStream_t st);
hipError_t launch_spec_fit(const NoiseFitArgs &a, int64_t nrows, hipStream_t st);
// wave-per-row noise (k_noise_w) for N = nbin/2 = 128..1024
bool noise_wave_supported(int log2N);
hipError_t launch_noise_wave(const NoiseArgs &a, int64_t nrows, hipStream_t st);
hipError_t launch_phase_shift(const PhaseShiftArgs &a, int nprof, hipStream_t st);
hipError_t launch_synth(const SynthArgs &a, hipStream_t st);
// per (model, channel): 1 + the last harmonic with |M_k|^2 > kCutRel max_k |M_k|^2
constexpr double kCutRel = 1e-28;   // |M_k| < 1e-14 max|M|: below the template's own FFT rounding floor
hipError_t launch_model_cut(const double *MP, int nchan, int nharm, int nmodel, bool off,
                            int32_t *KC, hipStream_t st);
hipError_t launch_model_pow_t(const double2 *Mft, int nchan, int nharm, int nmodel, double *MP,
                              hipStream_t st);

}  // namespace ppf
