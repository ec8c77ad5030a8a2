/*
 * ppfit.h -- C ABI of libppfit, the MI355X (gfx950) wideband FFTFIT engine.
 *
 * Drop-in boundary for the PulsePortraiture hot path.
 * The reference has no FFI: each entry point below replaces a Python/NumPy
 * routine of the reference and is bound from Python with ctypes
 * (pulseportraiture_amd/_lib.py; see INTEGRATION.md for the binding a
 * PulsePortraiture maintainer would add).
 *
 * Conventions
 *   - Every array pointer is a DEVICE pointer (hipMalloc / torch.cuda memory)
 *     unless stated otherwise; arrays are C-contiguous.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     calls are asynchronous on that stream; they never synchronise the
 *     device and never allocate device memory except the per-context
 *     twiddle-table cache (created on first use of an nbin).
 *   - Return value: PPF_OK (0) or a negative PPF_E* code; ppf_last_error()
 *     gives the message.  Per-sub-integration numerical outcomes are reported
 *     in ppf_result.status, never by aborting the batch.
 *   - nbin: even 32..8192 or odd 33..4095 (nbin/2 not a power of two: the
 *     mixed-radix LDS FFT, a generic-radix stage for prime factors above 7;
 *     odd nbin: the row transformed as nbin complex points on the same
 *     stages); other nbin returns PPF_EUNSUP.  Powers of two
 *     in [256, 2048] take the wave-per-row kernels.
 *   - Threads: ppf_fit_batch / ppf_fit2_batch must not run concurrently on
 *     the same context (they share its profiling event ring and pinned
 *     iteration counter); any other entry point may run on another host
 *     thread beside them (GetTOAs builds templates with
 *     ppf_gauss_portrait_batch while a worker thread fits).  The twiddle
 *     cache and the error message are guarded; ppf_last_error returns the
 *     message as last set by any thread, copied for the calling thread.
 */
#ifndef PPFIT_H
#define PPFIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 4 (round 5): the options PPF_OPT_MOM_X / PPF_OPT_FUSED_MOM, elem = 3
 * of ppf_unpack_psrfits_batch, PPF_EIO, ppf_read_rows and
 * ppf_copy_from_pinned (added in round 4 without a bump), and
 * ppf_kernel_ms_history slot 0 = the first moment pass of either kind;
 * ppf_solver_ms_history, ppf_host_copy. */
/* ABI 5 (round 6): ppf_rotate_batch_ref. */
/* ABI 6 (round 6): ppf_noise_long, ppf_rotate_long (+ their workspace
 * queries), ppf_align_phases, PPF_OPT_SPIN_WAIT; ppf_fit_batch /
 * ppf_gauss_portrait_batch / ppf_phase_shift_batch accept nbin past the LDS
 * transforms (even > 8192, odd > 4095) on the long transforms.
 * ppf_inst_response_batch, ppf_pack_psrfits_batch and
 * ppf_unpack_psrfits_pol_batch were added later without
 * a bump (purely additive: no structure or existing signature changed). */
#define PPF_ABI_VERSION 6

enum ppf_error {
    PPF_OK = 0,
    PPF_EINVAL = -1,   /* bad argument / shape */
    PPF_EHIP = -2,     /* HIP runtime error */
    PPF_ENOMEM = -3,   /* workspace too small */
    PPF_EUNSUP = -4,   /* unsupported configuration (e.g. nbin) */
    PPF_EIO = -5       /* file read failed or came up short */
};

enum ppf_dtype { PPF_F32 = 0, PPF_F64 = 1 };

/* ppf_result.status values (low byte = scipy trust-region warnflag) */
enum ppf_status {
    PPF_ST_SUCCESS = 0,      /* gradient test met (never, gtol = -1)        */
    PPF_ST_MAXITER = 1,      /* iteration cap reached                        */
    PPF_ST_CONVERGED = 2,    /* predicted reduction <= 0 (the usual stop)    */
    PPF_ST_LINALG = 3,       /* subproblem failure                           */
    PPF_ST_NO_ROOT = 0x100,  /* no positive real zero-covariance root:
                                the reference raises ValueError here         */
    PPF_ST_SINGULAR = 0x200, /* singular covariance (LinAlgError)            */
    PPF_ST_NONFINITE = 0x400,/* non-finite objective encountered             */
    PPF_ST_NOFIT = 0x800,    /* no parameter to fit / no usable channel      */
    PPF_ST_NOSPACE = 0x1000  /* the fit streams the cross spectrum but the
                                workspace holds fewer X slots (x_subints)    */
};
/* Degenerate sub-integrations end alone; the rest of the batch is fitted as
 * without them (tests/test_gpu_degenerate.py).
 *   - PPF_ST_NOFIT (no fit flag set, or no usable channel) and PPF_ST_NOSPACE:
 *     status holds exactly that value and the record is all zeros except
 *     status and phi_guess (the initial phase the fit would have used; the
 *     caller's init[0] where the guess stage had no channel to form one
 *     from).  Every field is finite.  scales, scale_errs and channel_snrs of
 *     the sub-int are written as 0; its covariance block is NOT written: a
 *     caller that reads it must have zeroed the array (engine.fit_batch
 *     does).
 *   - The values of a masked channel (chan_mask == 0) -- its data row, errs,
 *     guess_weights -- are never read into any result, whatever they hold
 *     (NaN, Inf, stale numbers): the outputs are bitwise those of the same
 *     call with ordinary values there.
 *   - A non-finite sample, or a channel whose noise is zero (errs == 0, or
 *     estimated from a row of zeros), in a USED channel ends that sub-int
 *     with PPF_ST_NONFINITE set (the reference raises from SciPy's
 *     finiteness check there); its parameter values are not meaningful. */

/* ppf_fit_desc.options bits */
enum ppf_option {
    PPF_OPT_NO_HCUT = 1,     /* sum every harmonic: no per-channel cutoff of
                                the harmonics whose template power is below
                                1e-28 of the channel's peak */
    PPF_OPT_NO_X = 2,        /* the caller has checked that no sub-int
                                streams the cross spectrum (no scattering
                                flag, zero initial tau): on the fused
                                phase+DM path no X slot is reserved, the
                                cross-spectrum pass is not launched and the
                                host does not read back which kinds of fit
                                the batch holds (a sub-int that would need X
                                ends with PPF_ST_NOSPACE).  Everywhere else
                                (block-FFT and long rows, moments from X:
                                PPF_OPT_MOM_X or its default) the option
                                changes no result: every sub-int holds an X
                                slot and a scattering sub-int is fitted as
                                without it; the host only learns of such a
                                sub-int with the first read-back of its
                                iteration loop instead of before it */
    PPF_OPT_SCIPY_TR = 4,    /* the fits follow scipy's trust-ncg path
                                step by step (pptoaslib.py:1055-1060:
                                radius 1 in raw parameter units,
                                CG-Steihaug subproblem).  Default: the
                                Newton trust region (Jacobi-scaled
                                coordinates, exact subproblem), which stops
                                at the same stationary point, closer (the
                                reference's Newton decrement at its end
                                point reaches 6e-6, this one's 1e-20), in
                                fewer evaluations: scattering fits 3x fewer
                                passes over the cross spectrum, ppalign
                                fits half the data passes.
                                Bounded (method='TNC') fits always take the
                                scipy path with projected steps. */
    PPF_OPT_MOM_X = 8,       /* phase/DM/GM fits on the wave-FFT shapes take
                                their Taylor moments from the cross spectrum
                                X (one spectrum pass writing X below the
                                harmonic cutoff, then k_moments: 16 moments
                                about the centre of each channel band's
                                harmonics), instead of the fused pass that
                                re-FFTs the data rows for every moment
                                centre (k_xmom_g): every sub-int then holds
                                an X slot (x_subints and PPF_OPT_NO_X are
                                overridden: nsub * nchan * (nbin/2 + 1) * 16
                                bytes of workspace, 8.4 MB per 512 x 2048
                                sub-int; ppf_fit_workspace_bytes includes
                                it.  At nbin = 2048 the slots of the fits
                                without scattering are tiled, 8 consecutive
                                harmonics of a channel per 128-byte line, and
                                every slot holds the harmonics rounded up to
                                whole tiles: nsub * nchan * 1032 * 16 bytes).
                                Default (neither this nor
                                PPF_OPT_FUSED_MOM) where the GetTOAs guess
                                rides along in the spectrum pass: guess != 0
                                and nbin = 2048 */
    PPF_OPT_FUSED_MOM = 16,  /* force the fused k_xmom_g pass (no X for the
                                phase/DM/GM fits) */
    PPF_OPT_SPIN_WAIT = 32   /* (ABI 6) the call's read-backs of the count
                                of fits still iterating are polled on the
                                host instead of waited for with
                                hipStreamSynchronize: 30-70 us less per
                                read-back, for a caller with no host threads
                                of its own competing for the cores (ppalign:
                                C4 +2-3 %; GetTOAs' readers and stagers lost
                                up to 20 % to it) */
};

enum ppf_mode {
    PPF_MODE_FULL = 0,    /* pptoaslib.fit_portrait_full semantics */
    PPF_MODE_LEGACY2 = 1  /* pplib.fit_portrait semantics (phase + DM)  */
};

/* One fixed-size record per sub-integration (all doubles, 32 of them). */
typedef struct ppf_result {
    double params[5];      /* phi_out, DM, GM, tau_out, alpha               */
    double param_errs[5];
    double nu_out[3];      /* nu_DM, nu_GM, nu_tau of the reported params   */
    double nu_fit[3];      /* reference frequencies used inside the fit     */
    double chi2, red_chi2, snr;
    double fun;            /* objective at the fit (chi2 - Sd)              */
    double Sd;             /* data power term                               */
    double phi_guess;      /* initial phase actually used                   */
    double nfeval;         /* objective evaluations (scipy nfev)            */
    double status;         /* ppf_status bits                               */
    double niter;          /* trust-region iterations                       */
    double dof;
    double nchanx;         /* channels used                                 */
    double x_fit_phi;      /* phi at nu_fit (before output transform)      */
    double x_fit_tau;      /* tau parameter at nu_fit                       */
    double npass;          /* streaming passes over the cross spectrum      */
    double reserved[2];
} ppf_result;

/* Batched wideband fit: replaces pptoaslib.fit_portrait_full
 * (pptoaslib.py:974-1144) per sub-integration, plus -- when guess != 0 --
 * the initial-phase stage of pptoas.GetTOAs.get_TOAs (pptoas.py:461-499),
 * and with mode == PPF_MODE_LEGACY2 pplib.fit_portrait (pplib.py:2185-2287). */
typedef struct ppf_fit_desc {
    int32_t nsub, nchan, nbin;
    int32_t data_dtype;           /* PPF_F32 or PPF_F64                        */
    const void *data;             /* [nsub][nchan][nbin]                       */
    const double *model;          /* [nmodel][nchan][nbin]                     */
    int32_t nmodel;
    const int32_t *model_index;   /* [nsub] or NULL (all use model 0)          */
    const uint8_t *chan_mask;     /* [nsub][nchan], 1 = use; NULL = all        */
    const double *freqs;          /* [nsub][nchan] MHz                         */
    const double *P;              /* [nsub] s                                  */
    const double *errs;           /* [nsub][nchan] time-domain sigma, or NULL:
                                     estimated as pplib.get_noise_PS           */
    const double *init;           /* [nsub][5] initial params                  */
    const int32_t *fit_flags;     /* [nsub][5]                                 */
    const double *nu_fits;        /* [nsub][3]; NaN -> mean(freqs)             */
    const double *nu_outs;        /* [nsub][3]; NaN -> zero-covariance freq    */
    int32_t log10_tau;
    int32_t option;               /* get_nu_zeros option (GM cases)            */
    int32_t is_toa;
    int32_t mode;                 /* ppf_mode                                  */
    int32_t max_iter;             /* <= 0: reference default 200 * 5           */
    /* optional initial-phase stage (GetTOAs): phi_guess from the weighted,
       DM-dedispersed mean profile (brute grid of guess_Ns points + fmin) */
    int32_t guess;
    const double *guess_weights;  /* [nsub][nchan]                             */
    const double *guess_DM;       /* [nsub] DM used to dedisperse              */
    const double *guess_tau;      /* [nsub] scattering time [rot] applied to the
                                     mean model profile (pptoas.py:484-489), or
                                     NULL for none                             */
    int32_t guess_Ns;
    /* outputs */
    ppf_result *results;          /* [nsub]                                    */
    double *scales;               /* [nsub][nchan] (0 for masked channels)     */
    double *scale_errs;           /* [nsub][nchan]                             */
    double *channel_snrs;         /* [nsub][nchan]                             */
    double *covariance;           /* [nsub][5][5], fit block in leading corner */
    void *workspace;
    size_t workspace_bytes;
    /* ABI 2 */
    int32_t x_subints;            /* cross-spectrum (X) slots the workspace
                                     holds: the number of sub-ints whose fit
                                     streams X (scattering fits: fit_flags[3]
                                     or [4] set, or a nonzero initial tau).
                                     <= 0: nsub.  Sub-ints past it end with
                                     PPF_ST_NOSPACE.  Off the fused phase+DM
                                     path (nbin outside 256..2048) every
                                     sub-int streams X and nsub slots are
                                     always reserved. */
    int32_t options;              /* ppf_option bits                           */
    int32_t guess_ref;            /* frame of the guess stage's dedispersed
                                     mean profile: 0 = the mean usable
                                     frequency, phase then moved to nu_fit
                                     (GetTOAs, pptoas.py:461-499); 1 = nu_fit
                                     itself (ppalign, ppalign.py:214-219) */
    /* ABI 3 */
    const double *bounds;         /* [nsub][5][2] lower, upper bound of each
                                     parameter (NaN: none), or NULL for an
                                     unbounded fit.  method='TNC' of
                                     fit_portrait_full / get_TOAs
                                     (pptoaslib.py:1041-1053, pptoas.py:503-513):
                                     the initial point is clipped into the box
                                     and the trust-region steps are projected
                                     (parameters at a bound whose descent
                                     direction leaves the box are held there,
                                     the step over the others is cut at the
                                     first bound it crosses), so the fit ends
                                     at the bounded stationary point. */
} ppf_fit_desc;

int ppf_abi_version(void);
/* sizeof(ppf_fit_desc) / sizeof(ppf_result) as compiled, for FFI layout checks */
size_t ppf_sizeof_fit_desc(void);
size_t ppf_sizeof_result(void);

/* context: one per device; owns twiddle tables and the error string */
typedef struct ppf_ctx ppf_ctx;
int ppf_create(int device, ppf_ctx **out);
void ppf_destroy(ppf_ctx *ctx);
const char *ppf_last_error(const ppf_ctx *ctx);

/* Stage timing with HIP events recorded on the caller's stream around each
 * kernel of ppf_fit_batch (model rfft, xspec, guess, solve).  Off by
 * default; ppf_last_stage_ms waits for the last call's events and returns
 * the four stage durations in milliseconds (0 for a skipped stage). */
int ppf_set_profiling(ppf_ctx *ctx, int enable);
int ppf_last_stage_ms(ppf_ctx *ctx, double *ms4);
/* The stage times of the last n (<= 256) profiled ppf_fit_batch calls,
 * oldest first, into ms[n][4]; returns the number written.  Events are kept
 * in a ring, so a timed loop records without synchronising. */
int ppf_stage_ms_history(ppf_ctx *ctx, int n, double *ms);
/* Single-kernel times of the last n profiled ppf_fit_batch calls into
 * ms[n][2]: [0] the call's first moment pass over every moment-mode sub-int
 * -- the fused k_xmom_g over the data rows, or, on the moments-from-X path
 * (PPF_OPT_MOM_X, and the GetTOAs default at nbin 2048), k_moments over the
 * stored cross spectrum; 0 if the call had none -- and [1] the separate
 * guess-profile pass (k_dsum_w; 0 without a guess or when the guess rides in
 * the spectrum pass).  The spectrum pass itself (k_xspec_w) is stage [1] of
 * ppf_stage_ms_history.  Same event ring as ppf_stage_ms_history. */
int ppf_kernel_ms_history(ppf_ctx *ctx, int n, double *ms);
/* The streaming passes (k_pass: one trust-region evaluation of every
 * scattering fit still iterating) of the last n profiled ppf_fit_batch calls
 * into ms[n][2]: [0] their summed duration in ms (HIP events around each
 * launch), [1] the number of launches. */
int ppf_pass_ms_history(ppf_ctx *ctx, int n, double *ms);
/* The solver kernels of the last n profiled ppf_fit_batch calls into
 * ms[n][6] (ABI 4): summed ms and launch count of k_tr_mom (the moment-path
 * trust-region iterations), of k_tr_step (+ k_tr_gates; the scattering
 * path's update), and of k_postfit (zero-covariance frequencies, output
 * transform, covariance, scales), each launch bracketed by HIP events. */
int ppf_solver_ms_history(ppf_ctx *ctx, int n, double *ms);

/* Workspace needed by ppf_fit_batch for `desc` (only sizes/flags are read). */
size_t ppf_fit_workspace_bytes(const ppf_fit_desc *desc);

/* pptoaslib.fit_portrait_full (pptoaslib.py:974) / pptoas.get_TOAs inner loop
 * (pptoas.py:384-533) / pplib.fit_portrait (pplib.py:2185). */
int ppf_fit_batch(ppf_ctx *ctx, const ppf_fit_desc *desc, void *stream);

/* Same as ppf_fit_batch with desc->mode forced to PPF_MODE_LEGACY2:
 * pplib.fit_portrait (pplib.py:2185-2287). */
int ppf_fit2_batch(ppf_ctx *ctx, const ppf_fit_desc *desc, void *stream);

/* Rotate rows: out_r = irfft(rfft(in_r) * exp(2 pi i k phase_r)).
 * Replaces the FFT core of pplib.rotate_data (pplib.py:2427-2515),
 * pplib.rotate_portrait (2518-2550), pplib.rotate_profile (2641-2652) and
 * pptoaslib.rotate_portrait_full (pptoaslib.py:61-90); the host computes the
 * per-row phase phase + Dconst*DM/P*(nu**-2 - nu_ref**-2) exactly as those
 * routines do.  in: [nrows][nbin] of in_dtype; phases: [nrows] double;
 * out: [nrows][nbin] double. */
int ppf_rotate_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin,
                     int32_t in_dtype, const void *in, const double *phases,
                     double *out, void *stream);

/* ppf_rotate_batch with the reference's output length (ABI 5): the public
 * rotate routines call numpy's irfft WITHOUT a length (pplib.py:2466,
 * 2508-2512, 2550, 2652; pptoaslib.py:89), which at odd nbin returns
 * nbin - 1 samples: the inverse of length nbin - 1 of X_0..X_{nbin/2}, the
 * last harmonic taken as the Nyquist term (its imaginary part dropped).
 * out: [nrows][nbin] at even nbin (identical to ppf_rotate_batch),
 * [nrows][nbin - 1] at odd nbin. */
int ppf_rotate_batch_ref(ppf_ctx *ctx, int64_t nrows, int32_t nbin,
                         int32_t in_dtype, const void *in, const double *phases,
                         double *out, void *stream);

/* Instrumental response on template rows (added within ABI 6: a library
 * without the symbol is a stale build):
 *   out_r = irfft(rfft(src[src_row[r]]) * table[k] * sinc(k * widths[r]))
 * with sinc(x) = sin(pi x) / (pi x).  Replaces the convolution of
 * pptoas.py:428-434, 983-989 and 1446-1452 with the multiplier of
 * pptoaslib.instrumental_response_port_FT (pptoaslib.py:158-192): table is
 * the product of its constant-width factors (wids / irf_types), widths[r] the
 * row's dispersive-smearing rectangle 8.3e-6 chan_bw / (nu_r / 1e3)**3 / P
 * [rot] (0: no such factor).  src_row lets one template portrait fan out into
 * its several (P, chan_bw) variants in one launch; every src_row[r] must
 * index a row of src (not checked on the device).  DC and Nyquist terms keep
 * their real parts only, as numpy.fft.irfft does.
 * src: [nsrc][nbin] double; src_row: [nrows] int32; table: [nbin / 2 + 1]
 * double, or NULL for all ones; widths: [nrows] double; out: [nrows][nbin]
 * double (must not overlap src).  Even nbin the LDS transforms take
 * (32..8192); odd nbin and longer rows return PPF_EUNSUP. */
int ppf_inst_response_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin,
                            const double *src, const int32_t *src_row,
                            const double *table, const double *widths,
                            double *out, void *stream);

/* ppalign.align_archives accumulation (ppalign.py:236-247, the inner
 * "aligned_port += weights * rotate_data(...)" / "total_weights += weights"
 * over every sub-integration of every archive):
 *   out[n][:] += sum_s w[s][n] * irfft(rfft(in[s][n]) * exp(2 pi i k ph[s][n]))
 *   wsum[n]   += sum_s w[s][n]
 * Rows with w == 0 are skipped.  in: [nsub][nchan][nbin] (in_dtype);
 * phases, weights: [nsub][nchan]; out: [nchan][nbin] f64; wsum: [nchan].
 * The sum over sub-ints is taken in a fixed order (bitwise reproducible).
 * workspace: device scratch of ppf_align_workspace_bytes() bytes. */
size_t ppf_align_workspace_bytes(int32_t nsub, int32_t nchan, int32_t nbin);
int ppf_align_accum(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                    int32_t in_dtype, const void *in, const double *phases,
                    const double *weights, double *out, double *wsum,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ppalign's per-row rotation phases and weights from a fit (ppalign.py:
 * 222-247; round 6, ABI 6): for sub-int s, channel n with mask[s][n] != 0
 *   phases[s][n]  = phi_s + Dconst DM_s / P_s (freqs[s][n]^-2 - nu_DM,s^-2)
 *   weights[s][n] = scales[s][n] / errs[s][n]^2
 * and 0 where masked; phi, DM, nu_DM from results[s] (ppf_result: params[0],
 * params[1], nu_out[0]).  One launch instead of the dozen elementwise
 * operations it replaces in each ppalign iteration.  results: [nsub]
 * ppf_result; freqs, scales, errs, phases, weights: [nsub][nchan]; P:
 * [nsub]; mask: [nsub][nchan] or NULL (all used). */
int ppf_align_phases(ppf_ctx *ctx, int32_t nsub, int32_t nchan, const double *results,
                     const double *freqs, const double *P, const uint8_t *mask,
                     const double *scales, const double *errs, double *phases,
                     double *weights, void *stream);

/* Channel reduced chi^2 of a fit (pptoas.get_channels_to_zap,
 * pptoas.py:1266-1343, through show_fit 1375-1480 and get_red_chi2
 * pplib.py:754-779): for each row r,
 *   out[r] = sum_t (rot(in[r], phases[r])[t] - scales[r] model[model_row[r]][t])^2
 *            / errs[r]^2 / dof
 * with rot the rfft-phasor-irfft rotation of ppf_rotate_batch.
 * in: [nrows][nbin]; model: [*][nbin] f64; phases, scales, errs, out: [nrows]. */
int ppf_resid_chi2_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype,
                         const void *in, const double *phases, const double *model,
                         const int32_t *model_row, const double *scales,
                         const double *errs, double dof, double *out, void *stream);

/* Per-row power-spectrum noise: pplib.get_noise_PS(chans=True)
 * (pplib.py:2312-2332): sqrt(mean(|rfft(x)|^2/nbin over k >= int((1-1/frac)
 * * nharm))).  in: [nrows][nbin]; out: [nrows]. */
int ppf_noise_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin,
                    int32_t in_dtype, const void *in, int32_t frac,
                    double *out, void *stream);

/* Power-spectrum noise of rows of ANY length (round 6, ABI 6):
 * pplib.get_noise_PS (pplib.py:2312-2338) where ppf_noise_batch's LDS
 * transforms do not reach -- chans=False ravels a whole portrait into one
 * row of nchan * nbin samples (2^20 at 512 x 2048), and rows past 8192 (even)
 * / 4095 (odd) samples.  The rFFT is a four-step transform of block LDS FFTs
 * (transform length a power of two) or Bluestein's chirp z-transform on one
 * (any other length), up to 2^24 complex points (2^25 samples for a
 * power-of-two row, 2^24 otherwise; PPF_EUNSUP past that).
 * in: [nrows][nbin] (in_dtype); out: [nrows] device doubles; workspace:
 * device scratch of ppf_noise_long_workspace_bytes(nrows, nbin) bytes
 * (0: nbin unsupported). */
size_t ppf_noise_long_workspace_bytes(int64_t nrows, int64_t nbin);
int ppf_noise_long(ppf_ctx *ctx, int64_t nrows, int64_t nbin, int32_t in_dtype,
                   const void *in, int32_t frac, double *out, void *workspace,
                   size_t workspace_bytes, void *stream);

/* Fitted noise floor: pplib.get_noise_fit (pplib.py:2341-2373) and the
 * find_kc it calls (pplib.py:1530-1561), added within ABI 6.  With pows =
 * |rfft(x)|^2 / nbin (N = nbin / 2 + 1 harmonics) and d = log10(pows),
 * find_kc minimises chi^2(a, b, dc) = sum_k ((d_k - dc - b e_k(a)) / errs_k)^2
 * over scipy.optimize.brute's 20 x 20 x 20 grid (np.mgrid[lo:hi:20j]) --
 * b over [0, max d - min d], dc over [min d, max d]; fn 0 (exp_dc):
 * e_k = exp(-a k), a over [1/N, 1]; fn 1 (half_tri): e_k = 1 - k / floor(a)
 * below floor(a), 0 from there, a over [1, N] -- and takes the first minimum
 * in C order (the first NaN if there is one; a NaN or zero-power harmonic
 * makes every row of the grid NaN: index 0).  kc depends on the winning a
 * alone, so the caller supplies both tables, HOST arrays read during the
 * call: a_grid[20], and kc_table[20], the kc of each of its values (>= 0).
 * get_noise_fit then has k_crit = fact * kc, lowered to min(int(0.99 N),
 * k_crit) when k_crit >= N, and noise = sqrt(mean(pows[int(k_crit):])).
 *
 * ppf_noise_fit_batch: the row lengths of ppf_noise_batch (fn 0, errs 1);
 * in: [nrows][nbin]; noise_out, kc_out: [nrows] device.
 * ppf_noise_fit_long: any length ppf_noise_long takes with nbin >= 3, on its
 * transforms; workspace: ppf_noise_fit_long_workspace_bytes(nrows, nbin)
 * bytes of device scratch (0: unsupported).
 * ppf_find_kc_batch: find_kc of power spectra pows [nrows][nharm] (device
 * f64, nharm >= 2); errs: NULL (errs = 1) or a DEVICE array of errs_len = 1
 * or nharm doubles shared by the rows; kc_out: [nrows] device.
 * Codes: PPF_EUNSUP for an unsupported length; PPF_EINVAL for a NULL array
 * or context, a bad in_dtype or fn, a fact that is not finite and positive,
 * errs_len other than 1 or nharm, a short workspace. */
int ppf_noise_fit_batch(ppf_ctx *ctx, int64_t nrows, int32_t nbin, int32_t in_dtype,
                        const void *in, double fact, const double *a_grid,
                        const int32_t *kc_table, double *noise_out, int32_t *kc_out,
                        void *stream);
size_t ppf_noise_fit_long_workspace_bytes(int64_t nrows, int64_t nbin);
int ppf_noise_fit_long(ppf_ctx *ctx, int64_t nrows, int64_t nbin, int32_t in_dtype,
                       const void *in, double fact, const double *a_grid,
                       const int32_t *kc_table, double *noise_out, int32_t *kc_out,
                       void *workspace, size_t workspace_bytes, void *stream);
int ppf_find_kc_batch(ppf_ctx *ctx, int64_t nrows, int64_t nharm, const double *pows,
                      const double *errs, int64_t errs_len, int32_t fn,
                      const double *a_grid, const int32_t *kc_table, int32_t *kc_out,
                      void *stream);

/* rotate_data's rotation of rows of ANY length (round 6, ABI 6): rows the
 * LDS transforms of ppf_rotate_batch do not take (even nbin > 8192, odd
 * nbin > 4095), as Bluestein transforms both ways (up to 2^23 complex
 * points).  out[r] = irfft(rfft(in[r]) * exp(2 pi i k phases[r])), nbin
 * samples, or nbin - 1 at odd nbin with ref_len != 0 (the reference's
 * length-less irfft, as ppf_rotate_batch_ref).  in: [nrows][nbin]
 * (in_dtype); phases: [nrows]; out: [nrows][nout] f64; workspace: device
 * scratch of ppf_rotate_long_workspace_bytes(nrows, nbin, ref_len) bytes
 * (0: unsupported). */
size_t ppf_rotate_long_workspace_bytes(int64_t nrows, int64_t nbin, int32_t ref_len);
int ppf_rotate_long(ppf_ctx *ctx, int64_t nrows, int64_t nbin, int32_t in_dtype,
                    const void *in, const double *phases, double *out, int32_t ref_len,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Batched 1-D FFTFIT: pplib.fit_phase_shift (pplib.py:2136-2182): brute
 * force over Ns points of [lo, hi] then Nelder-Mead (scipy fmin) polish.
 * data: [nprof][nbin] (in_dtype); model: [nmodel_prof][nbin] double with
 * model_index[nprof] (NULL -> 0); noise: [nprof] time-domain sigma or NULL
 * (estimated); out: [nprof][8] = phase, phase_err, scale, scale_err, snr,
 * red_chi2, nfev, status. */
int ppf_phase_shift_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin,
                          int32_t in_dtype, const void *data,
                          const double *model, const int32_t *model_index,
                          const double *noise, int32_t Ns, double lo,
                          double hi, double *out, void *stream);

/* Maximum-likelihood channel amplitudes at given parameters:
 * pptoaslib.get_scales_full (pptoaslib.py:953-971), a_n = C_n / S_n with
 * S_n = sum_k |B_nk|^2 |M_nk|^2 / e_n^2 (Sbp) and
 * C_n = Re sum_k D_nk conj(M_nk) conj(B_nk) exp(2 pi i k phi_n) / e_n^2 (Cdbp),
 * phi_n = phase_shifts(phi, DM, GM, nu_n, nu_DM, nu_GM, P), B the one-sided
 * exponential scattering FT at tau_n = tau (nu_n / nu_tau)^alpha
 * (10**tau with log10_tau).  D: [nsub][nchan][nharm] complex (re, im pairs);
 * M: [nmodel][nchan][nharm] complex with model_index[nsub] (NULL -> 0);
 * errs_FT: [nsub][nchan] or NULL; params: [nsub][5]; P: [nsub];
 * freqs: [nsub][nchan]; nus: [nsub][3] = nu_DM, nu_GM, nu_tau;
 * out: [nsub][nchan]. */
int ppf_scales_batch(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nharm, const double *D,
                     const double *M, const int32_t *model_index, const double *errs_FT,
                     const double *params, const double *P, const double *freqs, const double *nus,
                     int32_t log10_tau, double *out, void *stream);

/* PSRCHIVE-free PSRFITS fast path (pulseportraiture_amd/psrfits.py; replaces
 * the unpacking, baseline removal, pscrunch and per-profile statistics of
 * pplib.load_data, pplib.py:2749-2915, for fold-mode PSRFITS): raw SUBINT
 * DATA bytes as stored in the file (big-endian; elem 0 = int16, 1 = uint8,
 * 2 = float32; 3 = native little-endian float32 rows, load_data's second
 * statistics pass over dedispersed / tscrunched rows), one block of sub_stride bytes per sub-int holding
 * [npol][nchan][nbin] samples (at least the pols used: 1, or 2 with
 * pol_mode 1; scl / offs still index all npol), become float32 rows
 *   out[s][n][b] = sum_p (DATA * DAT_SCL + DAT_OFFS)   (float32 arithmetic)
 * over p = pol 0 (pol_mode 0: npol 1 or IQUV's I) or pols 0 + 1 (pol_mode 1:
 * AA+BB / AABBCRCI).  The baseline window of each sub-int is the circular
 * window of rint(0.15 nbin) bins with the smallest sum of the weighted
 * total profile (PSRCHIVE's default BaselineWindow); with rm_baseline its
 * mean is subtracted from every row.  scl, offs: float32 [nsub][npol*nchan];
 * wts: float32 [nsub][nchan] or NULL; stats: [nsub][nchan][3] = off-pulse
 * mean, off-pulse sigma, S/N (on-pulse sum / (sigma sqrt(n_on)));
 * total: [nsub][nbin] weighted total profiles; wstart: int32 [nsub] window
 * starts (the first minimum in bin order).  raw and sub_stride must be
 * multiples of the element size (2, 1, 4, 4 bytes for elem 0..3): PPF_EINVAL
 * otherwise, before any launch.  Any nbin >= 2: the total profile is held in
 * one workgroup's LDS up to 18,816 bins and read from `total` past that.
 * workspace: ppf_unpack_workspace_bytes(). */
size_t ppf_unpack_workspace_bytes(int32_t nsub, int32_t nchan, int32_t nbin);
int ppf_unpack_psrfits_batch(ppf_ctx *ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                             int32_t elem, const void *raw, int64_t sub_stride, const float *scl,
                             const float *offs, const float *wts, int32_t pol_mode,
                             int32_t rm_baseline, float *out, double *stats, double *total,
                             int32_t *wstart, void *workspace, size_t workspace_bytes,
                             void *stream);

/* ppf_unpack_psrfits_batch for all four polarisations of an npol = 4 file
 * (added within ABI 6: purely additive): every sub-int block of raw holds
 * [4][nchan][nbin] samples (elem as above; elem 3: native float32 rows, the
 * statistics pass of a polarised load), scl / offs are [nsub][4*nchan].  Per
 * sample the four values DATA * DAT_SCL + DAT_OFFS (float32, two roundings)
 * are converted in float32, one rounded operation per output:
 *   conv 0  keep (Stokes)            I, Q, U, V                 total = pol 0
 *   conv 1  keep (Coherence)         AA, BB, CR, CI             pol 0 + pol 1
 *   conv 2  Coherence -> Stokes LIN  AA+BB, AA-BB, 2CR, 2CI     pol 0
 *   conv 3  Coherence -> Stokes CIRC AA+BB, 2CR, 2CI, AA-BB     pol 0
 *   conv 4  Stokes -> Coherence LIN  (I+Q)/2, (I-Q)/2, U/2, V/2 pol 0 + pol 1
 *   conv 5  Stokes -> Coherence CIRC (I+V)/2, (I-V)/2, Q/2, U/2 pol 0 + pol 1
 * (PSRCHIVE's conventions as documented, not pinned to a PSRCHIVE run).
 * out: [nsub][4][nchan][nbin]; the baseline window of a sub-int is found on
 * the weighted total intensity (last column: formed in float32 from the
 * output rows) exactly as ppf_unpack_psrfits_batch finds it, and applies to
 * all four of its polarisations; stats: [nsub][4][nchan][3]; total, wstart,
 * wts, rm_baseline, workspace (ppf_unpack_workspace_bytes(nsub, nchan, nbin))
 * as there.  Rows with nbin % 4 == 0 whose raw, sub_stride, out and
 * workspace are aligned for it take 4 bins per lane with 8-byte loads
 * (16-bit samples; 4 / 16 bytes for 8-bit / float32) and 16-byte stores,
 * every other shape element-wide accesses: the same bits either way.
 * PPF_EINVAL, before any launch: a NULL ctx, nsub < 0, nchan < 1, nbin < 2,
 * elem outside 0..3, conv outside 0..5, sub_stride below 4 nchan nbin
 * elements, raw or sub_stride not multiples of the element size; then
 * nsub == 0 returns PPF_OK; then a NULL array (PPF_EINVAL), a short
 * workspace (PPF_ENOMEM). */
int ppf_unpack_psrfits_pol_batch(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                                 int32_t elem, const void *raw, int64_t sub_stride,
                                 const float *scl, const float *offs, const float *wts,
                                 int32_t conv, int32_t rm_baseline, float *out, double *stats,
                                 double *total, int32_t *wstart, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* The inverse of ppf_unpack_psrfits_batch (added within ABI 6: purely
 * additive, a library without the symbol is a stale build): float rows on
 * the device become the DATA bytes of a fold-mode SUBINT table, as
 * pplib.write_archive / unload_new_archive (pplib.py:3146-3300) store them.
 * rows: [nrow][nbin] float32 (PPF_F32) or float64 (PPF_F64), device; raw:
 * [nrow][nbin * esize] bytes in file order; scl, offs: float32 [nrow]
 * (DAT_SCL, DAT_OFFS of each row).
 *   elem 0, big-endian int16 (esize 2): per row, with lo / hi its minimum /
 *     maximum, offs = f32((lo + hi) / 2), scl = f32(max((hi - lo) / 2 / 32767,
 *     1e-30)), q = clip(rint((x - offs) / scl), -32768, 32767): float64
 *     arithmetic, one rounding per operation, round-half-even -- the numbers
 *     of psrfits.quantize bit for bit, and those of ppf_fake_batch's
 *     PPF_FAKE_I16.
 *   elem 2, big-endian float32 (esize 4): the sample is (float)x, scl = 1,
 *     offs = 0.
 * Any nbin >= 1 (rows are never staged in LDS); rows with nbin % 8 == 0 and
 * 16-byte aligned rows / raw take 16-byte accesses, every other shape
 * element-wide ones.  No atomics: the output is bitwise reproducible.  A row
 * holding a NaN or an Inf is the caller's error: its bytes are unspecified
 * (no fault).  PPF_EINVAL, before any launch: nrow < 0, nbin < 1, an elem
 * other than 0 / 2, an in_dtype other than PPF_F32 / PPF_F64, a byte count
 * past int64; then nrow == 0 returns PPF_OK (nothing else is looked at);
 * then a NULL ctx or array, rows / raw not aligned to their element. */
int ppf_pack_psrfits_batch(ppf_ctx *ctx, int64_t nrow, int32_t nbin, int32_t in_dtype,
                           const void *rows, int32_t elem, void *raw,
                           float *scl, float *offs, void *stream);

/* nbytes from page-locked host memory src (a pinned buffer: hipHostMalloc /
 * torch pin_memory) to device memory dst, read by a kernel over PCIe on
 * stream instead of by a copy engine.  GetTOAs stages each archive's fit
 * inputs (engine._stage_host: the per-sub-int arrays of the reference's
 * fit_portrait_full calls, pptoas.py:530-533) this way, so they never wait
 * behind the archive uploads the copy engines are busy with.  Both pointers
 * 16-byte aligned; src must stay untouched until the stream has passed the
 * copy. */
int ppf_copy_from_pinned(ppf_ctx *ctx, void *dst, const void *src, int64_t nbytes, void *stream);

/* Positioned reads of the PSRFITS DATA column into host memory (the file
 * side of the fast path above; psrfits.PSRFITS.read_data_into): for each of
 * nrows rows, nbytes bytes at file offset offset + r * row_stride go to
 * dst + r * dst_stride.  The rows are cut into pieces of at most 4 MiB that
 * nthreads threads (1..64) take in turn with pread(2); the call returns when
 * every piece is in (dst is typically a page-locked upload buffer).  No
 * device and no context: PPF_OK, PPF_EINVAL (bad arguments) or PPF_EIO (a
 * read failed or hit end of file). */
int ppf_read_rows(int32_t fd, int64_t offset, int64_t row_stride, int64_t nbytes,
                  int64_t nrows, void *dst, int64_t dst_stride, int32_t nthreads);

/* Parallel host memcpy (ABI 4): nbytes from src to dst in 4-MiB pieces taken
 * in turn by nthreads threads (1..64).  GetTOAs stages in-memory archives
 * (pageable numpy rows) into its page-locked upload buffers with it
 * (pptoas._Stager; the reference hands the rows to fit_portrait_full
 * directly, pptoas.py:530-533).  Host memory only: PPF_OK or PPF_EINVAL. */
int ppf_host_copy(void *dst, const void *src, int64_t nbytes, int32_t nthreads);

/* Gaussian-component model portraits: pplib.gen_gaussian_portrait
 * (pplib.py:886-963, join_ichans = []) as called by pplib.read_model
 * (pplib.py:2971-3057) for every sub-integration of GetTOAs.get_TOAs
 * (pptoas.py:392-419) and get_narrowband_TOAs.  One launch builds nport
 * portraits (one per distinct frequency set), each row by
 * gen_gaussian_profile / gaussian_profile (pplib.py:801-883) and, when
 * tau != 0, convolved with scattering_portrait_FT (pplib.py:4245-4260).
 * model_code: 3 chars '0' (power law) / '1' (linear) for loc, wid, amp
 * (anything else: PPF_EINVAL, the reference's KeyError).  params:
 * [nport][2 + 6*ngauss] = DC, tau [bin], then per component loc, m_loc,
 * wid, m_wid, amp, m_amp; scattering_index, nu_ref: [nport];
 * freqs: [nport][nchan]; out: [nport][nchan][nbin] f64 (device).
 * Rows past the LDS transforms (even nbin > 8192, odd > 4095; nbin ≤
 * 19,200, the row in LDS): built per bin, a scattered model's convolution
 * then on the long transforms (synchronous; PPF_EUNSUP for a scattered
 * model at odd nbin there). */
int ppf_gauss_portrait_batch(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin,
                             int32_t ngauss, const char *model_code, const double *params,
                             const double *scattering_index, const double *freqs,
                             const double *nu_ref, double *out, void *stream);

/* Normal equations of the Gaussian-component portrait model (added within
 * ABI 6): what a Levenberg-Marquardt fit of pplib.fit_gaussian_portrait
 * (pplib.py:2005-2144) needs per iteration, for nfit independent fits.
 * With m(p) the portrait ppf_gauss_portrait_batch builds for p (the same
 * device code builds the rows, so m(p) has the same bits), fit f has the
 * nfree + 1 columns over its nchan * nbin points
 *     c_j     = ((m(p + delta_j e_j) - m(p)) / delta_j) * inv_errs,  j < nfree
 *     c_nfree = (data - m(p)) * inv_errs
 * and gram[f] = C C^T, [nfree + 1][nfree + 1] f64, symmetric, both triangles
 * written: J^T J is the leading block, J^T r the last column, chi^2 the
 * corner.  nfree = 0 gives chi^2 alone (an LM trial step).
 * free_idx indexes the extended parameter vector: entries 0 .. npar - 1
 * (npar = 2 + 6 * ngauss) are params, entry npar is the scattering index;
 * strictly increasing.  free_idx [nfree] (int32) and delta [nfit][nfree] are
 * HOST arrays, checked here and copied by the call; they must stay untouched
 * until the stream has passed it.  Every other array is device memory:
 * params, scattering_index, freqs, nu_ref and model_code as for
 * ppf_gauss_portrait_batch; data [nfit][nchan][nbin] in in_dtype; inv_errs
 * [nfit][nchan][nbin] f64 (1 / sigma per point; no masks: 0 drops a point).
 * The contraction runs on the f64 MFMA over fixed chunks of the point axis,
 * the partial tiles summed in a fixed order without atomics: the result is
 * bitwise reproducible.
 * PPF_EUNSUP: nbin odd or outside [32, 8192] (the LDS row transforms),
 * nfree + 1 > 128.  PPF_EINVAL: bad model_code or in_dtype, free_idx out of
 * range or not increasing, a zero or non-finite delta, a workspace smaller
 * than ppf_gauss_lsq_workspace_bytes (0 for an unsupported shape), a NULL
 * array or context.  All of this is checked on the host before any launch. */
size_t ppf_gauss_lsq_workspace_bytes(int32_t nfit, int32_t nchan, int32_t nbin, int32_t nfree);
int ppf_gauss_lsq_batch(ppf_ctx *ctx, int32_t nfit, int32_t nchan, int32_t nbin, int32_t ngauss,
                        const char *model_code, const double *params,
                        const double *scattering_index, const double *freqs,
                        const double *nu_ref, int32_t nfree, const int32_t *free_idx,
                        const double *delta, int32_t in_dtype, const void *data,
                        const double *inv_errs, double *gram, void *workspace,
                        size_t workspace_bytes, void *stream);

/* The joined Gaussian model (added within ABI 6): several archives of one
 * pulsar under one model, each archive with a phase and a DM offset of its
 * own (gen_gaussian_portrait's join_ichans, pplib.py:956-962; the join
 * parameters of fit_gaussian_portrait, pplib.py:2073-2098).  The arguments
 * of ppf_gauss_portrait_batch / ppf_gauss_lsq_batch, plus
 *   njoin                  archives
 *   join_id  [n][nchan]    int32, HOST (as free_idx: checked here, copied by
 *                          the call): the archive of each channel, -1 for a
 *                          channel in none
 *   join_params [n][2 njoin]  f64, device: phase [rot], DM per archive
 *   P        [n]           f64, device: period [s]
 * (n = nport or nfit).  A row of archive a is rotated by
 *     rot = phi_a + (Dconst DM_a / P) (nu^-2 - nu_ref^-2)
 * as rotate_data does (pplib.py:2447-2512), in the row's one transform round
 * trip: harmonic k is multiplied by B_k e^{2 pi i k rot}, B_k the scattering
 * factor or 1, the imaginary parts of the DC and Nyquist bins dropped before
 * the phasor as the reference's intermediate irfft drops them.  A row of an
 * archive takes this path at rot = 0 too; a row of no archive is built by
 * the unrotated code and has the bits ppf_gauss_portrait_batch gives it.
 * In ppf_gauss_lsq_join_batch the extended parameter vector free_idx indexes
 * is [0, npar) params, [npar, npar + 2 njoin) join_params, npar + 2 njoin
 * the scattering index (the reference's lmfit order; today's layout at
 * njoin = 0).  A column that perturbs a join parameter of archive a is
 * exact zeros over the channels outside a: no row is built or read there.
 * The workspace is that of ppf_gauss_lsq_workspace_bytes.
 * With njoin = 0 both calls are the unjoined ones, bit for bit.  With
 * njoin > 0 they keep the device copy of join_id in the context's scratch
 * and return after the stream has finished.
 * PPF_EUNSUP: nbin odd or outside [32, 8192] (the reference cannot rotate an
 * odd-length model either: its irfft returns nbin - 1 bins).  PPF_EINVAL: a
 * join_id outside [-1, njoin), njoin < 0, a NULL array, and what the
 * unjoined calls refuse.  All checked on the host before any launch. */
int ppf_gauss_portrait_join_batch(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin,
                                  int32_t ngauss, const char *model_code, const double *params,
                                  const double *scattering_index, const double *freqs,
                                  const double *nu_ref, int32_t njoin, const int32_t *join_id,
                                  const double *join_params, const double *P, double *out,
                                  void *stream);
int ppf_gauss_lsq_join_batch(ppf_ctx *ctx, int32_t nfit, int32_t nchan, int32_t nbin, int32_t ngauss,
                             const char *model_code, const double *params,
                             const double *scattering_index, const double *freqs,
                             const double *nu_ref, int32_t njoin, const int32_t *join_id,
                             const double *join_params, const double *P, int32_t nfree,
                             const int32_t *free_idx, const double *delta, int32_t in_dtype,
                             const void *data, const double *inv_errs, double *gram,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Stationary-wavelet denoise-and-score engine (added within ABI 6): the
 * search of pplib.smart_smooth (pplib.py:1740-1838) over decomposition level
 * and threshold factor.  The transform is the undecimated 'db8' transform of
 * a periodic row of even length nbin, written from its definition (DESIGN.md
 * section 0, ppspline): a_0 = x, a_j / d_j the circular convolution of
 * a_{j-1} with dec_lo / dec_hi upsampled by 2^(j-1) (the filter wraps at
 * small nbin), synthesis half the adjoint.
 * ppf_swt_analyse_batch: per profile (prof [nprof][nbin] f64, device) the
 * rows a_j, d_j for j = 1 .. nlevel into the workspace, medians
 * [nprof][nlevel] = np.median(|a_j| u |d_j|) (2 nbin values, exact
 * selection, the mean of the two middle ones) and noise [nprof] =
 * get_noise_PS(prof) (ppf_noise_batch's rule, frac = 4); both device, f64.
 * ppf_swt_score_batch: ncase independent cases on the analysed batch (same
 * prof, medians, noise, workspace).  cases [ncase][3] int32 = (profile,
 * level L in [1, nlevel], 0 hard / 1 soft) and fact [ncase] f64 are HOST
 * arrays, checked here and copied by the call; they must stay untouched
 * until the stream has passed it.  Per case
 *     lambda = fact * (medians[profile][L - 1] / 0.6745) * sqrt(2 ln nbin)
 * thresholds a_L and d_1 .. d_L (hard: 0 where |c| < lambda; soft:
 * c * max(1 - lambda / |c|, 0)), the row s is synthesised and
 * out [ncase][3] = (sum_{k >= 1} |rfft(s)_k|^2, get_noise_PS(s) *
 * sqrt(nbin / 2), sum(((prof - s) / noise[profile])^2) / nbin), what
 * pplib.fit_wavelet_smooth_function combines; smooth [ncase][nbin] receives
 * s when not NULL.  No atomics: results are bitwise reproducible.
 * The workspace (ppf_swt_workspace_bytes; 0 for an unsupported shape) holds
 * the coefficients of one analysed batch and up to max_ncase cases per call.
 * PPF_EUNSUP: nbin odd or outside [32, 8192], nlevel > log2(nbin) for a
 * power of two, nlevel > 1 for any other nbin.  PPF_EINVAL: nlevel < 1, a
 * case naming a profile or level out of range or another threshold type, a
 * non-finite factor, a small workspace, a NULL array or context.  All of
 * this is checked on the host before any launch. */
size_t ppf_swt_workspace_bytes(int32_t nprof, int32_t nbin, int32_t nlevel, int32_t max_ncase);
int ppf_swt_analyse_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t nlevel,
                          const double *prof, double *medians, double *noise, void *workspace,
                          size_t workspace_bytes, void *stream);
int ppf_swt_score_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t nlevel,
                        const double *prof, const double *medians, const double *noise,
                        int32_t ncase, const int32_t *cases, const double *fact, double *out,
                        double *smooth, void *workspace, size_t workspace_bytes, void *stream);

/* ppf_swt_search_batch (added within ABI 6): the fmin finish of
 * scipy.optimize.brute(..., Ns = ngrid, full_output=True) for every (profile,
 * level L in 1 .. nlevel) of the analysed batch (same prof, medians, noise,
 * workspace), one workgroup each, with one threshold type (soft 0 / 1).  The
 * objective of a (signal, noise, red_chi2) triple is pplib._wavelet_snr:
 * -signal / noise (-inf for noise 0, 0 for signal 0), 0 where
 * |red_chi2 - 1| > rchi2_tol.  grid [ngrid] f64 is a HOST array (copied by
 * the call, untouched until the stream has passed it); table
 * [nprof][nlevel][ngrid][3] f64, device, is the out of one
 * ppf_swt_score_batch call over the cases (p, L, soft) x grid in that order.
 * From x0 = the first grid point of minimal objective the kernel runs
 * scipy's Nelder-Mead in one dimension (xatol = fatol = 1e-4, at most 200
 * calls; DESIGN.md gives the recurrence), every evaluation the scoring body
 * of ppf_swt_score_batch, and returns, [nprof][nlevel] each, device:
 * fact_min (f64) the best factor, fun_min (f64) its objective, nfev (int32)
 * the calls made.  The workspace must hold max(ngrid, 1) cases.  Errors as
 * ppf_swt_score_batch, and PPF_EINVAL for ngrid < 1, a non-finite grid value
 * or tolerance, soft outside {0, 1}; all checked on the host before any
 * launch. */
int ppf_swt_search_batch(ppf_ctx *ctx, int32_t nprof, int32_t nbin, int32_t nlevel,
                         const double *prof, const double *medians, const double *noise,
                         int32_t soft, double rchi2_tol, int32_t ngrid, const double *grid,
                         const double *table, double *fact_min, double *fun_min, int32_t *nfev,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Spline (PCA + B-spline) model portraits: pplib.gen_spline_portrait
 * (pplib.py:966-990) as called by pplib.read_spline_model (pplib.py:3060-3096)
 * from pptoas.GetTOAs.get_TOAs (pptoas.py:416-419) for make_spline_model
 * templates.  Per (portrait, channel): the B-spline curve (knots[nknots],
 * coefs[ncomp][nknots] -- splprep's c arrays, zero-padded --, degree
 * <= 5) evaluated at freqs[p][n] as FITPACK splev (ext = 0), expanded on
 * eigvec [nbin_model][ncomp] plus mean_prof [nbin_model]; ncomp = 0 tiles
 * mean_prof.  nbin != nbin_model: scipy.signal.resample to nbin, then the
 * reference's half-bin rotate_portrait.  nbin == nbin_model: any length;
 * resampled: both even in [32, 8192] on the LDS transforms (round 6: any
 * such length, was powers of two; else PPF_EUNSUP); ncomp <= 64.
 * out: [nport][nchan][nbin] f64 (device). */
int ppf_spline_portrait_batch(ppf_ctx *ctx, int32_t nport, int32_t nchan, int32_t nbin_model,
                              int32_t nbin, int32_t ncomp, int32_t nknots, int32_t degree,
                              const double *mean_prof, const double *eigvec,
                              const double *knots, const double *coefs, const double *freqs,
                              double *out, void *stream);

/* Synthetic sub-integrations for benchmarks/tests (make_fake_pulsar minus
 * PSRCHIVE, pplib.py:3355-3493): out[s][n] = rotate(model[n], -phi[s],
 * -DM[s], P[s], freqs[n], nu_ref) + N(0, noise) with a counter-based RNG
 * keyed by (seed, first_sub + s, n), so a sub-integration's data do not
 * depend on how a job is sharded.  model: [nchan][nbin]; out: [nsub][nchan][nbin]
 * in out_dtype. */
int ppf_synth_batch(ppf_ctx *ctx, int32_t nsub, int32_t nchan, int32_t nbin,
                    const double *model, const double *freqs,
                    const double *phi, const double *DM, const double *P,
                    double nu_ref, double noise, uint64_t seed,
                    int64_t first_sub, int32_t out_dtype, void *out,
                    void *stream);

/* Simulated fold-mode archives (added within ABI 6): the profiles
 * pplib.make_fake_pulsar (pplib.py:3302-3499) writes, built on the device and
 * stored as the samples a PSRFITS SUBINT table holds.  One workgroup per row
 * (sub-int s, polarisation p, channel n):
 *     X_k = M_k exp(2 pi i k phase[s][n]) B_k gain[s][p][n],   0 <= k < nbin/2,
 *     B_k = 1 / (1 + 2 pi i k tau_n[s][n])   (1 for tau_n = 0),
 * M = rfft(model[model_of[s]][n]); DC keeps its real part, and the Nyquist
 * harmonic is Re(M_N) cos(2 pi N phase) Re(B_N) gain, what the reference's
 * two real transforms (rotation, then scattering) leave of it.  The inverse
 * real transform of X plus N(0, noise[n]) per bin (none for noise[n] = 0) is
 * the row; the deviates come from ppf_synth_batch's counter RNG keyed by
 * (seed, first_sub + s, p, n, bin), so a sub-int's samples do not depend on
 * how a job is split into calls.
 * model [nmodel][nchan][nbin] f64, model_of [nsub] int32 (clamped to [0,
 * nmodel)), phase and tau_n [nsub][nchan] f64 (turns), gain
 * [nsub][npol][nchan] f64, noise [nchan] f64: device arrays.
 * out_kind PPF_FAKE_F64: out [nsub][npol][nchan][nbin] f64 rows (dat_scl,
 * dat_offs unused).  PPF_FAKE_I16: the same rows quantised per profile as
 * psrfits.quantize does it, bit for bit (offset f32((lo + hi) / 2), scale
 * f32(max((hi - lo) / 2 / 32767, 1e-30)), rint, clipped), out the big-endian
 * int16 of the DATA column in its layout [nsub][npol][nchan][nbin], dat_scl /
 * dat_offs [nsub][npol * nchan] f32 in host byte order.
 * PPF_EUNSUP: nbin odd or outside [32, 8192] (the LDS row transforms), more
 * than 2^31 - 1 rows.  PPF_EINVAL: a count below its minimum, first_sub < 0,
 * another out_kind, out not 16-byte aligned, a NULL array or context.  All of
 * this is checked on the host before any launch. */
enum ppf_fake_kind { PPF_FAKE_I16 = 0, PPF_FAKE_F64 = 1 };
int ppf_fake_batch(ppf_ctx *ctx, int32_t nsub, int32_t npol, int32_t nchan, int32_t nbin,
                   int32_t nmodel, const double *model, const int32_t *model_of,
                   const double *phase, const double *tau_n, const double *gain,
                   const double *noise, uint64_t seed, int64_t first_sub, int32_t out_kind,
                   void *out, float *dat_scl, float *dat_offs, void *stream);

/* The portrait likelihood evaluated at many parameter points (added within
 * ABI 6: purely additive): chi'^2 = -sum_n C_n^2 / S_n of
 * pptoaslib.fit_portrait_full_function (pptoaslib.py:564-581), its gradient
 * (_deriv, 584-614) and Hessian (_2deriv, 617-684), at npoint vectors
 * theta = (phi, DM, GM, tau, alpha) for each of nprob problems; a problem is
 * one (data_FT, model_FT) pair as the reference's functions take it.
 * Device arrays, f64 unless said otherwise:
 *   data_FT  [nprob][nchan][nharm]   complex128 (re, im), channel-major
 *   model_FT [nmodel][nchan][nharm]  complex128; problem s uses model
 *            model_index[s] (int32 [nprob]); model_index NULL: model s
 *            (nmodel == nprob) or the one model (nmodel == 1)
 *   errs_FT, freqs [nprob][nchan];  P [nprob];  nus [nprob][3] = nu_DM,
 *            nu_GM, nu_tau;  mask [nprob][nchan] uint8 or NULL (0 drops the
 *            channel: it adds exactly 0 to every sum and its data, which may
 *            be NaN, are never loaded)
 *   theta    [nprob][npoint][5];  fit_flags [5] or NULL (all 1): the gradient
 *            is multiplied by flags_i, the Hessian by flags_i flags_j
 *   log10_tau: tau = 10^theta_3 and the derivatives are with respect to theta_3
 *   order    0: f; 1: f and grad; 2: f, grad and hess
 *   f [nprob][npoint], grad [nprob][npoint][5], hess [nprob][npoint][5][5]
 *            (both triangles); grad / hess may be NULL below their order
 *   terms    NULL, or [nprob][npoint][62][nchan]: per channel C, S, dC[5],
 *            dS[5], d2C[5][5], d2S[5][5] (rows 0, 1, 2..6, 7..11, 12..36,
 *            37..61), the quantities of the reference's Cdbp* / Sbp* family;
 *            derivatives past `order` are 0
 * nharm is any value >= 2 (no transform is taken); harmonic 0 is summed as
 * given; the per-channel phase is not wrapped (phase_shifts, mod = False).
 * Linear tau = 0: B = 1 and every tau / alpha derivative is exactly 0 (the
 * reference's taus.sum() branches).  Where the reference divides 0 / 0 (a
 * channel with C = 0, a channel exactly at nu_tau) the closed-form finite
 * value is returned.  The points of a block of ppf_eval_point_block() share
 * one load of a channel's spectra; all sums run in a fixed order without
 * atomics, so results are bitwise reproducible, the same for a point however
 * the points are split over calls, and the same with a channel masked or
 * deleted.  The workspace holds the per-channel contributions
 * (ppf_eval_workspace_bytes; 0 for a bad shape).
 * PPF_EINVAL, before anything touches the device: a NULL ctx, nprob < 0,
 * nchan < 1, nharm < 2, npoint < 1, nmodel < 1, an order outside 0..2, a
 * model_index missing where nmodel is neither 1 nor nprob; then nprob == 0
 * returns PPF_OK; then a NULL array, more than 2^31 - 1 workgroups
 * (nprob x ceil(npoint / block) x nchan); a short workspace is PPF_ENOMEM. */
int ppf_eval_point_block(void);
int ppf_eval_harm_tile(void);
size_t ppf_eval_workspace_bytes(int32_t nprob, int32_t nchan, int32_t npoint, int32_t order);
int ppf_eval_batch(ppf_ctx *ctx, int32_t nprob, int32_t nchan, int32_t nharm, int32_t npoint,
                   const double *data_FT, const double *model_FT, int32_t nmodel,
                   const int32_t *model_index, const double *errs_FT, const double *P,
                   const double *freqs, const double *nus, const uint8_t *mask, const double *theta,
                   const double *fit_flags, int32_t log10_tau, int32_t order, double *f, double *grad,
                   double *hess, double *terms, void *workspace, size_t workspace_bytes, void *stream);

/* Host-side (CPU) helper: real roots of a degree <= 8 polynomial, highest
 * power first, with np.roots semantics (companion-matrix eigenvalues with an
 * exactly zero imaginary part; pptoaslib.py:834-836, 902-904).  Returns the
 * root count or a negative value on failure.  The same code runs on the
 * device inside ppf_fit_batch; this export exists for CPU tests. */
int ppf_poly_real_roots_host(const double *coeffs, int deg, double *out);

/* Host-side (CPU) helper: the exact trust-region subproblem of the Newton
 * solver, min g.p + p.H p / 2 over |p| <= R for a symmetric n x n H
 * (row-major, n <= 5).  Writes p[n]; returns 1 if the step is on the
 * boundary, 0 if interior, negative on a bad argument.  The same code runs
 * on the device; this export exists for CPU tests. */
int ppf_tr_subproblem_host(const double *H, const double *g, int n, double R, double *p);

#ifdef __cplusplus
}
#endif
#endif /* PPFIT_H */
