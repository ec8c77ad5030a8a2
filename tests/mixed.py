"""Mixed per-sub-int fit configurations in ONE engine.fit_batch call, for
every kernel family (TEST INFRASTRUCTURE; no pytest hooks).

ppf_fit_batch routes each sub-int on the device: k_classify marks the
sub-ints that stream the cross spectrum X and compacts their X slots,
k_tr_init sorts them into moment mode and streaming (k_pass) mode and counts
both kinds for the host's iteration loop, k_gflag decides per sub-int (by
kind and by its own model's harmonic cutoff) whether the GetTOAs guess rides
in the spectrum pass or goes through k_dsum_w.  The batches here vary, inside
one call, fit_flags (moment and streaming kinds interleaved, so the X slots
are a real compaction and the last sub-int streams), model_index (three
models, a non-monotone order with repeats), P, freqs, nu_fits, nu_outs and
the channel mask.  tests/test_mixed_inputs.py checks them on the host,
tests/test_gpu_mixed.py the device against the oracle's fit of each sub-int
alone.

Inputs come from tests/golden/synth_np.py only (host; write-protected and
cached); the templates, masks and warm-start stride are tests/ragged.py's."""
import functools

import numpy as np

import ragged as R
from ragged import S

# kind -> (fit_flags, streams X)
KINDS = {
    "P": ((1, 0, 0, 0, 0), False), "PD": ((1, 1, 0, 0, 0), False),
    "PDG": ((1, 1, 1, 0, 0), False), "PG": ((1, 0, 1, 0, 0), False),
    "PDT": ((1, 1, 0, 1, 0), True), "PDTA": ((1, 1, 0, 1, 1), True),
    # phase and DM held at the truth
    "TA": ((0, 0, 0, 1, 1), True),
    # phase + DM with tau held at a nonzero value: k_pass, two parameters
    "PDfix": ((1, 1, 0, 0, 0), True),
    "ALL": ((1, 1, 1, 1, 1), True), "PDGT": ((1, 1, 1, 1, 0), True),
}

# streaming and moment kinds interleaved; sub-int 0 is a moment fit, so no
# streaming sub-int's X slot is its index; the last sub-int streams
ORDER = ("P", "PDT", "PDTA", "PD", "PDG", "TA", "PG", "PDfix")
# guess batches: the phase is always fitted (a held phase would be the
# device's own guess), so TA is left out
ORDER_GUESS = ("P", "PDT", "PDTA", "PD", "PDG", "PDfix", "PG", "PDT")
# (streaming kinds on the unmasked sub-ints: mask 1 leaves 2 of 5 channels)
ORDER_LONG = ("PDT", "P", "PDfix", "PD", "PDT")
ORDER_SCAT = ("PDTA", "PDT", "TA", "ALL", "PDGT", "PDfix")
# bounds batches: a box on the rows marked True, all-NaN rows elsewhere
ORDER_BOUNDS = ("PDTA", "PD", "TA", "PDT", "PDTA", "PDG", "TA", "PDTA")
BOXED = (True, False, True, False, True, False, True, False)

# models: ragged's "cut", its "full", "cut" rotated by ROT; non-monotone
# order with repeats
MODEL_INDEX = (2, 0, 2, 1, 0, 1, 2, 0)
ROT = 0.123
ALPHA_UPPER = -4.5     # active: the data are injected with alpha = -4.0
TAU = 3e-3             # injected scattering time [rot] at 1500 MHz


def _batch(name, nchan, nbin, order, log10_tau=False, option=0, guess=False,
           mom_x=None, boxed=None, data_key=None):
    return dict(name=name, nchan=nchan, nbin=nbin, order=tuple(order),
                log10_tau=log10_tau, option=option, guess=guess, mom_x=mom_x,
                boxed=boxed, data_key=data_key or name)


BATCHES = (
    # fused k_xmom_g, X only for the streaming sub-ints
    _batch("fused-37x512", 37, 512, ORDER, mom_x=False),
    _batch("fused-100x1024", 100, 1024, ORDER, mom_x=False),
    # moments from X forced
    _batch("momx-100x512", 100, 512, ORDER, mom_x=True),
    # guess in the spectrum pass, default moments from X: gflag by model
    _batch("guess-100x2048", 100, 2048, ORDER_GUESS, guess=True),
    # guess with fused moments: gflag by kind and by model (same inputs)
    _batch("guessf-100x2048", 100, 2048, ORDER_GUESS, guess=True,
           mom_x=False, data_key="guess-100x2048"),
    # mixed-radix wave, odd nbin, block FFT, rows past the LDS transforms
    _batch("wm-45x1000", 45, 1000, ORDER),
    _batch("wo-33x1001", 33, 1001, ORDER),
    _batch("blk-17x512", 17, 512, ORDER),
    _batch("blk-45x4096", 45, 4096, ORDER),
    _batch("long-5x8194", 5, 8194, ORDER_LONG),
    # all-scattering, log10 tau; 257 channels: k_pass warm start, stride 2
    _batch("scat-257x256", 257, 256, ORDER_SCAT, log10_tau=True),
    _batch("scat-97x512", 97, 512, ORDER_SCAT, log10_tau=True),
    _batch("scat1-257x256", 257, 256, ORDER_SCAT, log10_tau=True, option=1,
           data_key="scat-257x256"),
    _batch("scat1-97x512", 97, 512, ORDER_SCAT, log10_tau=True, option=1,
           data_key="scat-97x512"),
    # method='TNC' boxes on half the rows
    _batch("bounds-37x512", 37, 512, ORDER_BOUNDS, boxed=BOXED),
    _batch("bounds-97x512", 97, 512, ORDER_BOUNDS, boxed=BOXED),
)
NAMES = [b["name"] for b in BATCHES]
MIXED_KIND = [b["name"] for b in BATCHES if not b["log10_tau"]]
ORACLE_NAMES = [b["name"] for b in BATCHES if not b["boxed"]]
BOUNDS_NAMES = [b["name"] for b in BATCHES if b["boxed"]]
WAVE_NAMES = ["fused-37x512", "fused-100x1024", "guess-100x2048",
              "guessf-100x2048"]
NO_X_NAMES = ["blk-45x4096", "momx-100x512", "guess-100x2048"]
TABLES = ("results", "scales", "scale_errs", "channel_snrs", "covariance")


def batch(name):
    return BATCHES[NAMES.index(name)]


def flags(c):
    return np.array([KINDS[k][0] for k in c["order"]], dtype=np.int32)


def streams(c):
    """Which sub-ints stream X (k_classify's test; with log10_tau every
    sub-int does: 10**x is never 0)."""
    return np.array([KINDS[k][1] or c["log10_tau"] for k in c["order"]])


def _noise(kind, boxed):
    """Noise per channel sample, chosen as tests/ragged.py had to: 1.5 for
    the phase/DM/GM fits, 0.5 where tau is fitted (so that a 20 % mask still
    constrains tau and alpha), 0.2 for the fits of GM with tau (flat
    directions otherwise) and for the boxed rows (the bound at alpha = -4.5
    must be active beyond doubt: high S/N)."""
    if boxed or kind in ("ALL", "PDGT"):
        return 0.2
    return 0.5 if KINDS[kind][1] else 1.5


@functools.lru_cache(maxsize=None)
def models(nchan, nbin):
    """([3, nchan, nbin] f64, freqs): cut, full, cut rotated by ROT, on one
    frequency axis."""
    cut, freqs = R.template("cut", nchan, nbin)
    full, f2 = R.template("full", nchan, nbin)
    assert np.array_equal(freqs, f2)
    m = np.stack([cut, full, S.rotate(cut, np.full(nchan, ROT))])
    m.setflags(write=False)
    return m, freqs


@functools.lru_cache(maxsize=None)
def _inputs(key):
    import oracle as O
    c = batch(key)
    nchan, nbin, order = c["nchan"], c["nbin"], c["order"]
    nsub = len(order)
    lt = c["log10_tau"]
    mods, freqs0 = models(nchan, nbin)
    boxed = c["boxed"] or (False,) * nsub
    seed = 9100 + 17 * nbin + nchan + 1009 * len(key)
    rng = np.random.default_rng(seed)
    sub = R.warm_stride(nchan) if lt else 1
    mi = np.array(MODEL_INDEX[:nsub], dtype=np.int32)
    fl = flags(c)
    data = np.empty((nsub, nchan, nbin))
    keep = np.empty((nsub, nchan), dtype=bool)
    freqs = np.empty((nsub, nchan))
    P = np.empty(nsub)
    truth, init = np.zeros((nsub, 5)), np.zeros((nsub, 5))
    nu_fits = np.empty((nsub, 3))
    nu_outs = np.full((nsub, 3), np.nan)
    errs = np.empty((nsub, nchan))
    gtau = np.zeros(nsub)
    bounds = np.full((nsub, 5, 2), np.nan)
    for i, kind in enumerate(order):
        scat = KINDS[kind][1]
        noise = _noise(kind, boxed[i])
        # ragged's mask 0 and mask 1 alternate (mask 1 reseeded per sub-int)
        keep[i] = R.masks(nchan, sub, seed=i)[i % 2]
        freqs[i] = freqs0 + 1.5 * i - 4.0       # the band shifted, per sub-int
        P[i] = S.P0 * (1.0 + 0.01 * i)
        phi = rng.uniform(-0.5, 0.5)
        DM = S.DM0 + rng.normal(3e-4, 2e-4)
        tau = TAU if scat else 0.0
        data[i] = S.subint(seed + 1 + i, mods[mi[i]], freqs[i], phi, DM, P[i],
                           noise=noise, tau=tau)
        truth[i] = [phi, DM, 0.0, tau, -4.0 if scat else 0.0]
        nf = O.guess_fit_freq(freqs[i][keep[i]])
        nu_fits[i] = nf
        if not c["guess"] and i % 3 == 1:
            nu_fits[i] = nf + 15.0, nf + 15.0, nf - 40.0
        elif not c["guess"] and i % 4 == 3 and not scat and nchan > 8:
            # the mean of the kept channels.  Not for a scattering sub-int:
            # with an odd number of evenly spaced channels the mean IS the
            # middle channel, ln(nu_n / nu_tau) = 0 there, and the
            # reference's Hessian divides by it (NaN)
            nu_fits[i] = np.nan
        nfd = [freqs[i][keep[i]].mean() if np.isnan(v) else v
               for v in nu_fits[i]]
        # (no reference frequency equals a channel's, for the same reason)
        if i % 3 == 1:
            nu_outs[i] = 1400.3 + 7 * i, 1400.3 + 7 * i, 1350.7 + 7 * i
        elif i % 3 == 2:
            nu_outs[i, 2] = 1487.3
        held = not fl[i, 0]
        init[i, 0] = O.phase_transform(phi + (0.0 if held else 2e-3), DM,
                                       1500.0, nfd[0], P[i], mod=True)
        init[i, 1] = S.DM0 if fl[i, 1] else DM
        if scat:
            t_fit = TAU * (nfd[2] / 1500.0) ** -4.0
            # (boxed rows start tau at the injected value: from 0.8 of it
            # scipy's TNC ran into its 100 evaluations on one PDTA row and
            # ended the TA rows with "linear search failed")
            t0 = t_fit * (0.8 if fl[i, 3] and not boxed[i] else 1.0)
            init[i, 3:] = (np.log10(t0) if lt else t0), -4.0
            gtau[i] = t0
        elif lt:
            raise ValueError("log10_tau batches hold scattering kinds only")
        if c["guess"]:
            init[i, 0] = 0.0                  # replaced by the device's guess
            init[i, 1] = S.DM0                # DM_stored
        if boxed[i]:
            bounds[i, 1] = S.DM0 - 0.01, S.DM0 + 0.01
            bounds[i, 4, 1] = ALPHA_UPPER
        errs[i] = noise * rng.uniform(0.9, 1.1, nchan)
    out = dict(data=data, models=mods, mi=mi, freqs=freqs, keep=keep, P=P,
               truth=truth, init=init, flags=fl, nu_fits=nu_fits,
               nu_outs=nu_outs, errs=errs, gtau=gtau, bounds=bounds)
    for a in out.values():
        a.setflags(write=False)
    out.update(errs_given=bool((nbin + nchan) % 2), nsub=nsub,
               boxed=tuple(boxed))
    return out


def inputs(c):
    """The batch's host inputs: data [nsub, nchan, nbin] (f32-rounded f64),
    models [3, nchan, nbin], mi, freqs / keep / errs [nsub, nchan], P, truth
    / init / flags [nsub, 5], nu_fits / nu_outs [nsub, 3] (NaN = default),
    gtau (guess tau [rot]), bounds [nsub, 5, 2] (NaN = none), errs_given."""
    return _inputs(c["data_key"])


def _opt(row):
    return [None if np.isnan(v) else float(v) for v in row]


@functools.lru_cache(maxsize=None)
def guess_phase(key, i):
    """GetTOAs' phase guess of sub-int i (pptoas.py:384-492 as
    oracle.get_toas_archive restates it) against the sub-int's own model."""
    import oracle as O
    c = batch(key)
    b = inputs(c)
    k = b["keep"][i]
    fx, px, mx = b["freqs"][i][k], b["data"][i][k], b["models"][b["mi"][i]][k]
    nu_mean = fx.mean()
    rot = O.rotate_data(px, 0.0, S.DM0, b["P"][i], fx, nu_mean)
    prof = np.average(rot, axis=0, weights=np.ones(len(fx)))
    mprof = mx.mean(axis=0)
    if b["gtau"][i]:
        kk = np.arange(c["nbin"] // 2 + 1)
        B = 1.0 / (1.0 + 2j * np.pi * b["gtau"][i] * kk)
        mprof = np.fft.irfft(B * np.fft.rfft(mprof), n=c["nbin"])
    ph = O.fit_phase_shift(prof, mprof, Ns=100)["phase"]
    return float(O.phase_transform(ph, S.DM0, nu_mean, b["nu_fits"][i, 0],
                                   b["P"][i], mod=True))


def start(c, i):
    """The parameters sub-int i's fit starts from."""
    x0 = inputs(c)["init"][i].copy()
    if c["guess"]:
        x0[0] = guess_phase(c["data_key"], i)
    return x0


def _fit(c, i, x0, bounded, maxiter=None):
    import oracle as O
    b = inputs(c)
    k = b["keep"][i]
    kw = {}
    if bounded:
        kw = dict(method="TNC", bounds=[tuple(_opt(r)) for r in b["bounds"][i]])
    return O.fit_portrait_full(
        b["data"][i][k], b["models"][b["mi"][i]][k], list(x0), b["P"][i],
        b["freqs"][i][k], _opt(b["nu_fits"][i]), _opt(b["nu_outs"][i]),
        b["errs"][i][k] if b["errs_given"] else None,
        [int(f) for f in b["flags"][i]], log10_tau=c["log10_tau"],
        option=c["option"], maxiter=maxiter, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_fit(name, i, bounded, maxiter):
    c = batch(name)
    return _fit(c, i, start(c, i), bounded, maxiter)


def oracle_fit(c, i, bounded=None, maxiter=None):
    """The oracle's fit of sub-int i alone: its kept channels, its own model,
    flags, P, freqs, nu_fits, nu_outs and the batch's option; trust-ncg, or
    TNC under the sub-int's box (bounded; default: where the row has one)."""
    if bounded is None:
        bounded = inputs(c)["boxed"][i]
    return _oracle_fit(c["name"], i, bool(bounded), maxiter)


def oracle_refit(c, i, first):
    """Well-posedness probe: the oracle restarted from its own x_fit plus
    1e-2 sigma in each fitted parameter."""
    x0 = np.asarray(first["x_fit"]) + 1e-2 * np.asarray(first["param_errs"])
    return _fit(c, i, x0, inputs(c)["boxed"][i])


def device_fit(c, subs=None, single_model=False, bounds="own", raw=False,
               **kw):
    """engine.fit_batch on the batch, or on its sub-ints subs in that order
    -> dict of numpy tables (raw: the device dict as well).  single_model:
    subs is one sub-int and its own model goes in as nmodel = 1.  bounds:
    "own" (the batch's box table where it has one) or None.  kw overrides
    engine.fit_batch's keywords (n_x, max_workspace, workspace, solver,
    max_iter)."""
    from pulseportraiture_amd import engine
    b = inputs(c)
    sl = np.arange(b["nsub"]) if subs is None else np.asarray(subs)
    n = len(sl)
    if single_model:
        assert n == 1
        model, mi = b["models"][b["mi"][sl[0]]], None
    else:
        model, mi = b["models"], b["mi"][sl].copy()
    args = dict(nu_fits=b["nu_fits"][sl].copy(),
                nu_outs=b["nu_outs"][sl].copy(),
                errs=b["errs"][sl].copy() if b["errs_given"] else None,
                chan_mask=b["keep"][sl].astype(np.uint8), model_index=mi,
                log10_tau=c["log10_tau"], option=c["option"],
                mom_x=c["mom_x"])
    if c["guess"]:
        args.update(guess=True, guess_weights=b["keep"][sl].astype(float),
                    guess_DM=np.full(n, S.DM0), guess_Ns=100,
                    guess_tau=b["gtau"][sl].copy())
    if c["boxed"] and bounds == "own":
        args["bounds"] = b["bounds"][sl].copy()
    args.update(kw)
    res = engine.fit_batch(
        b["data"][sl].astype(np.float32), model, b["freqs"][sl].copy(),
        b["P"][sl].copy(), b["init"][sl].copy(), b["flags"][sl].copy(),
        **args)
    out = engine.results_numpy(res)
    return (out, res) if raw else out


def x_subints(c):
    from pulseportraiture_amd import engine
    b = inputs(c)
    return engine.x_subints(b["flags"], b["init"], c["log10_tau"], b["nsub"])
