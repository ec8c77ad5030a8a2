"""The banded post-pass of the 2048-bin spectrum pass (k_xspec_w2, round 10):
slot i of every lane holds one pair (hl, N - hl) of the band 64 i <= hl < 64
i + 64; the fused guess lives in bands 0 .. 6, the last band is skipped when
it lies past the group's cutoff kw and the noise cutoff N - kc, and a tiled
row with kw <= 512 stores its X from registers, one store per band below kw,
while a higher cutoff keeps the LDS staging.

Templates: one Gaussian component on the example .gmodel's DC term, loc 0.4,
no evolution -- every channel has the same cutoff KC (tests/ragged.kc), which
the FWHM sets; template_for() finds the FWHM of a wanted KC by bisection.
The cutoffs: 64 / 65 (a band boundary either side), 256 / 257 (the noise
edge), 448 / 449 (the last fused-guess value, the first with the guess off),
512 / 513 (the last cutoff stored from registers, the first fallback).

All cases at nbin 2048, nchan 70 (one full block plus a ragged block of 6: a
last round with two live waves), 4 sub-ints with the masks of
tests/test_gpu_xtile.py, noise 0.5 per bin against a component of amplitude
1 (the oracle's S/N of a sub-int: 35 at the narrowest template with every
other channel masked, 140 at the widest).  Each case is held to
the oracle's GetTOAs loop (tests/ragged.compare_row: 0.01 sigma, chi2_red
1e-8 relative, the per-channel tables) and to the same call on the fused
moment pass (mom_x=False, which never touches X) at the bars of
tests/test_gpu_xtile.py."""
import functools

import numpy as np
import pytest

import ragged as R
from ragged import S

NBIN = 2048
NCHAN = 70
NOISE = 0.5
KCS = (64, 65, 256, 257, 448, 449, 512, 513)
LOC = 0.4
TAU = 3e-3                       # injected scattering time [rot] at 1500 MHz
PD, PDT = (1, 1, 0, 0, 0), (1, 1, 0, 1, 0)


def _portrait(fwhm, freqs):
    import oracle as O
    code, nu_ref, params, alpha = S.read_gmodel()
    p = np.array([params[0], 0.0, LOC, 0.0, fwhm, 0.0, 1.0, 0.0])
    return O.gen_gaussian_portrait(code, p, alpha, O.get_bin_centers(NBIN),
                                   freqs, nu_ref)


def _kc1(fwhm):
    return int(R.kc(_portrait(fwhm, S.channel_freqs(NCHAN)[:1]))[0])


@functools.lru_cache(maxsize=None)
def fwhm_for(kc):
    """A FWHM [rot] whose template has the cutoff kc: bisection (the cutoff
    falls as the component widens)."""
    lo, hi = 0.003, 0.08
    assert _kc1(lo) > kc > _kc1(hi), (kc, _kc1(lo), _kc1(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        k = _kc1(mid)
        if k == kc:
            return mid
        if k > kc:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no FWHM found for cutoff %d" % kc)


@functools.lru_cache(maxsize=None)
def template_for(kc):
    freqs = S.channel_freqs(NCHAN)
    m = _portrait(fwhm_for(kc), freqs)
    m.setflags(write=False)
    return m, freqs


def masks():
    """[4, NCHAN] bool, True = kept: none; a whole round of four channels,
    its neighbours and the last channel; a seeded random quarter plus the
    last channel; every other channel (tests/test_gpu_xtile.masks)."""
    rng = np.random.default_rng(4100 + NCHAN)
    m = np.ones((4, NCHAN), dtype=bool)
    m[1, 3:9] = False
    m[1, -1] = False
    m[2, rng.choice(NCHAN, NCHAN // 4, replace=False)] = False
    m[2, -1] = False
    m[3, 1::2] = False
    return m


# key -> (cutoffs of the templates, model index per sub-int, flags per
# sub-int, errs given, guess)
BATCHES = {("sweep", kc): ((kc,), (0, 0, 0, 0), (PD,) * 4, False, True)
           for kc in KCS}
# the register path and the fallback in one launch
BATCHES["two"] = ((64, 513), (0, 1, 1, 0), (PD,) * 4, False, True)
# given errors, with the fused guess and without any guess (GS = false)
BATCHES["errs"] = ((257,), (0, 0, 0, 0), (PD,) * 4, True, True)
BATCHES["noguess"] = ((257,), (0, 0, 0, 0), (PD,) * 4, True, False)
# scattering sub-ints (harmonic-major slots) with the guess fused (257) and
# through the time-domain pass (449), between phase + DM sub-ints
BATCHES["scat"] = ((257, 449), (0, 1, 1, 0), (PD, PDT, PD, PDT), False, True)


@functools.lru_cache(maxsize=None)
def inputs(key):
    import oracle as O
    kcs, mi, kinds, errs_given, guess = BATCHES[key]
    mods = np.stack([template_for(kc)[0] for kc in kcs])
    freqs = template_for(kcs[0])[1]
    keep = masks()
    nsub = len(kinds)
    seed = 8100 + 17 * sum(kcs) + 3 * len(key)
    rng = np.random.default_rng(seed)
    data = np.empty((nsub, NCHAN, NBIN))
    gtau = np.zeros(nsub)
    init = np.zeros((nsub, 5))
    nu_fit = np.zeros(nsub)
    errs = np.zeros((nsub, NCHAN))
    for i, fl in enumerate(kinds):
        scat = bool(fl[3] or fl[4])
        phi, dDM = rng.uniform(-0.5, 0.5), rng.normal(3e-4, 2e-4)
        data[i] = S.subint(seed + 1 + i, mods[mi[i]], freqs, phi, S.DM0 + dDM,
                           S.P0, noise=NOISE, tau=TAU if scat else 0.0)
        nu_fit[i] = O.guess_fit_freq(freqs[keep[i]])
        if scat:
            gtau[i] = 0.8 * TAU * (nu_fit[i] / 1500.0) ** -4.0
        init[i, 1] = S.DM0
        if not guess:
            init[i, 0] = O.phase_transform(phi + 2e-3, S.DM0 + dDM, 1500.0,
                                           nu_fit[i], S.P0, mod=True)
        # given errors differ from channel to channel and from the estimate
        errs[i] = NOISE * rng.uniform(0.9, 1.1, NCHAN)
    out = dict(data=data, models=mods, freqs=freqs, keep=keep,
               mi=np.array(mi, dtype=np.int32),
               flags=np.array(kinds, dtype=np.int32), gtau=gtau, init=init,
               nu_fit=nu_fit, errs=errs)
    for a in out.values():
        a.setflags(write=False)
    out.update(nsub=nsub, errs_given=errs_given, guess=guess)
    return out


@functools.lru_cache(maxsize=None)
def oracle_fit(key, i):
    """The oracle on sub-int i alone (its kept channels, model and flags):
    the GetTOAs loop, or with guess off its fit from the batch's start."""
    import oracle as O
    b = inputs(key)
    k = b["keep"][i]
    flags = tuple(int(f) for f in b["flags"][i])
    model = b["models"][b["mi"][i]]
    if not b["guess"]:
        return O.fit_portrait_full(
            b["data"][i][k], model[k], list(b["init"][i]), S.P0,
            b["freqs"][k], [b["nu_fit"][i]] * 3, [None] * 3,
            b["errs"][i][k] if b["errs_given"] else None, list(flags),
            log10_tau=False)
    o = O.get_toas_archive(
        b["data"][i:i + 1], model, b["freqs"][None], k.astype(float)[None],
        np.ones((1, NCHAN)), np.array([S.P0]), S.DM0, np.ones(1),
        noise_stds=b["errs"][i:i + 1] if b["errs_given"] else None,
        fit_flags=flags, tau_guess=b["gtau"][i], alpha_guess=-4.0,
        log10_tau=False)
    assert o["nu_fits"][0, 0] == b["nu_fit"][i]
    return o["fits"][0]


def device_fit(key, dtype, **kw):
    from pulseportraiture_amd import engine
    b = inputs(key)
    n = b["nsub"]
    init = b["init"].copy()
    scat = b["gtau"] != 0.0
    init[scat, 3] = b["gtau"][scat]
    init[scat, 4] = -4.0
    data = b["data"].astype(np.float32) if dtype == "f32" else b["data"].copy()
    args = dict(nu_fits=np.repeat(b["nu_fit"][:, None], 3, axis=1),
                nu_outs=np.full((n, 3), np.nan),
                errs=b["errs"].copy() if b["errs_given"] else None,
                chan_mask=b["keep"].astype(np.uint8),
                model_index=b["mi"].copy(), log10_tau=False)
    if b["guess"]:
        args.update(guess=True, guess_weights=b["keep"].astype(float),
                    guess_DM=np.full(n, S.DM0), guess_Ns=100,
                    guess_tau=b["gtau"].copy())
    args.update(kw)
    return engine.results_numpy(engine.fit_batch(
        data, b["models"], np.tile(b["freqs"], (n, 1)), np.full(n, S.P0), init,
        b["flags"].copy(), **args))


def _check(key, dtype, r):
    """r against the oracle and against the fused moment pass (the bars of
    tests/test_gpu_xtile._check)."""
    from pulseportraiture_amd import _lib
    b = inputs(key)
    for i in range(b["nsub"]):
        R.compare_row("%s %s sub-int %d" % (key, dtype, i), (key, dtype, i), r,
                      i, oracle_fit(key, i), b["keep"][i], S.P0, False)
    f = device_fit(key, dtype, mom_x=False)
    I = _lib.RESULT_INDEX
    ra, rb = f["results"], r["results"]
    err = ra[:, I["param_errs"]]
    dp = np.abs(rb[:, I["params"]] - ra[:, I["params"]])
    dp[:, 0] = np.abs((dp[:, 0] + 0.5) % 1.0 - 0.5)
    ok = err > 0
    print("%s %s vs fused moments: max %.2e sigma" %
          (key, dtype, (dp[ok] / err[ok]).max()))
    assert np.all(dp[ok] <= 1e-3 * err[ok]), (dp, err)
    np.testing.assert_allclose(rb[:, I["red_chi2"]], ra[:, I["red_chi2"]],
                               rtol=1e-10)
    np.testing.assert_allclose(r["scales"], f["scales"], rtol=1e-7, atol=0)


def test_templates_have_the_cutoffs():
    """Every channel of template_for(kc) has the cutoff kc (R.kc restates
    k_model_cut); runs without a GPU."""
    for kc in KCS:
        m, _ = template_for(kc)
        got = R.kc(m)
        assert (got == kc).all(), (kc, fwhm_for(kc), got)
    assert R.GUESS_HARMONICS == 448


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kc", KCS)
def test_cutoff_sweep(kc, dtype):
    key = ("sweep", kc)
    _check(key, dtype, device_fit(key, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_register_and_staged_rows_in_one_launch(dtype):
    """model_index mixes the KC = 64 and the KC = 513 template: tiled rows
    stored from registers and through the LDS staging in one launch."""
    _check("two", dtype, device_fit("two", dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["errs", "noguess"])
def test_given_errors(key):
    """KC = 257 with errs given (the noise sum is formed and not used): with
    the fused guess, and with guess off (the GS = false instantiation)."""
    _check(key, "f32", device_fit(key, "f32"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_scattering_subints_between_moment_ones(dtype):
    """Harmonic-major slots (flags 1,1,0,1,0) at KC = 257 and 449 next to
    tiled ones in one call."""
    from pulseportraiture_amd import engine
    b = inputs("scat")
    init = np.zeros((b["nsub"], 5))
    init[:, 3] = b["gtau"]
    assert engine.x_subints(b["flags"], init, False, b["nsub"]) == 2
    _check("scat", dtype, device_fit("scat", dtype))


@pytest.mark.gpu
def test_same_call_twice_is_bit_identical():
    for key in ("two", "scat"):
        a, c = device_fit(key, "f32"), device_fit(key, "f32")
        for t in ("results", "scales", "scale_errs", "channel_snrs"):
            np.testing.assert_array_equal(a[t], c[t], err_msg=str((key, t)))
