"""The tiled cross spectrum of the 2048-bin spectrum pass (k_xspec_w2 ->
k_moments): the moment-mode sub-ints' X slots hold X[k/8][n][k%8], written by
the wave that transformed the row with no barrier in the round loop, and
k_moments reads whole tiles; scattering sub-ints of the same call keep
harmonic-major slots.  Every case is at nbin = 2048 (the kernel exists for
1024-point rows only), 4-5 sub-ints, GetTOAs guess on.

Shapes: nchan 5 (fewer channels than a block: off the wave path, the
harmonic-major fallback), 37 (a last block of 5: a last round with one live
wave), 64 (two whole blocks), 70 (a last block of 6: a last round with two
live waves; the block ends inside a 64-channel cutoff group), 130 (three
cutoff groups, a last block of 2).  Rows float32 and float64.  Masks differ
between the sub-ints of a call: none; a whole round of four channels, the
round's neighbours and the last channel (the clamped prefetch address); a
seeded random quarter plus the last channel; every other channel.  Templates,
both in every call through model_index: tests/ragged.py's "cut" (the example
.gmodel: every cutoff <= 448, the guess rides in the spectrum pass) and
"narrow" (one more component of FWHM 0.005 rot at 1500 MHz whose width grows
with frequency: cutoffs between ~520 and ~700, different from channel to
channel and mostly no multiple of 8: the fused guess is off for those
sub-ints, kw > 512 stores the high harmonics, and the last tile is padded).

Each case holds the device to the oracle's GetTOAs loop on the same inputs
(tests/ragged.compare_row: parameters within 0.01 sigma, chi2_red 1e-8
relative, and the per-channel tables), and to the same call on the fused
moment pass (mom_x=False, which never touches X) at the tolerance of
test_gpu_parity.test_moments_from_x_equal_fused_pass."""
import functools

import numpy as np
import pytest

import ragged as R
from ragged import S

pytestmark = pytest.mark.gpu

NBIN = 2048
NCHANS = (5, 37, 64, 70, 130)
# loc, its slope, FWHM [rot], its power-law index, amplitude, its index
NARROW_COMPONENT = (0.62, 0.0, 0.005, 0.6, 3.0, -1.0)
MODEL_INDEX = (0, 1, 1, 0)
TAU = 3e-3                       # injected scattering time [rot] at 1500 MHz
PD, PDT, PDTA = (1, 1, 0, 0, 0), (1, 1, 0, 1, 0), (1, 1, 0, 1, 1)
# the mixed call: moment-mode and streaming sub-ints interleaved, sub-int 0
# a moment fit, the last one streaming; model 1 (narrow) on a moment sub-int
MIXED_KINDS = (PD, PDTA, PD, PDT, PD)
MIXED_MODELS = (0, 0, 1, 0, 1)
MIXED_NCHAN = 70


@functools.lru_cache(maxsize=None)
def models(nchan):
    """([2, nchan, NBIN] f64, freqs): cut, narrow."""
    import oracle as O
    cut, freqs = R.template("cut", nchan, NBIN)
    code, nu_ref, params, alpha = S.read_gmodel()
    narrow = O.gen_gaussian_portrait(
        code, np.concatenate([params, NARROW_COMPONENT]), alpha,
        O.get_bin_centers(NBIN), freqs, nu_ref)
    m = np.stack([cut, narrow])
    m.setflags(write=False)
    return m, freqs


def masks(nchan):
    """[4, nchan] bool, True = kept (see the module text)."""
    rng = np.random.default_rng(4100 + nchan)
    m = np.ones((4, nchan), dtype=bool)
    if nchan >= 16:
        m[1, 3:9] = False            # round 1 of block 0 (channels 4-7) and its neighbours
    m[1, -1] = False
    m[2, rng.choice(nchan, nchan // 4, replace=False)] = False
    m[2, -1] = False
    m[3, 1::2] = False
    assert (m.sum(axis=1) >= 2).all()
    return m


@functools.lru_cache(maxsize=None)
def inputs(nchan):
    """The plain batch: four phase + DM sub-ints."""
    mods, freqs = models(nchan)
    keep = masks(nchan)
    nsub = len(keep)
    rng = np.random.default_rng(5200 + nchan)
    data = np.empty((nsub, nchan, NBIN))
    for i in range(nsub):
        data[i] = S.subint(5300 + 10 * nchan + i, mods[MODEL_INDEX[i]], freqs,
                           rng.uniform(-0.5, 0.5),
                           S.DM0 + rng.normal(3e-4, 2e-4), S.P0)
    out = dict(data=data, models=mods, freqs=freqs, keep=keep,
               mi=np.array(MODEL_INDEX, dtype=np.int32),
               flags=np.tile(PD, (nsub, 1)).astype(np.int32),
               gtau=np.zeros(nsub))
    for a in out.values():
        a.setflags(write=False)
    out["nsub"] = nsub
    return out


@functools.lru_cache(maxsize=None)
def mixed_inputs():
    """The mixed batch: MIXED_KINDS at MIXED_NCHAN channels; the scattering
    sub-ints carry TAU (noise 0.5, as tests/ragged.py's) and start from 0.8
    of it at their nu_fit, linear tau."""
    import oracle as O
    nchan = MIXED_NCHAN
    mods, freqs = models(nchan)
    nsub = len(MIXED_KINDS)
    keep = masks(nchan)[[0, 2, 1, 0, 2]]
    rng = np.random.default_rng(6200)
    data = np.empty((nsub, nchan, NBIN))
    gtau = np.zeros(nsub)
    for i, fl in enumerate(MIXED_KINDS):
        scat = bool(fl[3] or fl[4])
        data[i] = S.subint(6300 + i, mods[MIXED_MODELS[i]], freqs,
                           rng.uniform(-0.5, 0.5),
                           S.DM0 + rng.normal(3e-4, 2e-4), S.P0,
                           noise=0.5 if scat else 1.5, tau=TAU if scat else 0.0)
        if scat:
            nu_fit = O.guess_fit_freq(freqs[keep[i]])
            gtau[i] = 0.8 * TAU * (nu_fit / 1500.0) ** -4.0
    out = dict(data=data, models=mods, freqs=freqs, keep=keep,
               mi=np.array(MIXED_MODELS, dtype=np.int32),
               flags=np.array(MIXED_KINDS, dtype=np.int32), gtau=gtau)
    for a in out.values():
        a.setflags(write=False)
    out["nsub"] = nsub
    return out


def _batch(key):
    return mixed_inputs() if key == "mixed" else inputs(key)


@functools.lru_cache(maxsize=None)
def oracle_fit(key, i):
    """The oracle's GetTOAs loop on sub-int i alone (its kept channels, its
    own model and flags; the float32-rounded data serve both row types)."""
    import oracle as O
    b = _batch(key)
    nchan = b["data"].shape[1]
    o = O.get_toas_archive(
        b["data"][i:i + 1], b["models"][b["mi"][i]], b["freqs"][None],
        b["keep"][i].astype(float)[None], np.ones((1, nchan)),
        np.array([S.P0]), S.DM0, np.ones(1),
        fit_flags=tuple(int(f) for f in b["flags"][i]),
        tau_guess=b["gtau"][i], alpha_guess=-4.0, log10_tau=False)
    return o["fits"][0], float(o["nu_fits"][0, 0])


def device_fit(key, dtype, **kw):
    from pulseportraiture_amd import engine
    b = _batch(key)
    n = b["nsub"]
    nu_fit = np.array([oracle_fit(key, i)[1] for i in range(n)])
    init = np.zeros((n, 5))
    init[:, 1] = S.DM0
    scat = b["gtau"] != 0.0
    init[scat, 3] = b["gtau"][scat]
    init[scat, 4] = -4.0
    data = b["data"].astype(np.float32) if dtype == "f32" else b["data"].copy()
    args = dict(nu_fits=np.repeat(nu_fit[:, None], 3, axis=1),
                nu_outs=np.full((n, 3), np.nan),
                chan_mask=b["keep"].astype(np.uint8),
                model_index=b["mi"].copy(), log10_tau=False, guess=True,
                guess_weights=b["keep"].astype(float),
                guess_DM=np.full(n, S.DM0), guess_Ns=100,
                guess_tau=b["gtau"].copy())
    args.update(kw)
    return engine.results_numpy(engine.fit_batch(
        data, b["models"], np.tile(b["freqs"], (n, 1)), np.full(n, S.P0), init,
        b["flags"].copy(), **args))


def _check(key, dtype, r):
    """r against the oracle and against the fused moment pass."""
    from pulseportraiture_amd import _lib
    b = _batch(key)
    for i in range(b["nsub"]):
        o, _ = oracle_fit(key, i)
        R.compare_row("%s %s sub-int %d" % (key, dtype, i), (key, dtype, i), r,
                      i, o, b["keep"][i], S.P0, False)
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


def test_templates_are_what_the_cases_need():
    """The cut template's cutoffs stay inside the fused guess (448
    harmonics); the narrow one's pass 512 in some channels, differ between
    channels and are no multiples of 8 (R.kc restates k_model_cut)."""
    for nchan in NCHANS:
        mods, _ = models(nchan)
        kc_cut, kc_nar = R.kc(mods[0]), R.kc(mods[1])
        assert kc_cut.max() <= R.GUESS_HARMONICS, (nchan, kc_cut.max())
        assert kc_nar.max() > 512 and kc_nar.max() < NBIN // 2, (nchan, kc_nar)
        assert (kc_nar % 8 != 0).any(), (nchan, kc_nar)
        if nchan > 5:
            assert len(set(kc_nar)) > 1, (nchan, kc_nar)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nchan", NCHANS)
def test_tiled_x_matches_oracle_and_fused_moments(nchan, dtype):
    _check(nchan, dtype, device_fit(nchan, dtype))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_tiled_and_harmonic_major_slots_in_one_call(dtype):
    """Phase + DM sub-ints (tiled slots, k_moments) interleaved with
    scattering ones (harmonic-major slots, k_pass) in one call."""
    from pulseportraiture_amd import engine
    b = mixed_inputs()
    init = np.zeros((b["nsub"], 5))
    init[:, 3] = b["gtau"]
    assert engine.x_subints(b["flags"], init, False, b["nsub"]) == 2
    _check("mixed", dtype, device_fit("mixed", dtype))


def test_x_subints_smaller_than_nsub_changes_nothing():
    """With the moments taken from X every sub-int holds a slot whatever
    n_x says (ppfit.h, PPF_OPT_MOM_X): the tables are those of the default
    call bit for bit, for the plain batch and for the mixed one."""
    for key in (70, "mixed"):
        a = device_fit(key, "f32")
        for n_x in (0, 1):
            if key == "mixed" and n_x == 0:
                continue             # (a promise of no streaming fit)
            c = device_fit(key, "f32", n_x=n_x)
            for t in ("results", "scales", "scale_errs", "channel_snrs"):
                np.testing.assert_array_equal(a[t], c[t], err_msg=str((key, n_x, t)))
