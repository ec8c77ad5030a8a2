"""Ragged channel counts and per-sub-int masks for every fit kernel family
(TEST INFRASTRUCTURE; no pytest hooks).

Every fit kernel tiles the channel axis (32-channel spectrum blocks in
rounds of 4 or 8 rows, 16-channel MFMA tiles in 64-channel workgroups,
256-channel k_pass workgroups with a warm start on every sub-th 64-channel
group, 128-channel k_dsum blocks, X stored [k][nchan]).  The cases here put
a partial last tile, and masks that empty whole tiles, in front of each
family; tests/test_ragged_inputs.py checks the inputs on the host,
tests/test_gpu_ragged.py the device against the oracle.

Inputs are built on the host only (tests/golden/synth_np.py): a device
synthesis kernel cannot cancel a device bug.  Each case is a batch of four
sub-integrations (different noise seeds, phases and DMs), one per mask of
masks(), fitted in ONE engine.fit_batch call; the oracle fits the kept
channel subset of each."""
import functools
import os
import sys

import numpy as np

import goldens as G

sys.path.insert(0, G.GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import synth_np as S  # noqa: E402

PD, PDG = (1, 1, 0, 0, 0), (1, 1, 1, 0, 0)
PDT, PDTA, ALL = (1, 1, 0, 1, 0), (1, 1, 0, 1, 1), (1, 1, 1, 1, 1)

GUESS_HARMONICS = 448      # harmonics the fused guess of the spectrum pass holds


def _case(family, nbin, nchan, flags, template="cut", guess=False, mom_x=None,
          dtype="f32", noise=1.5, tau=0.0):
    tag = "".join(n for n, f in zip(("p", "d", "g", "t", "a"), flags) if f)
    name = "%s-%dx%d-%s-%s-%s" % (family, nchan, nbin, tag, template, dtype)
    return dict(name=name, family=family, nbin=nbin, nchan=nchan,
                flags=tuple(flags), template=template, guess=guess,
                mom_x=mom_x, dtype=dtype, noise=noise, tau=tau)


# scattering cases: tau = 3e-3 rot injected at 1500 MHz, noise 0.5 (a third
# of the other cases') so that the 1-in-8 mask still constrains tau and alpha
_SC = dict(noise=0.5, tau=3e-3)

CASES = (
    # k_xspec_w2 + k_moments: the GetTOAs guess rides in the spectrum pass,
    # moments from X; 250 channels: 8 blocks (XCD swizzle), the last of 26
    [_case("w2_guess", 2048, n, PD, guess=True, dtype=dt)
     for n in (33, 100, 250) for dt in ("f32", "f64")] +
    # the same with a template that is not cut: the guess through k_dsum_w
    [_case("w2_dsum", 2048, n, PD, template="full", guess=True)
     for n in (100, 250)] +
    # fused k_xmom_g (no guess, moments from the data rows)
    [_case("xmom", 256, 250, PD, mom_x=False),
     _case("xmom", 512, 37, PD, mom_x=False),
     _case("xmom", 1024, 100, PD, mom_x=False),
     _case("xmom", 1024, 100, PDG, mom_x=False),
     _case("xmom", 2048, 161, PD, mom_x=False)] +
    # moments from X forced
    [_case("momx", 512, 100, PD, mom_x=True)] +
    # k_xspec_w + k_pass, warm-start stride 1
    [_case("pass", 512, 97, PDTA, **_SC),
     # (noise 0.2: at 0.5 the oracle restarted 1e-2 sigma from its solution
     # of the group-masked sub-int -- 36 channels above 1600 MHz, five
     # parameters -- stays where it starts: not sharply defined)
     _case("pass", 2048, 100, ALL, noise=0.2, tau=3e-3)] +
    # k_pass warm start: stride 2 with a one-channel last group, stride 4
    # (harmonic split) with a one-channel workgroup
    [_case("warm", 256, 257, PDTA, **_SC),
     _case("warm", 256, 513, PDTA, **_SC)] +
    # mixed-radix wave transforms
    [_case("wm", 1000, 45, PD), _case("wm", 1536, 100, PDTA, **_SC)] +
    # odd nbin: two rows per transform; last blocks of 1 and 5 rows
    [_case("wo", 1001, n, fl, **(kw))
     for n in (33, 37) for fl, kw in ((PD, {}), (PDTA, _SC))] +
    # block-FFT k_xspec: off the wave path by channel count or by nbin
    [_case("blk", 512, 3, PD), _case("blk", 512, 17, PD),
     _case("blk", 512, 17, PDT, **_SC), _case("blk", 512, 31, PD),
     _case("blk", 4096, 45, PD), _case("blk", 128, 45, PD)] +
    # rows past the LDS transforms
    [_case("long", 8194, 5, PD, guess=True)] +
    # 256 channels = 8 spectrum blocks of 32: the smallest count at which the
    # XCD-aware block map (xcd_swizzle) turns on, one case per spectrum kernel
    # that takes it, X consumed by the fit: k_xspec_w, k_xspec_wm (moments
    # from X), k_xspec_wo, k_xspec, k_xspec_any
    [_case("swz", 256, 256, PDTA, **_SC),
     _case("swz", 100, 256, PD, mom_x=True),
     _case("swz", 35, 256, PD), _case("swz", 64, 256, PD),
     _case("swz", 2050, 256, PD)])

CASE_NAMES = [c["name"] for c in CASES]
SWIZZLED = [c["name"] for c in CASES if c["family"] == "swz"]

# the cases whose four masks the host test fits twice each (well-posedness);
# the others fit mask 1 only there
ALL_MASKS_ON_HOST = ("w2_guess-100x2048-pd-cut-f32",
                     "w2_guess-250x2048-pd-cut-f32",
                     "warm-257x256-pdta-cut-f32", "warm-513x256-pdta-cut-f32",
                     "wo-37x1001-pdta-cut-f32")


def case(name):
    return CASES[CASE_NAMES.index(name)]


def warm_stride(nchan):
    """k_tr_init's warm-start stride: the largest power of two <= 16 with
    sub <= ((nchan + 63) / 64) / 2 (integer divisions)."""
    ng = (nchan + 63) // 64
    sub = 1
    while sub * 2 <= 16 and sub * 2 <= ng // 2:
        sub *= 2
    return sub


def masks(nchan, sub, seed=0):
    """[4, nchan] bool, True = channel kept:
    0 nothing masked;
    1 a seeded random 20 % masked, plus the first and the last channel
      (while two channels stay);
    2 every 64-channel group whose index is a multiple of max(sub, 2) masked
      (with sub > 1 the warm start sees no usable channel, and the leading
      block is gone); where that leaves nothing (nchan <= 64) the
      upper-frequency half instead;
    3 every 8th channel and the last kept: one live row per 8-row round."""
    rng = np.random.default_rng(977 + 31 * nchan + seed)
    m = np.ones((4, nchan), dtype=bool)
    m[1, rng.choice(nchan, int(0.2 * nchan), replace=False)] = False
    for n in (0, nchan - 1):
        if m[1].sum() - m[1, n] >= 2:
            m[1, n] = False
    grp = np.arange(nchan) // 64
    m[2] = grp % max(sub, 2) != 0
    if not m[2].any():
        m[2] = np.arange(nchan) < (nchan + 1) // 2
    m[3] = np.arange(nchan) % 8 == 0
    m[3, -1] = True
    return m


def kc(model):
    """k_model_cut's rule restated (as test_gpu_fullshape.
    _kept_harmonic_fraction): per channel 1 + the last k >= 1 with
    |M_k|^2 > 1e-28 max_k |M_k|^2."""
    mp = np.abs(np.fft.rfft(model, axis=1)) ** 2
    mp[:, 0] = 0.0
    above = mp > 1e-28 * mp.max(axis=1, keepdims=True)
    return mp.shape[1] - np.argmax(above[:, ::-1], axis=1)


@functools.lru_cache(maxsize=None)
def template(kind, nchan, nbin):
    """(model [nchan, nbin] f64, freqs): "cut" is the example .gmodel in
    f64, NOT rounded to f32 (its spectrum falls to the f64 rounding floor,
    so k_model_cut cuts, differently from block to block); "full" is
    synth_np.template, rounded to f32 (the rounding noise reaches Nyquist:
    KC = nharm everywhere)."""
    import oracle as O
    if kind == "full":
        return S.template(nchan, nbin)
    code, nu_ref, params, alpha = S.read_gmodel()
    freqs = S.channel_freqs(nchan)
    model = O.gen_gaussian_portrait(code, params, alpha,
                                    O.get_bin_centers(nbin), freqs, nu_ref)
    return model, freqs


@functools.lru_cache(maxsize=None)
def _inputs(nbin, nchan, flags, kind, noise, tau, guess):
    import oracle as O
    model, freqs = template(kind, nchan, nbin)
    seed = 7000 + 13 * nbin + nchan + 100003 * sum(
        f << i for i, f in enumerate(flags))
    rng = np.random.default_rng(seed)
    scat = bool(flags[3] or flags[4])
    keep = masks(nchan, warm_stride(nchan) if scat else 1)
    nsub = len(keep)
    P = S.P0
    data = np.empty((nsub, nchan, nbin))
    truth = np.zeros((nsub, 5))
    init = np.zeros((nsub, 5))
    nu_fit = np.zeros(nsub)
    errs_given = bool((nbin + nchan + sum(flags)) % 2)
    errs = np.zeros((nsub, nchan))
    for i in range(nsub):
        phi = rng.uniform(-0.5, 0.5)
        dDM = rng.normal(3e-4, 2e-4)
        data[i] = S.subint(seed + 1 + i, model, freqs, phi, S.DM0 + dDM, P,
                           noise=noise, tau=tau)
        truth[i] = [phi, S.DM0 + dDM, 0.0, tau, -4.0]
        nu_fit[i] = O.guess_fit_freq(freqs[keep[i]])
        init[i, 0] = O.phase_transform(phi + 2e-3, S.DM0 + dDM, 1500.0,
                                       nu_fit[i], P, mod=True)
        init[i, 1] = S.DM0
        if scat:
            init[i, 3:] = np.log10(1.0 / nbin), -4.0
        # given errors differ from channel to channel and from the noise
        # estimate: a mis-weighted channel shows
        errs[i] = noise * rng.uniform(0.9, 1.1, nchan)
    for a in (data, freqs, keep, init, nu_fit, errs, truth):
        a.setflags(write=False)
    return dict(data=data, model=model, freqs=freqs, keep=keep, P=P,
                truth=truth, init=init, nu_fit=nu_fit,
                errs=errs if errs_given else None, scat=scat, nsub=nsub)


def inputs(c):
    """The batch of a case: data [4, nchan, nbin] (f32-rounded float64),
    model, freqs, keep [4, nchan], P, truth / init [4, 5], nu_fit [4], errs
    [4, nchan] or None (estimated from the data), scat."""
    return _inputs(c["nbin"], c["nchan"], c["flags"], c["template"],
                   c["noise"], c["tau"], c["guess"])


@functools.lru_cache(maxsize=None)
def _oracle_fit(nbin, nchan, flags, kind, noise, tau, guess, i):
    import oracle as O
    b = _inputs(nbin, nchan, flags, kind, noise, tau, guess)
    k = b["keep"][i]
    if guess:
        w = k.astype(float)[None]
        o = O.get_toas_archive(
            b["data"][i:i + 1], b["model"], b["freqs"][None], w,
            np.ones((1, nchan)), np.array([b["P"]]), b["init"][i, 1],
            np.ones(1), noise_stds=None if b["errs"] is None else
            b["errs"][i:i + 1], fit_flags=flags, log10_tau=True)
        assert o["nu_fits"][0, 0] == b["nu_fit"][i]
        return o["fits"][0]
    return O.fit_portrait_full(
        b["data"][i][k], b["model"][k], list(b["init"][i]), b["P"],
        b["freqs"][k], [b["nu_fit"][i]] * 3, [None] * 3,
        None if b["errs"] is None else b["errs"][i][k], list(flags),
        log10_tau=b["scat"])


def oracle_fit(c, i):
    """The oracle's fit of sub-int i's kept channels (arrays over the kept
    channels only): get_toas_archive with zero weights where masked for the
    guess cases, fit_portrait_full from the case's start otherwise."""
    return _oracle_fit(c["nbin"], c["nchan"], c["flags"], c["template"],
                       c["noise"], c["tau"], c["guess"], i)


def oracle_refit(c, i, first):
    """Well-posedness probe: the oracle restarted from its own x_fit plus
    1e-2 sigma in each fitted parameter."""
    import oracle as O
    b = inputs(c)
    k = b["keep"][i]
    x0 = np.asarray(first["x_fit"]) + 1e-2 * np.asarray(first["param_errs"])
    return O.fit_portrait_full(
        b["data"][i][k], b["model"][k], list(x0), b["P"], b["freqs"][k],
        [b["nu_fit"][i]] * 3, [None] * 3,
        None if b["errs"] is None else b["errs"][i][k], list(c["flags"]),
        log10_tau=b["scat"])


def compare_row(label, tag, r, j, o, keep, P, log10_tau):
    """Row j of the device tables r against the oracle fit o of the kept
    channels, at the project's bars (goldens.SIGMA_TOL, goldens.RCHI2_RTOL,
    errors 1e-4, S/N 1e-6, per-channel scales and S/N, zeros where masked);
    shared by tests/test_gpu_ragged.py and tests/test_gpu_mixed.py.  Prints
    one line (label ...) and returns (max deviation in sigma, chi2_red
    rel)."""
    from pulseportraiture_amd import _lib
    I = _lib.RESULT_INDEX
    assert o["return_code"] == 2, tag
    res = r["results"][j]
    assert (int(res[I["status"]]) & 0xff) in (1, 2), (tag, res[I["status"]])
    assert int(res[I["status"]]) >> 8 == 0, (tag, res[I["status"]])
    assert res[I["nchanx"]] == keep.sum(), tag
    assert res[I["dof"]] == o["dof"], tag
    got = dict(params=res[I["params"]], nu_DM=res[I["nu_out"]][0],
               nu_GM=res[I["nu_out"]][1], nu_tau=res[I["nu_out"]][2])
    dev = G.param_deviation_sigma(got, o, P, log10_tau)
    rel = abs(res[I["red_chi2"]] / o["red_chi2"] - 1)
    print("%s kept %d: dev %.2e sigma, chi2_red rel %.1e" %
          (label, keep.sum(), dev.max(), rel))
    assert dev.max() < G.SIGMA_TOL, (tag, dev)
    assert rel < G.RCHI2_RTOL, (tag, rel)
    np.testing.assert_allclose(res[I["param_errs"]], o["param_errs"],
                               rtol=1e-4, err_msg=str(tag))
    np.testing.assert_allclose(res[I["snr"]], o["snr"], rtol=1e-6,
                               err_msg=str(tag))
    np.testing.assert_allclose(r["scale_errs"][j][keep], o["scale_errs"],
                               rtol=1e-4, err_msg=str(tag))
    atol = 1e-3 * np.abs(o["scale_errs"]).min()
    for key in ("scales", "channel_snrs"):
        np.testing.assert_allclose(r[key][j][keep], o[key], rtol=1e-4,
                                   atol=atol, err_msg="%s %s" % (key, tag))
    for key in ("scales", "scale_errs", "channel_snrs"):
        assert np.all(r[key][j][~keep] == 0.0), (key, tag)
    return dev.max(), rel


def device_fit(c, subs=None, over=None):
    """engine.fit_batch on the case's batch (or on the sub-ints subs of it,
    which may repeat) -> dict of numpy arrays.  over: a dict that replaces,
    for the len(subs) sub-ints of the call, any of data [n, nchan, nbin],
    errs [n, nchan], guess_weights [n, nchan], mask [n, nchan] (True =
    kept), flags ([5] or [n, 5]), solver and n_x (tests/degenerate.py);
    what it does not name is the case's own."""
    from pulseportraiture_amd import engine
    b = inputs(c)
    o = {} if over is None else over
    sl = np.arange(b["nsub"]) if subs is None else np.asarray(subs)
    n = len(sl)
    data = np.asarray(o["data"]) if "data" in o else b["data"][sl]
    data = data.astype(np.float32) if c["dtype"] == "f32" else data.copy()
    keep = np.asarray(o["mask"]) if "mask" in o else b["keep"][sl]
    errs = b["errs"]
    if "errs" in o:
        errs = np.array(o["errs"], dtype=float)
    elif errs is not None:
        errs = errs[sl].copy()
    kw = {}
    if c["guess"]:
        gw = np.array(o["guess_weights"], dtype=float) \
            if "guess_weights" in o else keep.astype(float)
        kw = dict(guess=True, guess_weights=gw,
                  guess_DM=b["init"][sl, 1].copy(), guess_Ns=100)
    return engine.results_numpy(engine.fit_batch(
        data, b["model"], np.tile(b["freqs"], (n, 1)), np.full(n, b["P"]),
        b["init"][sl].copy(),
        np.array(o["flags"], dtype=np.int32) if "flags" in o else
        list(c["flags"]),
        nu_fits=np.repeat(b["nu_fit"][sl][:, None], 3, axis=1),
        nu_outs=np.full((n, 3), np.nan), errs=errs,
        chan_mask=keep.astype(np.uint8), log10_tau=b["scat"],
        mom_x=c["mom_x"], solver=o.get("solver"), n_x=o.get("n_x"), **kw))
