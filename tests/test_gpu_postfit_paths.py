"""The two post-fit kernels against the f64 oracle, on every path they take.

k_postfit_mom serves the sub-ints without scattering (phase / DM / GM
fitted): it forms the channel powers nu^-2, nu^-4 once per channel, and only
those a fitted parameter or the zero-covariance case reads.  k_postfit serves
the scattering fits.  A batch may hold both kinds and unfitted sub-ints.
The cases here reach every zero-covariance branch a flag mask selects
(get_nu_zeros: 0x3, 0x5, 0x7 with option 0 and 1 in k_postfit_mom; 0x18,
0x1b, 0x1f in k_postfit), given and default nu_outs, is_toa false, the
two-parameter legacy mode, one partial wave (20 channels), one full wave,
80 channels with a different mask per sub-int, and a sub-int wide enough
(2100 channels) for the 256-thread form, whose powers are recomputed per loop.

Bars: the project's (goldens.SIGMA_TOL = 0.01 sigma on the parameters,
goldens.RCHI2_RTOL on chi2_red), through ragged.compare_row, which also
compares param_errs, S/N, scales, scale_errs and channel_snrs; the covariance
block and nu_out are compared here at the bars of the errors (1e-4) and of
the mixed tests' nu_out (1e-5).

The CPU tests show what the comparison notices of a wrongly skipped power,
on the oracle alone (its frequency axis replaced by one whose nu ** -4 or
log is zero): nu_tau moves to 1 MHz without the ln(nu) weights; without the
nu^-4 weights the zero-covariance search has no finite answer (shown
explicitly); scale_errs move by 7e-4 and 1.5e-3 without nu^-4 in a DM + GM
fit of 20 and 32 channels (3.8e-5 at 64: below the 1e-4 bar, hence those
widths), and are not finite without the log term of an alpha fit.  Seeds:
those of _batch (SEED)."""
import functools

import numpy as np
import pytest

import goldens as G
import ragged as R
from ragged import S

gpu = pytest.mark.gpu

NBIN = 256
SEED = 4242
TAU = 3e-3
MOM = {"P": (1, 0, 0, 0, 0), "D": (0, 1, 0, 0, 0), "PD": (1, 1, 0, 0, 0),
       "PG": (1, 0, 1, 0, 0), "PDG": (1, 1, 1, 0, 0), "DG": (0, 1, 1, 0, 0)}
SCAT = {"PDTA": (1, 1, 0, 1, 1), "ALL": (1, 1, 1, 1, 1), "TA": (0, 0, 0, 1, 1)}
KIND = dict(MOM, **SCAT)
# sub-int kinds of a moment batch; the trailing "PD+" has its nu_outs given
MOM_ORDER = ("P", "D", "PD", "PG", "PDG", "PD+")
SCAT_ORDER = ("PDTA", "ALL", "TA")
SCAT_GIVEN = ("PDTA+", "TA+")          # scattering fits with their nu_outs given
# moment and scattering kinds in one call, one sub-int with every channel
# masked ("none": PPF_ST_NOFIT)
MIX_ORDER = ("PD", "PDTA", "none", "PDG", "TA", "P")


@functools.lru_cache(maxsize=None)
def _batch(nchan, order, log10_tau, ragged_mask):
    import oracle as O
    model, freqs = R.template("cut", nchan, NBIN)
    nsub = len(order)
    rng = np.random.default_rng(SEED + nchan + 7 * len(order) + log10_tau)
    b = dict(data=np.empty((nsub, nchan, NBIN)), keep=np.ones((nsub, nchan), bool),
             init=np.zeros((nsub, 5)), flags=np.zeros((nsub, 5), np.int32),
             nu_fits=np.empty((nsub, 3)), nu_outs=np.full((nsub, 3), np.nan),
             P=np.full(nsub, S.P0))
    for i, kind in enumerate(order):
        base = kind.rstrip("+")
        scat = base in SCAT
        fl = KIND.get(base, MOM["PD"])
        if ragged_mask:
            b["keep"][i] = R.masks(nchan, 1, seed=i)[1]     # another 20 % per sub-int
        if kind == "none":
            b["keep"][i] = False
        phi = rng.uniform(-0.5, 0.5)
        DM = S.DM0 + rng.normal(3e-4, 2e-4)
        tau = TAU if scat else 0.0
        noise = 0.2 if base == "ALL" else 0.5
        b["data"][i] = S.subint(SEED + 100 * nchan + i, model, freqs, phi, DM, S.P0,
                                noise=noise, tau=tau)
        k = b["keep"][i] if b["keep"][i].any() else np.ones(nchan, bool)
        nf = O.guess_fit_freq(freqs[k])
        b["nu_fits"][i] = nf, nf, nf - 40.0 if scat else nf
        b["flags"][i] = fl
        held = not fl[0]
        b["init"][i, 0] = O.phase_transform(phi + (0.0 if held else 2e-3), DM, 1500.0,
                                            nf, S.P0, mod=True)
        b["init"][i, 1] = S.DM0 if fl[1] else DM
        if scat:
            t0 = TAU * ((nf - 40.0) / 1500.0) ** -4.0 * (0.8 if fl[3] else 1.0)
            b["init"][i, 3:] = (np.log10(t0) if log10_tau else t0), -4.0
        if kind.endswith("+"):
            b["nu_outs"][i] = 1400.3, 1400.3, 1350.7
    for a in b.values():
        a.setflags(write=False)
    b.update(model=model, freqs=freqs, order=order, nchan=nchan, log10_tau=log10_tau)
    return b


@functools.lru_cache(maxsize=None)
def _oracle(nchan, order, log10_tau, ragged_mask, i, option, is_toa):
    import oracle as O
    b = _batch(nchan, order, log10_tau, ragged_mask)
    k = b["keep"][i]
    opt = lambda row: [None if np.isnan(v) else float(v) for v in row]
    return O.fit_portrait_full(
        b["data"][i][k], b["model"][k], list(b["init"][i]), b["P"][i], b["freqs"][k],
        opt(b["nu_fits"][i]), opt(b["nu_outs"][i]), None, [int(f) for f in b["flags"][i]],
        log10_tau=log10_tau, option=option, is_toa=is_toa)


def _device(b, option=0, is_toa=True):
    from pulseportraiture_amd import engine
    n = len(b["order"])
    res = engine.fit_batch(
        b["data"].astype(np.float32), b["model"], np.tile(b["freqs"], (n, 1)), b["P"].copy(),
        b["init"].copy(), b["flags"].copy(), nu_fits=b["nu_fits"].copy(),
        nu_outs=b["nu_outs"].copy(), chan_mask=b["keep"].astype(np.uint8),
        log10_tau=b["log10_tau"], option=option, is_toa=is_toa)
    return engine.results_numpy(res)


def _check(key, option=0, is_toa=True):
    from pulseportraiture_amd import _lib
    I = _lib.RESULT_INDEX
    b = _batch(*key)
    r = _device(b, option, is_toa)
    for a in r.values():
        assert np.all(np.isfinite(a)), key
    for i, kind in enumerate(b["order"]):
        tag = (key[0], kind, "option %d" % option, "is_toa %d" % is_toa)
        res = r["results"][i]
        if kind == "none":
            assert int(res[I["status"]]) == _lib.ST_NOFIT, tag
            for t in ("scales", "scale_errs", "channel_snrs", "covariance"):
                assert not r[t][i].any(), (t, tag)
            continue
        o = _oracle(*key, i, option, is_toa)
        R.compare_row("POSTFIT %d %s opt %d toa %d" % (key[0], kind, option, is_toa), tag,
                      r, i, o, b["keep"][i], b["P"][i], b["log10_tau"])
        nf = int(b["flags"][i].sum())
        cov = r["covariance"][i]
        np.testing.assert_allclose(cov[:nf, :nf], o["covariance_matrix"], rtol=1e-4,
                                   atol=1e-4 * np.abs(np.diag(o["covariance_matrix"])).min(),
                                   err_msg=str(tag))
        assert not cov[nf:].any() and not cov[:, nf:].any(), tag
        np.testing.assert_allclose(res[I["nu_out"]], [o["nu_DM"], o["nu_GM"], o["nu_tau"]],
                                   rtol=1e-5, err_msg=str(tag))


@gpu
@pytest.mark.parametrize("option", [0, 1])
@pytest.mark.parametrize("nchan,ragged_mask", [(20, False), (64, False), (80, True)])
def test_moment_fits(nchan, ragged_mask, option):
    """k_postfit_mom: every (phi, DM, GM) flag mask, both np.roots options,
    default and given nu_outs; 20 channels (one partial wave), 64, and 80
    with a different 20 % masked in every sub-int."""
    _check((nchan, MOM_ORDER, False, ragged_mask), option)


@gpu
def test_moment_fits_wide():
    """More than 2048 channels: the 256-thread form, channel powers
    recomputed in every loop instead of tabulated."""
    _check((2100, ("PD", "PDG"), False, False))


@gpu
def test_moment_fits_not_toa():
    _check((64, MOM_ORDER, False, False), 0, False)


@gpu
@pytest.mark.parametrize("log10_tau", [False, True])
def test_scattering_fits(log10_tau):
    """k_postfit: zero-covariance cases 0x1b, 0x1f -> 0x1b and 0x18.

    128 channels: at 64 the five-parameter fit with log10 tau is not
    well-posed at the 1e-4 bar of the errors -- restarted from its own x_fit
    plus 0.01 sigma the oracle's own param_errs move by 2.3e-4 there (the
    other kinds, and every kind at 128 channels, by 5e-7 at most)."""
    _check((128, SCAT_ORDER, log10_tau, False))


@gpu
def test_mixed_batch_with_unfitted_subint():
    """Both kernels on one batch; the sub-int with every channel masked ends
    PPF_ST_NOFIT with a finite, zeroed record."""
    _check((80, MIX_ORDER, False, True))


@gpu
def test_legacy_two_parameter_mode():
    """PPF_MODE_LEGACY2 (pplib.fit_portrait): zero-covariance case 0x3 whatever
    the mask, scale errors S^-1/2."""
    import oracle as O
    from pulseportraiture_amd import pplib
    b = _batch(64, MOM_ORDER, False, False)
    i = MOM_ORDER.index("PD")
    args = (b["data"][i], b["model"], b["init"][i, :2], b["P"][i], b["freqs"],
            b["nu_fits"][i, 0], None, None)
    d = pplib.fit_portrait(*args)
    o = O.fit_portrait(*args)
    assert abs(G.phase_diff(d.phase, o["phase"])) < G.SIGMA_TOL * o["phase_err"]
    assert abs(d.DM - o["DM"]) < G.SIGMA_TOL * o["DM_err"]
    assert abs(d.red_chi2 / o["red_chi2"] - 1) < G.RCHI2_RTOL
    np.testing.assert_allclose(d.nu_ref, o["nu_ref"], rtol=1e-5)
    np.testing.assert_allclose([d.phase_err, d.DM_err], [o["phase_err"], o["DM_err"]], rtol=1e-4)
    np.testing.assert_allclose(d.scales, o["scales"], rtol=1e-4)
    np.testing.assert_allclose(d.scale_errs, o["scale_errs"], rtol=1e-4)


@gpu
@pytest.mark.parametrize("is_toa", [True, False])
def test_scattering_fits_given_nu_outs(is_toa):
    """k_postfit with the output frequencies given (no zero-covariance
    search), as a TOA and not."""
    _check((128, SCAT_GIVEN, False, False), 0, is_toa)


# ---- sensitivity on the CPU ------------------------------------------------
class _Skip(np.ndarray):
    """A frequency axis whose nu ** -4 (skip4) or log (skiplog) comes out as
    zeros: what a kernel computes when it wrongly leaves that power out.  A
    quotient of it (nu / nu_tau) is one again; every other result is plain."""

    def __array_finalize__(self, obj):
        self.skip4 = getattr(obj, "skip4", False)
        self.skiplog = getattr(obj, "skiplog", False)

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        raw = [np.asarray(x) if isinstance(x, _Skip) else x for x in inputs]
        if method != "__call__":
            return getattr(ufunc, method)(*raw, **kw)
        if ufunc is np.power and isinstance(inputs[0], _Skip) and self.skip4 \
                and np.all(raw[1] == -4):
            return np.zeros(raw[0].shape)
        if ufunc is np.log and self.skiplog:
            return np.zeros(raw[0].shape)
        out = ufunc(*raw, **kw)
        if ufunc is np.true_divide and isinstance(inputs[0], _Skip):
            out = out.view(_Skip)
            out.skip4, out.skiplog = self.skip4, self.skiplog
        return out


def _skipping(monkeypatch, where, skip4=False, skiplog=False):
    """The oracle with the term left out in `where`: "nu_zeros" -- the
    per-channel weights nu^-4 / ln(nu) of the zero-covariance sums alone (the
    channel terms inside get_nu_zeros stay whole); "channel_terms" -- every
    use of the power in the channel derivatives (d phi_n / d GM, ln(nu_n /
    nu_tau)), in the search and in the covariance."""
    from oracle import ppfit_oracle as PO
    real, real_ct = getattr(PO, where), PO.channel_terms

    def wrapped(*a, **kw):
        a = list(a)
        f = np.array(a[5], dtype=float).view(_Skip)      # (theta, Dft, Mft, errs_FT, P, freqs, ...)
        f.skip4, f.skiplog = skip4, skiplog
        a[5] = f
        return real(*a, **kw)

    def whole(*a, **kw):
        a = list(a)
        a[5] = np.asarray(a[5])
        return real_ct(*a, **kw)
    if where == "nu_zeros":
        monkeypatch.setattr(PO, "channel_terms", whole)
    monkeypatch.setattr(PO, where, wrapped)


def _postfit_at(key, i, first, option=0):
    """The oracle's post-fit quantities at its own x_fit (no minimiser)."""
    import oracle as O
    b = _batch(*key)
    with np.errstate(all="ignore"):
        return O.fit_portrait_full(
            b["data"][i], b["model"], list(b["init"][i]), b["P"][i], b["freqs"],
            list(b["nu_fits"][i]), [None] * 3, None, [int(f) for f in b["flags"][i]],
            log10_tau=key[2], option=option, x_fit=np.asarray(first["x_fit"]))


def _nu(o):
    return np.array([o["nu_DM"], o["nu_GM"], o["nu_tau"]])


@pytest.mark.parametrize("kind,log10_tau", [("TA", True), ("PDTA", False), ("ALL", False)])
def test_nu_out_needs_the_log_weights(monkeypatch, kind, log10_tau):
    """Cases 0x18, 0x1b, 0x1f: without ln(nu_n) in the sums nu_tau comes out
    as exp(0) = 1 MHz, a finite change far above the 1e-5 bar of nu_out; the
    other two frequencies do not read it."""
    key = (64, SCAT_ORDER, log10_tau, False)
    i = SCAT_ORDER.index(kind)
    first = _oracle(*key, i, 0, True)
    np.testing.assert_array_equal(_nu(_postfit_at(key, i, first)), _nu(first))
    _skipping(monkeypatch, "nu_zeros", skiplog=True)
    off = _nu(_postfit_at(key, i, first))
    change = np.abs(off / _nu(first) - 1)
    print("POSTFIT sensitivity %s: nu_out %s -> %s" % (kind, _nu(first), off))
    assert np.all(np.isfinite(off))
    assert change[2] > 1e2 * 1e-5 and np.all(change[:2] == 0.0), change


def test_nu_out_needs_the_nu4_weights(monkeypatch):
    """Cases 0x5 and 0x7: with the nu^-4 weights zero the closed form of
    0x5 is (0 / sum h) ** -1/4 = inf whatever the data, and the polynomial of
    0x7 loses every coefficient but one (B D - F H = 0 identically: B = H,
    D = F), so that np.roots has no positive root and the oracle's argmin
    over them fails: nothing finite to compare, and no seed changes that."""
    key = (64, MOM_ORDER, False, False)
    i, j = MOM_ORDER.index("PG"), MOM_ORDER.index("PDG")
    first = _oracle(*key, i, 0, True)
    whole = [_oracle(*key, j, option, True) for option in (0, 1)]
    for o in [first] + whole:
        assert np.all(np.isfinite(_nu(o)))
    _skipping(monkeypatch, "nu_zeros", skip4=True)
    off = _nu(_postfit_at(key, i, first))
    assert np.isinf(off[1]) and off[2] == _nu(first)[2], off
    for option in (0, 1):
        with pytest.raises(ValueError, match="empty sequence"):
            _postfit_at(key, j, whole[option], option)


@pytest.mark.parametrize("nchan", [20, 32])
def test_scale_errs_need_the_nu4_term(monkeypatch, nchan):
    """DM and GM fitted, the phase held (mask 0x6): with nu_n^-4 left out of
    d phi_n / d GM the GM column turns into a phase column, the covariance
    stays regular, and the oracle's scale_errs move by 6.7e-4 (20 channels)
    and 1.5e-3 (32 channels) with the seeds of _batch (SEED) -- above the
    1e-4 bar of the comparison.  (The share of the parameters in a channel's
    scale error falls with the channel count: at 64 channels the same change
    is 3.8e-5 and would pass unseen, which is why these widths are used.)
    With the phase fitted as well the two columns are parallel and the
    covariance singular."""
    key = (nchan, ("DG",), False, False)
    first = _oracle(*key, 0, 0, True)
    same = _postfit_at(key, 0, first)
    np.testing.assert_allclose(same["scale_errs"], first["scale_errs"], rtol=1e-12)
    _skipping(monkeypatch, "channel_terms", skip4=True)
    off = _postfit_at(key, 0, first)
    se = np.asarray(off["scale_errs"])
    assert np.all(np.isfinite(se)) and np.all(np.isfinite(off["param_errs"]))
    change = np.abs(se / first["scale_errs"] - 1).max()
    print("POSTFIT sensitivity DG %d channels: scale_errs move by %.2e, GM_err %.4g -> %.4g" %
          (nchan, change, first["param_errs"][2], off["param_errs"][2]))
    assert change > 1e-4, change


def test_scale_errs_need_the_log_term(monkeypatch):
    """alpha fitted: with ln(nu_n / nu_tau) = 0 every alpha derivative is an
    exact zero, the Hessian has a zero row, and the oracle's errors are not
    finite -- necessarily, for any data."""
    key = (64, SCAT_ORDER, True, False)
    i = SCAT_ORDER.index("TA")
    first = _oracle(*key, i, 0, True)
    assert np.all(np.isfinite(first["scale_errs"])) and np.all(np.isfinite(first["param_errs"]))
    _skipping(monkeypatch, "channel_terms", skiplog=True)
    off = _postfit_at(key, i, first)
    assert not np.isfinite(off["param_errs"][4]), off["param_errs"]
    assert not np.isfinite(np.asarray(off["scale_errs"])).any()
