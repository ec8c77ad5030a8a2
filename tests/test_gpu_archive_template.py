"""The PSRFITS-only chain ppalign -> template file -> pptoas: align_archives
writes the portrait it returns (pplib.unload_new_archive on the template's
metadata), and GetTOAs takes a FITS archive as its template (pptoas.py:358-377,
922-946, 1041-1042, 1420-1430).

The archives are pplib.make_fake_pulsar's from tests/golden/example.gmodel and
example.par: 16 channels, 128 bins, two sub-ints, noise 0.01 on a template of
peak ~10 (S/N of a sub-int in the thousands), channel 5 given weight 0 in every
file."""
import os

import numpy as np
import pytest

import oracle as O
from pulseportraiture_amd import pplib, psrfits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GMODEL = os.path.join(HERE, "golden", "example.gmodel")
PAR = os.path.join(HERE, "golden", "example.par")

SIGMA_TOL = 0.01          # the project's parity bar (tests/test_gpu_gaussfit.py)
EPS32 = float(np.finfo(np.float32).eps)
NSUB, NCHAN, NBIN, NU0, BW = 2, 16, 128, 1500.0, 800.0
ZAPPED = 5
ARCH = dict(nsub=NSUB, npol=1, nchan=NCHAN, nbin=NBIN, nu0=NU0, bw=BW,
            tsub=60.0, noise_stds=0.01)
DDMS = (1e-4, -2e-4, 3e-4)
PHASES = (0.03, -0.05, 0.11)
# chi^2_red, FITS template against .gmodel: see
# test_fits_template_matches_gmodel
RCHI2_MEASURED = 3.233e-7
RCHI2_ALLOW = 4 * RCHI2_MEASURED


def build_archives(d, seed0=4100):
    """Three archives and their metafile in directory d."""
    weights = np.ones((NSUB, NCHAN))
    weights[:, ZAPPED] = 0.0
    files = []
    for i, (dDM, ph) in enumerate(zip(DDMS, PHASES)):
        fn = os.path.join(str(d), "a%d.fits" % i)
        pplib.make_fake_pulsar(GMODEL, PAR, outfile=fn, dDM=dDM, phase=ph,
                               weights=weights, quiet=True, seed=seed0 + i,
                               **ARCH)
        files.append(fn)
    meta = os.path.join(str(d), "meta.txt")
    with open(meta, "w") as fh:
        fh.write("\n".join(files) + "\n")
    return files, meta


def gaussian_template(nbin=NBIN):
    """(freqs [NCHAN], gen_gaussian_portrait of example.gmodel there)."""
    cw = BW / NCHAN
    freqs = np.linspace(NU0 - BW / 2 + cw / 2, NU0 + BW / 2 - cw / 2, NCHAN)
    (_name, code, nu_ref, _ng, params, _ff, alpha,
     _fa) = pplib.read_model(GMODEL, quiet=True)
    port = pplib.gen_gaussian_portrait(code, params, alpha,
                                       pplib.get_bin_centers(nbin), freqs,
                                       nu_ref)
    return freqs, port


def write_template(d, name, port, freqs):
    fn = os.path.join(str(d), name)
    pplib.write_archive(port[None, None], PAR, freqs, nu0=NU0, bw=BW,
                        outfile=fn, tsub=60.0, quiet=True, elem="E")
    return fn


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The archives, the templates as files, and the .gmodel run every test
    compares with (fitted once)."""
    from pulseportraiture_amd import pptoas
    d = tmp_path_factory.mktemp("tmpl")
    files, meta = build_archives(d)
    freqs, port = gaussian_template()
    w = dict(dir=d, files=files, meta=meta, freqs=freqs, port=port,
             template=write_template(d, "template.fits", port, freqs))
    gm = pptoas.GetTOAs(meta, GMODEL, quiet=True)
    gm.get_TOAs(quiet=True)
    w["gmodel"] = gm
    return w


def _sigma_devs(a, b):
    """max over archives and sub-ints of |phi_a - phi_b| / phi_err_b and the
    same for DM; the largest relative chi^2_red difference."""
    dphi = ddm = drc = 0.0
    assert len(a.phis) == len(b.phis) > 0
    for i in range(len(b.phis)):
        ok = np.asarray(b.ok_isubs[i])
        np.testing.assert_array_equal(ok, a.ok_isubs[i])
        p = (np.asarray(a.phis[i]) - np.asarray(b.phis[i]))[ok]
        p = (p + 0.5) % 1.0 - 0.5
        dphi = max(dphi, np.abs(p / np.asarray(b.phi_errs[i])[ok]).max())
        ddm = max(ddm, np.abs((np.asarray(a.DMs[i]) - np.asarray(b.DMs[i]))[ok]
                              / np.asarray(b.DM_errs[i])[ok]).max())
        drc = max(drc, np.abs(np.asarray(a.red_chi2s[i])[ok] /
                              np.asarray(b.red_chi2s[i])[ok] - 1.0).max())
    return dphi, ddm, drc


# ------------------------------------------------------------- ppalign ----
def test_align_archives_writes_what_it_returns(world):
    from pulseportraiture_amd import ppalign, ppspline
    out = os.path.join(str(world["dir"]), "aligned.fits")
    r = ppalign.align_archives(world["meta"], world["files"][0], outfile=out,
                               niter=1, quiet=True)
    assert r.nsub_fit == 3 * NSUB
    assert os.path.isfile(out)
    port = r.port[0]
    f = psrfits.PSRFITS(out)
    assert (f.nsub, f.npol, f.nchan, f.nbin) == (1, 1, NCHAN, NBIN)
    scl, offs = f.scales_offsets()
    assert float(f.subint.header["DM"]) == 0.0
    assert float(f.primary["CHAN_DM"]) == 0.0
    f.close()
    s, o = scl[0].astype(float)[:, None], offs[0].astype(float)[:, None]
    bound = 0.5 * s + 2 * EPS32 * (np.abs(o) + 32768 * s)
    # the stored samples themselves: the round-trip bound as it stands
    raw = psrfits.load_data(out, rm_baseline=False, quiet=True)
    err = np.abs(np.asarray(raw.subints)[0, 0].astype(float) - port)
    print("\nstored vs returned: max err / bound %.3f" % (err / bound).max())
    assert (err <= bound).all()
    # the default load removes a baseline: compared about each channel's
    # mean, where a sample's error e_i becomes e_i - mean(e), at most twice
    # the bound
    d = psrfits.load_data(out, quiet=True)
    got = np.asarray(d.subints)[0, 0].astype(float)
    res = (got - got.mean(axis=1, keepdims=True)) - \
        (port - port.mean(axis=1, keepdims=True))
    print("baseline-removed vs returned: max err / bound %.3f"
          % (np.abs(res) / bound).max())
    assert (np.abs(res) <= 2 * bound).all()
    assert d.DM == 0.0 and d.nsub == 1
    want = np.ones(NCHAN)
    want[ZAPPED] = 0.0
    np.testing.assert_array_equal(d.weights[0], want)
    assert (r.total_weights[ZAPPED] == 0.0).all()
    # the template's metadata
    t = psrfits.load_data(world["files"][0], tscrunch=True, quiet=True)
    np.testing.assert_array_equal(d.freqs, t.freqs)
    assert d.Ps[0] == t.Ps[0] and d.source == t.source
    assert abs(d.epochs[0].in_days() - t.epochs[0].in_days()) * 86400 < 1e-5
    dp = ppspline.DataPortrait(out, quiet=True)
    assert (dp.nchan, dp.nbin, dp.nchanx) == (NCHAN, NBIN, NCHAN - 1)


class _Arch(object):
    """The PSRCHIVE calls of ppalign.py:259-277 on a stand-in object."""

    def __init__(self):
        self.amps = np.zeros((1, NCHAN, NBIN))
        self.weights = np.full(NCHAN, -1.0)
        self.dm = self.outfile = None

    def tscrunch(self):
        pass

    def pscrunch(self):
        pass

    def set_dispersion_measure(self, dm):
        self.dm = dm

    def get_npol(self):
        return 1

    def get_nchan(self):
        return NCHAN

    def __iter__(self):
        arch = self

        class _Sub(object):
            def get_Profile(self, ipol, ichan):
                class _Prof(object):
                    def get_amps(self):
                        return arch.amps[ipol, ichan]
                return _Prof()

            def set_weight(self, ichan, w):
                arch.weights[ichan] = w
        return iter([_Sub()])

    def unload(self, outfile):
        self.outfile = outfile


def test_align_archives_untouched_paths(world, monkeypatch, tmp_path):
    from pulseportraiture_amd import ppalign, pptoas
    guess = world["files"][0]
    before = sorted(os.listdir(str(world["dir"])))
    # no outfile (a list of names has no default): nothing is written
    r0 = ppalign.align_archives(list(world["files"]), guess, outfile=None,
                                niter=1, quiet=True)
    assert sorted(os.listdir(str(world["dir"]))) == before
    # an attached archive object is written through, and only through
    arch = _Arch()
    real = pptoas.load_data

    def load(name, **kw):
        d = real(name, **kw)
        if kw.get("return_arch"):
            d["arch"] = arch
        return d
    monkeypatch.setattr(pptoas, "load_data", load)
    out = str(tmp_path / "via_arch.fits")
    r = ppalign.align_archives(list(world["files"]), guess, outfile=out,
                               niter=1, quiet=True)
    assert arch.outfile == out and arch.dm == 0.0
    assert not os.path.exists(out)
    np.testing.assert_array_equal(arch.amps[0], r.port[0])
    np.testing.assert_array_equal(r.port, r0.port)
    want = np.ones(NCHAN)
    want[ZAPPED] = 0.0
    np.testing.assert_array_equal(arch.weights, want)


# -------------------------------------------------------- FITS template ----
def test_fits_template_matches_gmodel(world, capsys):
    """The Gaussian portrait written as a float32 archive against the same
    portrait from the .gmodel: phi and DM within 0.01 sigma.  chi^2_red
    differs by the template's float32 rounding: on the CPU
    (oracle.get_toas_archive on these sub-ints, template in float64 against
    the same template rounded to float32: oracle_rchi2_change below) the
    largest relative change over the six sub-ints is 3.233e-7
    (RCHI2_MEASURED); four times that, 1.293e-6, is allowed (RCHI2_ALLOW), for
    the device's other summation order."""
    from pulseportraiture_amd import pptoas
    gt = pptoas.GetTOAs(world["meta"], world["template"], quiet=True)
    assert gt.is_FITS_model
    capsys.readouterr()
    gt.get_TOAs(quiet=True)
    out = capsys.readouterr().out
    assert out.count("experimental functionality") == 1
    assert "Frequency mismatch" not in out
    assert gt.model_name == world["template"]
    assert len(gt.TOA_list) == 3 * NSUB
    dphi, ddm, drc = _sigma_devs(gt, world["gmodel"])
    print("\nFITS vs .gmodel: phi %.2e sigma, DM %.2e sigma, chi2_red rel "
          "%.2e (allowed %.2e)" % (dphi, ddm, drc, RCHI2_ALLOW))
    assert dphi <= SIGMA_TOL and ddm <= SIGMA_TOL
    assert drc <= RCHI2_ALLOW
    assert all(t.flags["tmplt"] == world["template"] for t in gt.TOA_list)


def oracle_rchi2_change(files, port):
    """The measurement behind RCHI2_ALLOW (run on the CPU once the archives
    exist): the largest relative change of the oracle's chi^2_red when its
    template is rounded to float32."""
    worst = 0.0
    for fn in files:
        d = psrfits.load_data(fn, quiet=True)
        args = (np.asarray(d.subints)[:, 0].astype(float),)
        rest = (d.freqs, d.weights, d.SNRs[:, 0], d.Ps, d.DM,
                d.doppler_factors)
        kw = dict(noise_stds=d.noise_stds[:, 0])
        a = O.get_toas_archive(*args, port, *rest, **kw)
        b = O.get_toas_archive(
            *args, port.astype(np.float32).astype(np.float64), *rest, **kw)
        worst = max(worst, np.abs(b["red_chi2s"] / a["red_chi2s"] - 1).max())
    return worst


def test_fits_template_with_fit_scat(world):
    """pptoas.py:951-975: with fit_scat the reference rebuilds an UNSCATTERED
    portrait from a .gmodel (TAU set to 0) and uses an archive template as it
    is.  example.gmodel has TAU 0, so the two paths fit the same portrait from
    the same guesses (no gparams on the FITS path: tau_guess 0, alpha the
    default -4.0, which is the .gmodel's ALPHA) and are meant to agree.

    Both runs quote phi at NU0 (nu_refs): left to itself the fit quotes it at
    its zero-covariance frequency, itself a fitted number, and these archives
    are not scattered, so tau is all but unconstrained (tau_err 0.4 to 1.2
    dex) and that frequency moves with the last bits of the template.
    Measured: without nu_refs the two runs' phi differ by 2.2 sigma with DM,
    tau and chi^2_red agreeing to 5e-6 sigma, 2e-5 sigma and 3e-7, the phi
    difference being DM (nu_ref_F^-2 - nu_ref_G^-2) Dconst / P; at NU0 they
    differ by 1.7e-5 sigma."""
    from pulseportraiture_amd import pptoas
    kw = dict(fit_scat=True, nu_refs=(NU0, NU0), quiet=True)
    gm = pptoas.GetTOAs(world["meta"], GMODEL, quiet=True)
    gm.get_TOAs(**kw)
    gt = pptoas.GetTOAs(world["meta"], world["template"], quiet=True)
    gt.get_TOAs(**kw)
    dphi, ddm, drc = _sigma_devs(gt, gm)
    dtau = max(np.abs((np.asarray(gt.taus[i]) - np.asarray(gm.taus[i])) /
                      np.asarray(gm.tau_errs[i])).max() for i in range(3))
    print("\nfit_scat, FITS vs .gmodel: phi %.2e sigma, DM %.2e sigma, tau "
          "%.2e sigma, chi2_red rel %.2e" % (dphi, ddm, dtau, drc))
    assert dphi <= SIGMA_TOL and ddm <= SIGMA_TOL and dtau <= SIGMA_TOL
    assert drc <= RCHI2_ALLOW


def test_one_channel_template_is_tiled(world, capsys):
    """The template f-scrunched to one channel on the host: fitted as that
    profile tiled over the data's channels, with the reference's frequency
    message for every sub-int."""
    from pulseportraiture_amd import pptoas
    prof = world["port"].mean(axis=0)
    one = os.path.join(str(world["dir"]), "one.fits")
    pplib.write_archive(prof[None, None, None], PAR, np.array([NU0]), nu0=NU0,
                        bw=BW, outfile=one, tsub=60.0, quiet=True, elem="E")
    tiled = write_template(world["dir"], "tiled.fits",
                           np.tile(prof, (NCHAN, 1)), world["freqs"])
    capsys.readouterr()
    g1 = pptoas.GetTOAs(world["meta"], one, quiet=True)
    g1.get_TOAs(quiet=True)
    out = capsys.readouterr().out
    assert out.count("Frequency mismatch between template and data!") == \
        3 * NSUB
    assert "skipping it" not in out
    gn = pptoas.GetTOAs(world["meta"], tiled, quiet=True)
    gn.get_TOAs(quiet=True)
    assert len(g1.TOA_list) == len(gn.TOA_list) == 3 * NSUB
    dphi, ddm, drc = _sigma_devs(g1, gn)
    print("\none channel vs tiled: phi %.2e sigma, DM %.2e sigma, chi2_red "
          "rel %.2e" % (dphi, ddm, drc))
    assert dphi <= SIGMA_TOL and ddm <= SIGMA_TOL and drc <= RCHI2_ALLOW


def test_template_of_another_nbin_skips_the_archive(world, capsys):
    from pulseportraiture_amd import pptoas
    freqs, port = gaussian_template(nbin=64)
    short = write_template(world["dir"], "short.fits", port, freqs)
    fn = world["files"][1]
    gt = pptoas.GetTOAs(fn, short, quiet=True)
    capsys.readouterr()
    gt.get_TOAs(quiet=True)
    out = capsys.readouterr().out
    assert "Model nbin 64 != data nbin %d for %s; skipping it." % (NBIN, fn) \
        in out
    assert gt.TOA_list == [] and gt.phis == [] and gt.order == []
    gt.get_narrowband_TOAs(quiet=True)
    assert "Model nbin 64 != data nbin" in capsys.readouterr().out
    assert gt.TOA_list == []
    # another channel count is refused the same way
    wide = write_template(world["dir"], "wide.fits", world["port"][:8],
                          world["freqs"][:8])
    gt = pptoas.GetTOAs(fn, wide, quiet=True)
    gt.get_TOAs(quiet=True)
    assert "Model nchan 8 != data nchan %d for %s; skipping it." % (NCHAN, fn) \
        in capsys.readouterr().out
    assert gt.TOA_list == []


def _flagged(gt, i):
    """Fitted channels of archive i without a usable narrowband result."""
    phi, err = np.asarray(gt.phis[i]), np.asarray(gt.phi_errs[i])
    return ~(np.isfinite(phi) & np.isfinite(err) & (err > 0))


def test_narrowband_toas_match_gmodel(world):
    from pulseportraiture_amd import pptoas
    gm = pptoas.GetTOAs(world["meta"], GMODEL, quiet=True)
    gm.get_narrowband_TOAs(quiet=True)
    gt = pptoas.GetTOAs(world["meta"], world["template"], quiet=True)
    gt.get_narrowband_TOAs(quiet=True)
    assert len(gt.TOA_list) == len(gm.TOA_list) == 3 * NSUB * (NCHAN - 1)
    fitted = np.ones((NSUB, NCHAN), dtype=bool)
    fitted[:, ZAPPED] = False
    left_out = total = 0
    worst = 0.0
    for i in range(3):
        assert not _flagged(gm, i)[fitted].any()     # the seed's choice
        use = fitted & ~_flagged(gt, i)
        left_out += int((fitted & ~use).sum())
        total += int(fitted.sum())
        p = (np.asarray(gt.phis[i]) - np.asarray(gm.phis[i]))[use]
        p = (p + 0.5) % 1.0 - 0.5
        worst = max(worst, np.abs(p / np.asarray(gm.phi_errs[i])[use]).max())
        # the channel without weight is not fitted by either
        assert gt.phi_errs[i][0, ZAPPED] == 0 == gm.phi_errs[i][0, ZAPPED]
    print("\nnarrowband FITS vs .gmodel: %.2e sigma, %d of %d channels left "
          "out" % (worst, left_out, total))
    assert left_out * 16 <= total
    assert worst <= SIGMA_TOL


def test_narrowband_skips_channels_the_template_gives_no_weight(world):
    from pulseportraiture_amd import pptoas
    fn = os.path.join(str(world["dir"]), "template_w.fits")
    w = np.ones((1, NCHAN))
    w[0, 9] = 0.0
    pplib.write_archive(world["port"][None, None], PAR, world["freqs"],
                        nu0=NU0, bw=BW, outfile=fn, tsub=60.0, weights=w,
                        quiet=True, elem="E")
    gt = pptoas.GetTOAs(world["files"][0], fn, quiet=True)
    gt.get_narrowband_TOAs(quiet=True)
    chans = sorted(set(t.flags["chan"] for t in gt.TOA_list))
    assert chans == [c for c in range(NCHAN) if c not in (ZAPPED, 9)]
    assert len(gt.TOA_list) == NSUB * (NCHAN - 2)


def test_show_fit_and_zap_serve_the_portrait(world):
    from pulseportraiture_amd import pptoas
    gt = pptoas.GetTOAs(world["meta"], world["template"], quiet=True)
    gt.get_TOAs(quiet=True)
    fn = world["files"][1]
    data = gt._load_fit_data(fn, True)
    name, model = gt._fit_model(data, 1, 0, True)
    assert name == world["template"] and model.shape == (NCHAN, NBIN)
    # the file's float32 samples, less the loader's baseline
    want = world["port"].astype(np.float32).astype(float)
    res = (model - model.mean(axis=1, keepdims=True)) - \
        (want - want.mean(axis=1, keepdims=True))
    assert np.abs(res).max() <= 2 * EPS32 * np.abs(want).max()
    port, scaled, ok, freqs, noise = gt.show_fit(fn, isub=1, show=False,
                                                 return_fit=True, quiet=True)
    np.testing.assert_array_equal(
        scaled, np.asarray(gt.scales[1][1])[:, None] * model)
    assert list(ok) == [c for c in range(NCHAN) if c != ZAPPED]
    # the .gmodel run serves the same rotated data and, within the parity
    # bar on the fitted scales (0.01 of the channel's noise; the template's
    # float32 rounding is 1e-5 of that), the same scaled model about each
    # channel's mean
    gm = world["gmodel"]
    port_g, scaled_g = gm.show_fit(fn, isub=1, show=False, return_fit=True,
                                   quiet=True)[:2]
    res = (scaled - scaled.mean(axis=1, keepdims=True)) - \
        (scaled_g - scaled_g.mean(axis=1, keepdims=True))
    print("\nshow_fit model, FITS vs .gmodel: %.2e of the noise"
          % (np.abs(res[ok]) / noise[ok][:, None]).max())
    assert (np.abs(res[ok]) <= SIGMA_TOL * noise[ok][:, None]).all()
    assert np.abs(port - port_g)[ok].max() <= SIGMA_TOL * noise[ok].min()
    gt.get_channels_to_zap()
    gm.get_channels_to_zap()
    assert len(gt.zap_channels) == 3
    for i in range(3):
        for s in range(NSUB):
            np.testing.assert_array_equal(gt.zap_channels[i][s],
                                          gm.zap_channels[i][s])
            assert len(gt.channel_red_chi2s[i][s]) == NCHAN - 1
