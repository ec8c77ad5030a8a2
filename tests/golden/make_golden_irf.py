#!/usr/bin/env python
"""Golden vectors of the instrumental response (tests/golden/irf.npz),
produced by running the REFERENCE in this container (never on the GPU box)
through the import shims of make_golden.py.

  resp      pptoaslib.instrumental_response_port_FT (pptoaslib.py:158-192)
            for the parameter sets of irf_inputs.RESP at 8 channels x nbin
            64, 1000, 2048
  toa_pd    get_TOAs(add_instrumental_response=True), .gmodel, phase + DM,
            DM smearing + rect + gauss; three sub-ints of different P,
            channel 1 zapped in one (pptoas.py:424-434)
  toa_scat  the same shape, fit_GM + fit_scat, DM smearing only
  toa_spl   spline template, constant responses only, nbin = 1000
  nb        get_narrowband_TOAs (pptoas.py:983-989), DM smearing + rect
  zap       after toa_pd: get_channels_to_zap's channel_red_chi2s and
            show_fit(return_fit=True)'s scaled model of sub-int 0
            (pptoas.py:1446-1452)

Every GetTOAs case is run twice, with and without the response, on the same
data; both runs are stored (out_* / nr_*), and the generator asserts that
the response moves the fitted DM (the phases, for the narrowband case) by at
least 10 of the response run's own sigma, so that a product ignoring the
response cannot pass the 0.01 sigma comparison.

Inputs are NOT stored: they are rebuilt from irf_inputs.CASES and checked
against the stored SHA-256.

Usage:  python tests/golden/make_golden_irf.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # repo (oracle)
import make_golden as mg  # noqa: E402  (imports the reference with the shims)
import numpy as np  # noqa: E402
import synth_np as S  # noqa: E402
import irf_inputs as II  # noqa: E402
from make_golden_zap import ATTRS  # noqa: E402

OUT = os.path.join(HERE, "irf.npz")
MIN_SIGMA = 10.0


class _NumPy(object):
    """numpy as the reference's pptoaslib sees it, with the dtype alias
    'complex_' (removed in NumPy 2; pptoaslib.py:182) understood by ones():
    the reference's own instrumental_response_port_FT runs unchanged."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def ones(shape, dtype=None, **kw):
        if isinstance(dtype, str) and dtype == "complex_":
            dtype = np.complex128
        return np.ones(shape, dtype=dtype, **kw)


mg.pptoaslib.np = _NumPy()


def run_resp():
    """The reference's multipliers, and how far its 'gauss' factor (the erf
    formula of pplib.gaussian_profile_FT) is from the closed-form Gaussian."""
    out, worst = {}, 0.0
    freqs = II.resp_freqs()
    for name, DM, P, wids, types in II.RESP:
        for nbin in II.RESP_NBINS:
            with contextlib.redirect_stdout(io.StringIO()):
                r = mg.pptoaslib.instrumental_response_port_FT(
                    nbin, freqs, DM, P, list(wids), list(types))
            out["%s_%d" % (name, nbin)] = np.asarray(r)
    k = np.arange(2048 // 2 + 1)
    for nbin in II.RESP_NBINS:
        for wid in (0.002, 0.05, 0.1):
            with contextlib.redirect_stdout(io.StringIO()):
                g = mg.pptoaslib.instrumental_response_FT(nbin, wid, "gauss")
            kk = k[:nbin // 2 + 1]
            closed = np.exp(-(np.pi * kk * wid) ** 2 / (4.0 * np.log(2.0)))
            worst = max(worst, float(np.abs(np.real(g) - closed).max()),
                        float(np.abs(np.imag(g)).max()))
    print("gauss factor: max |reference - closed form| = %.3g" % worst)
    out["gauss_closed_form_err"] = np.float64(worst)
    return out


def _files(c):
    from pplib import DataBunch
    import psrchive as pr
    files_in, freqs = II.inputs(c)
    files, extra, hashes = {}, {}, []
    for f, fi in enumerate(files_in):
        subints = fi["subints"][:, None]
        nsub_f = subints.shape[0]
        noise = np.array([mg.pplib.get_noise(subints[i, 0], chans=True)
                          for i in range(nsub_f)])
        snrs = np.abs(subints[:, 0].max(axis=-1)) / noise * 3.0
        name = "%s_%d.fits" % (c["name"], f)
        files[name] = DataBunch(
            epochs=[pr.MJD(e) for e in fi["epochs"]], filename=name,
            phases=mg.pplib.get_bin_centers(c["nbin"]),
            **II.archive_fields(c, fi, freqs, noise, snrs))
        hashes.append(S.sha(fi["subints"].astype(np.float32)))
        extra["f%d_noise" % f] = noise
        extra["f%d_snrs" % f] = snrs
        extra["f%d_weights" % f] = fi["weights"]
        extra["f%d_dfs" % f] = fi["dfs"]
        extra["f%d_epochs" % f] = fi["epochs"]
        extra["f%d_Ps" % f] = fi["Ps"]
    extra["sha"] = np.array(hashes)
    extra["freqs"] = freqs
    return files, extra


def _gt(c, files, respond):
    mg.pptoas.load_data = lambda filename, **kw: files[filename]
    gt = mg.pptoas.GetTOAs.__new__(mg.pptoas.GetTOAs)
    gt.datafiles = list(files.keys())
    gt.is_FITS_model = False
    gm = II.gmodel(c)
    gt.modelfile = mg.GMODEL if gm == S.GMODEL else gm
    for attr in ATTRS:
        setattr(gt, attr, [])
    ird = c["ird"] if respond else dict(DM=0.0, wids=[], irf_types=[])
    gt.instrumental_response_dict = gt.ird = dict(
        DM=ird["DM"], wids=list(ird["wids"]),
        irf_types=list(ird["irf_types"]))
    gt.quiet = True
    return gt


TOA_KEYS = ["phis", "phi_errs", "DMs", "DM_errs", "red_chi2s", "snrs",
            "scales", "scale_errs", "channel_snrs", "covariances",
            "DeltaDM_means", "DeltaDM_errs", "GMs", "GM_errs", "taus",
            "tau_errs", "alphas", "alpha_errs", "nu_fits", "rcs", "nfevals",
            "nu_refs"]
NB_KEYS = ["phis", "phi_errs", "scales", "scale_errs", "channel_snrs",
           "channel_red_chi2s"]


def _tim(gt):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mg.pplib.write_TOAs(gt.TOA_list)
    return np.array(buf.getvalue().splitlines())


def newton_step_sigma(c, files, out):
    """How far the reference's own end point is from the stationary point
    of its objective: the Newton step there (gradient and Hessian of the
    oracle's restatement of pptoaslib.py:564-684, on the reference's own
    response-convolved model), per fitted parameter in units of the
    reference's reported error.  scipy's trust-ncg can stop short along the
    flat direction of a five-parameter fit; an end point more than
    MAX_STEP sigma out would use up the 0.01 sigma bar of the comparison,
    so such a case is not a usable golden."""
    import oracle.ppfit_oracle as O
    kw = c.get("kw", {})
    scat = bool(kw.get("fit_scat"))
    flags = [1, 1, int(bool(kw.get("fit_GM"))), int(scat), int(scat)]
    idx = [i for i in range(5) if flags[i]]
    d = files[list(files)[0]]
    nbin, ird = c["nbin"], c["ird"]
    gm = II.gmodel(c)
    gm = mg.GMODEL if gm == S.GMODEL else gm
    steps = np.zeros((d.nsub, 5))
    for s in range(d.nsub):
        ok, P = d.ok_ichans[s], d.Ps[s]
        with contextlib.redirect_stdout(io.StringIO()):
            if c.get("spline"):
                _, model = mg.pplib.read_spline_model(gm, d.freqs[s], nbin,
                                                      quiet=True)
            elif scat:
                (_, code, nu_ref, _, gp, _, _, _) = mg.pplib.read_model(
                    gm, quiet=True)
                gp = np.copy(gp)
                gp[1] = 0.0
                model = mg.pplib.gen_gaussian_portrait(
                    code, gp, 0.0, d.phases, d.freqs[s], nu_ref)
            else:
                _, _, model = mg.pplib.read_model(gm, d.phases, d.freqs[s],
                                                  P, quiet=True)
            resp = mg.pptoaslib.instrumental_response_port_FT(
                nbin, d.freqs[s, ok], ird["DM"], P, list(ird["wids"]),
                list(ird["irf_types"]))
        mx = np.fft.irfft(resp * np.fft.rfft(model[ok], axis=-1), axis=-1)
        Dft, Mft = O._spectra(d.subints[s, 0, ok], mx)
        eFT = d.noise_stds[s, 0, ok] * np.sqrt(nbin / 2.0)
        df = d.doppler_factors[s]
        th = np.array([out["out_phis"][0][s], out["out_DMs"][0][s] / df,
                       out["out_GMs"][0][s] / df ** 3 if flags[2] else 0.0,
                       out["out_taus"][0][s], out["out_alphas"][0][s]])
        nus = out["out_nu_refs"][0][s]
        t = O.channel_terms(th, Dft, Mft, eFT, P, d.freqs[s, ok], nus[0],
                            nus[1], nus[2], scat)
        g, H = O.gradient(t, flags)[idx], O.hessian(t, flags)[np.ix_(idx,
                                                                      idx)]
        errs = np.array([out["out_" + k][0][s] for k in
                         ("phi_errs", "DM_errs", "GM_errs", "tau_errs",
                          "alpha_errs")])[idx]
        steps[s, idx] = -np.linalg.solve(H, g) / errs
    return steps


MAX_STEP = 0.003


def run_toas(c):
    files, out = _files(c)
    keep = None
    for prefix, respond in (("out_", True), ("nr_", False)):
        gt = _gt(c, files, respond)
        with contextlib.redirect_stdout(io.StringIO()):
            gt.get_TOAs(quiet=True, add_instrumental_response=respond,
                        **c.get("kw", {}))
        for key in TOA_KEYS:
            out[prefix + key] = np.array(getattr(gt, key), dtype=np.float64)
        out[prefix + "tim_lines"] = _tim(gt)
        if respond:
            keep = gt
    moved = np.abs(out["out_DMs"] - out["nr_DMs"]) / out["out_DM_errs"]
    print("%s: response moves DM by %s sigma" % (c["name"],
                                                 np.round(moved, 1)))
    assert moved.min() >= MIN_SIGMA, moved
    steps = newton_step_sigma(c, files, out)
    print("%s: reference end point to its stationary point, max |Newton "
          "step| / sigma per sub-int: %s" % (c["name"], np.round(
              np.abs(steps).max(axis=1), 5)))
    assert np.abs(steps).max() <= MAX_STEP, steps
    out["ref_newton_step_sigma"] = steps
    out.update(nfile=np.int64(c["nfile"]), nsub=np.int64(c["nsub"]),
               nchan=np.int64(c["nchan"]), nbin=np.int64(c["nbin"]),
               DM0=np.float64(S.DM0))
    return out, keep, files


def run_nb(c):
    files, out = _files(c)
    for prefix, respond in (("out_", True), ("nr_", False)):
        gt = _gt(c, files, respond)
        with contextlib.redirect_stdout(io.StringIO()):
            gt.get_narrowband_TOAs(quiet=True,
                                   add_instrumental_response=respond)
        for key in NB_KEYS:
            out[prefix + key] = np.array(getattr(gt, key), dtype=np.float64)
        out[prefix + "tim_lines"] = _tim(gt)
    used = out["out_phi_errs"] > 0
    d = (out["out_phis"] - out["nr_phis"] + 0.5) % 1.0 - 0.5
    moved = np.abs(d[used]) / out["out_phi_errs"][used]
    print("nb: response moves the channel phases by %.1f sigma (median), "
          "%.1f (min)" % (np.median(moved), moved.min()))
    # narrowband TOAs carry no DM: the phases themselves must move (median
    # over the usable channels; a channel whose two biases happen to agree
    # does not matter)
    assert np.median(moved) >= MIN_SIGMA, moved
    out.update(nfile=np.int64(c["nfile"]), nsub=np.int64(c["nsub"]),
               nchan=np.int64(c["nchan"]), nbin=np.int64(c["nbin"]),
               DM0=np.float64(S.DM0))
    return out


def run_zap(gt, files):
    """On the GetTOAs object of the toa_pd response run."""
    gt.add_instrumental_response = True
    name = list(files)[0]
    with contextlib.redirect_stdout(io.StringIO()):
        gt.get_channels_to_zap()
        port, model, ok, freqs, noise = gt.show_fit(
            name, isub=0, show=False, return_fit=True, quiet=True)
    chi, chi_n = [], []
    for c in gt.channel_red_chi2s[0]:
        chi.extend(c)
        chi_n.append(len(c))
    zap, zap_n = [], []
    for z in gt.zap_channels[0]:
        zap.extend(int(v) for v in z)
        zap_n.append(len(z))
    return dict(chi2=np.array(chi, dtype=np.float64),
                chi2_n=np.array(chi_n, dtype=np.int64),
                zap=np.array(zap, dtype=np.int64),
                zap_n=np.array(zap_n, dtype=np.int64),
                show_model=np.asarray(model, dtype=np.float64),
                show_ok=np.asarray(ok, dtype=np.int64))


def main():
    from full_inputs import write_scat, write_spline
    write_scat()
    write_spline()
    store = {}

    def put(key, r):
        for k, v in r.items():
            store[key + "/" + k] = v
    put("resp", run_resp())
    for c in II.CASES:
        if c["name"] == "nb":
            put("nb", run_nb(c))
            continue
        r, gt, files = run_toas(c)
        put(c["name"], r)
        if c["name"] == "toa_pd":
            put("zap", run_zap(gt, files))
    np.savez_compressed(OUT, **store)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(store),
                                              os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
