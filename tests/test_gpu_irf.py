"""GPU: the instrumental response on the template -- the device kernel
(ppf_inst_response_batch, k_inst_resp) against its NumPy arithmetic, and
GetTOAs with add_instrumental_response=True against the reference's own runs
(tests/golden/irf.npz, make_golden_irf.py; inputs rebuilt by
tests/golden/irf_inputs.py and checked against the stored SHA-256)."""
import sys

import numpy as np
import pytest

import goldens as G
from test_gpu_fullshape import _MJD, _tim_tokens_match, _same_printed_number

sys.path.insert(0, G.GOLDEN)
import irf_inputs as II  # noqa: E402
import synth_np as S  # noqa: E402

pytestmark = pytest.mark.gpu

SIG, RCHI2 = G.SIGMA_TOL, G.RCHI2_RTOL


# ------------------------------------------------------------- kernel ------
@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("nbin", [32, 64, 1000, 1022, 2048, 8192])
def test_inst_response_kernel_matches_numpy(nbin, with_table):
    """engine.inst_response_rows against irfft(rfft(src[src_row]) T
    sinc(k w)) at the smallest and the largest length, mixed radix (1000),
    generic radix (1022 = 2 x 7 x 73) and the widest register tile: 5 rows
    fanned out of 2 sources, w with 0 and a value with nharm w > 1; T NULL
    and given.  atol 1e-11 on unit-normal rows: the bar
    test_rotate_any_nbin_matches_numpy holds rotate_data to at these
    lengths."""
    from pulseportraiture_amd import engine
    rng = np.random.default_rng(nbin)
    src = rng.normal(size=(2, nbin))
    src_row = np.array([1, 0, 0, 1, 0], dtype=np.int32)
    k = np.arange(nbin // 2 + 1)
    w = np.array([0.0, 0.013, 3.3 / len(k), 0.1, 1e-4])
    assert len(k) * w[2] > 1
    T = np.sinc(k * 0.02) * np.exp(-(np.pi * k * 0.01) ** 2 /
                                   (4 * np.log(2))) if with_table else None
    X = np.fft.rfft(src[src_row], axis=-1) * np.sinc(np.outer(w, k))
    if with_table:
        X = X * T
    want = np.fft.irfft(X, axis=-1)
    got = engine.inst_response_rows(src, src_row, T, w).cpu().numpy()
    assert got.shape == want.shape == (5, nbin)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-11)
    if not with_table:
        # w = 0 and no table: the row itself
        np.testing.assert_allclose(got[0], src[1], rtol=0, atol=1e-11)


@pytest.mark.parametrize("nbin", [33, 1001, 16384])
def test_inst_response_kernel_refuses_odd_and_long_rows(nbin):
    """Odd nbin and nbin > 8192: PPF_EUNSUP from the library itself, seen
    as NotImplementedError."""
    import ctypes
    import torch
    from pulseportraiture_amd import _lib, engine
    dev = engine.device()
    src = torch.zeros((1, nbin), dtype=torch.float64, device=dev)
    out = torch.zeros((1, nbin), dtype=torch.float64, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    w = torch.zeros(1, dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_inst_response_batch(
        ctx, 1, nbin, ctypes.c_void_p(src.data_ptr()),
        ctypes.c_void_p(idx.data_ptr()), None, ctypes.c_void_p(w.data_ptr()),
        ctypes.c_void_p(out.data_ptr()), None)
    assert rc == _lib.PPF_EUNSUP
    with pytest.raises(NotImplementedError):
        _lib.check(rc, ctx)
    with pytest.raises(NotImplementedError):
        engine.inst_response_rows(np.zeros((1, nbin)), [0], None, [0.0])


def test_inst_response_rows_validates_indices():
    from pulseportraiture_amd import engine
    with pytest.raises(ValueError):
        engine.inst_response_rows(np.zeros((2, 64)), [0, 2], None, [0., 0.])
    with pytest.raises(ValueError):
        engine.inst_response_rows(np.zeros((2, 64)), [0, 1], np.ones(32),
                                  [0., 0.])


# ------------------------------------------------------------ GetTOAs ------
_CASES = {}


def _case(name):
    """(golden case, {file name: DataBunch}, template path), rebuilt once."""
    if name in _CASES:
        return _CASES[name]
    from pulseportraiture_amd.pplib import DataBunch, get_bin_centers
    c = G.load_case("irf.npz", name)
    conf = II.conf(name)
    files_in, freqs = II.inputs(conf)
    files = {}
    for f, fi in enumerate(files_in):
        sub = fi["subints"].astype(np.float32)
        assert S.sha(sub) == str(c["sha"][f]), \
            "rebuilt inputs of %s archive %d differ" % (name, f)
        np.testing.assert_array_equal(fi["weights"], c["f%d_weights" % f])
        np.testing.assert_array_equal(fi["Ps"], c["f%d_Ps" % f])
        fname = "%s_%d.fits" % (name, f)
        files[fname] = DataBunch(
            epochs=[_MJD(e) for e in fi["epochs"]], filename=fname,
            phases=get_bin_centers(conf["nbin"]),
            **II.archive_fields(conf, fi, freqs, c["f%d_noise" % f],
                                c["f%d_snrs" % f]))
    _CASES[name] = (c, files, II.gmodel(conf))
    return _CASES[name]


def _gettoas(name, monkeypatch, tmp_path, ird=None, **kw):
    from pulseportraiture_amd import pptoas
    c, files, gm = _case(name)
    monkeypatch.setattr(pptoas, "load_data", lambda fn, **k: files[fn])
    monkeypatch.setattr(pptoas, "_MJD", _MJD)
    meta = tmp_path / "meta.txt"
    meta.write_text("".join(n + "\n" for n in files))
    gt = pptoas.GetTOAs(str(meta), gm, quiet=True)
    if ird is not None:
        gt.ird.update(DM=ird["DM"], wids=list(ird["wids"]),
                      irf_types=list(ird["irf_types"]))
    return c, files, gt, dict(II.conf(name).get("kw", {}), **kw)


def _tim_lines(gt, capsys):
    from pulseportraiture_amd import pplib
    capsys.readouterr()
    pplib.write_TOAs(gt.TOA_list)
    return capsys.readouterr().out.splitlines()


@pytest.mark.parametrize("name", ["toa_pd", "toa_spl"])
def test_gettoas_with_response_matches_reference(name, monkeypatch, tmp_path,
                                                 capsys):
    """get_TOAs(add_instrumental_response=True), phase + DM: toa_pd (.gmodel;
    DM smearing + rect + gauss; three sub-ints of different P, channel 1
    zapped in one so that its chan_bw doubles) and toa_spl (spline template,
    constant responses, nbin = 1000) against the reference's runs, at the
    bars of test_fullshape_gettoas_matches_reference: phases and DMs within
    0.01 sigma, chi2_red 1e-8, errors 1e-5, every .tim token to its printed
    precision.  The reference's no-response run of the same data sits more
    than 10 sigma away in DM (asserted here and by the generator), so a
    response that is ignored, or built with the wrong P or chan_bw, fails."""
    c, files, gt, kw = _gettoas(name, monkeypatch, tmp_path,
                                II.conf(name)["ird"])
    gt.get_TOAs(quiet=True, add_instrumental_response=True, **kw)
    for f in range(int(c["nfile"])):
        assert np.all(np.abs(c["out_DMs"][f] - c["nr_DMs"][f]) >
                      10 * c["out_DM_errs"][f])
        dphi = np.abs(G.phase_diff(gt.phis[f], c["out_phis"][f]))
        assert np.all(dphi < SIG * c["out_phi_errs"][f]), dphi
        assert np.all(np.abs(gt.DMs[f] - c["out_DMs"][f]) <
                      SIG * c["out_DM_errs"][f])
        np.testing.assert_allclose(gt.red_chi2s[f], c["out_red_chi2s"][f],
                                   rtol=RCHI2)
        np.testing.assert_allclose(gt.phi_errs[f], c["out_phi_errs"][f],
                                   rtol=1e-5)
        np.testing.assert_allclose(gt.DM_errs[f], c["out_DM_errs"][f],
                                   rtol=1e-5)
        np.testing.assert_allclose(gt.snrs[f], c["out_snrs"][f], rtol=1e-6)
        np.testing.assert_allclose(np.array(gt.nu_refs[f], dtype=float),
                                   c["out_nu_refs"][f], rtol=1e-6)
        assert abs(gt.DeltaDM_means[f] - c["out_DeltaDM_means"][f]) < \
            SIG * c["out_DeltaDM_errs"][f]
    _tim_tokens_match(_tim_lines(gt, capsys), list(c["out_tim_lines"]))


def test_gettoas_scattering_fit_with_response_matches_reference(
        monkeypatch, tmp_path, capsys):
    """toa_scat: fit_GM + fit_scat (all five parameters) with the DM-smearing
    response on the unscattered template (pptoas.py:408-434), at the bars of
    test_gettoas_branches_match_reference: parameters within 0.01 sigma at
    the reference's reference frequencies, chi2_red 1e-8, phase errors 1e-4
    and nu_refs 1e-5 (the reference's trust-ncg stops short along the flat
    GM / tau / alpha direction, see that test), .tim tokens to printed
    precision or 1e-5."""
    name = "toa_scat"
    c, files, gt, kw = _gettoas(name, monkeypatch, tmp_path,
                                II.conf(name)["ird"])
    gt.get_TOAs(quiet=True, add_instrumental_response=True, **kw)
    for f in range(int(c["nfile"])):
        assert np.all(np.abs(c["out_DMs"][f] - c["nr_DMs"][f]) >
                      10 * c["out_DM_errs"][f])
        data = files["%s_%d.fits" % (name, f)]
        dfs = data.doppler_factors
        for s_ in range(len(c["out_phis"][f])):
            ferr = [c["out_" + k][f][s_] for k in
                    ("phi_errs", "DM_errs", "GM_errs", "tau_errs",
                     "alpha_errs")]
            got = dict(params=[gt.phis[f][s_], gt.DMs[f][s_] / dfs[s_],
                               gt.GMs[f][s_] / dfs[s_] ** 3, gt.taus[f][s_],
                               gt.alphas[f][s_]])
            got.update(zip(("nu_DM", "nu_GM", "nu_tau"),
                           np.array(gt.nu_refs[f][s_], dtype=float)))
            ref = dict(params=[c["out_phis"][f][s_],
                               c["out_DMs"][f][s_] / dfs[s_],
                               c["out_GMs"][f][s_] / dfs[s_] ** 3,
                               c["out_taus"][f][s_], c["out_alphas"][f][s_]],
                       param_errs=ferr)
            ref.update(zip(("nu_DM", "nu_GM", "nu_tau"),
                           c["out_nu_refs"][f][s_]))
            dev = G.param_deviation_sigma(got, ref, float(data.Ps[s_]), True)
            assert dev.max() < SIG, (f, s_, dev)
        np.testing.assert_allclose(gt.red_chi2s[f], c["out_red_chi2s"][f],
                                   rtol=RCHI2)
        np.testing.assert_allclose(gt.phi_errs[f], c["out_phi_errs"][f],
                                   rtol=1e-4)
        np.testing.assert_allclose(gt.snrs[f], c["out_snrs"][f], rtol=1e-6)
        np.testing.assert_allclose(np.array(gt.nu_refs[f], dtype=float),
                                   c["out_nu_refs"][f], rtol=1e-5)
    _tim_tokens_match(_tim_lines(gt, capsys), list(c["out_tim_lines"]),
                      nu0_rtol=1e-5, tok_rtol=1e-5)


def test_narrowband_toas_with_response_match_reference(monkeypatch, tmp_path,
                                                       capsys):
    """get_narrowband_TOAs(add_instrumental_response=True) (pptoas.py:
    983-989), DM smearing + rect, at the bars of
    test_narrowband_toas_match_reference: phases within 0.01 of their
    errors, errors / scales / S/N / gof to 1e-6, .tim lines to their printed
    precision."""
    name = "nb"
    c, files, gt, kw = _gettoas(name, monkeypatch, tmp_path,
                                II.conf(name)["ird"])
    gt.get_narrowband_TOAs(quiet=True, add_instrumental_response=True)
    for f in range(int(c["nfile"])):
        used = c["out_phi_errs"][f] > 0
        moved = np.abs(G.phase_diff(c["out_phis"][f], c["nr_phis"][f]))[used]
        assert np.median(moved / c["out_phi_errs"][f][used]) > 10
        dphi = np.abs(G.phase_diff(gt.phis[f], c["out_phis"][f]))[used]
        assert np.all(dphi < SIG * c["out_phi_errs"][f][used]), dphi
        for key in ("phi_errs", "scales", "scale_errs", "channel_snrs",
                    "channel_red_chi2s"):
            np.testing.assert_allclose(getattr(gt, key)[f],
                                       c["out_" + key][f], rtol=1e-6,
                                       err_msg=key)
    lines, ref = _tim_lines(gt, capsys), list(c["out_tim_lines"])
    assert len(lines) == len(ref)
    for a, b in zip(lines, ref):
        ta, tb = a.split(), b.split()
        assert len(ta) == len(tb)
        for x, y in zip(ta, tb):
            if x.endswith(".gmodel"):            # -tmplt path differs
                continue
            assert _same_printed_number(x, y), (a, b)


def test_zap_and_show_fit_with_response_match_reference(monkeypatch,
                                                        tmp_path):
    """After toa_pd's get_TOAs: get_channels_to_zap's channel chi^2s within
    1e-5 relative of the reference's and identical zap lists (the bars of
    test_channels_to_zap_matches_reference), and show_fit's scaled model of
    sub-int 0 (the response of ALL the channels' freqs at data.Ps[isub],
    pptoas.py:1446-1452).  The model is linear in the fitted scales, which
    the chi^2 bar holds to 1e-5 relative: 1e-5 of the model's peak."""
    c, files, gt, kw = _gettoas("toa_pd", monkeypatch, tmp_path,
                                II.conf("toa_pd")["ird"])
    z = G.load_case("irf.npz", "zap")
    gt.get_TOAs(quiet=True, add_instrumental_response=True, **kw)
    gt.get_channels_to_zap()
    pos = zpos = 0
    for s, (n, m) in enumerate(zip(z["chi2_n"], z["zap_n"])):
        np.testing.assert_allclose(gt.channel_red_chi2s[0][s],
                                   z["chi2"][pos:pos + n], rtol=1e-5, atol=0)
        assert [int(v) for v in gt.zap_channels[0][s]] == \
            [int(v) for v in z["zap"][zpos:zpos + m]]
        pos, zpos = pos + n, zpos + m
    port, model, ok, freqs, noise = gt.show_fit(list(files)[0], isub=0,
                                                show=False, return_fit=True)
    np.testing.assert_array_equal(ok, z["show_ok"])
    np.testing.assert_allclose(model, z["show_model"], rtol=0,
                               atol=1e-5 * np.abs(z["show_model"]).max())


def test_empty_response_is_bitwise_the_default_path(monkeypatch, tmp_path):
    """add_instrumental_response=True with the default (empty)
    instrumental_response_dict: no extra launch, model_index untouched,
    results bitwise equal to add_instrumental_response=False."""
    from pulseportraiture_amd import engine
    runs = []
    for on in (False, True):
        c, files, gt, kw = _gettoas("toa_pd", monkeypatch, tmp_path)

        def no_launch(*a, **k):
            raise AssertionError("response launch on the default path")
        monkeypatch.setattr(engine, "inst_response_rows", no_launch)
        gt.get_TOAs(quiet=True, add_instrumental_response=on, **kw)
        runs.append(gt)
    a, b = runs
    for key in ("phis", "phi_errs", "DMs", "DM_errs", "red_chi2s", "snrs",
                "scales", "scale_errs", "channel_snrs", "covariances",
                "nu_refs", "nfevals"):
        for x, y in zip(getattr(a, key), getattr(b, key)):
            np.testing.assert_array_equal(np.asarray(x, dtype=float),
                                          np.asarray(y, dtype=float), key)
