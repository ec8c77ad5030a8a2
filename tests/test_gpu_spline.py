"""GPU: the stationary-wavelet engine (ppf_swt_analyse_batch /
ppf_swt_score_batch) against the NumPy evaluator at the shapes where the
kernels can go wrong, the golden grids of make_golden_spline.py, and
pplib.smart_smooth / ppspline.DataPortrait end to end on the device.

The golden data come from the reference's own functions on a NumPy stand-in
for PyWavelets; agreement with the real PyWavelets is unverified."""
import sys
import os

import numpy as np
import pytest

import splinecases as SC
from pulseportraiture_amd import _lib, _swt, engine, pplib, ppspline

pytestmark = pytest.mark.gpu

G, EPS = SC.G, SC.EPS
NP = _swt.NumpyEvaluator()
# The largest relative differences of signal, noise and red_chi2 between the
# device and the golden grids over every stored profile, level and factor,
# measured on one MI355X (test_device_matches_golden_grids prints them; the
# kernels are bitwise reproducible, so these are constants of the build).
# Each figure is asserted at 16 times its own measured value: a
# power-spectrum tail is a sum of small terms, and the margin covers the
# other shapes.  The noise figure comes from rows whose spectrum tail is
# ~1e-10 of the signal; the red_chi2 figure comes from the fact = 0 points
# alone, where chi^2 ~ 4e-20 is the rounding of the reconstruction itself
# (elsewhere it is below 1e-12).
GRID_MEASURED = np.array([8.88e-16, 3.81e-10, 1.087e-4])
GRID_RTOL = 16 * GRID_MEASURED


def _profile(n, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return np.exp(-0.5 * ((i - 0.37 * n) / (0.02 * n + 1.5)) ** 2) + \
        0.4 * np.exp(-0.5 * ((i - 0.6 * n) / (0.05 * n + 2.0)) ** 2) + \
        rng.normal(0, noise, n)


def _floors(prof, nlevel, noise):
    """The absolute floor under the relative tolerance: what the three
    figures move by when the smoothed row moves by its own bound B (they
    are norms of the row: n B / sqrt(2) on sqrt(signal) and the noise, B /
    sigma on sqrt(red_chi2)); a figure below it is rounding alone."""
    n = len(prof)
    B = SC.row_tol(nlevel, prof)
    return n * B / np.sqrt(2.0), B / noise if noise else 0.0


def _compare(profs, nlevel, cases, facts):
    """Device against the NumPy evaluator: medians, noise, rows, figures."""
    profs = np.atleast_2d(profs)
    hd = engine.swt_analyse(profs, nlevel, len(cases))
    hn = NP.analyse(profs, nlevel)
    for ip, x in enumerate(profs):
        for j in range(nlevel):
            assert abs(hd.medians[ip, j] - hn.medians[ip, j]) <= \
                SC.row_tol(j + 1, x), (ip, j)
    np.testing.assert_allclose(hd.noise, hn.noise, rtol=64 * EPS, atol=0)
    od, rd = engine.swt_score(hd, cases, facts, smooth=True)
    on, rn = NP.score(hn, cases, facts, smooth=True)
    for ic, (ip, lev, soft) in enumerate(cases):
        x = profs[ip]
        err = np.abs(rd[ic] - rn[ic]).max()
        assert err <= SC.row_tol(lev, x), (ic, ip, lev, facts[ic], err)
        amp, chi = _floors(x, lev, hn.noise[ip])
        if not x.any():
            assert od[ic, 0] == 0 and od[ic, 1] == 0 and np.isnan(od[ic, 2])
            continue
        # the floors as movements of the figures themselves
        floor = np.array([2 * np.sqrt(on[ic, 0]) * amp + amp * amp, amp,
                          2 * np.sqrt(on[ic, 2]) * chi + chi * chi])
        assert (np.abs(od[ic] - on[ic]) <= GRID_RTOL * on[ic] + floor).all(), \
            (ic, cases[ic], facts[ic], od[ic], on[ic], floor)
    # bitwise reproducible
    hd2 = engine.swt_analyse(profs, nlevel, len(cases))
    np.testing.assert_array_equal(hd2.medians, hd.medians)
    od2, rd2 = engine.swt_score(hd2, cases, facts, smooth=True)
    np.testing.assert_array_equal(od2, od)
    np.testing.assert_array_equal(rd2, rd)
    return od, rd


@pytest.mark.parametrize("n,L", [(32, 5), (34, 1), (2048, 11), (8192, 13)])
def test_shapes_against_numpy(n, L):
    """n = 32: the upsampled 16-tap filter wraps several times at every
    level; 34: not a power of two; 8192: the LDS limit (two rows)."""
    x = _profile(n, n)
    levels = range(1, L + 1) if n == 32 else [L]
    cases = [(0, lev, soft) for lev in levels for soft in (0, 1)]
    facts = [0.8] * len(cases)
    _compare(x, L, cases, facts)


def test_batch_of_one_case():
    x = _profile(64, 1)
    od, rd = _compare(x, 3, [(0, 2, 0)], [1.0])
    assert od.shape == (1, 3) and rd.shape == (1, 64)
    # without the rows
    h = engine.swt_analyse(x, 3, 1)
    o2, none = engine.swt_score(h, [(0, 2, 0)], [1.0])
    assert none is None
    np.testing.assert_array_equal(o2, od)


def test_mixed_batch():
    """37 cases over 3 profiles (one all zero): fact = 0 (nothing zeroed,
    chi^2 = 0 to rounding), 3, a factor that zeroes everything (signal 0),
    hard and soft."""
    n, L = 128, 7
    profs = np.array([_profile(n, 2), np.zeros(n), _profile(n, 3, 0.3)])
    rng = np.random.default_rng(9)
    cases = [(0, 1, 0), (0, 7, 0), (2, 4, 1), (2, 7, 0), (0, 3, 1),
             (1, 2, 0), (1, 7, 1)]
    facts = [0.0, 0.0, 0.0, 3.0, 3.0, 1.0, 0.0]
    cases += [(0, 5, 0), (2, 2, 1)]
    facts += [1e6, 1e6]
    while len(cases) < 37:
        cases.append((int(rng.integers(0, 3)), int(rng.integers(1, L + 1)),
                      int(rng.integers(0, 2))))
        facts.append(float(rng.uniform(0.0, 3.0)))
    od, rd = _compare(profs, L, cases, facts)
    for ic in (0, 1, 2):                       # fact = 0: the row comes back
        x = profs[cases[ic][0]]
        assert np.abs(rd[ic] - x).max() <= 4 * cases[ic][1] * 1e-11 * \
            np.abs(x).max()
        sig = pplib.get_noise(x)
        assert od[ic, 2] <= (4 * cases[ic][1] * 1e-11 * np.abs(x).max() /
                             sig) ** 2
    for ic in (7, 8):                          # everything zeroed
        assert not rd[ic].any() and od[ic, 0] == 0.0 and od[ic, 1] == 0.0
    assert not rd[5].any() and not rd[6].any()   # the all-zero profile


def test_argument_checks_run_on_the_host():
    lib = _lib.load()
    x = _profile(64, 4)
    for n, L in ((63, 1), (30, 1), (8194, 1), (64, 7), (96, 2)):
        assert lib.ppf_swt_workspace_bytes(1, n, L, 1) == 0
        with pytest.raises(NotImplementedError):
            engine.swt_analyse(np.zeros(n), L)
    with pytest.raises(ValueError):
        engine.swt_analyse(x, 0)
    h = engine.swt_analyse(x, 3, 4)
    for bad in ([(1, 1, 0)], [(-1, 1, 0)], [(0, 4, 0)], [(0, 0, 0)],
                [(0, 1, 2)]):
        with pytest.raises(ValueError):
            engine.swt_score(h, bad, [1.0])
    with pytest.raises(ValueError):
        engine.swt_score(h, [(0, 1, 0)], [np.nan])
    # the Python layer
    with pytest.raises(NotImplementedError):
        pplib.wavelet_smooth(np.zeros(63), nlevel=1)
    with pytest.raises(NotImplementedError):
        pplib.wavelet_smooth(x, nlevel=7)


def test_device_matches_golden_grids():
    """Largest relative difference between the device and the golden grids
    (the reference's functions on the PyWavelets stand-in), all stored
    profiles, levels and factors, per figure: measured 8.88e-16 (signal),
    3.81e-10 (noise), 1.087e-4 (red_chi2, from the fact = 0 points where
    chi^2 ~ 4e-20 is rounding alone); asserted at 16 x each."""
    worst = np.zeros(3)
    for case, what in SC.SEARCHED:
        key = "%s_%s_" % (case, what)
        prof, grids = G[key + "prof"], G[key + "grids"]
        nlev, ns = grids.shape[:2]
        facts = np.mgrid[slice(0.0, 3.0, complex(ns))]
        cases = [(0, lev, 0) for lev in range(1, nlev + 1) for _ in range(ns)]
        h = engine.swt_analyse(prof, nlev, len(cases))
        out = engine.swt_score(h, cases, np.tile(facts, nlev))[0]
        out = out.reshape(nlev, ns, 3)
        zero = grids == 0
        np.testing.assert_array_equal(out[zero], 0.0)
        rel = np.array([np.abs(out[..., q][~zero[..., q]] /
                               grids[..., q][~zero[..., q]] - 1).max()
                        for q in range(3)])
        print("%s %s: max rel signal %.3e noise %.3e red_chi2 %.3e" %
              (case, what, *rel))
        worst = np.maximum(worst, rel)
    print("largest relative differences: %s (asserted at %s)" %
          (worst, GRID_RTOL))
    assert (worst <= GRID_RTOL).all()


@pytest.mark.parametrize("case,what", SC.SEARCHED)
def test_smart_smooth_on_device_reproduces_golden(case, what):
    SC.check_search(case, what, engine.SwtEvaluator())


@pytest.mark.parametrize("name", SC.CASES)
def test_make_spline_model_on_device_reproduces_golden(name):
    dp = ppspline.DataPortrait(SC.databunch(name))
    dp.make_spline_model(quiet=True, **SC.kwargs(name))
    SC.check_model(name, dp)


def test_normalize_portrait_device_methods():
    port = G["norm_in_port"]
    for method in ("rms", "prof"):
        out, vals = pplib.normalize_portrait(port, method, return_norms=True)
        gold = G["norm_%s_vals" % method]
        np.testing.assert_allclose(vals, gold, rtol=1e-8)
        np.testing.assert_allclose(out, G["norm_%s_port" % method],
                                   rtol=1e-8, atol=1e-12)
    out = pplib.normalize_portrait(port, "prof", weights=G["norm_in_weights"])
    np.testing.assert_allclose(out, G["norm_profw_port"], rtol=1e-8,
                               atol=1e-12)
    dp = ppspline.DataPortrait(SC.databunch("b256"))
    before = dp.portx.copy()
    dp.normalize_portrait("rms")
    np.testing.assert_allclose(pplib.get_noise(dp.portx, chans=True), 1.0,
                               rtol=1e-12)
    dp.unnormalize_portrait()
    np.testing.assert_allclose(dp.portx, before, rtol=1e-14)
    assert not hasattr(dp, "unnorm_noise_stds")


def test_written_model_is_a_template_for_get_TOAs(tmp_path, monkeypatch):
    """A .spl written by ppspline reads back to dp.model (1e-12) through
    read_spline_model + gen_spline_portrait on the device, and GetTOAs
    measures one sub-integration made from the same portrait (dispersed
    with the archive's DM) with it: that DM and zero phase at infinite
    frequency within 5 sigma."""
    sys.path.insert(0, os.path.join(SC.HERE, "golden"))
    import full_inputs as FI
    from pulseportraiture_amd import pptoas
    name = "b256"
    dp = ppspline.DataPortrait(SC.databunch(name))
    dp.make_spline_model(quiet=True, **SC.kwargs(name))
    spl = str(tmp_path / "model.spl")
    dp.write_model(spl, quiet=True)
    mname, model = pplib.read_spline_model(spl, dp.freqs[0], quiet=True)
    assert mname == dp.model_name
    assert np.abs(model - dp.model).max() <= 1e-12 * np.abs(dp.model).max()
    d = SC.inputs(name)
    nchan, nbin = d["port"].shape
    weights = np.zeros((1, nchan))
    weights[0, d["ok"]] = 1.0
    # GetTOAs fits dispersed data: the archive's DM put back about infinite
    # frequency (rotate_data's sign: negative values delay)
    P = float(FI.S.P0)
    DM0 = float(FI.S.DM0)
    disp = pplib.rotate_data(d["port"], 0.0, -DM0, P, d["freqs"], np.inf)
    fi = dict(subints=disp[None], weights=weights, dfs=np.ones(1),
              parangles=np.zeros(1))
    conf = dict(nbin=nbin, bw=800.0, lo=1100.0)
    arch = pplib.DataBunch(
        epochs=[pplib.MJD(55000.0)], filename="one.fits",
        phases=pplib.get_bin_centers(nbin),
        **FI.archive_fields(conf, fi, d["freqs"], d["noise_stds"][None],
                            d["SNRs"][None]))
    monkeypatch.setattr(pptoas, "load_data", lambda fn, **k: arch)
    meta = tmp_path / "meta.txt"
    meta.write_text("one.fits\n")
    gt = pptoas.GetTOAs(str(meta), spl, quiet=True)
    gt.get_TOAs(quiet=True)
    assert len(gt.TOA_list) == 1
    phi, phi_err = gt.phis[0][0], gt.phi_errs[0][0]
    DM, DM_err = gt.DMs[0][0], gt.DM_errs[0][0]
    nu_ref = float(np.ravel(gt.nu_refs[0][0])[0])
    # the phase at infinite frequency, where nothing was injected; at the
    # zero-covariance frequency the two errors are independent
    phi_inf = float(pplib.phase_transform(phi, DM, nu_ref, np.inf, P,
                                          mod=True))
    err_inf = np.hypot(phi_err, pplib.Dconst * DM_err / P * nu_ref ** -2.0)
    print("DM - DM0 %.2e +/- %.2e, phase at infinity %.2e +/- %.2e "
          "(nu_ref %.1f)" % (DM - DM0, DM_err, phi_inf, err_inf, nu_ref))
    assert gt.DM0s[0] == DM0
    assert 0 < DM_err < 1e-2 and abs(DM - DM0) <= 5 * DM_err
    assert 0 < phi_err < 1e-2 and abs(phi_inf) <= 5 * err_inf
