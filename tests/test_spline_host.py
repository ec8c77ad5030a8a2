"""ppspline on the host: the wavelet filter, the NumPy evaluator, pca, and
the drivers (smart_smooth, find_significant_eigvec, make_spline_model) on the
NumPy evaluator against the golden cases of make_golden_spline.py (the
reference's own functions on a NumPy stand-in for PyWavelets; agreement with
the real PyWavelets is unverified).  No GPU."""
import numpy as np
import pytest

import splinecases as SC
from pulseportraiture_amd import _swt, pplib, ppspline

G, EPS = SC.G, SC.EPS
EV = _swt.NumpyEvaluator()


def _defect():
    """max_m |sum_k h_k h_{k+2m} - delta_m0| of the db8 table."""
    h = _swt.REC_LO
    return max(abs(np.dot(h[:16 - 2 * m], h[2 * m:]) - (m == 0))
               for m in range(8))


def test_filter_identities():
    h = _swt.REC_LO
    assert abs(h.sum() - np.sqrt(2.0)) <= 4 * EPS
    delta = _defect()
    print("orthonormality defect %.2e" % delta)
    assert delta < 1e-11
    # eight vanishing moments of the high-pass filter
    k = np.arange(16.0)
    for p in range(8):
        m = np.dot(_swt.DEC_HI, k ** p)
        assert abs(m) <= 1e-9 * np.dot(np.abs(_swt.DEC_HI), k ** p), (p, m)
    np.testing.assert_array_equal(_swt.DEC_LO, h[::-1])
    np.testing.assert_array_equal(_swt.DEC_HI, h * (-1.0) ** (k + 1))


@pytest.mark.parametrize("n,L", [(32, 5), (34, 1), (250, 1), (256, 8),
                                 (2048, 11)])
def test_perfect_reconstruction(n, L):
    x = np.random.default_rng(n).normal(size=n)
    co = _swt.swt(x, L)
    back = _swt.iswt(co[-1][0], [c[1] for c in co])
    err = np.abs(back - x).max()
    bound = 4 * L * _defect() * np.abs(x).max()
    print("n %d L %d: %.2e (bound %.2e)" % (n, L, err, bound))
    assert err <= bound


@pytest.mark.parametrize("threshtype", ["hard", "soft"])
def test_shift_equivariance(threshtype):
    rng = np.random.default_rng(5)
    x = np.exp(-0.5 * ((np.arange(256) - 90) / 5.0) ** 2) + \
        rng.normal(0, 0.05, 256)
    both = pplib.wavelet_smooth(np.array([x, np.roll(x, 37)]), nlevel=6,
                                threshtype=threshtype, fact=1.2, evaluator=EV)
    assert both.shape == (2, 256) and np.abs(both[0] - x).max() > 1e-3
    assert np.abs(np.roll(both[0], 37) - both[1]).max() <= SC.row_tol(6, x)
    one = pplib.wavelet_smooth(x, nlevel=6, threshtype=threshtype, fact=1.2,
                               evaluator=EV)
    np.testing.assert_array_equal(one, both[0])


def grid_bounds(prof, nlevel, noise):
    """What two float64 evaluations of the same (signal, noise, red_chi2) may
    differ by: with e the difference of the smoothed rows, |e_i| <= B =
    row_tol, the three are norms of s (Parseval: sum_k>=1 |S_k|^2 <= n/2
    sum s_i^2), so sqrt(signal) and the noise move by at most n B / sqrt(2)
    and sqrt(n red_chi2) sigma by at most sqrt(n) B."""
    n = len(prof)
    B = SC.row_tol(nlevel, prof)
    return n * B / np.sqrt(2.0), B / noise


@pytest.mark.parametrize("case,what", SC.SEARCHED)
def test_numpy_evaluator_matches_golden_grids(case, what):
    key = "%s_%s_" % (case, what)
    prof, grids = G[key + "prof"], G[key + "grids"]
    nlev, ns = grids.shape[:2]
    h = EV.analyse(prof[None], nlev, nlev * ns)
    facts = np.mgrid[slice(0.0, 3.0, complex(ns))]
    cases = [(0, lev, 0) for lev in range(1, nlev + 1) for _ in range(ns)]
    out = EV.score(h, cases, np.tile(facts, nlev))[0].reshape(nlev, ns, 3)
    for il in range(nlev):
        amp, chi = grid_bounds(prof, il + 1, h.noise[0])
        assert np.abs(np.sqrt(out[il, :, 0]) -
                      np.sqrt(grids[il, :, 0])).max() <= amp
        assert np.abs(out[il, :, 1] - grids[il, :, 1]).max() <= amp
        assert np.abs(np.sqrt(out[il, :, 2]) -
                      np.sqrt(grids[il, :, 2])).max() <= \
            chi + 16 * EPS * np.sqrt(grids[il, :, 2]).max()


@pytest.mark.parametrize("nchan,nbin", [(30, 256), (40, 32)])
def test_pca_matches_eigh_of_np_cov(nchan, nbin):
    rng = np.random.default_rng(nchan)
    shape = np.exp(-0.5 * ((np.arange(nbin) - nbin / 3.0) / 3.0) ** 2)
    port = np.outer(1 + 0.3 * rng.normal(size=nchan), shape) + \
        np.outer(rng.normal(size=nchan), np.roll(shape, 4)) + \
        0.05 * rng.normal(size=(nchan, nbin))
    w = rng.uniform(0.5, 2.0, nchan)
    mean_prof = (port.T * w).T.sum(axis=0) / w.sum()
    eigval, eigvec = pplib.pca(port, mean_prof, w, quiet=True)
    ncol = min(nchan, nbin)
    assert eigval.shape == (nbin,) and eigvec.shape == (nbin, ncol)
    cov = np.cov((port - mean_prof).T, aweights=w, ddof=1)
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1], vec[:, ::-1]
    K = nbin if nchan < nbin else nchan          # the contraction length
    E = 2 * K * EPS * lam[0]
    assert np.abs(eigval - lam).max() <= E
    rank = min(nchan - 1, nbin)
    assert (eigval[rank:] == 0).all() and (eigvec[:, rank:] == 0).all()
    np.testing.assert_allclose(np.linalg.norm(eigvec[:, :rank], axis=0), 1.0,
                               rtol=0, atol=8 * EPS)
    for i in range(5):
        gap = min(lam[i - 1] - lam[i] if i else np.inf, lam[i] - lam[i + 1])
        s = np.sign(np.dot(eigvec[:, i], vec[:, i]))
        assert np.abs(s * eigvec[:, i] - vec[:, i]).max() <= 2 * E / gap
    # default mean profile and weights
    ev2, _ = pplib.pca(port, quiet=True)
    lam2 = np.linalg.eigvalsh(np.cov((port - port.mean(axis=0)).T,
                                     ddof=1))[::-1]
    assert np.abs(ev2[:ncol] - lam2[:ncol]).max() <= 2 * K * EPS * lam2[0]
    # reconstruct_portrait on the full basis of the row space gives port back
    rec = pplib.reconstruct_portrait(port, mean_prof, eigvec[:, :rank])
    cen = port - mean_prof
    cen = cen - (cen * w[:, None]).sum(axis=0) / w.sum()
    assert np.abs(rec - mean_prof - cen).max() <= 1e-12 * np.abs(port).max()


def test_find_significant_eigvec_stays_inside_the_columns():
    """pca returns min(nchan, nbin) columns: fewer than check_max."""
    rng = np.random.default_rng(1)
    vec = np.linalg.qr(rng.normal(size=(64, 4)))[0]
    ieig, sm = pplib.find_significant_eigvec(vec, check_max=10,
                                             return_max=10, evaluator=EV)
    assert len(ieig) == 0 and sm.shape == vec.shape
    ieig = pplib.find_significant_eigvec(np.zeros((64, 0)),
                                         return_smooth=False, evaluator=EV)
    assert len(ieig) == 0


@pytest.mark.parametrize("case,what", SC.SEARCHED)
def test_smart_smooth_reproduces_golden_search(case, what):
    SC.check_search(case, what, EV)


def test_smart_smooth_early_returns():
    x = np.random.default_rng(2).normal(size=(2, 64))
    assert pplib.smart_smooth(x, try_nlevels=0, evaluator=EV) is x
    odd = x[:, :63]
    assert pplib.smart_smooth(odd, evaluator=EV) is odd
    # one odd-length profile comes back as [1, nbin], as the reference's
    back = pplib.smart_smooth(odd[0], evaluator=EV)
    assert back.shape == (1, 63)
    np.testing.assert_array_equal(back[0], odd[0])
    z = np.array([x[0], np.zeros(64)])
    out = pplib.smart_smooth(z, evaluator=EV)
    assert out.shape == z.shape and not out[1].any()
    one = pplib.smart_smooth(x[0], evaluator=EV)
    np.testing.assert_array_equal(one, out[0])
    # not a power of two: one level, whatever is asked for
    y = np.random.default_rng(3).normal(size=96)
    np.testing.assert_array_equal(
        pplib.smart_smooth(y, try_nlevels=5, evaluator=EV),
        pplib.smart_smooth(y, try_nlevels=1, evaluator=EV))


def _make(name, monkeypatch):
    monkeypatch.setattr(ppspline, "gen_spline_portrait",
                        SC.numpy_spline_portrait)
    dp = ppspline.DataPortrait(SC.databunch(name))
    dp.make_spline_model(quiet=True, evaluator=EV, **SC.kwargs(name))
    return dp


@pytest.mark.parametrize("name", SC.CASES)
def test_make_spline_model_reproduces_golden(name, monkeypatch, capsys):
    dp = _make(name, monkeypatch)
    SC.check_model(name, dp)
    assert dp.reconst_port.shape == dp.portx.shape
    assert dp.eigvec.shape == (dp.nbin, min(dp.nchanx, dp.nbin))


@pytest.mark.parametrize("name", ["b256", "b256_raw", "b255_raw"])
def test_write_model_round_trip(name, monkeypatch, tmp_path):
    dp = _make(name, monkeypatch)
    path = str(tmp_path / "m.spl")
    dp.write_model(path, quiet=True)
    import pickle
    with open(path, "rb") as fh:
        raw = pickle.load(fh)
    assert isinstance(raw, list) and len(raw) == 6
    mname, source, datafile, mean_prof, eigvec, tck = \
        pplib.read_spline_model(path, quiet=True)
    assert (mname, source, datafile) == (dp.model_name, "J0000+0000",
                                         dp.datafile)
    assert eigvec.shape == (dp.nbin, dp.ncomp)
    want = dp.smooth_mean_prof if bool(G[name + "_smooth"]) else dp.mean_prof
    np.testing.assert_array_equal(mean_prof, want)
    model = SC.numpy_spline_portrait(mean_prof, dp.freqs[0], eigvec, tck)
    assert np.abs(model - dp.model).max() <= 1e-12 * np.abs(dp.model).max()


def test_missing_weights_are_unit_on_ok_ichans():
    dp = ppspline.DataPortrait(SC.databunch("b256"))
    w = np.zeros(32)
    w[G["b256_in_ok"]] = 1.0
    np.testing.assert_array_equal(dp.weights, w[None])


@pytest.mark.parametrize("method", ["mean", "max", "abs"])
def test_normalize_portrait_host_methods(method):
    port = G["norm_in_port"]
    out, vals = pplib.normalize_portrait(port, method, return_norms=True)
    np.testing.assert_allclose(out, G["norm_%s_port" % method], rtol=4 * EPS,
                               atol=0)
    np.testing.assert_allclose(vals, G["norm_%s_vals" % method],
                               rtol=4 * EPS, atol=0)
    assert not out[5].any() and vals[5] == 1.0
    np.testing.assert_array_equal(
        pplib.normalize_portrait(port, method), out)


def test_count_crossings():
    x = np.array([0.0, 2.0, 0.0, 2.0, 1.0, 0.0])
    assert pplib.count_crossings(x, 0.5) == 4
    assert pplib.count_crossings(x, 1.0) == 4     # one sample on the level


def test_not_implemented_paths(tmp_path, capsys):
    x = np.random.default_rng(4).normal(size=64)
    with pytest.raises(NotImplementedError):
        pplib.wavelet_smooth(x, wavelet="db4", evaluator=EV)
    with pytest.raises(NotImplementedError):
        pplib.smart_smooth(x, wavelet="sym8", evaluator=EV)
    with pytest.raises(NotImplementedError):
        pplib.fit_wavelet_smooth_function(1.0, x, "haar", 2, "hard", 0.1, EV)
    for bad, lev in ((x[:63], 1), (x[:30], 1), (np.zeros(8194), 1), (x, 7),
                     (np.zeros(96), 2), (x, 0)):
        with pytest.raises(NotImplementedError):
            pplib.wavelet_smooth(bad, nlevel=lev, evaluator=EV)
    assert pplib.normalize_portrait(x[None], "median") is None
    dp = ppspline.DataPortrait(SC.databunch("b256"))
    for call in (dp.write_model_archive, dp.show_eigenprofiles,
                 dp.show_spline_curve_projections, dp.show_model_fit):
        with pytest.raises(NotImplementedError):
            call("x")
    meta = tmp_path / "meta.txt"
    meta.write_text("a.fits\nb.fits\n")
    with pytest.raises(NotImplementedError):
        ppspline.DataPortrait(str(meta))
    with pytest.raises(NotImplementedError):
        ppspline.DataPortrait(SC.databunch("b256"), joinfile="j")


def test_find_significant_eigvec_borderline_branch():
    """An S/N in [cutoff, 3 cutoff) is decided by the zero crossings of the
    smoothed eigenvector: a smooth one (fewer than 2 % of nbin crossings of
    its 10 % level) stays; without the check the S/N alone decides; below
    the cutoff it goes."""
    vec = G["b256_ev0_prof"][:, None]
    row = pplib.smart_smooth(vec[:, 0], rchi2_tol=0.1, evaluator=EV)
    snr = np.sum(np.abs(np.fft.rfft(row)[1:]) ** 2) / \
        (EV.noise(vec.T)[0] * np.sqrt(128.0))
    ncross = pplib.count_crossings(abs(row), 0.1 * abs(row).max())
    print("snr %.1f, crossings %d" % (snr, ncross))
    assert row.any() and 0 <= ncross < int(0.02 * 256)
    kw = dict(rchi2_tol=0.1, evaluator=EV)
    ieig, sm = pplib.find_significant_eigvec(vec, snr_cutoff=snr / 2.0, **kw)
    assert list(ieig) == [0]
    np.testing.assert_array_equal(sm[:, 0], row)
    ieig = pplib.find_significant_eigvec(vec, snr_cutoff=snr / 2.0,
                                         check_crossings=False,
                                         return_smooth=False, **kw)
    assert list(ieig) == [0]
    ieig, sm = pplib.find_significant_eigvec(vec, snr_cutoff=snr * 2.0, **kw)
    assert list(ieig) == [] and not sm.any()
