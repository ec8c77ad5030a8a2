"""Shared by test_spline_host.py and test_gpu_spline.py: the golden cases of
tests/golden/splinefit.npz (make_golden_spline.py: the reference's
make_spline_model / smart_smooth on a NumPy stand-in for PyWavelets) and the
comparisons both evaluators have to pass."""
import json
import os

import numpy as np
import scipy.interpolate as si

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "splinefit.npz"))
CASES = [str(n) for n in G["case_names"]]
EPS = np.finfo(np.float64).eps
# profiles whose search (level, factor, row, grids) is stored
SEARCHED = [(c, w) for c in ("b256", "b256_hi")
            for w in ("mean", "ev0", "ev1", "ev2")]


def row_tol(nlevel, x):
    """The smoothed-row bound: every level contributes 32 taps and the
    halving, each within eps of its exact value: 64 L eps max|x|."""
    return 64 * nlevel * EPS * np.abs(x).max()


def inputs(name):
    src = str(G[name + "_in_from"])
    flip = -1 if bool(G[name + "_in_flip"]) else 1
    d = {k: G["%s_in_%s" % (src, k)] for k in
         ("port", "freqs", "noise_stds", "SNRs")}
    d = {k: v[::flip] for k, v in d.items()}
    d["ok"] = G[src + "_in_ok"]
    d["bw"] = flip * float(G[src + "_in_bw"])
    return d


def kwargs(name):
    return json.loads(str(G[name + "_kw"]))


def databunch(name):
    from pulseportraiture_amd import pplib
    d = inputs(name)
    nchan, nbin = d["port"].shape
    masks = np.zeros((1, 1, nchan, nbin))
    masks[0, 0, d["ok"]] = 1.0
    return pplib.DataBunch(
        subints=d["port"][None, None], masks=masks, freqs=d["freqs"][None],
        ok_ichans=[d["ok"]], noise_stds=d["noise_stds"][None, None],
        SNRs=d["SNRs"][None, None], Ps=np.array([0.003]),
        phases=pplib.get_bin_centers(nbin), nu0=1500.0, bw=d["bw"],
        source="J0000+0000", nbin=nbin, nchan=nchan,
        filename="golden_%s.fits" % name)


def numpy_spline_portrait(mean_prof, freqs, eigvec, tck, nbin=None):
    """pplib.gen_spline_portrait at the model's own nbin with SciPy's splev
    (the host tests have no device)."""
    assert nbin is None or nbin == len(mean_prof)
    if not eigvec.shape[1]:
        return np.tile(mean_prof, (len(freqs), 1))
    proj = np.array(si.splev(freqs, tck, der=0, ext=0)).T
    return np.dot(proj, eigvec.T) + mean_prof


def golden_modelx(name):
    if name + "_modelx" in G.files:
        return G[name + "_modelx"]
    return G[name + "_model"][G[name + "_modelx_rows"]]


def check_model(name, dp):
    """make_spline_model's attributes against the golden case: ieig and the
    knots equal, rows and model within 1e-11 max|model|, eigenvector
    quantities up to one sign per component."""
    smooth = bool(G[name + "_smooth"])
    model = G[name + "_model"]
    tol = 1e-11 * np.abs(model).max()
    np.testing.assert_array_equal(dp.ieig, G[name + "_ieig"])
    assert dp.ncomp == len(G[name + "_ieig"])
    np.testing.assert_array_equal(dp.tck[0], G[name + "_tck_t"])
    assert int(dp.tck[2]) == int(G[name + "_tck_k"])
    ev = G[name + "_eigval"]
    np.testing.assert_allclose(dp.eigval[:10], ev, rtol=0,
                               atol=2 * dp.portx.shape[1] * EPS * ev[0])
    np.testing.assert_allclose(dp.mean_prof, G[name + "_mean_prof"], rtol=0,
                               atol=tol)
    ie = np.asarray(dp.ieig, dtype=int)
    gold_vec = G[name + "_eigvec_sel"]
    sign = np.array([np.sign(np.dot(dp.eigvec[:, i], gold_vec[:, j]))
                     for j, i in enumerate(ie)])
    if len(ie):
        # eigenvectors: Davis-Kahan with the summation bound on the matrix
        gaps = np.array([min(abs(dp.eigval[i] - dp.eigval[i - 1]) if i else
                             np.inf, abs(dp.eigval[i] - dp.eigval[i + 1]))
                         for i in ie])
        vtol = 2 * (2 * dp.portx.shape[1] * EPS * ev[0]) / gaps
        dv = np.abs(dp.eigvec[:, ie] * sign - gold_vec).max(axis=0)
        assert (dv <= np.maximum(vtol, 1e-11)).all(), (dv, vtol)
    if smooth:
        np.testing.assert_allclose(dp.smooth_mean_prof,
                                   G[name + "_smooth_mean_prof"], rtol=0,
                                   atol=tol)
        assert dp.smooth_mean_prof.any()          # it passed the chi^2 gate
        np.testing.assert_allclose(dp.smooth_eigvec[:, ie] * sign,
                                   G[name + "_smooth_eigvec_sel"], rtol=0,
                                   atol=tol)
    gp = G[name + "_proj_port"]
    if len(ie):
        np.testing.assert_allclose(
            dp.proj_port * sign, gp, rtol=0,
            atol=1e-11 * np.abs(gp).max() * max(1.0, np.abs(model).max()))
        gc = G[name + "_tck_c"]
        np.testing.assert_allclose(np.array(dp.tck[1]) * sign[:, None], gc,
                                   rtol=0, atol=1e-11 * np.abs(gc).max())
        assert dp.ier == int(G[name + "_ier"])
    else:
        assert dp.proj_port.shape == gp.shape
        assert dp.ier is None and len(dp.tck[0]) == 0
    np.testing.assert_allclose(dp.model, model, rtol=0, atol=tol)
    np.testing.assert_allclose(dp.modelx, golden_modelx(name), rtol=0,
                               atol=tol)
    np.testing.assert_array_equal(dp.model_masked,
                                  dp.model * dp.masks[0, 0])
    assert dp.model_name == dp.datafile + ".spl"


def check_search(case, what, evaluator):
    """pplib.smart_smooth on one stored profile: level equal, factor to 1e-9
    relative, row within 1e-11 max|row| (checked through the chosen pair,
    which the evaluator reports back)."""
    from pulseportraiture_amd import pplib
    key = "%s_%s_" % (case, what)
    prof = G[key + "prof"]
    picked = {}
    inner = evaluator

    class Spy(object):
        noise = staticmethod(inner.noise)
        analyse = staticmethod(inner.analyse)

        @staticmethod
        def score(h, cases, facts, smooth=False):
            if smooth:
                picked["level"], picked["fact"] = cases[0][1], facts[0]
            return inner.score(h, cases, facts, smooth)

    row = pplib.smart_smooth(prof, rchi2_tol=0.1, evaluator=Spy)
    assert picked["level"] == int(G[key + "level"])
    assert abs(picked["fact"] - float(G[key + "fact"])) <= \
        1e-9 * float(G[key + "fact"])
    gold = G[key + "row"]
    np.testing.assert_allclose(row, gold, rtol=0,
                               atol=1e-11 * max(np.abs(gold).max(),
                                                np.abs(prof).max()))
