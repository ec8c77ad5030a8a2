"""CPU: the host side of the Gaussian-component fits.  The Levenberg-Marquardt
driver (_gaussfit) runs on a NumPy evaluator built from the oracle's portrait
builder and must reproduce every golden case of tests/golden/gaussfit.npz
(make_golden_gaussfit.py: MINPACK on lmfit's internal variables, on the
reference's own model) at the project's parity bar: parameters within 0.01
sigma, chi^2 within 1e-8 relative.  write_model is byte-exact against the
reference's text; ppf_gauss_lsq_batch validates its arguments on the host."""
import ctypes
import os

import numpy as np
import pytest

import gausshost as H
import oracle as O
from pulseportraiture_amd import _gaussfit, _lib, pplib

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "gaussfit.npz"))
SIGMA_TOL, CHI2_RTOL = 0.01, 1e-8


def portrait_evaluator(name):
    code, freqs = str(G[name + "__code"]), G[name + "__freqs"]
    data, nu_ref = G[name + "__data"], float(G[name + "__nu_ref"])
    phases = O.get_bin_centers(data.shape[1])

    def model(p):
        return O.gen_gaussian_portrait(code, p[:-1], p[-1], phases, freqs,
                                       nu_ref)
    return _gaussfit.numpy_evaluator(model, data, G[name + "__errs"])


def check_case(name, p, perr, chi2, dof, vary):
    sol, errs = G[name + "__solution"], G[name + "__sol_errs"]
    dev = np.abs(p - sol)[vary] / errs[vary]
    print(name, "max dev %.2e sigma, chi2 rel %.1e, errs rel %.1e (spread "
          "%.1e)" % (dev.max(), abs(chi2 / float(G[name + "__chi2"]) - 1),
                     np.abs(perr[vary] / errs[vary] - 1).max(),
                     float(G[name + "__spread_errs"])))
    assert dev.max() <= SIGMA_TOL
    assert abs(chi2 / float(G[name + "__chi2"]) - 1) <= CHI2_RTOL
    assert dof == int(G[name + "__dof"])
    # error bars: within twice the spread of the two golden solvers' own
    assert np.abs(perr[vary] / errs[vary] - 1).max() <= \
        2 * float(G[name + "__spread_errs"])
    np.testing.assert_array_equal(p[~vary], sol[~vary])


@pytest.mark.parametrize("name", [str(n) for n in G["portraits"]])
def test_driver_reproduces_golden_portrait_fits(name):
    vary = G[name + "__vary"]
    p0 = G[name + "__init"]
    lo, hi = _gaussfit.portrait_bounds(len(p0) - 1)
    p, perr, chi2, dof, res = _gaussfit.levenberg_marquardt(
        portrait_evaluator(name), p0, vary, lo, hi, G[name + "__data"].size)
    assert res.success and res.nfev < 2000 * (vary.sum() + 1)
    check_case(name, p, perr, chi2, dof, vary)
    assert (perr[~vary] == 0.0).all()


@pytest.mark.parametrize("name", [str(n) for n in G["profiles"]])
def test_fit_gaussian_profile_with_numpy_evaluator(name):
    """The public profile fit (flag splicing, the 3-per-component layout)
    through an injected evaluator: one channel at freqs = [nu_ref], '111'."""
    data, errs, init = G[name + "__data"], G[name + "__errs"], G[name + "__init"]
    phases = O.get_bin_centers(len(data))

    def model(p):
        return O.gen_gaussian_portrait("111", p[:-1], p[-1], phases, [1.0],
                                       1.0)
    ev = _gaussfit.numpy_evaluator(model, data[None, :], errs[None, :])
    fit_tau = bool(G[name + "__fit_tau"])
    r = pplib.fit_gaussian_profile(data, init, errs, None, fit_tau,
                                   evaluator=ev)
    vary = np.ones(len(init), dtype=bool)
    vary[1] = fit_tau
    check_case(name, r.fitted_params, r.fit_errs, r.chi2, r.dof, vary)
    # a given fit_flags has no tau entry (pplib.py:1948-1953): DC fixed here
    flags = np.ones(len(init) - 1)
    flags[0] = 0
    r2 = pplib.fit_gaussian_profile(data, init, errs, flags, fit_tau,
                                    evaluator=ev)
    assert r2.fitted_params[0] == init[0] and r2.fit_errs[0] == 0.0
    assert r2.dof == r.dof + 1 and r2.fitted_params[2] != init[2]


def test_bound_transforms_invert():
    rng = np.random.default_rng(3)
    lo = np.array([np.nan, 0.0, 0.0, np.nan, -2.0])
    hi = np.array([np.nan, np.nan, 0.25, 3.0, 5.0])
    for _ in range(200):
        p = np.array([rng.normal(), rng.uniform(0, 50), rng.uniform(0, 0.25),
                      3.0 - rng.uniform(0, 40), rng.uniform(-2, 5)])
        x = _gaussfit.to_internal(p, lo, hi)
        np.testing.assert_allclose(_gaussfit.to_external(x, lo, hi), p,
                                   rtol=1e-9, atol=1e-12)
    # any internal value lands inside the bounds
    x = rng.normal(size=(1000, 5)) * 100
    for row in x:
        p = _gaussfit.to_external(row, lo, hi)
        assert p[1] >= 0 and 0 <= p[2] <= 0.25 and p[3] <= 3 and -2 <= p[4] <= 5
    # the formulas of the issue: lower only and both bounds
    assert _gaussfit.to_external(np.array([2.0]), np.array([1.0]),
                                 np.array([np.nan]))[0] == 1.0 - 1 + np.sqrt(5.0)
    assert _gaussfit.to_external(np.array([0.3]), np.array([0.0]),
                                 np.array([0.25]))[0] == \
        (np.sin(0.3) + 1) * 0.25 / 2
    lo_p, hi_p = _gaussfit.portrait_bounds(14)
    assert lo_p[1] == 0 and np.isnan(hi_p[1]) and np.isnan(lo_p[[0, 2, 3, 5, 7, 14]]).all()
    assert (lo_p[[4, 10]] == 0).all() and (hi_p[[4, 10]] == pplib.wid_max).all()
    assert (lo_p[[6, 12]] == 0).all() and np.isnan(hi_p[[6, 12]]).all()


def test_nonfinite_trial_is_rejected():
    """A trial point with a non-finite chi^2 counts as an uphill step."""
    calls = []

    def ev(p, fi, d):
        calls.append(p[0])
        if p[0] < 0:                       # a power law of a negative value
            return np.full((len(fi) + 1,) * 2, np.nan)
        r = np.array([np.sqrt(p[0]) - 0.5, 0.1 * (p[0] - 0.25)])
        J = np.array([[-(np.sqrt(p[0] + dd) - np.sqrt(p[0])) / dd,
                       -0.1] for dd in d])
        C = np.vstack([J.reshape(len(fi), 2), r])
        return C @ C.T
    p, perr, chi2, dof, res = _gaussfit.levenberg_marquardt(
        ev, [9.0], [True], [np.nan], [np.nan], 2)
    assert min(calls) < 0                  # the first Gauss-Newton step overshoots
    assert res.success and abs(p[0] - 0.25) < 1e-6 and chi2 < 1e-12


def test_write_model_matches_reference_text(tmp_path):
    path = str(tmp_path / "m.gmodel")
    name, code = [str(s) for s in G["write__args"]]
    pplib.write_model(path, name, code, float(G["write__nu_ref"]),
                      G["write__params"], G["write__flags"],
                      float(G["write__alpha"]), 1, quiet=True)
    assert open(path).read() == str(G["write__text"])
    # round trip through read_model (8 decimals, ALPHA 3)
    back = pplib.read_model(path)
    assert back[:2] == (name, code) and back[3] == 3
    np.testing.assert_allclose(back[4], G["write__params"], atol=5.1e-9)
    np.testing.assert_array_equal(back[5], G["write__flags"])
    assert back[6] == -4.4 and back[7] == 1
    # append mode adds a second model after the first
    pplib.write_model(path, name, code, 1.0, G["write__params"],
                      G["write__flags"], -4.0, 0, append=True, quiet=True)
    assert open(path).read().startswith(str(G["write__text"]))
    assert open(path).read().count("MODEL") == 2


def test_join_params_raise():
    with pytest.raises(NotImplementedError):
        pplib.fit_gaussian_portrait("000", np.zeros((2, 32)), np.zeros(8),
                                    -4.0, np.ones((2, 32)), np.ones(8), False,
                                    np.zeros(32), [1.0, 2.0], 1.0,
                                    join_params=[[0], [0.0, 0.0], [1, 1]])


def test_ppgauss_refuses_what_is_outside_the_accelerated_path(tmp_path):
    from pulseportraiture_amd import ppgauss
    meta = tmp_path / "meta.txt"
    meta.write_text("a.fits\nb.fits\n")
    with pytest.raises(NotImplementedError):
        ppgauss.DataPortrait(str(meta))
    with pytest.raises(NotImplementedError):
        ppgauss.GaussianSelector(None, None, None)


def _call(lib, nfit=1, nchan=2, nbin=64, ngauss=1, code=b"000", nfree=2,
          free_idx=(0, 2), delta=(1e-8, 1e-8), dtype=None, ws=1 << 30):
    fi = np.array(free_idx, dtype=np.int32)
    dl = np.array(delta, dtype=np.float64)
    one = ctypes.c_void_p(8)       # never dereferenced: no context, no launch
    return lib.ppf_gauss_lsq_batch(
        None, nfit, nchan, nbin, ngauss, code, one, one, one, one, nfree,
        fi.ctypes.data, dl.ctypes.data,
        _lib.PPF_F64 if dtype is None else dtype, one, one, one, one, ws, None)


def test_gauss_lsq_validates_on_the_host():
    """The documented codes, before the context is looked at (no GPU)."""
    lib = _lib.load()
    wsb = lib.ppf_gauss_lsq_workspace_bytes
    assert wsb(1, 2, 64, 2) >= 2 * 3 * 64 * 8 + 2 * 256 * 8
    assert wsb(3, 7, 64, 16) >= 3 * 7 * 17 * 64 * 8 + 3 * 7 * 3 * 256 * 8
    assert wsb(1, 1, 32, 0) > 0 and wsb(1, 1, 8192, 127) > 0
    for nbin in (30, 33, 1001, 8194, 16384):
        assert wsb(1, 2, nbin, 2) == 0, nbin
        assert _call(lib, nbin=nbin) == _lib.PPF_EUNSUP, nbin
    assert wsb(1, 2, 64, 128) == 0
    assert _call(lib, nfree=128, free_idx=range(128),
                 delta=[1.0] * 128, ngauss=30) == _lib.PPF_EUNSUP
    assert _call(lib, code=b"0x0") == _lib.PPF_EINVAL
    assert _call(lib, free_idx=(2, 2)) == _lib.PPF_EINVAL      # not increasing
    assert _call(lib, free_idx=(2, 0)) == _lib.PPF_EINVAL
    assert _call(lib, free_idx=(0, 9)) == _lib.PPF_EINVAL      # npar = 8
    assert _call(lib, free_idx=(-1, 3)) == _lib.PPF_EINVAL
    assert _call(lib, delta=(1e-8, 0.0)) == _lib.PPF_EINVAL
    assert _call(lib, delta=(np.nan, 1.0)) == _lib.PPF_EINVAL
    assert _call(lib, dtype=7) == _lib.PPF_EINVAL
    assert _call(lib, ws=wsb(1, 2, 64, 2) - 1) == _lib.PPF_EINVAL
    assert _call(lib, nchan=0) == _lib.PPF_EINVAL
    # the scattering index (entry npar) is a valid free index; a valid call
    # then stops at the NULL context
    assert _call(lib, free_idx=(1, 8)) == _lib.PPF_EINVAL
    from pulseportraiture_amd import engine
    with pytest.raises(KeyError):
        engine.gauss_lsq("0x0", np.zeros((1, 8)), [0.0], [[1.0]], [1.0], [0],
                         [[1e-8]], np.zeros((1, 1, 64)), np.ones((1, 1, 64)))


def test_plain_gauss_entry_points_pin_their_refusals():
    """ppf_gauss_portrait_batch and ppf_gauss_lsq_batch: the code and the
    ppf_last_error text of each refused call (gausshost.check).  The portrait
    call looks at the context first, the least-squares call last."""
    E, U, OK = _lib.PPF_EINVAL, _lib.PPF_EUNSUP, _lib.PPF_OK
    digit = "model_code '0x0': digit 1 must be '0' or '1'"
    span = "nbin=%d: even lengths in [32, 8192] (the LDS row transforms)"
    H.check("port", E, digit, code=b"0x0")
    H.check("port", E, "model_code is NULL", code=None)
    H.check("port", U, "nbin=31 unsupported", null_rc=E, nbin=31)
    # 8194 bins are long rows to the portrait builder: an empty batch is fine
    ctx = H.live_context()
    assert H.call("port", ctx, nrow=0, nbin=8194)[0] == (E if ctx is None else OK)
    H.check("lsq", E, digit, code=b"0x0")
    H.check("lsq", E, "model_code is NULL", code=None)
    for nbin in (31, 33, 8194):
        H.check("lsq", U, span % nbin, nbin=nbin)
    H.check("lsq", U, "nfree=128: at most 127 free parameters", nfree=128,
            free_idx=range(128), delta=[1.0] * 128, ngauss=30)
    H.check("lsq", E, "free_idx[1] = 2: strictly increasing in [0, 8]",
            free_idx=(2, 2))
    H.check("lsq", E, "delta[0][1] = 0: a finite non-zero step",
            delta=(1e-8, 0.0))
