"""Host: _swt.fmin_1d against scipy.optimize.fmin, NumpyEvaluator.search
against scipy.optimize.brute, and pplib.smart_smooth(search="batched")
against the default path, all bit for bit (no GPU)."""
import numpy as np
import pytest
import scipy.optimize as opt

from pulseportraiture_amd import _swt, pplib

EV = _swt.NumpyEvaluator()
GRID = np.mgrid[slice(0.0, 3.0, 30j)]


def _x(x):
    return float(np.ravel(x)[0])


OBJECTIVES = {
    "quadratic": (lambda x: (_x(x) - 1.234) ** 2 - 7.0, 1.0344827586206897),
    "plateaus": (lambda x: np.floor(4.0 * abs(_x(x) - 0.61)) / 4.0, 2.0),
    "zero": (lambda x: 0.0, 1.5517241379310345),
    "from_zero": (lambda x: (_x(x) - 0.01) ** 2, 0.0),
    "capped": (lambda x: -_x(x), 0.10344827586206896),
}


@pytest.mark.parametrize("name", sorted(OBJECTIVES))
def test_fmin_1d_is_scipy_fmin(name):
    func, x0 = OBJECTIVES[name]
    x, fval, _, calls, flag = opt.fmin(func, x0, full_output=True, disp=False)
    got = _swt.fmin_1d(func, x0)
    assert got[0] == x[0] and got[1] == fval and got[2] == calls, \
        (got, x, fval, calls)
    assert np.float64(got[0]).tobytes() == x[:1].tobytes()
    assert np.float64(got[1]).tobytes() == np.float64(fval).tobytes()
    if name == "capped":
        assert calls == 200 and flag == 1
    else:
        assert calls < 200 and flag == 0


def _row(n, seed, noise):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return np.exp(-0.5 * ((i - 0.37 * n) / (0.02 * n + 1.5)) ** 2) + \
        0.4 * np.exp(-0.5 * ((i - 0.6 * n) / (0.05 * n + 2.0)) ** 2) + \
        rng.normal(0, noise, n)


def brute_search(ev, h, nprof, nlevel, soft, rchi2_tol):
    """opt.brute per (profile, level) over ev.score -> fact_min, fun_min and
    the calls beyond the 30 grid points (the fmin finish's)."""
    fact = np.zeros((nprof, nlevel))
    fun = np.zeros((nprof, nlevel))
    nfev = np.zeros((nprof, nlevel), dtype=np.int32)
    for ip in range(nprof):
        for il in range(nlevel):
            calls = [0]

            def objective(x, ip=ip, lev=il + 1):
                calls[0] += 1
                return _swt.wavelet_snr(
                    ev.score(h, [(ip, lev, soft)], [_x(x)])[0][0], rchi2_tol)

            res = opt.brute(objective, ranges=[(0.0, 3.0)], Ns=30,
                            full_output=True)
            fact[ip, il], fun[ip, il] = res[0][0], res[1]
            nfev[ip, il] = calls[0] - 30
    return fact, fun, nfev


@pytest.mark.parametrize("soft", [0, 1])
@pytest.mark.parametrize("nbin", [32, 64, 96])
def test_numpy_search_is_brute(nbin, soft):
    nlevel = _swt.max_level(nbin)
    rows = np.array([_row(nbin, nbin + 1, 0.05), _row(nbin, nbin + 2, 0.5)])
    h = EV.analyse(rows, nlevel)
    want = brute_search(EV, h, len(rows), nlevel, soft, 0.1)
    got = EV.search(h, soft, 0.1, GRID)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        assert g.tobytes() == w.tobytes(), (g, w)


@pytest.mark.parametrize("threshtype", ["hard", "soft"])
def test_smart_smooth_batched_is_default(threshtype):
    n = 64
    rng = np.random.default_rng(5)
    port = np.array([_row(n, 1, 0.05), np.zeros(n), rng.normal(0, 1.0, n),
                     _row(n, 2, 1e-3), _row(n, 3, 0.3), _row(n, 4, 0.02)])
    want = pplib.smart_smooth(port, threshtype=threshtype, evaluator=EV)
    got = pplib.smart_smooth(port, threshtype=threshtype, evaluator=EV,
                             search="batched")
    assert np.array_equal(got, want)
    assert not got[1].any() and got[0].any() and got[3].any()
    # a single profile
    one = pplib.smart_smooth(port[0], threshtype=threshtype, evaluator=EV,
                             search="batched")
    assert one.shape == (n,) and np.array_equal(one, want[0])


def test_smart_smooth_search_keyword():
    port = np.array([_row(64, 1, 0.05)])
    with pytest.raises(ValueError):
        pplib.smart_smooth(port, evaluator=EV, search="simplex")
    # the early returns are the default path's
    assert pplib.smart_smooth(port, try_nlevels=0, search="batched") is port
    odd = np.ones((2, 33))
    assert np.array_equal(
        pplib.smart_smooth(odd, search="batched", evaluator=EV), odd)
    z = pplib.smart_smooth(np.zeros((2, 64)), search="batched", evaluator=EV)
    assert z.shape == (2, 64) and not z.any()
