"""Host side of the joined Gaussian fit (no GPU): the package's LM driver on
a NumPy evaluator of the joined model against tests/golden/gaussjoin.npz at
the project's parity bar, the bounds of the joined parameter vector, the
metafile assembly of pplib.DataPortrait from DataBunches, the join file in
both formats, and the two new C symbols."""
import os
import re

import numpy as np
import pytest

import gausshost as H
import joincases as J
import oracle as O
from pulseportraiture_amd import _gaussfit, _lib, pplib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "gaussjoin.npz"))
SIGMA_TOL, CHI2_RTOL = 0.01, 1e-8


def _host(c):
    def model(p):
        return J.host_model(O.gen_gaussian_portrait, O.rotate_data, c["code"],
                            p, c["njoin"], c["nbin"], c["freqs"], J.NU_REF,
                            c["join_ichans"], J.P)
    return model


@pytest.mark.parametrize("name", sorted(J.FIT_CASES))
def test_lm_driver_reaches_joined_golden(name):
    c = J.fit_case(name)
    data, errs = G[name + "__data"], G[name + "__errs"]
    lo, hi = _gaussfit.portrait_bounds(c["npar"], c["njoin"])
    ev = _gaussfit.numpy_evaluator(_host(c), data, errs)
    p, perr, chi2, dof, res = _gaussfit.levenberg_marquardt(
        ev, c["start"], c["vary"], lo, hi, data.size)
    v = c["vary"]
    sol, serr = G[name + "__solution"], G[name + "__sol_errs"]
    dev = (np.abs(p - sol)[v] / serr[v]).max()
    rel = abs(chi2 / float(G[name + "__chi2"]) - 1)
    erel = np.abs(perr[v] / serr[v] - 1).max()
    print(name, "dev %.2e sigma, chi2 rel %.1e, errs rel %.1e, nfev %d" % (
        dev, rel, erel, res.nfev))
    assert res.success
    assert dev <= SIGMA_TOL
    assert rel <= CHI2_RTOL
    assert erel <= 2 * float(G[name + "__spread_errs"])
    assert dof == int(G[name + "__dof"])
    np.testing.assert_array_equal(p[~v], c["start"][~v])
    assert (perr[~v] == 0.0).all()


def test_portrait_bounds_with_joins():
    lo0, hi0 = _gaussfit.portrait_bounds(14)
    lo, hi = _gaussfit.portrait_bounds(14, 0)
    np.testing.assert_array_equal(lo, lo0)
    np.testing.assert_array_equal(hi, hi0)
    lo, hi = _gaussfit.portrait_bounds(14, 3)
    assert lo.shape == hi.shape == (14 + 6 + 1,)
    np.testing.assert_array_equal(lo[:14], lo0[:14])
    np.testing.assert_array_equal(hi[:14], hi0[:14])
    assert np.isnan(lo[14:]).all() and np.isnan(hi[14:]).all()
    # wid of the second component: the pattern must not run into the joins
    lo, hi = _gaussfit.portrait_bounds(8, 2)
    assert np.isnan(lo[8:]).all() and np.isnan(hi[8:]).all()


def test_join_symbols_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "ppfit.h")).read()
    for name in ("ppf_gauss_portrait_join_batch", "ppf_gauss_lsq_join_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        nargs = len(re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name,
                              text).group(1).split(","))
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)


# ------------------------------------------------- metafile assembly (host) --
def _bunch(name, freqs, nbin, zap=(), seed=0, bw=None, P=0.003):
    rng = np.random.default_rng(seed)
    nchan = len(freqs)
    sub = rng.normal(size=(1, 1, nchan, nbin)) + 5.0
    masks = np.ones((1, 1, nchan, nbin))
    masks[0, 0, list(zap)] = 0.0
    ok = np.array([i for i in range(nchan) if i not in zap])
    return pplib.DataBunch(
        subints=sub, masks=masks, freqs=np.asarray(freqs, dtype=float)[None],
        ok_ichans=[ok], noise_stds=rng.uniform(0.5, 1.5, (1, 1, nchan)),
        SNRs=rng.uniform(10, 100, (1, 1, nchan)), Ps=np.array([P]),
        phases=pplib.get_bin_centers(nbin), nu0=float(np.mean(freqs)),
        bw=float(bw if bw is not None else
                 (freqs[-1] - freqs[0]) * nchan / (nchan - 1)),
        source="PSR_JOIN", nbin=nbin, nchan=nchan, filename=name)


@pytest.fixture
def phase_shift(monkeypatch):
    """fit_phase_shift without the device: records its calls."""
    calls = []

    def fake(prof, refprof, noise=None, bounds=[-0.5, 0.5], Ns=100):
        calls.append((np.array(prof), np.array(refprof), Ns))
        return pplib.DataBunch(phase=0.01 * len(calls))
    monkeypatch.setattr(pplib, "fit_phase_shift", fake)
    return calls


def _three(nbin=64):
    # interleaved, unequal bands; no frequency appears twice
    fa = np.linspace(1100.0, 1500.0, 6)
    fb = np.linspace(1450.0, 1900.0, 5)
    fc = np.linspace(705.0, 1210.0, 4)
    return [_bunch("a.fits", fa, nbin, zap=(2,), seed=1, P=0.0030),
            _bunch("b.fits", fb, nbin, zap=(0, 4), seed=2, P=0.0032),
            _bunch("c.fits", fc, nbin, seed=3, P=0.0034)]


def test_metafile_assembly_from_databunches(phase_shift):
    bs = _three()
    dp = pplib.DataPortrait(bs)
    assert dp.njoin == 3 and dp.datafiles == ["a.fits", "b.fits", "c.fits"]
    assert dp.nbin == 64 and dp.nchan == 15 and dp.nchanx == 12
    assert dp.join_nchans == [0, 6, 11, 15]
    assert dp.join_nchanxs == [0, 5, 8, 12]
    fall = np.concatenate([b.freqs[0] for b in bs])
    src = np.repeat([0, 1, 2], [6, 5, 4])
    okall = np.concatenate([b.masks[0, 0].mean(axis=1) > 0 for b in bs])
    order = np.argsort(fall)
    np.testing.assert_array_equal(dp.isort, order)
    np.testing.assert_array_equal(dp.freqs, np.sort(fall)[None])
    np.testing.assert_array_equal(dp.freqsxs[0], np.sort(fall[okall]))
    assert (np.diff(dp.freqs[0]) > 0).all()
    # the indices from their definition: where each archive's channels land
    for a in range(3):
        want = np.flatnonzero(src[order] == a)
        np.testing.assert_array_equal(dp.join_ichans[a], want)
        np.testing.assert_array_equal(dp.freqs[0, want], bs[a].freqs[0])
        fx = fall[okall]
        wantx = np.flatnonzero(src[okall][np.argsort(fx)] == a)
        np.testing.assert_array_equal(dp.join_ichanxs[a], wantx)
        np.testing.assert_array_equal(
            dp.portx[wantx], bs[a].subints[0, 0][bs[a].ok_ichans[0]])
        np.testing.assert_array_equal(
            dp.port[want], bs[a].subints[0, 0] * bs[a].masks[0, 0])
        np.testing.assert_array_equal(
            dp.noise_stdsxs[wantx], bs[a].noise_stds[0, 0][bs[a].ok_ichans[0]])
        np.testing.assert_array_equal(
            dp.SNRs[0, 0][want], bs[a].SNRs[0, 0])
    # archives interleave: some archive's channels are not contiguous
    assert any(np.any(np.diff(ic) > 1) for ic in dp.join_ichans)
    assert dp.masks.shape == (1, 1, 15, 64)
    assert dp.noise_stds.shape == dp.SNRs.shape == (1, 1, 15)
    assert dp.weights.shape == (1, 15) and dp.weightsxs.shape == (1, 12)
    np.testing.assert_array_equal(dp.ok_ichans[0], np.flatnonzero(okall[order]))
    np.testing.assert_array_equal(dp.flux_prof, dp.port.mean(axis=1))
    np.testing.assert_array_equal(dp.flux_profx, dp.portx.mean(axis=1))
    assert dp.Ps == [pytest.approx((0.0030 + 0.0032 + 0.0034) / 3, rel=1e-15)]
    assert dp.nu0 == fall.mean()
    lo = min(b.freqs.min() - abs(b.bw) / (2 * b.nchan) for b in bs)
    hi = max(b.freqs.max() + abs(b.bw) / (2 * b.nchan) for b in bs)
    assert (dp.lofreq, dp.hifreq, dp.bw) == (lo, hi, hi - lo)
    # join parameters: first phase 0 and fixed, the others from the profiles
    np.testing.assert_array_equal(dp.join_params,
                                  [0.0, 0.0, -0.01, 0.0, -0.02, 0.0])
    np.testing.assert_array_equal(dp.join_fit_flags, [0, 1, 1, 1, 1, 1])
    assert len(phase_shift) == 2 and all(c[2] == 64 for c in phase_shift)
    ref = bs[0].subints[0, 0][bs[0].ok_ichans[0]].mean(axis=0)
    np.testing.assert_array_equal(phase_shift[0][1], ref)
    np.testing.assert_array_equal(
        phase_shift[1][0], bs[2].subints[0, 0].mean(axis=0))
    assert dp.all_join_params[0] is dp.join_ichanxs
    assert dp.all_join_params[1] is dp.join_params
    assert dp.all_join_params[2] is dp.join_fit_flags


def test_metafile_mismatched_nbin_raises(phase_shift):
    bs = _three()
    bs[1] = _bunch("b.fits", np.linspace(1450.0, 1900.0, 5), 128)
    with pytest.raises(ValueError):
        pplib.DataPortrait(bs)


def test_joinfile_both_formats_and_write_round_trip(tmp_path, phase_shift):
    old = tmp_path / "old.join"
    old.write_text("# header\nc.fits  0.25 -0.002\na.fits 0.0 0.001\n"
                   "b.fits -0.125 0.0005\n")
    dp = pplib.DataPortrait(_three(), joinfile=str(old))
    np.testing.assert_array_equal(
        dp.join_params, [0.0, 0.001, -0.125, 0.0005, 0.25, -0.002])
    new = tmp_path / "new.join"
    new.write_text("# header\n"
                   "a.fits   0.0000000000 0.0000000000   0.001000 0.000010\n"
                   "b.fits  -0.1250000000 0.0000100000   0.000500 0.000020\n"
                   "c.fits   0.2500000000 0.0000200000  -0.002000 0.000030\n")
    dp = pplib.DataPortrait(_three(), joinfile=str(new))
    np.testing.assert_array_equal(
        dp.join_params, [0.0, 0.001, -0.125, 0.0005, 0.25, -0.002])
    # what write_join_parameters appends is read back (10 / 6 decimals)
    out = tmp_path / "out.join"
    dp = pplib.DataPortrait(_three())
    dp.joinfile = str(out)
    dp.join_params = np.array([0.0, 3.25e-4, 0.0123456789012, -2.5e-4,
                               -0.25, 1e-3])
    dp.join_param_errs = np.array([0.0, 1e-5, 2e-5, 3e-5, 4e-5, 5e-5])
    dp.write_join_parameters()
    text = out.read_text()
    header = "# archive name" + " " * 32 + "-phase offset & err [rot]" + \
        "  " + "-delta-DM & err [cm**-3 pc]\n"
    assert text == header + \
        "a.fits" + " " * 39 + " 0.0000000000 0.0000000000   0.000325 0.000010\n" + \
        "b.fits" + " " * 39 + " 0.0123456789 0.0000200000  -0.000250 0.000030\n" + \
        "c.fits" + " " * 39 + "-0.2500000000 0.0000400000   0.001000 0.000050\n"
    back = pplib.DataPortrait(_three(), joinfile=str(out))
    np.testing.assert_allclose(back.join_params[0::2], dp.join_params[0::2],
                               rtol=0, atol=0.5e-10)
    np.testing.assert_allclose(back.join_params[1::2], dp.join_params[1::2],
                               rtol=0, atol=0.5e-6)
    # a second write appends; the reader takes the last njoin lines
    dp.join_params[2] = 0.5
    dp.write_join_parameters()
    assert out.read_text().startswith(text)
    back = pplib.DataPortrait(_three(), joinfile=str(out))
    assert back.join_params[2] == 0.5
    # a bad file leaves the start values
    bad = tmp_path / "bad.join"
    bad.write_text("x.fits 0 0\ny.fits 0 0\nz.fits 0 0\n")
    back = pplib.DataPortrait(_three(), joinfile=str(bad))
    np.testing.assert_array_equal(back.join_params[1::2], 0.0)


def test_apply_joinfile_then_undo_restores_the_data(phase_shift, monkeypatch):
    monkeypatch.setattr(pplib, "rotate_data", O.rotate_data)
    bs = _three()
    for b in bs:
        # no power in the Nyquist bin: a rotation by a fraction of a bin
        # keeps only that bin's real part, which no rotation back restores
        alt = (-1.0) ** np.arange(64)
        b.subints -= (b.subints * alt).mean(axis=-1, keepdims=True) * alt
    dp = pplib.DataPortrait(bs)
    dp.join_params = np.array([0.0, 2e-4, 0.013, -3e-4, -0.21, 5e-4])
    port, portx = dp.port.copy(), dp.portx.copy()
    dp.apply_joinfile(1400.0)
    for a in range(3):
        jic = dp.join_ichans[a]
        want = O.rotate_data(port[jic], -dp.join_params[2 * a],
                             -dp.join_params[2 * a + 1], dp.Ps[0],
                             dp.freqs[0, jic], 1400.0)
        np.testing.assert_array_equal(dp.port[jic], want)
    assert np.abs(dp.portx - portx).max() > 0.1
    dp.apply_joinfile(1400.0, undo=True)
    # two FFT round trips of O(10) data at nbin 64
    tol = 64 * np.finfo(float).eps * np.abs(port).max()
    assert np.abs(dp.port - port).max() <= tol
    assert np.abs(dp.portx - portx).max() <= tol


def test_metafile_of_missing_or_foreign_archives_is_refused(tmp_path):
    from pulseportraiture_amd import ppspline
    meta = tmp_path / "meta.txt"
    meta.write_text("%s\n" % (tmp_path / "nothing.fits"))
    with pytest.raises(NotImplementedError):
        pplib.DataPortrait(str(meta))
    with pytest.raises(NotImplementedError):       # ppspline joins: not built
        ppspline.DataPortrait(_three())


@pytest.mark.parametrize("entry", ["port_join", "lsq_join"])
def test_joined_gauss_entry_points_pin_their_refusals(entry):
    """The code and the ppf_last_error text of each refused call
    (gausshost.check), two archives joined unless said otherwise."""
    E, U = _lib.PPF_EINVAL, _lib.PPF_EUNSUP
    digit = "model_code '0x0': digit 1 must be '0' or '1'"
    H.check(entry, E, digit, code=b"0x0")
    H.check(entry, E, digit, code=b"0x0", njoin=0, join_id=(-1, -1))
    H.check(entry, E, "model_code is NULL", code=None)
    H.check(entry, E, "njoin=-1", njoin=-1)
    H.check(entry, E, "join_id[1] = 2: -1 or an archive in [0, 2)",
            join_id=(0, 2))
    for nbin in (31, 33, 8194):
        H.check(entry, U, "nbin=%d: even lengths in [32, 8192] (the LDS row "
                "transforms)" % nbin, nbin=nbin)
    if entry == "port_join":
        return
    H.check(entry, U, "nfree=128: at most 127 free parameters", nfree=128,
            free_idx=range(128), delta=[1.0] * 128, ngauss=30)
    # the scattering index is entry npar + 2 njoin = 12 of the free indices
    H.check(entry, E, "free_idx[1] = 2: strictly increasing in [0, 12]",
            free_idx=(2, 2))
    H.check(entry, E, "delta[0][1] = 0: a finite non-zero step",
            delta=(1e-8, 0.0))
