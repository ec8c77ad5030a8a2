#!/usr/bin/env python
"""Golden vectors for the joined Gaussian model: several archives under one
evolving-Gaussian model, each with a phase and a DM offset of its own
(pplib.gen_gaussian_portrait(join_ichans=...) pplib.py:886-963, the join
parameters of fit_gaussian_portrait pplib.py:2073-2098, ppgauss.py:192-310).

The fit cases are solved as make_golden_gaussfit.py solves its own: its
solve_case (lmfit restated with SciPy, two solvers) on the REFERENCE's
gen_gaussian_portrait with join_ichans, in the reference's lmfit order
[params, join params, scattering index]; the join parameters are unbounded.
solve_case refuses a case whose solvers differ by more than 1e-3 sigma or
whose minimum sits on a bound.

Model portraits of the reference are stored with their inputs (cases of
tests/joincases.py): the 3 x 64 case that separates the correct fold of the
rotation into the scattering multiply from the naive one (the Nyquist bin),
and unscattered / scattered portraits at nbin 100 and 1536 with six
interleaved channels, two archives and one channel in none.

Before anything is written the host model of the tests
(oracle.gen_gaussian_portrait, then oracle.rotate_data per archive) is
checked against the reference's joined portrait to 1e-13 of its maximum, on
every stored portrait and at every fit case's truth.

The end-to-end data (ppgauss.DataPortrait on two archives) is built here and
its loop run with the package's own driver on the NumPy evaluator; a seed
with a pull above 3 is refused.

Usage:  python tests/golden/make_golden_gaussjoin.py
"""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_gaussfit as gf  # noqa: E402  (imports the reference)
import numpy as np  # noqa: E402
import joincases as J  # noqa: E402
import oracle as O  # noqa: E402

pplib = gf.pplib
mg = gf.mg


def ref_model(code, nbin, freqs, nu_ref, join_ichans, njoin, P):
    phases = pplib.get_bin_centers(nbin)

    def model(p):
        return pplib.gen_gaussian_portrait(code, p[:-1], p[-1], phases, freqs,
                                           nu_ref, join_ichans, P)
    return model


def host_model(code, p, njoin, nbin, freqs, nu_ref, join_ichans, P):
    return J.host_model(O.gen_gaussian_portrait, O.rotate_data, code, p,
                        njoin, nbin, freqs, nu_ref, join_ichans, P)


def cross_check(name, ref, host):
    d = np.abs(ref - host).max() / np.abs(ref).max()
    print("%s: host composition vs reference %.1e of max" % (name, d))
    if not d <= 1e-13:
        raise SystemExit("refused: the host model differs from the reference "
                         "by %.2e of its maximum (%s)" % (d, name))


def join_bounds(npar, njoin):
    def bounds_of(n):
        assert n == npar + 2 * njoin
        lo, hi = np.full(n + 1, np.nan), np.full(n + 1, np.nan)
        lo[1] = 0.0
        lo[4:npar:6], hi[4:npar:6] = 0.0, gf.WID_MAX
        lo[6:npar:6] = 0.0
        return lo, hi
    return bounds_of


def main():
    out = {}
    for name in J.FIT_CASES:
        c = J.fit_case(name)
        rng = np.random.default_rng(c["seed"])
        nchan = len(c["freqs"])
        model = ref_model(c["code"], c["nbin"], c["freqs"], J.NU_REF,
                          c["join_ichans"], c["njoin"], J.P)
        clean = model(c["truth"])
        cross_check(name, clean, host_model(
            c["code"], c["truth"], c["njoin"], c["nbin"], c["freqs"],
            J.NU_REF, c["join_ichans"], J.P))
        data = clean + J.NOISE * rng.standard_normal((nchan, c["nbin"]))
        errs = np.full(data.shape, J.NOISE)
        gf.bounds_of = join_bounds(c["npar"], c["njoin"])
        with contextlib.redirect_stdout(io.StringIO()):
            g = gf.solve_case(model, data, errs, c["start"].copy(), c["vary"])
        pull = (np.abs(g["solution"] - c["truth"])[c["vary"]] /
                g["sol_errs"][c["vary"]]).max()
        print("%s: spread %.1e sigma, chi2 %.1e, errs %.1e, largest pull %.2f"
              % (name, g["spread_sigma"], g["spread_chi2"], g["spread_errs"],
                 pull))
        out.update({name + "__" + k: np.asarray(v) for k, v in g.items()})
        out.update({name + "__data": data, name + "__errs": errs})
    for name in J.PORT_CASES:
        c = J.port_case(name)
        ref = ref_model(c["code"], c["nbin"], c["freqs"], J.NU_REF,
                        c["join_ichans"], c["njoin"], J.P)(c["p_ext"])
        cross_check(name, ref, host_model(
            c["code"], c["p_ext"], c["njoin"], c["nbin"], c["freqs"],
            J.NU_REF, c["join_ichans"], J.P))
        out[name + "__port"] = ref
    out.update(end_to_end())
    path = os.path.join(HERE, "gaussjoin.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def end_to_end(seed=11, nchan=8, nbin=256, noise=0.08, phi=0.004, dDM=3e-4):
    """Two archives of 8 x 256 from the example model (1100-1500 and
    1450-1900 MHz), the second rotated by (phi, dDM); the joined fit and the
    convergence check of ppgauss (ppgauss.py:247-341) on the CPU."""
    from pulseportraiture_amd import _gaussfit
    ex = pplib.read_model(mg.GMODEL, quiet=True)
    code, nu_ref, mtruth, alpha = ex[1], float(ex[2]), np.array(ex[4]), ex[6]
    f1 = np.linspace(1100.0, 1500.0, nchan)
    f2 = np.linspace(1450.0, 1900.0, nchan)
    P = mg.P0
    phases = pplib.get_bin_centers(nbin)
    rng = np.random.default_rng(seed)
    ports = []
    for f, (ph, dm) in zip((f1, f2), ((0.0, 0.0), (phi, dDM))):
        m = pplib.gen_gaussian_portrait(code, mtruth, alpha, phases, f, nu_ref)
        m = pplib.rotate_data(m, ph, dm, P, f, nu_ref)
        ports.append(m + noise * rng.standard_normal(m.shape))
    fall = np.concatenate([f1, f2])
    isort = np.argsort(fall)
    freqs, port = fall[isort], np.concatenate(ports)[isort]
    src = np.concatenate([np.zeros(nchan, int), np.ones(nchan, int)])[isort]
    join_ichans = [np.flatnonzero(src == a) for a in range(2)]
    flags = np.array(ex[5], dtype=float)
    flags[1] = 0                                     # tau stays 0
    jflags = np.array([0.0, 1.0, 1.0, 1.0])
    start = np.where(flags != 0, mtruth * 1.02, mtruth)
    jstart = np.array([0.0, 0.0, phi + 0.001, 0.0])
    npar = len(mtruth)
    truth = np.concatenate([mtruth, [0.0, 0.0, phi, dDM]])
    vary = np.concatenate([flags != 0, jflags != 0, [False]])
    lo, hi = _gaussfit.portrait_bounds(npar, 2)
    errs = np.full(port.shape, noise)
    model = ref_model(code, nbin, freqs, nu_ref, join_ichans, 2, P)
    ev = _gaussfit.numpy_evaluator(model, port, errs)
    p, perr, chi2, dof, res = _gaussfit.levenberg_marquardt(
        ev, np.concatenate([start, jstart, [alpha]]), vary, lo, hi, port.size)
    jp = p[npar:-1]
    mod = model(p)
    dport, dmod = np.zeros(port.shape), np.zeros(port.shape)
    for a, ic in enumerate(join_ichans):
        dport[ic] = pplib.rotate_data(port[ic], -jp[2 * a], -jp[2 * a + 1], P,
                                      freqs[ic], nu_ref)
        dmod[ic] = pplib.rotate_data(mod[ic], -jp[2 * a], -jp[2 * a + 1], P,
                                     freqs[ic], nu_ref)
    nu_fit = pplib.guess_fit_freq(freqs, np.ones(len(freqs)))
    pg = pplib.fit_phase_shift(dport.mean(axis=0), dmod.mean(axis=0)).phase % 1
    pg = pg - 1.0 if pg >= 0.5 else pg
    with contextlib.redirect_stdout(io.StringIO()):
        fp = pplib.fit_portrait(dport, dmod, np.array([pg, 0.0]), P, freqs,
                                nu_fit, None, None,
                                bounds=[(None, None), (None, None)], id=None,
                                quiet=True)
    done = min(abs(fp.phase), abs(1 - fp.phase)) < abs(fp.phase_err) and \
        abs(fp.DM) < abs(fp.DM_err)
    print("e2e: phase %.2e +/- %.2e, DM %.2e +/- %.2e, chi2/dof %.3f, nfev %d"
          % (fp.phase, fp.phase_err, fp.DM, fp.DM_err, chi2 / dof, res.nfev))
    if not done:
        raise SystemExit("refused: the end-to-end fit did not converge")
    pull = (np.abs(p[:-1] - truth)[vary[:-1]] / perr[:-1][vary[:-1]])
    print("e2e largest pull %.2f" % pull.max())
    if pull.max() > 3:
        raise SystemExit("refused: seed %d has a pull of %.2f" % (seed,
                                                                  pull.max()))
    return {"e2e__ports": np.array(ports), "e2e__freqs": np.array([f1, f2]),
            "e2e__P": np.float64(P), "e2e__noise": np.float64(noise),
            "e2e__truth": truth, "e2e__start": start, "e2e__flags": flags,
            "e2e__code": np.array(code), "e2e__nu_ref": np.float64(nu_ref),
            "e2e__alpha": np.float64(alpha),
            "e2e__cpu_pull": np.float64(pull.max())}


if __name__ == "__main__":
    main()
