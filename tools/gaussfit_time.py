"""Time one pplib.fit_gaussian_portrait on cuda:0 (no threshold): the wall
time of the whole fit and, by HIP events around every ppf_gauss_lsq_batch
call, the device time of its evaluator, at
  64 x 512 with the example model (3 components), and
  512 x 2048 with 10 components;
the same Levenberg-Marquardt driver on the NumPy evaluator (the oracle's
portrait builder, forward differences, C @ C.T) at 64 x 512 for comparison.
One warm-up fit, then `reps` fits; the median and the min-max spread are
printed, and one JSON line at the end.
--join times instead the joined fit (fit_gaussian_portrait(join_params=...),
ppf_gauss_lsq_join_batch) at 64 x 512 with the example model, the band split
into two archives of 32 channels, the second offset by (0.004 rot, 3e-4
cm**-3 pc): the first archive's phase fixed, the other three join parameters
fitted from (0, 0.005, 0).
usage: python tools/gaussfit_time.py [reps] [--no-cpu] [--small] [--join]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pulseportraiture_amd import _gaussfit, engine, pplib, synth  # noqa: E402


def problem(nchan, nbin, ngauss, seed=1):
    """Truth, data (float64) and a start 2 % off for a fit of every
    parameter but tau."""
    rng = np.random.default_rng(seed)
    if ngauss == 3:
        truth = np.asarray(synth.GMODEL_PARAMS, dtype=float)
    else:
        truth = np.zeros(2 + 6 * ngauss)
        truth[0] = 0.01
        truth[2::6] = np.linspace(0.15, 0.85, ngauss)
        truth[3::6] = 0.002 * rng.normal(size=ngauss)
        truth[4::6] = rng.uniform(0.015, 0.04, ngauss)
        truth[5::6] = 0.3 * rng.normal(size=ngauss)
        truth[6::6] = rng.uniform(2.0, 8.0, ngauss)
        truth[7::6] = -1.0 + 0.5 * rng.normal(size=ngauss)
    freqs = synth.channel_freqs(nchan)
    phases = pplib.get_bin_centers(nbin)
    model = pplib.gen_gaussian_portrait("000", truth, -4.0, phases, freqs,
                                        synth.GMODEL_NU_REF)
    noise = 0.1
    data = model + noise * rng.standard_normal(model.shape)
    flags = np.ones(len(truth))
    flags[1] = 0
    start = np.where(flags != 0, truth * 1.02, truth)
    return dict(data=data, errs=np.full(model.shape, noise), start=start,
                flags=flags, freqs=freqs, phases=phases)


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()),
                max=float(v.max()))


def time_device(pb, reps):
    wall, kern, nfev, ncall = [], [], 0, 0
    for r in range(reps + 1):
        ev = engine.GaussLsqEvaluator("000", pb["data"], 1.0 / pb["errs"],
                                      pb["freqs"], synth.GMODEL_NU_REF,
                                      time_kernels=True)
        t0 = time.perf_counter()
        res = pplib.fit_gaussian_portrait(
            "000", pb["data"], pb["start"], -4.0, pb["errs"], pb["flags"],
            False, pb["phases"], pb["freqs"], synth.GMODEL_NU_REF,
            evaluator=ev)
        dt = time.perf_counter() - t0
        if r:                                   # the first fit warms up
            wall.append(dt * 1e3)
            kern.append(sum(ev.kernel_ms))
        nfev, ncall = res.lm_results.nfev, len(ev.kernel_ms)
        assert res.lm_results.success, res.lm_results.message
    return dict(wall_ms=stats(wall), evaluator_ms=stats(kern), nfev=nfev,
                calls=ncall, chi2_red=float(res.chi2 / res.dof))


JOIN_TRUTH = [0.0, 0.0, 0.004, 3e-4]


def time_device_join(reps, nchan=64, nbin=512, seed=1):
    rng = np.random.default_rng(seed)
    truth = np.asarray(synth.GMODEL_PARAMS, dtype=float)
    freqs = synth.channel_freqs(nchan)
    phases = pplib.get_bin_centers(nbin)
    ichans = [np.arange(nchan // 2), np.arange(nchan // 2, nchan)]
    P, nu_ref, noise = 0.003, synth.GMODEL_NU_REF, 0.1
    model = pplib.gen_gaussian_portrait("000", np.r_[truth, JOIN_TRUTH], -4.0,
                                        phases, freqs, nu_ref, ichans, P)
    data = model + noise * rng.standard_normal(model.shape)
    errs = np.full(model.shape, noise)
    flags = np.ones(len(truth))
    flags[1] = 0
    start = np.where(flags != 0, truth * 1.02, truth)
    join_id = pplib._join_ids(ichans, nchan)
    wall, kern = [], []
    for r in range(reps + 1):
        ev = engine.GaussLsqEvaluator("000", data, 1.0 / errs, freqs, nu_ref,
                                      time_kernels=True, join_id=join_id,
                                      P=P, njoin=2)
        t0 = time.perf_counter()
        res = pplib.fit_gaussian_portrait(
            "000", data, start, -4.0, errs, flags, False, phases, freqs,
            nu_ref, join_params=[ichans, [0.0, 0.0, 0.005, 0.0],
                                 [0, 1, 1, 1]], P=P, evaluator=ev)
        dt = time.perf_counter() - t0
        if r:
            wall.append(dt * 1e3)
            kern.append(sum(ev.kernel_ms))
        assert res.lm_results.success, res.lm_results.message
    return dict(wall_ms=stats(wall), evaluator_ms=stats(kern),
                nfev=res.lm_results.nfev, calls=len(ev.kernel_ms),
                chi2_red=float(res.chi2 / res.dof),
                join_params=[float(v) for v in res.fitted_params[-4:]])


def time_numpy(pb, reps):
    import oracle as O
    code, freqs, phases = "000", pb["freqs"], pb["phases"]

    def model(p):
        return O.gen_gaussian_portrait(code, p[:-1], p[-1], phases, freqs,
                                       synth.GMODEL_NU_REF)
    ev = _gaussfit.numpy_evaluator(model, pb["data"], pb["errs"])
    wall = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        res = pplib.fit_gaussian_portrait(
            code, pb["data"], pb["start"], -4.0, pb["errs"], pb["flags"],
            False, phases, freqs, synth.GMODEL_NU_REF, evaluator=ev)
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    return dict(wall_ms=stats(wall), nfev=res.lm_results.nfev)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 5
    out = {}
    if "--join" in sys.argv:
        out["64x512_g3_join2"] = time_device_join(reps)
        print(json.dumps(out))
        return
    shapes = [(64, 512, 3)] + ([] if "--small" in sys.argv else [(512, 2048, 10)])
    for nchan, nbin, ngauss in shapes:
        pb = problem(nchan, nbin, ngauss)
        key = "%dx%d_g%d" % (nchan, nbin, ngauss)
        out[key] = time_device(pb, reps)
        print(key, "device:", json.dumps(out[key]), flush=True)
        if (nchan, nbin) == (64, 512) and "--no-cpu" not in sys.argv:
            out[key + "_numpy"] = time_numpy(pb, max(1, reps // 2))
            print(key, "numpy:", json.dumps(out[key + "_numpy"]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
