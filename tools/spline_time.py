"""Time one ppspline.DataPortrait.make_spline_model(smooth=True) on cuda:0
(no threshold) at 30 x 256 and 512 x 2048, on the device evaluator and on the
NumPy evaluator (_swt.NumpyEvaluator; the model portraits are built on the
device either way).  Counted per run: the wall time, the share of pplib.pca
(host), the evaluator calls (batched and single) and the time inside them.
One warm-up run, then `reps` runs; the median and the min-max spread are
printed, and one JSON line at the end.
usage: python tools/spline_time.py [reps] [--no-cpu] [--small]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pulseportraiture_amd import _swt, engine, pplib, ppspline, synth  # noqa: E402


def archive(nchan, nbin, seed=1):
    rng = np.random.default_rng(seed)
    freqs = synth.channel_freqs(nchan)
    phases = pplib.get_bin_centers(nbin)
    model = pplib.gen_gaussian_portrait(
        "000", np.asarray(synth.GMODEL_PARAMS, dtype=float), -4.0, phases,
        freqs, synth.GMODEL_NU_REF)
    noise = 0.4
    port = model + noise * rng.standard_normal(model.shape)
    return pplib.DataBunch(
        subints=port[None, None], masks=np.ones((1, 1, nchan, nbin)),
        freqs=freqs[None], ok_ichans=[np.arange(nchan)],
        noise_stds=np.full((1, 1, nchan), noise),
        SNRs=(model.max(axis=1) / noise)[None, None], Ps=np.array([0.003]),
        phases=phases, nu0=freqs.mean(), bw=800.0, source="PSR_SYNTH",
        nbin=nbin, nchan=nchan, filename="synth")


class Counting(object):
    """An evaluator that counts and times the calls of another."""

    def __init__(self, inner):
        self.inner, self.batched, self.single, self.seconds = inner, 0, 0, 0.0

    def _timed(self, fn, *a, **k):
        t0 = time.perf_counter()
        out = fn(*a, **k)
        self.seconds += time.perf_counter() - t0
        return out

    def noise(self, rows):
        return self._timed(self.inner.noise, rows)

    def analyse(self, profs, nlevel, max_ncase=0):
        return self._timed(self.inner.analyse, profs, nlevel, max_ncase)

    def score(self, h, cases, facts, smooth=False):
        if len(cases) > 1:
            self.batched += 1
        else:
            self.single += 1
        return self._timed(self.inner.score, h, cases, facts, smooth)


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()),
                max=float(v.max()))


def run(data, make_evaluator, reps):
    wall, pca_s, ev_s = [], [], []
    real_pca = pplib.pca
    for r in range(reps + 1):
        ev = Counting(make_evaluator())
        spent = [0.0]

        def timed_pca(*a, **k):
            t0 = time.perf_counter()
            out = real_pca(*a, **k)
            spent[0] += time.perf_counter() - t0
            return out
        ppspline.pca = timed_pca
        try:
            dp = ppspline.DataPortrait(data)
            t0 = time.perf_counter()
            dp.make_spline_model(smooth=True, quiet=True, evaluator=ev)
            dt = time.perf_counter() - t0
        finally:
            ppspline.pca = real_pca
        if r:                                   # the first run warms up
            wall.append(dt * 1e3)
            pca_s.append(spent[0] * 1e3)
            ev_s.append(ev.seconds * 1e3)
    return dict(wall_ms=stats(wall), pca_ms=stats(pca_s),
                evaluator_ms=stats(ev_s), batched_calls=ev.batched,
                single_calls=ev.single, ncomp=int(dp.ncomp))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 3
    out = {}
    shapes = [(30, 256)] + ([] if "--small" in sys.argv else [(512, 2048)])
    for nchan, nbin in shapes:
        data = archive(nchan, nbin)
        key = "%dx%d" % (nchan, nbin)
        out[key] = run(data, engine.SwtEvaluator, reps)
        print(key, "device:", json.dumps(out[key]), flush=True)
        if "--no-cpu" not in sys.argv:
            out[key + "_numpy"] = run(data, _swt.NumpyEvaluator,
                                      1 if nbin > 256 else max(1, reps // 2))
            print(key, "numpy:", json.dumps(out[key + "_numpy"]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
