"""Time get_noise_fit on cuda:0 (no threshold): engine.noise_fit_rows
(k_noise_fit) and engine.noise_rows (get_noise_PS, the same bytes read) on
the same 512 x 2048 float32 rows, by HIP events around the calls.  One
warm-up call each (twiddles, tables), then `reps` calls; the median and the
min-max spread are printed and written to profiles/noise_fit.json, beside
the reference's seconds per row on the CPU (REFERENCE_S_PER_ROW, measured
once with the reference's get_noise_fit: scipy.optimize.brute's 8000 NumPy
evaluations per profile).
usage: python tools/noisefit_time.py [reps] [--no-write]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pulseportraiture_amd import engine  # noqa: E402

# the reference's get_noise_fit(chans=True) on one CPU core, seconds per row
# (0.11 at 100 bins to 0.20 at 2048 bins)
REFERENCE_S_PER_ROW = {"nbin_100": 0.11, "nbin_2048": 0.20}
NROWS, NBIN = 512, 2048


def rows(seed=1):
    """A Gaussian pulse (amplitude 20, FWHM 0.03 rot) in unit noise."""
    rng = np.random.default_rng(seed)
    x = (np.arange(NBIN) + 0.5) / NBIN
    sigma = 0.03 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    prof = 20.0 * np.exp(-0.5 * ((x - 0.5) / sigma) ** 2)
    return (prof + rng.standard_normal((NROWS, NBIN))).astype(np.float32)


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()),
                max=float(v.max()))


def time_ms(fn, reps):
    """Device milliseconds of fn(), reps times after one warm-up call."""
    out = []
    for r in range(reps + 1):
        beg = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        beg.record()
        fn()
        end.record()
        end.synchronize()
        if r:
            out.append(beg.elapsed_time(end))
    return stats(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    dev = engine.device()
    x = engine.to_dev(rows(), dev, torch.float32)
    fit = time_ms(lambda: engine.noise_fit_rows(x), reps)
    ps = time_ms(lambda: engine.noise_rows(x), reps)
    out = dict(shape=[NROWS, NBIN], dtype="float32", reps=reps,
               noise_fit_rows_ms=fit, noise_rows_ms=ps,
               fit_over_ps=fit["median"] / ps["median"],
               fit_us_per_row=1e3 * fit["median"] / NROWS,
               reference_s_per_row=REFERENCE_S_PER_ROW,
               device=torch.cuda.get_device_name(dev))
    print(json.dumps(out))
    if "--no-write" not in sys.argv:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "noise_fit.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
