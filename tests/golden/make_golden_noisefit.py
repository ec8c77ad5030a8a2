#!/usr/bin/env python
"""Golden vectors for the fitted noise floor: the REFERENCE's get_noise_fit
(pplib.py:2341-2373) and find_kc (pplib.py:1530-1561), imported with the shims
of make_golden.py (this script runs in the build container only; SciPy is
there).

Per case the file holds the input rows, and per row the reference's
get_noise_fit, find_kc, pows, the flat index of the winner on
scipy.optimize.brute's 20 x 20 x 20 grid and the a grid brute walked.  The
grid and its chi-squared come from the same brute call find_kc makes, with
full_output=True; find_kc itself is run as well and must agree.

Parity of kc is only defined where the grid winner is no rounding accident:
for every row whose spectrum is finite the best chi-squared among the grid
points with ANOTHER a index must exceed the winner's by a relative GAP_MIN,
or the case is refused.  The gap is stored.

Cases
  pulse_<nbin>   three rows of a Gaussian pulse (amplitude 20, FWHM 0.03 rot)
                 in unit noise at nbin 64, 100, 256, 1001, 2048, as float64
                 and rounded to float32 ("__f32" keys)
  clamp_64       one such 64-bin row whose fact * kc reaches N: the
                 k_crit >= N branch (asserted here)
  edge_<nbin>    one row at 4095 and at 8192 bins, the longest odd and even
                 rows of the LDS transforms; stored as float32
  port_8x2048,   chans=False on whole portraits: one 16384-sample row (a
  port_9x1000    power-of-two long transform) and one 9000-sample row
                 (Bluestein); stored as float32
  half_tri       find_kc(fn="half_tri") with a scalar and a length-N errs
  zero, nan      an all-zero row and a row holding NaNs, in a batch with two
                 clean rows; whatever the reference returns is recorded

Usage:  python tests/golden/make_golden_noisefit.py
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference with the shims)
import numpy as np  # noqa: E402
import scipy.optimize as so  # noqa: E402

pplib = mg.pplib
GAP_MIN = 1e-6
FACT = 1.1


def pulse_rows(rng, nrows, nbin, amp=20.0, fwhm=0.03, noise=1.0):
    x = (np.arange(nbin) + 0.5) / nbin
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    prof = amp * np.exp(-0.5 * ((x - 0.5) / sigma) ** 2)
    return prof + noise * rng.standard_normal((nrows, nbin))


def pows_of(row):
    FFT = np.fft.rfft(row)
    return np.real(FFT * np.conj(FFT)) / len(row)


def brute_of(pows, errs=1.0, fn="exp_dc"):
    """find_kc's own brute call with the grid kept: (a grid, flat winner,
    relative gap to the best point of another a index)."""
    data = np.log10(pows)
    if fn == "exp_dc":
        ranges = [(len(data) ** -1, 1.0), (0, data.max() - data.min()),
                  (data.min(), data.max())]
    else:
        ranges = [(1, len(data)), (0, data.max() - data.min()),
                  (data.min(), data.max())]
    x0, fval, grid, J = so.brute(pplib.find_kc_function, ranges,
                                 args=(data, errs, fn), Ns=20,
                                 full_output=True, finish=None)
    win = int(np.argmin(J.ravel()))
    a_grid = grid[0][:, 0, 0].copy()
    if not np.all(np.isfinite(data)):
        return a_grid, win, np.nan
    others = np.delete(J, win // 400, axis=0)
    gap = others.min() / J.ravel()[win] - 1.0
    return a_grid, win, gap


def reference_row(row, errs=1.0, fn="exp_dc", degenerate=False):
    """Everything stored for one row."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        pows = pows_of(row)
        kc = pplib.find_kc(pows, errs, fn)
        a_grid, win, gap = brute_of(pows, errs, fn)
        noise = pplib.get_noise_fit(row, FACT) if fn == "exp_dc" else np.nan
    if not degenerate:
        if not gap > GAP_MIN:
            raise SystemExit("refused: the winner's margin is %.2e" % gap)
        # the winner's a decides kc: the two runs of brute agree
        ref_tab = kc_of(a_grid, len(pows), fn)
        assert ref_tab[win // 400] == kc, (ref_tab[win // 400], kc)
    return dict(pows=pows, kc=np.int64(kc), a_grid=a_grid,
                win=np.int64(win), gap=np.float64(gap),
                noise=np.float64(noise))


def kc_of(a_grid, N, fn):
    """The kc of each a (pplib.py:1553-1559)."""
    out = np.empty(len(a_grid), dtype=np.int64)
    for i, a in enumerate(a_grid):
        if fn == "exp_dc":
            try:
                out[i] = np.where(np.exp(-a * np.arange(N)) < 0.005)[0].min()
            except ValueError:
                out[i] = N - 1
        else:
            out[i] = int(np.floor(a))
    return out


def stack(recs):
    return {k: np.array([r[k] for r in recs]) for k in recs[0]}


def store(out, name, rows, recs, suffix=""):
    out[name + "__rows" + suffix] = rows
    s = stack(recs)
    for k, v in s.items():
        out[name + "__" + k + suffix] = v
    out[name + "__kc_table" + suffix] = kc_of(s["a_grid"][0], s["pows"].shape[1],
                                              "exp_dc")
    print("%s%s: kc %s of N %d, gaps %s" % (
        name, suffix, s["kc"], s["pows"].shape[1],
        np.array2string(s["gap"], precision=2)))


def main():
    out = {}
    rng = np.random.default_rng(20261)
    names = []
    for nbin in (64, 100, 256, 1001, 2048):
        name = "pulse_%d" % nbin
        rows = pulse_rows(rng, 3, nbin)
        store(out, name, rows, [reference_row(r) for r in rows])
        r32 = rows.astype(np.float32)
        store(out, name, r32, [reference_row(r.astype(np.float64))
                               for r in r32], "__f32")
        names.append(name)
    # the k_crit >= N branch (pplib.py:2360-2362)
    for seed in range(200):
        row = pulse_rows(np.random.default_rng(seed), 1, 64)[0]
        row = row.astype(np.float32).astype(np.float64)
        try:
            rec = reference_row(row)
        except SystemExit:
            continue
        if FACT * rec["kc"] >= len(rec["pows"]):
            break
    else:
        raise SystemExit("refused: no seed reaches the clamp")
    assert FACT * rec["kc"] >= len(rec["pows"])
    print("clamp_64: seed %d" % seed)
    store(out, "clamp_64", row[None, :].astype(np.float32), [rec])
    # the longest rows of the LDS transforms, odd and even (more than 48 KB
    # of LDS per workgroup)
    for nbin in (4095, 8192):
        r32 = pulse_rows(np.random.default_rng(nbin), 1, nbin)
        r32 = r32.astype(np.float32)
        store(out, "edge_%d" % nbin, r32,
              [reference_row(r32[0].astype(np.float64))])
    # chans=False on portraits: long rows
    for nchan, nbin in ((8, 2048), (9, 1000)):
        name = "port_%dx%d" % (nchan, nbin)
        port = pulse_rows(rng, nchan, nbin).astype(np.float32)
        rec = reference_row(port.astype(np.float64).ravel())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            whole = pplib.get_noise(port.astype(np.float64), method="fit",
                                    chans=False)
        assert whole == rec["noise"]
        store(out, name, port, [rec])
    # find_kc(fn="half_tri"), scalar and array errs
    row = out["pulse_256__rows"][0]
    N = 129
    errs_arr = 0.3 + 0.4 * np.arange(N) / N
    for key, errs in (("scalar", 0.5), ("array", errs_arr)):
        rec = reference_row(row, errs, "half_tri")
        out["half_tri__errs_" + key] = np.asarray(errs, dtype=np.float64)
        for k, v in rec.items():
            out["half_tri__%s_%s" % (k, key)] = v
        out["half_tri__kc_table_" + key] = kc_of(rec["a_grid"], N, "half_tri")
        print("half_tri %s: kc %d, gap %.2e" % (key, rec["kc"], rec["gap"]))
    # the same spectrum through exp_dc with the array errs
    rec = reference_row(row, errs_arr, "exp_dc")
    out["exp_dc__kc_array"] = rec["kc"]
    out["exp_dc__gap_array"] = rec["gap"]
    # degenerate rows beside clean ones
    rows = pulse_rows(rng, 4, 256)
    rows[1] = 0.0
    rows[2, 17] = np.nan
    rows[2, 200] = np.nan
    recs = [reference_row(r, degenerate=i in (1, 2))
            for i, r in enumerate(rows)]
    store(out, "degenerate", rows, recs)
    print("degenerate: noise %s" % out["degenerate__noise"])
    # the host one-liners (pplib.py:1450-1527) on the first 256-bin row
    prof, d = row, np.log10(pows_of(row))
    out["host__prof"] = prof
    out["host__half_tri_args"] = np.array([[7.6, 2.5, -1.0, 16],
                                           [16.0, 0.3, 4.0, 16],
                                           [1.2, 3.0, 0.5, 5]])
    for i, (a, b, dc, n) in enumerate(out["host__half_tri_args"]):
        out["host__half_tri_%d" % i] = pplib.half_triangle_function(a, b, dc,
                                                                    int(n))
    prm = np.array([[0.05, 2.0, -0.5], [0.9, 0.7, 0.1], [40.3, 3.0, -1.0]])
    out["host__chi2_params"] = prm
    out["host__chi2_exp_dc"] = np.array(
        [pplib.find_kc_function(p, d, 0.5, "exp_dc") for p in prm])
    out["host__chi2_half_tri"] = np.array(
        [pplib.find_kc_function(p, d, errs_arr, "half_tri") for p in prm])
    out["host__brickwall_12_5"] = pplib.brickwall_filter(12, 5)
    out["host__wiener"] = pplib.wiener_filter(prof, 1.3)
    out["host__fit_brickwall"] = np.int64(pplib.fit_brickwall(prof, 1.3))
    out["cases"] = np.array(names)
    out["fact"] = np.float64(FACT)
    out["gap_min"] = np.float64(GAP_MIN)
    path = os.path.join(HERE, "noisefit.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
