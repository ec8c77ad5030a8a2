#!/usr/bin/env python
"""Golden vectors for the PCA + B-spline model maker (ppspline.py:39-244) and
the wavelet search under it (pplib.smart_smooth 1740-1811, wavelet_smooth
1692-1737, fit_wavelet_smooth_function 1814-1838, find_significant_eigvec
1625-1689, pca 1564-1602, normalize_portrait 2553-2598).

PyWavelets is not installed next to the reference.  The reference's own
functions run here (build container only) on refshim/pywt.py, a NumPy
stand-in for pywt.swt / iswt / threshold written from the definition of the
transform; that the stand-in agrees with the real PyWavelets is unverified,
and so is everything downstream of it in splinefit.npz.

make_spline_model is called unbound on a plain namespace carrying the
attributes it reads (portx, SNRsxs, noise_stdsxs, freqsxs, freqs, bw, masks,
datafile, source).  The portraits are the example.gmodel portrait over
1100-1900 MHz in 32 channels plus seeded white noise, channels 3 and 17
removed from the condensed arrays.

Every profile the reference smooths (the mean profile and the ten leading
eigenvectors of each case) is also searched here with the reference's
fit_wavelet_smooth_function under the same scipy.optimize.brute call, which
must reproduce the reference's row bit for bit and exposes what a parity
test needs to know.  A case is refused when, for any of its profiles,
  - the final |red_chi2 - 1| is within 1e-6 of rchi2_tol,
  - the two best levels' (non-zero) objective values differ by less than
    1e-6 relative -- for the mean profile and the selected eigenvectors,
    whose rows enter the model.  Noise-like eigenvectors do tie, exactly
    (deep levels that zero the same coefficients), so for a rejected
    eigenvector the rule is instead that the row of EVERY level within 1e-6
    of the best is rejected by find_significant_eigvec's test too, with its
    S/N further than 1e-6 relative from the cutoffs: whichever level an
    implementation picks, the eigenvector stays out,
  - a coefficient lies within 1e-9 relative of the chosen threshold:
parity is only defined away from those discontinuities.

For the mean profile and eigenvectors 0-2 of the 256-bin cases the chosen
(level, factor, row) and the 30-point grid of (signal, noise, red_chi2) per
level are stored.

Usage:  python tests/golden/make_golden_spline.py
"""
import contextlib
import io
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference with the shims)
import numpy as np  # noqa: E402
import scipy.optimize as opt  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import ppspline as ref_ppspline  # noqa: E402
import pywt  # noqa: E402  (the stand-in)

pplib = mg.pplib
NS = 30
RCHI2_TOL = 0.1

CASES = [
    dict(name="b256", nbin=256, noise=0.4, seed=11, kw=dict(smooth=True)),
    dict(name="b256_raw", nbin=256, noise=0.4, seed=11, inputs_of="b256",
         kw=dict(smooth=False)),
    dict(name="b256_desc", nbin=256, noise=0.4, seed=11, descending=True,
         inputs_of="b256", kw=dict(smooth=True)),
    dict(name="b256_nbreak", nbin=256, noise=0.4, seed=11, inputs_of="b256",
         kw=dict(smooth=True, max_nbreak=2)),
    dict(name="b256_hi", nbin=256, noise=0.05, seed=13,
         kw=dict(smooth=True, snr_cutoff=50.0)),
    dict(name="b250", nbin=250, noise=0.4, seed=13, kw=dict(smooth=True)),
    dict(name="b255_raw", nbin=255, noise=0.4, seed=14,
         kw=dict(smooth=False)),
]
EXPECT_NCOMP = dict(b256=1, b256_raw=1, b256_desc=1, b256_nbreak=1, b256_hi=3,
                    b250=1, b255_raw=0)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def make_inputs(c):
    nchan, nbin = 32, c["nbin"]
    freqs = mg.channel_freqs(nchan, 1100.0, 800.0)
    phases = pplib.get_bin_centers(nbin)
    _, _, model = quiet(pplib.read_model, mg.GMODEL, phases, freqs, mg.P0,
                        quiet=True)
    rng = np.random.default_rng(c["seed"])
    port = model + rng.normal(0.0, c["noise"], model.shape)
    bw = 800.0
    if c.get("descending"):
        freqs, port, bw = freqs[::-1].copy(), port[::-1].copy(), -800.0
    ok = np.array([i for i in range(nchan) if i not in (3, 17)])
    noise_stds = pplib.get_noise(port, chans=True)
    SNRs = np.array([pplib.get_SNR(p) for p in port])
    masks = np.zeros((1, 1, nchan, nbin))
    masks[0, 0, ok] = 1.0
    return dict(port=port, freqs=freqs, ok=ok, bw=bw, noise_stds=noise_stds,
                SNRs=SNRs, masks=masks)


def search(prof, rchi2_tol=RCHI2_TOL, threshtype="hard"):
    """The reference's smart_smooth for one even-length profile, restated
    around its own fit_wavelet_smooth_function so that the chosen level and
    factor, the per-level objective values and the grids can be stored."""
    nbin = len(prof)
    nlev = int(np.log2(nbin)) if np.modf(np.log2(nbin))[0] == 0.0 else 1
    fun_vals, fact_mins = np.zeros(nlev), np.zeros(nlev)
    grids = np.zeros((nlev, NS, 3))
    facts = np.mgrid[slice(0.0, 3.0, complex(NS))]
    for il in range(nlev):
        args = (prof, "db8", il + 1, threshtype, rchi2_tol)
        res = opt.brute(pplib.fit_wavelet_smooth_function,
                        ranges=[(0.0, 3.0)], args=args, Ns=NS,
                        full_output=True)
        fact_mins[il], fun_vals[il] = res[0][0], res[1]
        for ig, f in enumerate(facts):
            s = pplib.wavelet_smooth(prof, nlevel=il + 1,
                                     threshtype=threshtype, fact=f)
            grids[il, ig] = (np.sum(np.abs(np.fft.rfft(s)[1:]) ** 2),
                             pplib.get_noise(s) * np.sqrt(nbin / 2.0),
                             pplib.get_red_chi2(prof, s))
    lev = int(fun_vals.argmin()) + 1
    fact = fact_mins[lev - 1]
    row = pplib.wavelet_smooth(prof, nlevel=lev, threshtype=threshtype,
                               fact=fact)
    red_chi2 = pplib.get_red_chi2(prof, row)
    # the distance of every coefficient from the threshold
    co = np.array(pywt.swt(prof, "db8", level=lev))
    lam = fact * (np.median(np.abs(co[0])) / 0.6745) * \
        np.sqrt(2 * np.log(nbin))
    used = np.concatenate([co[0, 0]] + [co[m, 1] for m in range(lev)])
    margin = np.min(np.abs(np.abs(used) - lam)) / lam if lam > 0 else np.inf
    if abs(red_chi2 - 1.0) > rchi2_tol:
        row = row * 0.0
    order = np.sort(fun_vals)
    tie = np.inf
    if len(order) > 1 and order[0] != 0.0:
        tie = abs(order[1] - order[0]) / abs(order[0])
    return dict(level=lev, fact=fact, row=row, red_chi2=red_chi2,
                fun_vals=fun_vals, fact_mins=fact_mins, grids=grids,
                margin=margin, tie=tie)


def significant(raw, row, snr_cutoff):
    """find_significant_eigvec's decision for one smoothed eigenvector
    (pplib.py:1657-1678, default checks) and the relative distance of its
    S/N from the two cutoffs."""
    noise = pplib.get_noise(raw) * np.sqrt(len(row) / 2.0)
    snr = np.sum(np.abs(np.fft.rfft(row)[1:]) ** 2) / noise
    margin = min(abs(snr / snr_cutoff - 1.0), abs(snr / (3 * snr_cutoff) - 1.0))
    if not snr >= snr_cutoff:
        return False, margin
    if snr < 3 * snr_cutoff:
        ncross = pplib.count_crossings(abs(row), 0.1 * abs(row).max())
        return bool(ncross < int(0.02 * len(row))), margin
    return True, margin


def vet(name, what, prof, ref_row, keep, rejected_at=None):
    """Search prof as the reference does; refuse near a discontinuity.
    rejected_at: the S/N cutoff of a rejected eigenvector (see the module
    docstring), None for a profile whose row enters the model."""
    s = search(prof)
    if rejected_at is not None:
        best = s["fun_vals"].min()
        for il, (fv, fm) in enumerate(zip(s["fun_vals"], s["fact_mins"])):
            if best != 0.0 and abs(fv - best) > 1e-6 * abs(best):
                continue
            row = pplib.wavelet_smooth(prof, nlevel=il + 1, fact=fm)
            if abs(pplib.get_red_chi2(prof, row) - 1.0) > RCHI2_TOL:
                row = row * 0.0
            sig, margin = significant(prof, row, rejected_at)
            if sig or margin < 1e-6:
                raise SystemExit("%s %s: rejected by the reference, but "
                                 "level %d's row is not clearly so" %
                                 (name, what, il + 1))
        s["tie"] = np.inf
    if ref_row is not None and not np.array_equal(s["row"], ref_row):
        raise SystemExit("%s %s: the restated search does not reproduce the "
                         "reference's smart_smooth" % (name, what))
    if abs(abs(s["red_chi2"] - 1.0) - RCHI2_TOL) < 1e-6:
        raise SystemExit("%s %s: final red_chi2 on the gate" % (name, what))
    if s["tie"] < 1e-6:
        raise SystemExit("%s %s: two levels tie" % (name, what))
    if s["margin"] < 1e-9:
        raise SystemExit("%s %s: a coefficient on the threshold" %
                         (name, what))
    if keep:
        s["prof"] = prof
        return {"%s_%s_%s" % (name, what, k): np.asarray(s[k]) for k in
                ("prof", "level", "fact", "row", "red_chi2", "fun_vals",
                 "fact_mins", "grids")}
    return {}


def run_case(c):
    name = c["name"]
    inp = make_inputs(c)
    ok = inp["ok"]
    ns = types.SimpleNamespace(
        portx=inp["port"][ok], SNRsxs=inp["SNRs"][ok],
        noise_stdsxs=inp["noise_stds"][ok], freqsxs=[inp["freqs"][ok]],
        freqs=inp["freqs"][None, :], bw=inp["bw"], masks=inp["masks"],
        datafile="golden_%s.fits" % name, source="J0000+0000")
    quiet(ref_ppspline.DataPortrait.make_spline_model, ns, quiet=True,
          **c["kw"])
    if c["kw"].get("smooth") and not ns.smooth_mean_prof.any():
        raise SystemExit("%s: the mean profile fails the chi^2 gate" % name)
    if ns.ncomp != EXPECT_NCOMP[name]:
        raise SystemExit("%s: ncomp %d, expected %d" %
                         (name, ns.ncomp, EXPECT_NCOMP[name]))
    out = {}
    # inputs are stored once per (nbin, noise, seed); the descending case
    # reads them reversed (in_flip)
    out[name + "_in_from"] = np.array(c.get("inputs_of", name))
    out[name + "_in_flip"] = np.array(bool(c.get("descending")))
    if "inputs_of" not in c:
        for k in ("port", "freqs", "ok", "bw", "noise_stds", "SNRs"):
            out["%s_in_%s" % (name, k)] = np.asarray(inp[k])
    smooth = bool(c["kw"].get("smooth"))
    out[name + "_smooth"] = np.array(smooth)
    out[name + "_kw"] = np.array(json.dumps(c["kw"]))
    out[name + "_ieig"] = np.asarray(ns.ieig, dtype=np.int64)
    out[name + "_eigval"] = ns.eigval[:10]
    out[name + "_mean_prof"] = ns.mean_prof
    ie = np.asarray(ns.ieig, dtype=np.int64)
    out[name + "_eigvec_sel"] = ns.eigvec[:, ie]
    if smooth:
        out[name + "_smooth_mean_prof"] = ns.smooth_mean_prof
        out[name + "_smooth_eigvec_sel"] = ns.smooth_eigvec[:, ie]
    out[name + "_proj_port"] = np.asarray(ns.proj_port)
    out[name + "_tck_t"] = np.asarray(ns.tck[0])
    out[name + "_tck_c"] = np.asarray(ns.tck[1])
    out[name + "_tck_k"] = np.array(ns.tck[2])
    out[name + "_ier"] = np.array(-99 if ns.ier is None else ns.ier)
    out[name + "_model"] = ns.model
    # modelx is the model at the condensed frequencies: when it equals the
    # rows of model bit for bit only the row indices are stored
    if np.array_equal(ns.modelx, ns.model[ok]):
        out[name + "_modelx_rows"] = ok
    else:
        out[name + "_modelx"] = ns.modelx
    # every profile the reference searched, vetted; a few kept
    nbin = c["nbin"]
    if nbin % 2 == 0:
        keep = nbin == 256 and name in ("b256", "b256_hi")
        if smooth:
            out.update(vet(name, "mean", ns.mean_prof, ns.smooth_mean_prof,
                           keep))
        for iv in range(10):
            ref_row = ns.smooth_eigvec[:, iv] if smooth and iv in ie else None
            cutoff = None if iv in ie else c["kw"].get("snr_cutoff", 150.0)
            out.update(vet(name, "ev%d" % iv, ns.eigvec[:, iv], ref_row,
                           keep and iv < 3, cutoff))
    print("%-12s ncomp %d ieig %s ier %s knots %d" %
          (name, ns.ncomp, list(ie), ns.ier, len(ns.tck[0])))
    return out


def run_normalize():
    """normalize_portrait, all five methods, on a small noisy portrait with
    one zeroed channel."""
    c = dict(nbin=64, noise=0.2, seed=21)
    inp = make_inputs(c)
    port = inp["port"][:8].copy()
    port[5] = 0.0
    out = {"norm_in_port": port}
    for method in ("mean", "max", "prof", "rms", "abs"):
        p, v = pplib.normalize_portrait(port, method, return_norms=True)
        out["norm_%s_port" % method], out["norm_%s_vals" % method] = p, v
    w = np.linspace(1.0, 2.0, len(port))
    out["norm_in_weights"] = w
    out["norm_profw_port"] = pplib.normalize_portrait(port, "prof", weights=w)
    return out


def main():
    out = {}
    for c in CASES:
        out.update(run_case(c))
    out.update(run_normalize())
    out["case_names"] = np.array([c["name"] for c in CASES])
    path = os.path.join(HERE, "splinefit.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.0f kB)" % (path, len(out),
                                             os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
