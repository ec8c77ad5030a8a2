#!/usr/bin/env python
"""Golden vectors of the likelihood evaluators (tests/golden/eval.npz) from the
REFERENCE: pptoaslib.fit_portrait_full_function / _deriv / _2deriv /
_2deriv_with_scales, its own Cdbp* / Sbp* per-channel terms, and the pplib
fit_portrait_function* / fit_phase_shift_function* families on the same
spectra.  Runs only where the reference is importable (see make_golden.py for
the import shims and the scattering_portrait_FT rebinding).

Inputs are rebuilt by the tests from tests/evalcases.py (a SHA-256 of each is
stored); only the reference's outputs, the absolute companions of every
harmonic sum (float32, rounded down: never a wider bar) and the propagated
scales of f, g and H are stored.  Per-channel terms are packed to their 27
distinct entries (evalcases.PACK).

Usage:  python tests/golden/make_golden_eval.py
"""
import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(HERE, "refshim"), REF, ROOT,
                os.path.join(ROOT, "tests")]
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    import pplib  # noqa: E402
    import pptoaslib as R  # noqa: E402

import evalcases as E  # noqa: E402


def _scattering_portrait_FT(taus, nbin, binshift=1.0):
    # NumPy>=2 stand-in for pplib.scattering_portrait_FT (see make_golden.py)
    nchan = len(taus)
    nharm = nbin // 2 + 1
    if not np.any(taus):
        return np.ones([nchan, nharm])
    out = np.zeros([nchan, nharm], dtype=np.complex128)
    for ichan in range(nchan):
        out[ichan] = pplib.scattering_profile_FT(taus[ichan], nbin, binshift)
    return out


for _mod in (pplib, R):
    _mod.scattering_portrait_FT = _scattering_portrait_FT


def ref_terms(theta, p, log10_tau, nharm):
    """C, S, dC, dS, d2C, d2S per channel from the reference's own functions,
    chained as fit_portrait_full_function_2deriv chains them."""
    phi, DM, GM, tau, alpha = theta
    if log10_tau:
        tau = 10 ** tau
    D, M, e, P, fr = p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]
    nu_DM, nu_GM, nu_tau = p["nus"]
    nbin = 2 * (nharm - 1)
    phis = R.phase_shifts(phi, DM, GM, fr, nu_DM, nu_GM, P, mod=False)
    dph = R.phase_shifts_deriv(fr, nu_DM, nu_GM, P)
    d2ph = R.phase_shifts_2deriv(fr, nu_GM, P)
    phsr = R.phasor(phis, nharm)
    taus = R.scattering_times(tau, alpha, fr, nu_tau)
    dt = R.scattering_times_deriv(tau, fr, nu_tau, log10_tau, taus)
    d2t = R.scattering_times_2deriv(tau, fr, nu_tau, log10_tau, taus, dt)
    B = R.scattering_portrait_FT(taus, nbin)
    dB = R.scattering_portrait_FT_deriv(taus, dt, B)
    d2B = R.scattering_portrait_FT_2deriv(taus, dt, d2t, B)
    adB = R.abs_scattering_portrait_FT_deriv(B, dB)
    ad2B = R.abs_scattering_portrait_FT_2deriv(B, dB, d2B)
    dCp = R.Cdbp_deriv_phase_shifts(D, M, B, phsr)
    d2Cp = R.Cdbp_2deriv_phase_shifts(D, M, B, phsr)
    return dict(C=R.Cdbp(D, M, B, phsr, e), S=R.Sbp(B, M, e),
                dC=R.Cdbp_deriv(D, M, dB, phsr, dph, dCp, e),
                dS=R.Sbp_deriv(adB, M, e),
                d2C=R.Cdbp_2deriv(D, M, dB, d2B, phsr, dph, d2ph, dCp, d2Cp,
                                  e),
                d2S=R.Sbp_2deriv(ad2B, M, e))


def down32(x):
    """float32 not above x (x >= 0)."""
    y = np.asarray(x, dtype=np.float32)
    return np.where(y.astype(np.float64) > x, np.nextafter(y, np.float32(0)),
                    y).astype(np.float32)


def ref_point(theta, p, log10_tau, nharm, per_channel_H):
    a = (p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]) + tuple(p["nus"])
    out = {}
    fA, fB = np.array(E.FLAGS_A), np.array(E.FLAGS_B)
    out["f"] = R.fit_portrait_full_function(theta, *a, fA, log10_tau)
    out["g"] = R.fit_portrait_full_function_deriv(theta, *a, fA, log10_tau)
    out["gB"] = R.fit_portrait_full_function_deriv(theta, *a, fB, log10_tau)
    Hn, scl = R.fit_portrait_full_function_2deriv(
        theta, *a, fA, log10_tau, per_channel=True, return_scales=True)
    out["H"] = R.fit_portrait_full_function_2deriv(theta, *a, fA, log10_tau)
    out["HB"] = R.fit_portrait_full_function_2deriv(theta, *a, fB, log10_tau)
    out["scl"] = scl
    t = ref_terms(theta, p, log10_tau, nharm)
    h = E.companions(theta, p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"],
                     *p["nus"], log10_tau)
    tp, hp = E.pack_terms(t), E.pack_terms(h)
    assert np.all(np.abs(tp) <= hp * (1 + 1e-12) + 1e-300), "companion < term"
    out["terms"] = tp
    out["hat"] = down32(hp)
    sf, sg, sH = E.scales(t, h, E.FLAGS_A)
    out["sf"], out["sg"], out["sH"] = sf, sg, sH
    if per_channel_H:
        out["Hn"] = Hn
        out["sHn"] = down32(E.scales(t, h, E.FLAGS_A, per_channel=True)[2])
    out["ratioC"] = np.min(np.abs(t["C"]) / h["C"])
    return out


def ref_pplib(theta, p):
    """The pplib families at (phase, DM) = theta[:2] on the same spectra:
    p_n = sum |M|^2, nu_ref = nu_DM; the phase-shift functions on channel 0."""
    D, M, e, P, fr = p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]
    p_n = np.real(np.sum(M * np.conj(M), axis=1))
    nu = p["nus"][0]
    x = theta[:2]
    h2, nz = pplib.fit_portrait_function_2deriv(x, M, p_n, D, e, P, fr, nu)
    return dict(
        fp=pplib.fit_portrait_function(x, M, p_n, D, e, P, fr, nu),
        fp_noP=pplib.fit_portrait_function(x, M, p_n, D, e, None, None, nu),
        fp_d=pplib.fit_portrait_function_deriv(x, M, p_n, D, e, P, fr, nu),
        fp_2d=h2, fp_nz=nz,
        ps=pplib.fit_phase_shift_function(x[0], M[0], D[0], e[0]),
        ps_d=pplib.fit_phase_shift_function_deriv(x[0], M[0], D[0], e[0]),
        ps_2d=pplib.fit_phase_shift_function_2deriv(x[0], M[0], D[0], e[0]))


def sigmas(p, nharm):
    """Conditional 1-sigma of each parameter at the generating point
    (sqrt(2 / |H_ii|)), for the spread of the near points."""
    th = p["truth"].copy()
    th[3] = np.log10(th[3])
    H = R.fit_portrait_full_function_2deriv(
        th, p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"], *p["nus"],
        np.array(E.FLAGS_A), True)
    return np.sqrt(2.0 / np.abs(np.diag(H)))


def run_problem(out, name, p, nharm, seed, per_channel_H, nnear=3):
    out[name + "/sha"] = np.array(E.input_sha(p))
    log_pts, lin_pts = E.make_points(p["truth"], sigmas(p, nharm), seed)
    worst = np.inf
    for mode, pts, lt in (("log", log_pts, True), ("lin", lin_pts, False)):
        rs = [ref_point(th, p, lt, nharm, per_channel_H) for th in pts]
        out["%s/%s/theta" % (name, mode)] = pts
        for k in rs[0]:
            if k != "ratioC":
                out["%s/%s/%s" % (name, mode, k)] = np.array([r[k] for r in rs])
        near = rs[:nnear] if lt else rs[:1]
        worst = min([worst] + [r["ratioC"] for r in near])
    # the generator's conditions: every near point well inside |C| >= 0.1 C^
    assert worst >= 0.1, "%s: |C_n| / C^_n = %g at a near point" % (name, worst)
    for i, th in ((0, log_pts[0]), (4, log_pts[4])):
        for k, v in ref_pplib(th, p).items():
            out["%s/pplib%d/%s" % (name, i, k)] = np.asarray(v)
    return worst


def main():
    out, manifest = {}, {}
    for nchan, nharm in E.SHAPES:
        p = E.inputs(nchan, nharm)
        name = E.case_name(nchan, nharm)
        w = run_problem(out, name, p, nharm, 1000 * nchan + nharm,
                        (nchan, nharm) in E.PER_CHANNEL_H)
        manifest[name] = dict(nchan=nchan, nharm=nharm, min_C_over_Chat=w)
        if (nchan, nharm) == E.WITH_SCALES:
            a = (p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]) + \
                tuple(p["nus"])
            th = out[name + "/log/theta"][0]
            for tag, fl in (("A", E.FLAGS_A), ("B", E.FLAGS_B)):
                Hs, cov, scl = R.fit_portrait_full_function_2deriv_with_scales(
                    th, *a, np.array(fl), True, return_covariance_matrix=True,
                    return_scales=True)
                out["%s/ws%s/H" % (name, tag)] = Hs
                out["%s/ws%s/cov" % (name, tag)] = cov
                out["%s/ws%s/scl" % (name, tag)] = scl
                H2, cov2 = R.fit_portrait_full_function_2deriv(
                    th, *a, np.array(fl), True, return_covariance_matrix=True)
                out["%s/cov%s" % (name, tag)] = cov2
            out[name + "/wsA/Hn"] = \
                R.fit_portrait_full_function_2deriv_with_scales(
                    th, *a, np.array(E.FLAGS_A), True, per_channel=True)
    # the batched case: the reference sees each problem with its masked
    # channels deleted
    probs, _ = E.batch_inputs()
    for s, p in enumerate(probs):
        ok = np.array(E.BATCH["mask"][s], dtype=bool)
        q = dict(p)
        q.update(D=p["D"][ok], M=p["M"][ok], errs_FT=p["errs_FT"][ok],
                 freqs=p["freqs"][ok])
        out["batch%d/sha_full" % s] = np.array(E.input_sha(p))
        w = run_problem(out, "batch%d" % s, q, E.BATCH["nharm"], 7000 + s,
                        False)
        manifest["batch%d" % s] = dict(nchan=int(ok.sum()),
                                       nharm=E.BATCH["nharm"],
                                       min_C_over_Chat=w)
    for k, v in out.items():
        v = np.asarray(v)
        if v.dtype.kind in "fc":
            assert np.all(np.isfinite(v)), "non-finite golden value in " + k
    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < (1 << 20), "eval.npz is %d bytes" % size
    # a manifest of its own, as make_golden_full.py's MANIFEST_full.json
    with open(os.path.join(HERE, "MANIFEST_eval.json"), "w") as f:
        json.dump(dict(eval=dict(file="eval.npz", bytes=size, cases=manifest,
                                 numpy=np.__version__)), f, indent=1)
        f.write("\n")
    print("eval.npz: %d arrays, %d bytes; min |C| / C^ at near points %.4f" %
          (len(out), size, min(c["min_C_over_Chat"] for c in manifest.values())))


if __name__ == "__main__":
    main()
