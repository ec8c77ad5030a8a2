#!/usr/bin/env python
"""Golden vectors for make_fake_pulsar's noiseless rows and per-row tables
(pplib.py:3302-3499), add_DM_nu (2601-2638) and add_scintillation (1190-1218).

make_fake_pulsar itself needs PSRCHIVE, so its rows are composed here from
the REFERENCE's own functions (imported with the shims of make_golden.py;
this script runs in the build container only), per case with nsub = npol = 1
so that the reference's compounding `phase` (pplib.py:3464) does not enter:

    model = read_model(modelfile, phases, freqs, P)
    row_n = rotate_data(model[n], phi_n)                      per channel
    rows  = irfft(scattering_portrait_FT(scattering_times(t_scat / P, alpha,
            freqs, nu0), nbin) * rfft(rows))    if t_scat and the model's TAU = 0
    rows  = add_scintillation(rows, scint)                    if scint
    rows  = scales[:, None] * rows

with phi_n the rotation the archive's profile carries:
    xs None:  -phase - DM_delay(DM + dDM, freqs, nu0, P)
              (the reference's commented-out rotate_data(model, -phase,
              -(DM + dDM), P, freqs, nu0), pplib.py:3462)
    xs given: add_DM_nu(model, -phase', -dDM, P, freqs, xs, Cs, nu_DM)'s phase
              (pplib.py:2626-2636) with phase' = phase_transform(phase, DM +
              dDM, nu0, nu_DM, P), minus DM_delay(DM, freqs, nu0, P)
and P = 1 / (F0 + F1 * tsub / 2), the period at the centre of the first
sub-int of an archive that starts at PEPOCH.

Usage:  python tests/golden/make_golden_fake.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference with the shims)
import numpy as np  # noqa: E402

pplib = mg.pplib
PAR = os.path.join(HERE, "example.par")
TSUB = 300.0

CASES = {
    "plain": dict(modelfile="example.gmodel", nchan=8, nbin=64, phase=0.013,
                  dDM=3e-4),
    "tscat": dict(modelfile="example.gmodel", nchan=5, nbin=100, phase=-0.21,
                  dDM=1e-4, t_scat=4e-5, alpha=-4.4),
    "modeltau": dict(modelfile="scat.gmodel", nchan=4, nbin=64, phase=0.3,
                     dDM=-2e-4, t_scat=5e-5),
    "scint": dict(modelfile="example.gmodel", nchan=6, nbin=128, phase=0.05,
                  dDM=2e-4,
                  scint=[0.7, 1.3, 0.2, 0.4, 3.1, 0.6, 0.25, 0.5, 0.9],
                  scales=[1.0, 0.5, 0.0, 2.0, 1.5, 0.25]),
    "dmnu": dict(modelfile="example.gmodel", nchan=4, nbin=64, phase=0.02,
                 dDM=5e-4, xs=[-2.0, -4.0], Cs=[1.0], nu_DM=1400.0),
}
DEFAULTS = dict(nu0=1500.0, bw=800.0, t_scat=0.0, alpha=-4.0, scint=False,
                scales=1.0, xs=None, Cs=None, nu_DM=np.inf)


def read_par(path):
    par = {}
    for line in open(path):
        w = line.split()
        if len(w) > 1 and w[0] in ("F0", "F1", "PEPOCH", "DM"):
            par[w[0]] = np.float64(w[1].replace("D", "E"))
    return par


def compose(c, par):
    c = dict(DEFAULTS, **c)
    nchan, nbin, nu0, bw = c["nchan"], c["nbin"], c["nu0"], c["bw"]
    DM, dDM, phase = par["DM"], c["dDM"], c["phase"]
    P = 1.0 / (par["F0"] + par["F1"] * (TSUB / 2.0))
    cw = bw / nchan
    lofreq = nu0 - bw / 2
    freqs = np.linspace(lofreq + cw / 2.0, lofreq + bw - cw / 2.0, nchan)
    phases = pplib.get_bin_centers(nbin, lo=0.0, hi=1.0)
    modelfile = os.path.join(HERE, c["modelfile"])
    model_tau = pplib.read_model(modelfile, quiet=True)[4][1]
    model = pplib.read_model(modelfile, phases, freqs, P, quiet=True)[2]
    if c["xs"] is None:
        phi = -phase - pplib.DM_delay(DM + dDM, freqs, nu0, P)
    else:
        php = pplib.phase_transform(phase, DM + dDM, nu0, c["nu_DM"], P)
        D = pplib.Dconst * -dDM / P
        Cs, xs = c["Cs"], c["xs"]
        if not hasattr(Cs, "__iter__"):
            Cs = np.ones(len(xs))
        if len(Cs) < len(xs):
            Cs = list(Cs) + list(np.ones(len(xs) - len(Cs)))
        freq_term = 0.0
        for C, x in zip(Cs, xs):
            freq_term = freq_term + C * (freqs ** x - c["nu_DM"] ** x)
        phi = (-php + (D * freq_term)) - pplib.DM_delay(DM, freqs, nu0, P)
    rows = np.array([pplib.rotate_data(model[n], phi[n])
                     for n in range(nchan)])
    tau_n = np.zeros(nchan)
    if c["t_scat"] and not model_tau:
        tau_n = pplib.scattering_times(c["t_scat"] / P, c["alpha"], freqs, nu0)
        sp_FT = pplib.scattering_portrait_FT(tau_n, nbin)
        rows = np.fft.irfft(sp_FT * np.fft.rfft(rows, axis=-1), axis=-1)
    scales = c["scales"] * np.ones(nchan)
    gain = scales.copy()
    if c["scint"] is not False:
        rows = pplib.add_scintillation(rows, c["scint"])
        gain = scales * pplib.add_scintillation(np.ones((nchan, 1)),
                                                c["scint"])[:, 0]
    rows = scales[:, None] * rows
    out = dict(rows=rows, phi=phi, tau_n=tau_n, gain=gain, P=P, freqs=freqs,
               model_tau=model_tau, modelfile=c["modelfile"], nchan=nchan,
               nbin=nbin, nu0=nu0, bw=bw, phase=phase, dDM=dDM,
               t_scat=c["t_scat"], alpha=c["alpha"], scales=scales,
               nu_DM=c["nu_DM"], tsub=TSUB)
    if c["scint"] is not False:
        out["scint"] = np.asarray(c["scint"], dtype=float)
    if c["xs"] is not None:
        out["xs"] = np.asarray(c["xs"], dtype=float)
        out["Cs"] = np.asarray(c["Cs"], dtype=float)
    return out


def main():
    par = read_par(PAR)
    out = {"cases": np.array(sorted(CASES))}
    for name in sorted(CASES):
        for k, v in compose(CASES[name], par).items():
            out["%s__%s" % (name, k)] = v
    # add_DM_nu / add_scintillation on the plain case's 4 x 64 template
    nchan, nbin = 4, 64
    freqs = np.linspace(1200.0, 1800.0, nchan)
    P = 1.0 / par["F0"]
    port = pplib.read_model(os.path.join(HERE, "example.gmodel"),
                            pplib.get_bin_centers(nbin), freqs, P,
                            quiet=True)[2]
    out["fn__port"], out["fn__freqs"], out["fn__P"] = port, freqs, P
    out["fn__dmnu_args"] = np.array([0.0123, 2.5e-3, 1400.0])   # phase, DM, nu_ref
    out["fn__xs"], out["fn__Cs"] = np.array([-2.0, -4.0]), np.array([1.0])
    out["fn__dmnu"] = pplib.add_DM_nu(port, 0.0123, 2.5e-3, P, freqs,
                                      [-2.0, -4.0], [1.0], 1400.0)
    out["fn__dmnu_plain"] = pplib.add_DM_nu(port, phase=-0.31)
    out["fn__scint_params"] = np.array([0.7, 1.3, 0.2, 0.4, 3.1, 0.6])
    out["fn__scint"] = pplib.add_scintillation(port, list(out["fn__scint_params"]))
    np.savez_compressed(os.path.join(HERE, "fake.npz"), **out)
    print("wrote fake.npz:", ", ".join(sorted(CASES)))


if __name__ == "__main__":
    main()
