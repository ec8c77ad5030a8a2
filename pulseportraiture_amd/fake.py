"""Host side of pplib.make_fake_pulsar (pplib.py:3302-3499): the ephemeris,
the epochs and periods, and the per-row tables (rotation, scattering time,
gain, noise) that engine.fake_subints turns into profiles on the device.
Nothing here needs a GPU.
"""
import numpy as np

from . import pplib


def read_par(ephemeris):
    """The reference's plain-text ephemeris parser (pplib.py:3397-3415): PSR
    or PSRJ, RAJ, DECJ, F0 or P0, PEPOCH, DM; F1 as well when present
    (default 0).  Fortran 'D' exponents are accepted; every other line,
    'C'-commented and blank ones included, is ignored.

    The reference's test `param[0] == ("PSR" or "PSRJ")` matches only PSR;
    both keys are accepted here.  Returns a DataBunch (PSR, RAJ, DECJ, F0,
    F1, P0, PEPOCH, DM); a missing key raises KeyError."""
    def num(s):
        return np.float64(s.replace("D", "E").replace("d", "e"))
    par = {"F1": np.float64(0.0)}
    with open(ephemeris, "r") as fh:
        for line in fh:
            w = line.split()
            if len(w) < 2:
                continue
            key = w[0]
            if key in ("PSR", "PSRJ"):
                par["PSR"] = w[1]
            elif key in ("RAJ", "DECJ"):
                par[key] = w[1]
            elif key == "F0":
                par["F0"] = num(w[1])
                par["P0"] = par["F0"] ** -1
            elif key == "P0":
                par["P0"] = num(w[1])
                par["F0"] = par["P0"] ** -1
            elif key in ("F1", "PEPOCH", "DM"):
                par[key] = num(w[1])
    for key in ("PSR", "RAJ", "DECJ", "P0", "PEPOCH", "DM"):
        if key not in par:
            raise KeyError("%s: no %s line" % (ephemeris, key))
    return pplib.DataBunch(**par)


def fake_epochs(par, nsub, tsub, start_MJD=None):
    """Epochs and folding periods of nsub sub-ints of tsub seconds: sub-int
    i is centred tsub / 2 + i tsub seconds after start_MJD (a pplib.MJD or a
    float [day]; default PEPOCH), and its period is 1 / (F0 + F1 dt), dt the
    seconds from PEPOCH to that centre.

    Returns a DataBunch: stt_imjd, stt_smjd, stt_offs (the start, as the
    primary header stores it), offs_sub [nsub] [s], epochs (pplib.MJD per
    sub-int), Ps [nsub] [s]."""
    if start_MJD is None:
        start_MJD = par.PEPOCH
    if not isinstance(start_MJD, pplib.MJD):
        start_MJD = pplib.MJD(float(start_MJD))
    pepoch = pplib.MJD(float(par.PEPOCH))
    sec = start_MJD.fracday() * 86400.0
    smjd = int(np.floor(sec))
    offs_sub = tsub / 2.0 + np.arange(nsub) * float(tsub)
    dt0 = (start_MJD.intday() - pepoch.intday()) * 86400.0 + \
        (start_MJD.fracday() - pepoch.fracday()) * 86400.0
    Ps = 1.0 / (par.F0 + par.F1 * (dt0 + offs_sub))
    return pplib.DataBunch(stt_imjd=start_MJD.intday(), stt_smjd=smjd,
                           stt_offs=sec - smjd, offs_sub=offs_sub,
                           epochs=[start_MJD + t for t in offs_sub],
                           Ps=np.asarray(Ps, dtype=np.float64))


def fake_setup(modelfile, ephemeris, nsub=1, npol=1, nchan=512, nbin=2048,
               nu0=1500.0, bw=800.0, tsub=300.0, phase=0.0, dDM=0.0,
               start_MJD=None, noise_stds=1.0, scales=1.0, t_scat=0.0,
               alpha=pplib.scattering_alpha, scint=False, xs=None, Cs=None,
               nu_DM=np.inf):
    """Everything make_fake_pulsar works out on the host, from its own
    arguments: (par, epochs, tables, model) = (read_par, fake_epochs,
    fake_tables, the modelfile's read_model fields as a DataBunch: code,
    nu_ref, params, alpha), or 0 where fake_tables returns 0."""
    par = read_par(ephemeris)
    (name, code, nu_ref, ngauss, params, fit_flags, model_alpha,
     fit_alpha) = pplib.read_model(modelfile, quiet=True)
    ep = fake_epochs(par, nsub, tsub, start_MJD)
    tab = fake_tables(params[1], par.DM, ep.Ps, nsub=nsub, npol=npol,
                      nchan=nchan, nbin=nbin, nu0=nu0, bw=bw, phase=phase,
                      dDM=dDM, noise_stds=noise_stds, scales=scales,
                      t_scat=t_scat, alpha=alpha, scint=scint, xs=xs, Cs=Cs,
                      nu_DM=nu_DM)
    if not isinstance(tab, pplib.DataBunch):
        return 0
    mdl = pplib.DataBunch(name=name, code=code, nu_ref=nu_ref, params=params,
                          alpha=model_alpha)
    return par, ep, tab, mdl


def templates(mdl, tab, dev=None):
    """The template portraits [nmodel, nchan, nbin] on the device: one
    ppf_gauss_portrait_batch portrait per distinct TAU [bin] of tab.tau_bins
    (read_model's TAU [s] -> [bin] with the sub-int's period,
    pplib.py:3036-3039)."""
    from . import engine
    nmodel = len(tab.tau_bins)
    prm = np.tile(mdl.params, (nmodel, 1))
    prm[:, 1] = tab.tau_bins
    return engine.gauss_portraits(mdl.code, prm, [mdl.alpha] * nmodel,
                                  np.tile(tab.freqs, (nmodel, 1)),
                                  [mdl.nu_ref] * nmodel, len(tab.phases),
                                  dev=dev)


def scint_pattern(nchan, params):
    """add_scintillation's pattern (pplib.py:1203-1217) of explicit (amp,
    freq [cycles], phase [cycles]) triplets."""
    pattern = np.zeros(nchan)
    for isin in range(len(params) // 3):
        a, w, p = params[isin * 3:isin * 3 + 3]
        pattern += a * np.sin(np.linspace(0, w * np.pi, nchan) +
                              p * np.pi) ** 2
    return pattern


def random_scint_params(nsin=2, amax=1.0, wmax=3.0):
    """add_scintillation's random triplets, drawn from np.random in the
    reference's order (pplib.py:1213-1215)."""
    params = []
    for isin in range(nsin):
        params += [np.random.uniform(0, amax), np.random.chisquare(wmax),
                   np.random.uniform(0, 1)]
    return params


def fake_tables(model_tau, DM, Ps, nsub=1, npol=1, nchan=512, nbin=2048,
                nu0=1500.0, bw=800.0, phase=0.0, dDM=0.0, noise_stds=1.0,
                scales=1.0, t_scat=0.0, alpha=pplib.scattering_alpha,
                scint=False, xs=None, Cs=None, nu_DM=np.inf):
    """The per-row tables of a simulated archive, make_fake_pulsar's
    arguments (pplib.py:3302-3307) with the ephemeris DM, the per-sub-int
    periods Ps [nsub] and the modelfile's TAU [s] (model_tau).

    freqs = linspace(lofreq + cw / 2, lofreq + bw - cw / 2, nchan) and
    phases = get_bin_centers(nbin) (pplib.py:3355-3361).

    phi [nsub, nchan], the rotation of each row in turns:
      xs is None: -phase - DM_delay(DM + dDM, freqs, nu0, P_s): the line the
        reference has commented out, rotate_data(model, -phase, -(DM + dDM),
        P, freqs, nu0) (pplib.py:3462), because PSRCHIVE's dededisperse()
        applies the ephemeris DM to its archive; as the reference stands,
        phase and dDM have no effect unless xs is given.  This is the
        documented behaviour.
      xs given: phase' = phase_transform(phase, DM + dDM, nu0, nu_DM, P_s)
        from the caller's phase for every sub-int (the reference overwrites
        phase inside its loops, pplib.py:3464, so its transform compounds
        over sub-ints and polarisations; that is not copied), then
        add_DM_nu(model, -phase', -dDM, P_s, freqs, xs, Cs, nu_DM)'s
        rotation (pplib.py:2626-2636; a non-iterable Cs is all ones, a short
        one is padded with ones) minus DM_delay(DM, freqs, nu0, P_s).
    tau_n [nsub, nchan]: scattering_times(t_scat / P_s, alpha, freqs, nu0)
      when t_scat != 0 and the modelfile's TAU is 0 (the modelfile overrides,
      pplib.py:3470), else 0.
    tau_bins [nmodel], model_of [nsub]: the distinct values of the template's
      TAU in bins, model_tau * nbin / P_s (read_model, pplib.py:3038), and
      which one each sub-int takes.
    gain [nsub, npol, nchan] = scales[n] * pattern[s][p][n], the pattern of
      add_scintillation: an explicit scint list gives one pattern for every
      row; scint=True draws nsin = 3 triplets (amax = 1, wmax = 5) per
      (sub-int, polarisation) from np.random in the reference's order.
    noise [nchan].

    Returns a DataBunch of these, or 0 after the reference's message when
    noise_stds or scales has the wrong length."""
    cw = bw / nchan
    lofreq = nu0 - bw / 2
    freqs = np.linspace(lofreq + cw / 2.0, lofreq + bw - cw / 2.0, nchan)
    phases = pplib.get_bin_centers(nbin, lo=0.0, hi=1.0)
    try:
        if len(noise_stds) != nchan:
            print("\nlen(noise_stds) != nchan\n")
            return 0
        noise_stds = np.asarray(noise_stds, dtype=np.float64)
    except TypeError:
        noise_stds = noise_stds * np.ones(nchan)
    try:
        if len(scales) != nchan:
            print("\nlen(scales) != nchan\n")
            return 0
        scales = np.asarray(scales, dtype=np.float64)
    except TypeError:
        scales = scales * np.ones(nchan)
    Ps = np.asarray(Ps, dtype=np.float64).reshape(nsub)
    phi = np.zeros((nsub, nchan))
    tau_n = np.zeros((nsub, nchan))
    for isub in range(nsub):
        P = Ps[isub]
        if xs is None:
            phi[isub] = -phase - pplib.DM_delay(DM + dDM, freqs, nu0, P)
        else:
            php = pplib.phase_transform(phase, DM + dDM, nu0, nu_DM, P)
            D = pplib.Dconst * -dDM / P
            C = Cs
            if not hasattr(C, "__iter__"):
                C = np.ones(len(xs))
            if len(C) < len(xs):
                C = list(C) + list(np.ones(len(xs) - len(C)))
            freq_term = 0.0
            for c, x in zip(C, xs):
                freq_term = freq_term + c * (freqs ** x - nu_DM ** x)
            phi[isub] = (-php + (D * freq_term)) - \
                pplib.DM_delay(DM, freqs, nu0, P)
        if t_scat and not model_tau:
            tau_n[isub] = pplib.scattering_times(t_scat / P, alpha, freqs, nu0)
    tau_bins, model_of = np.unique(model_tau * nbin / Ps, return_inverse=True)
    gain = np.empty((nsub, npol, nchan))
    for isub in range(nsub):
        for ipol in range(npol):
            if scint is False:
                gain[isub, ipol] = scales
            elif scint is True:
                gain[isub, ipol] = scales * scint_pattern(
                    nchan, random_scint_params(nsin=3, amax=1.0, wmax=5.0))
            elif scint is None:     # add_scintillation(rotmodel, None)
                gain[isub, ipol] = scales * scint_pattern(
                    nchan, random_scint_params())
            else:
                gain[isub, ipol] = scales * scint_pattern(nchan, scint)
    return pplib.DataBunch(freqs=freqs, phases=phases, phi=phi, tau_n=tau_n,
                           tau_bins=tau_bins,
                           model_of=model_of.reshape(nsub).astype(np.int32),
                           gain=gain, noise=noise_stds, scales=scales)
