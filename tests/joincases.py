"""The joined Gaussian model's test cases, shared by the golden generator
(tests/golden/make_golden_gaussjoin.py) and the tests: several archives of
one pulsar under one evolving-Gaussian model, each archive with a phase and a
DM offset of its own (the reference's join parameters, pplib.py:956-962,
2073-2098).

Layout of the extended parameter vector: [params (2 + 6 ngauss), join params
(phase, DM per archive), scattering index], the reference's lmfit order.

The host model here is oracle.gen_gaussian_portrait followed by
oracle.rotate_data per archive; the generator checks that composition
against the reference's gen_gaussian_portrait(join_ichans=...) to 1e-13 of
the portrait's maximum before it writes anything.
"""
import numpy as np

NU_REF, ALPHA, P = 1500.0, -4.0, 1.0 / 345.67890123456789
NOISE = 0.05

COMPS_000 = [[0.30, 0.01, 0.08, -0.5, 5.0, -1.5],
             [0.60, -0.02, 0.12, 0.4, 3.0, -0.8]]        # port_5x64_000
COMPS_111 = [[0.30, 2e-5, 0.07, -1e-5, 5.0, -2e-3],
             [0.62, -1e-5, 0.11, 2e-5, 3.0, 1e-3]]       # port_33x100_111

BANDS = {"lo": (700.0, 900.0), "mid": (1100.0, 1500.0),
         "hi": (1450.0, 1900.0)}

# name: (channels per band, bands, nbin, code, components, tau [bin],
#        fit tau, join truth (phase, DM per archive), seed)
FIT_CASES = {
    "join2_11x64_000": ((6, 5), ("mid", "hi"), 64, "000", COMPS_000, 0.0,
                        False, [0.0, 3e-4, 0.013, -2e-4], 1),
    "join3_15x128_000_tau": ((5, 6, 4), ("lo", "mid", "hi"), 128, "000",
                             COMPS_000, 2.0, True,
                             [0.0, 2e-4, 0.021, -3e-4, -0.008, 5e-4], 2),
    "join2_9x100_111": ((4, 5), ("mid", "hi"), 100, "111", COMPS_111, 0.0,
                        False, [0.0, 3e-4, 0.013, -2e-4], 3),
}


def assemble(nchans, bands):
    """The archives' np.linspace bands concatenated and sorted by frequency:
    (freqs, join_ichans), join_ichans[a] the sorted positions of archive a's
    channels in increasing order."""
    f = np.concatenate([np.linspace(BANDS[b][0], BANDS[b][1], n)
                        for n, b in zip(nchans, bands)])
    src = np.concatenate([np.full(n, a) for a, n in enumerate(nchans)])
    isort = np.argsort(f)
    freqs, src = f[isort], src[isort]
    return freqs, [np.flatnonzero(src == a) for a in range(len(nchans))]


def join_ids(join_ichans, nchan):
    ids = np.full(nchan, -1, dtype=np.int32)
    for a, ic in enumerate(join_ichans):
        ids[np.asarray(ic)] = a
    return ids


def host_model(gen, rotate, code, p_ext, njoin, nbin, freqs, nu_ref,
               join_ichans, P):
    """gen (a gen_gaussian_portrait without joins) then rotate (a
    rotate_data) per archive, on the extended vector p_ext."""
    p_ext = np.asarray(p_ext, dtype=float)
    npar = len(p_ext) - 1 - 2 * njoin
    phases = np.zeros(nbin)
    port = np.array(gen(code, p_ext[:npar], p_ext[-1], phases, freqs, nu_ref))
    jp = p_ext[npar:-1]
    for a, ic in enumerate(join_ichans):
        port[ic] = rotate(port[ic], jp[2 * a], jp[2 * a + 1], P, freqs[ic],
                          nu_ref)
    return port


def fit_case(name):
    """truth, start, vary (all extended), freqs, join_ichans, nbin, code of a
    fit case.  The first archive's phase, m_loc1, tau (unless fitted) and the
    index are fixed; start = truth * 1.03 on the model parameters, join
    phases truth + 0.002, join DMs 0."""
    nchans, bands, nbin, code, comps, tau, fit_tau, jtruth, seed = \
        FIT_CASES[name]
    freqs, join_ichans = assemble(nchans, bands)
    njoin = len(nchans)
    mp = np.array([0.02, tau] + [v for c in comps for v in c])
    truth = np.concatenate([mp, jtruth, [ALPHA]])
    npar = len(mp)
    vary = np.ones(len(truth), dtype=bool)
    vary[1], vary[3], vary[-1] = fit_tau, False, False
    vary[npar] = False                              # the first archive's phase
    start = truth.copy()
    start[:npar] = np.where(vary[:npar], mp * 1.03, mp)
    start[npar + 1:-1:2] = 0.0                      # every DM starts at 0
    start[npar + 2:-1:2] = truth[npar + 2:-1:2] + 0.002
    return dict(truth=truth, start=start, vary=vary, freqs=freqs,
                join_ichans=join_ichans, nbin=nbin, code=code, njoin=njoin,
                npar=npar, seed=seed)


# model portraits: name -> (nbin, tau)
PORT_CASES = {"nyq_3x64": (64, 2.0), "p100": (100, 0.0),
              "p100_tau": (100, 3.0), "p1536": (1536, 0.0),
              "p1536_tau": (1536, 5.0)}


def port_case(name):
    """Inputs of a model-portrait case (extended parameter vector)."""
    nbin, tau = PORT_CASES[name]
    if name == "nyq_3x64":
        # one component of FWHM 0.02 rot, tau 2 bins, join (0.0137, 3e-4)
        freqs = np.array([1200.0, 1500.0, 1800.0])
        p = [0.0, tau, 0.40, 0.0, 0.02, 0.0, 2.0, 0.0, 0.0137, 3e-4, ALPHA]
        return dict(code="000", p_ext=np.array(p), freqs=freqs, nbin=nbin,
                    join_ichans=[np.arange(3)], njoin=1)
    # 6 interleaved channels, two archives, channel 4 in no archive
    freqs = np.array([1110.0, 1230.0, 1370.0, 1490.0, 1610.0, 1790.0])
    mp = [0.02, tau] + [v for c in COMPS_000 for v in c]
    p = mp + [0.0137, 3e-4, -0.31, -2e-4, ALPHA]
    return dict(code="000", p_ext=np.array(p), freqs=freqs, nbin=nbin,
                join_ichans=[np.array([0, 2, 5]), np.array([1, 3])], njoin=2)
