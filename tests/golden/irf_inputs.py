"""Inputs of the instrumental-response golden cases (tests/golden/irf.npz),
rebuilt from a few stored parameters (TEST INFRASTRUCTURE; no reference
import).

make_golden_irf.py builds the inputs here, hands them to the REFERENCE with
GetTOAs.instrumental_response_dict set and stores only its outputs plus a
SHA-256 of the inputs; the tests rebuild the inputs here and check the hash
(as full_inputs.py / synth_np.py).

The archives hold the template rotated to the sub-int's phase and DM at the
sub-int's OWN period, scattered, plus white noise, rounded to float32.  The
scattering is a model mismatch whose phase bias in a channel depends on which
harmonics the fit weighs; the response on the template changes those weights
by a channel-dependent amount, so it moves the fitted DM by many sigma
(make_golden_irf.py asserts at least 10).
"""
import numpy as np

import full_inputs as FI
import synth_np as S

# instrumental_response_port_FT parameter sets (pptoaslib.py:158-192):
# (name, DM, P, wids, irf_types), each at 8 channels x nbin 64, 1000, 2048
RESP_NBINS = (64, 1000, 2048)
RESP_NCHAN = 8
RESP = [
    ("rect", 0.0, 1.0, [0.013], ["rect"]),
    ("gauss", 0.0, 1.0, [0.002, 0.1], ["gauss", "gauss"]),
    ("dm", 34.5, 0.0029, [], []),
    ("all", 12.3, 0.0046, [0.021, 0.05, 0.007], ["rect", "gauss", "rect"]),
]


def resp_freqs():
    return S.channel_freqs(RESP_NCHAN)


# get_TOAs / get_narrowband_TOAs cases, in the layout of full_inputs.TOAS plus
#   ird   the instrumental_response_dict
#   Pf    per-sub-int period factors (P = Pf * synth_np.P0)
#   zap1  the sub-int whose channel 1 is zapped (chan_bw of its usable
#         channels doubles, pptoaslib.py:187 with pptoas.py:424)
CASES = [
    # phase + DM, .gmodel, DM smearing and two constant responses
    dict(name="toa_pd", nfile=1, nsub=3, nchan=64, nbin=512, seed=501,
         tau=8e-3, noise=0.3, Pf=[1.0, 1.25, 0.8], zap1=1,
         ird=dict(DM=S.DM0, wids=[0.02, 0.05], irf_types=["rect", "gauss"])),
    # every flag (phi, DM, GM, tau, alpha), DM smearing only, on the
    # unscattered template of the scattering fit (pptoas.py:408-434)
    # (seed: one at which the reference's own trust-ncg end points sit
    # within 0.003 sigma of their stationary points, which
    # make_golden_irf.py measures and asserts; at seed 502 its third
    # sub-int stopped 0.039 sigma short, four times the comparison's bar)
    dict(name="toa_scat", nfile=1, nsub=3, nchan=64, nbin=512, seed=522,
         gmodel="scat", tau=2e-3, noise=0.1, Pf=[0.5, 0.62, 0.55],
         kw=dict(fit_GM=True, fit_scat=True),
         ird=dict(DM=S.DM0, wids=[], irf_types=[])),
    # spline template, constant responses only, nbin not a power of two
    dict(name="toa_spl", nfile=1, nsub=2, nchan=64, nbin=1000, seed=503,
         spline=True, tau=8e-3, noise=0.3, Pf=[1.0, 1.1],
         ird=dict(DM=0.0, wids=[0.015, 0.06], irf_types=["rect", "gauss"])),
    # get_narrowband_TOAs, DM smearing and a rectangle
    dict(name="nb", nfile=1, nsub=2, nchan=16, nbin=512, seed=504,
         tau=2e-2, Pf=[1.0, 1.2], zap1=0, noise=0.1,
         ird=dict(DM=S.DM0, wids=[0.02], irf_types=["rect"])),
]


def conf(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def inputs(c):
    """Per archive: subints [nsub, nchan, nbin] f32-rounded, weights, Ps,
    doppler factors, epochs (full_inputs.toa_inputs' layout); plus freqs.
    Rebuilt identically by the tests."""
    files, freqs = FI.toa_inputs(c)     # weights, dfs, epochs, parangles, dDM
    nchan, nbin, nsub = c["nchan"], c["nbin"], c["nsub"]
    model, _ = S.template(nchan, nbin)
    rng = np.random.default_rng(20251019 + c["seed"])
    for f, fi in enumerate(files):
        Ps = S.P0 * np.asarray(c["Pf"], dtype=float)
        subs = np.zeros((nsub, nchan, nbin))
        for s in range(nsub):
            phi = rng.uniform(-0.5, 0.5)
            clean = S.subint(0, model, freqs, phi, S.DM0 + fi["dDM"], Ps[s],
                             tau=c.get("tau", 0.0), noise=0.0)
            subs[s] = S.f32(clean + rng.normal(0.0, c.get("noise", 1.5),
                                               clean.shape))
        w = fi["weights"]
        w[:, :3] = 1.0                  # chan_bw from channels 0, 1 ...
        if "zap1" in c:
            w[c["zap1"], 1] = 0.0       # ... or from 0, 2 in this sub-int
        fi.update(subints=subs, Ps=Ps)
    return files, freqs


def archive_fields(c, fi, freqs, noise, snrs):
    """full_inputs.archive_fields with the per-sub-int periods."""
    d = FI.archive_fields(c, fi, freqs, noise, snrs)
    d["Ps"] = np.asarray(fi["Ps"], dtype=float)
    return d


def gmodel(c):
    return FI.toa_gmodel(c)
