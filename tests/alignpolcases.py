"""The polarised ppalign golden (tests/golden/align_pol.npz, made by
tests/golden/make_golden_align_pol.py from the reference's
align_archives(pscrunch=False)): its DataBunches rebuilt as the script handed
them to the reference, and the same inputs as PSRFITS files."""
import functools
import os

import numpy as np

import goldens as G

COEFF = (1.0, 0.5, -0.3, 0.2)            # make_golden_align_pol.COEFF
POL_NOISE, SEED_POL = 0.5, 4242


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             "golden", "align_pol.npz"))
    c = {k: z[k] for k in z.files}
    for v in c.values():
        v.setflags(write=False)
    return c


def _rep(a):
    """[nsub, nchan, ...] -> [nsub, 4, nchan, ...], the same in every pol."""
    return np.repeat(np.asarray(a)[:, None], 4, axis=1)


def inputs(c=None):
    """(archives, model_data): four-polarisation Stokes DataBunches."""
    c = golden() if c is None else c
    nfile, nsub = int(c["nfile"]), int(c["nsub"])
    nchan, nbin = int(c["nchan"]), int(c["nbin"])
    freqs, P = c["freqs"], float(c["P"])
    archives = []
    for i in range(nfile):
        w = c["f%d_weights" % i]
        wn = np.where(w == 0.0, 0.0, 1.0)
        archives.append(G.Bunch(
            DM=float(c["DM0"]), dmc=0, freqs=np.tile(freqs, (nsub, 1)),
            masks=_rep(np.einsum("ij,k", wn, np.ones(nbin))), nbin=nbin,
            nchan=nchan, noise_stds=_rep(c["f%d_noise" % i]), npol=4,
            nsub=nsub, ok_ichans=[np.compress(wn[j], list(range(nchan)))
                                  for j in range(nsub)],
            ok_isubs=np.arange(nsub), prof_SNR=100.0, Ps=np.ones(nsub) * P,
            SNRs=_rep(c["f%d_snrs" % i]),
            subints=c["f%d_subints" % i].astype(np.float64), weights=w,
            state="Stokes"))
    model_data = G.Bunch(
        DM=0.0, dmc=1, freqs=freqs[None, :],
        masks=np.ones([1, 4, nchan, nbin]), nbin=nbin, nchan=nchan,
        noise_stds=np.ones([1, 4, nchan]), npol=4, nsub=1,
        ok_ichans=[np.arange(nchan)], ok_isubs=np.arange(1), prof_SNR=100.0,
        Ps=np.ones(1) * P, SNRs=np.ones([1, 4, nchan]),
        subints=np.array(c["guess"])[None], weights=np.ones([1, nchan]),
        arch=None, state="Stokes")
    return archives, model_data


def rebuilt_pols(c=None):
    """Pols 1..3 of every file and the guess, rebuilt from pol 0 by the
    recipe of make_golden_align_pol.polarise: ([file] [nsub, 3, nchan,
    nbin] float32, guess [4, nchan, nbin])."""
    c = golden() if c is None else c
    rng = np.random.default_rng(SEED_POL)
    files = []
    for i in range(int(c["nfile"])):
        I = c["f%d_subints" % i][:, 0].astype(np.float64)
        files.append(np.stack(
            [(COEFF[p] * I + rng.normal(0.0, POL_NOISE, I.shape)
              ).astype(np.float32) for p in range(1, 4)], axis=1))
    g0 = c["guess"][0]
    guess = np.stack([(k * g0).astype(np.float32).astype(np.float64)
                      for k in COEFF])
    return files, guess


def write_files(tmp, c=None):
    """The golden's inputs as three IQUV PSRFITS files of float32 samples
    and a four-polarisation template file (DM 0: its dedispersion rotates
    nothing); returns (metafile, template).  The files' DM is the golden's
    DM0, their weights the golden's."""
    from pulseportraiture_amd import psrfits as PF
    c = golden() if c is None else c
    nfile, nsub = int(c["nfile"]), int(c["nsub"])
    nchan = int(c["nchan"])
    freqs, P = c["freqs"], float(c["P"])
    names = []
    for i in range(nfile):
        fn = os.path.join(str(tmp), "arch%d.fits" % i)
        PF.write_archive_rows(
            fn, np.array(c["f%d_subints" % i]), np.tile(freqs, (nsub, 1)),
            np.array(c["f%d_weights" % i]), np.full(nsub, P),
            5.0 + 10.0 * np.arange(nsub), np.full(nsub, 10.0),
            pol_type="IQUV", dm=float(c["DM0"]), elem="E")
        names.append(fn)
    tmpl = os.path.join(str(tmp), "guess.fits")
    PF.write_archive_rows(
        tmpl, np.array(c["guess"], dtype=np.float32)[None], freqs[None],
        np.ones((1, nchan)), np.full(1, P), np.array([5.0]), np.full(1, 10.0),
        pol_type="IQUV", dm=0.0, elem="E")
    meta = os.path.join(str(tmp), "meta")
    with open(meta, "w") as fh:
        fh.write("".join(n + "\n" for n in names))
    return meta, tmpl
