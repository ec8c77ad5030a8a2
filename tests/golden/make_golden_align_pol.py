#!/usr/bin/env python
"""Golden vectors for ppalign.align_archives(pscrunch=False) (ppalign.py:65-280,
the "average Stokes portraits" output), produced by running the REFERENCE on
the CPU (never on the GPU box), under the shims of make_golden_align.py.

The synthetic total-intensity DataBunches of make_golden_align.make_archives
become four-polarisation ones: pol p = c_p * I + independent noise, c = (1,
0.5, -0.3, 0.2), every amplitude exact in float32; noise_stds, SNRs and masks
are repeated per polarisation (the reference fits pol 0 only); the guess gets
a four-polarisation recorder archive.  3 files x 2 sub-ints x 17 channels x
64 bins, one file with zapped channels, 2 iterations.

Usage:  python tests/golden/make_golden_align_pol.py
"""
import contextlib
import io
import os
import time

import make_golden_align as ga          # (imports the reference, shimmed)
import numpy as np

mg, ppalign = ga.mg, ga.ppalign
HERE = os.path.dirname(os.path.abspath(__file__))

COEFF = (1.0, 0.5, -0.3, 0.2)
POL_NOISE = 0.5
NFILE, NSUB, NCHAN, NBIN, NITER = 3, 2, 17, 64, 2
SEED_POL = 4242


def polarise(files, nfile, nchan, nbin):
    """The four-polarisation DataBunches of the npol = 1 ones, in place;
    returns the inputs to save."""
    rng = np.random.default_rng(SEED_POL)
    inputs = {}
    for ifile in range(nfile):
        d = files["arch%d.fits" % ifile]
        I = d.subints[:, 0]                              # [nsub, nchan, nbin]
        sub = np.empty((I.shape[0], 4) + I.shape[1:])
        sub[:, 0] = I                                    # c_0 = 1, its own noise
        for p in range(1, 4):
            sub[:, p] = mg.f32(COEFF[p] * I +
                               rng.normal(0.0, POL_NOISE, I.shape))
        d.subints = d["subints"] = sub
        d.npol = d["npol"] = 4
        for k in ("noise_stds", "SNRs", "masks"):
            d[k] = np.repeat(d[k], 4, axis=1)
        inputs["f%d_subints" % ifile] = sub.astype(np.float32)
        assert np.array_equal(inputs["f%d_subints" % ifile].astype(float), sub)
    g = files["guess.fits"]
    guess = np.stack([mg.f32(c * g.subints[0, 0]) for c in COEFF])
    g.subints = g["subints"] = guess[None]
    g.npol = g["npol"] = 4
    for k in ("noise_stds", "SNRs", "masks"):
        g[k] = np.repeat(g[k], 4, axis=1)
    arch = ga.FakeArch(4, nchan, nbin)
    g.arch = g["arch"] = arch
    inputs["guess"] = guess
    return inputs, arch


def run_align():
    files, inputs, _ = ga.make_archives(NFILE, NSUB, NCHAN, NBIN)
    inputs.update(polarise(files, NFILE, NCHAN, NBIN)[0])
    arch = files["guess.fits"].arch
    ppalign.load_data = lambda filename, **kw: files[filename]
    ppalign.sub.Popen = lambda *a, **kw: ga._VapPopen(NCHAN, NBIN)
    datafiles = ["arch%d.fits" % i for i in range(NFILE)]
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        ppalign.align_archives(list(datafiles), "guess.fits", fit_dm=True,
                               pscrunch=False, niter=NITER,
                               outfile="aligned.fits", quiet=True)
    dt = time.time() - t0
    out = dict(inputs)
    out.update(nfile=np.int64(NFILE), nsub=np.int64(NSUB),
               nchan=np.int64(NCHAN), nbin=np.int64(NBIN),
               niter=np.int64(NITER), P=np.float64(mg.P0),
               DM0=np.float64(mg.DM0), ref_seconds=np.float64(dt),
               coeff=np.array(COEFF), out_aligned=arch.amps.copy(),
               out_weights=arch.weights.copy(), out_dm=np.float64(arch.dm))
    return out


def main():
    out = run_align()
    path = os.path.join(HERE, "align_pol.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.2f s of reference time, %d bytes)"
          % (path, float(out["ref_seconds"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
