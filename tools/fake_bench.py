#!/usr/bin/env python
"""Time writing simulated archives: pplib.make_fake_pulsar (profiles built
and digitised on the device, 2 bytes per sample over PCIe, bytes written as
they are) against the same files from the pieces that preceded it
(engine.synth float32 -> download -> psrfits.quantize -> write_psrfits).

One run writes --archives files of --nsub x --nchan x --nbin into one
directory (both paths the same one, the files overwritten run after run);
the figure of a path is the median of --runs runs after one warm-up run.
The device's own share of the new path is timed with events around
engine.fake_subints on the same shape.  Needs a HIP device.

  python tools/fake_bench.py --out profiles/make_fake_pulsar.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from pulseportraiture_amd import engine, fake, pplib, psrfits  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
GMODEL = os.path.join(GOLDEN, "example.gmodel")
PAR = os.path.join(GOLDEN, "example.par")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archives", type=int, default=32)
    ap.add_argument("--nsub", type=int, default=64)
    ap.add_argument("--nchan", type=int, default=512)
    ap.add_argument("--nbin", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files go")
    ap.add_argument("--out", default=None, help="JSON result file")
    a = ap.parse_args()
    dev = engine.device(None)
    kw = dict(nsub=a.nsub, nchan=a.nchan, nbin=a.nbin, nu0=1500.0, bw=800.0,
              tsub=60.0, phase=0.1, dDM=3e-4, noise_stds=0.05)
    par, ep, tab, mdl = fake.fake_setup(GMODEL, PAR, **kw)
    model = fake.templates(mdl, tab, dev=dev)
    freqs2 = np.tile(tab.freqs, (a.nsub, 1))
    ones = np.ones((a.nsub, a.nchan))

    def new_path(d):
        for i in range(a.archives):
            pplib.make_fake_pulsar(GMODEL, PAR, outfile=os.path.join(
                d, "new%02d.fits" % i), quiet=True, seed=i, dev=dev, **kw)

    def old_path(d):
        for i in range(a.archives):
            rows = engine.synth(model[0], tab.freqs, np.full(a.nsub, 0.1),
                                np.full(a.nsub, par.DM + 3e-4), ep.Ps, 1500.0,
                                0.05, i, dev=dev).cpu().numpy()
            q, scl, offs = psrfits.quantize(rows[:, None])
            psrfits.write_psrfits(os.path.join(d, "old%02d.fits" % i), q, scl,
                                  offs, freqs2, ones, ep.Ps, ep.offs_sub,
                                  np.full(a.nsub, 60.0), dm=par.DM)

    def timed(fn, d):
        t = []
        for r in range(a.runs + 1):          # run 0 warms up
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(d)
            torch.cuda.synchronize(dev)
            t.append(time.perf_counter() - t0)
        return t[1:]

    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        t_new = timed(new_path, d)
        t_old = timed(old_path, d)
    # the device's share: rfft of the template + k_fake, events around the call
    ev = []
    for r in range(a.runs + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        e0.record()
        out = engine.fake_subints(model, tab.model_of, tab.phi, tab.tau_n,
                                  tab.gain, tab.noise, r, quantized=True,
                                  dev=dev)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
        del out
    samples = a.nsub * a.nchan * a.nbin
    res = dict(
        shape=dict(archives=a.archives, nsub=a.nsub, nchan=a.nchan,
                   nbin=a.nbin, runs=a.runs),
        device=torch.cuda.get_device_name(dev),
        make_fake_pulsar_s=dict(median=float(np.median(t_new)), runs=t_new),
        synth_quantize_write_s=dict(median=float(np.median(t_old)), runs=t_old),
        speedup=float(np.median(t_old) / np.median(t_new)),
        fake_subints_ms_per_archive=dict(median=float(np.median(ev[1:])),
                                         runs=ev[1:]),
        fake_subints_gsamples_per_s=float(samples / np.median(ev[1:]) / 1e6),
        bytes_over_pcie_per_sample=dict(make_fake_pulsar=2,
                                        synth_quantize_write=4))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
