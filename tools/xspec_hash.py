#!/usr/bin/env python
"""SHA-256 of what the spectrum-pass kernels and their two wave-per-row
siblings return on the tests' own seeded inputs, to compare two builds of the
library (env PPFIT_LIB) bit for bit, in the manner of tools/rowcore_hash.py.

  fit     ragged.device_fit on a case of tests/ragged.py or tests/fftplans.py:
          result table, scales, scale errors, channel S/N and covariance of
          the batch of four sub-ints.  One case per spectrum kernel and input
          type:
            k_xspec_w     pass / warm at 256, 512 and 1024 bins
            k_xspec_wm    a wm512 and a wm1024 case
            k_xspec_wo    a wo512 and a wo1024 case
            k_xspec       blk at 128, 512 x 17 (two fits) and 4096 bins
            k_xspec_any   any-even, any-odd
            k_xspec_spec  long-5x8194
          and the five 256-channel cases on the swizzled block map (swz).
  noise   engine.noise_rows, 3 rows                            (k_noise_w)
  align   engine.align_accum, 5 sub-ints x 3 channels, one weight 0
                                                          (k_align_part_w)
          at nbin 256, 512, 1024 and 2048, float32 and float64.

One line per case, then the digest of all lines.  These fits are required to
be bitwise reproducible (each sub-int alone equals the batch), so a digest
that differs between two builds is a real change.  Needs a HIP device.

  python tools/xspec_hash.py
  PPFIT_LIB=/other/build/libppfit.so python tools/xspec_hash.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import fftplans as F  # noqa: E402
import ragged as R  # noqa: E402
from pulseportraiture_amd import engine  # noqa: E402

RAGGED = ("warm-257x256-pdta-cut-f32", "pass-97x512-pdta-cut-f32",
          "blk-45x128-pd-cut-f32", "blk-17x512-pd-cut-f32",
          "blk-17x512-pdt-cut-f32", "blk-45x4096-pd-cut-f32",
          "long-5x8194-pd-cut-f32")
# (path, nbin) of tests/fftplans.py's FIT_CASES: f32 and f64 rows alternate
FFTPLANS = (("wm512", 242), ("wm512", 286), ("wm1024", 1200), ("wm1024", 1372),
            ("wo512", 243), ("wo512", 511), ("wo1024", 513),
            ("any-even", 2050), ("any-odd", 1025))
WAVE_NBINS = (256, 512, 1024, 2048)
KEYS = ("results", "scales", "scale_errs", "channel_snrs", "covariance")


def fit_cases():
    for n in RAGGED:
        yield R.case(n)
    # k_xspec_w at 1024 bins has no case in the suite (2048 bins take
    # k_xspec_w2): pass-97x512's, at twice the length
    for dt in ("f32", "f64"):
        yield R._case("pass", 1024, 97, R.PDTA, dtype=dt, **R._SC)
    # float64 rows where the suites' cases of a kernel are all float32
    yield R._case("pass", 512, 97, R.PDTA, dtype="f64", **R._SC)
    yield R._case("blk", 512, 17, R.PD, dtype="f64")
    yield R._case("wo", 1001, 37, R.PDTA, dtype="f64", **R._SC)
    for path, nbin in FFTPLANS:
        yield next(c for c in F.FIT_CASES
                   if c["family"] == path and c["nbin"] == nbin)
    for n in R.SWIZZLED:
        yield R.case(n)


def fit_digest(c):
    r = R.device_fit(c)
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(r[k]).tobytes())
    return h.hexdigest()


def tensor_digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def wave_routes(nbin, dtype):
    rng = np.random.default_rng(nbin)
    rows = rng.normal(size=(3, nbin)).astype(dtype)
    yield "noise", lambda: tensor_digest(engine.noise_rows(rows))
    data = rng.normal(size=(5, 3, nbin)).astype(dtype)
    aph = rng.uniform(-0.5, 0.5, size=(5, 3))
    aw = rng.uniform(0.5, 2.0, size=(5, 3))
    aw[3, 1] = 0.0

    def align():
        dev = engine.device()
        out = torch.zeros((3, nbin), dtype=torch.float64, device=dev)
        wsum = torch.zeros(3, dtype=torch.float64, device=dev)
        engine.align_accum(data, aph, aw, out, wsum)
        return tensor_digest(out, wsum)
    yield "align", align


def main():
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    for c in fit_cases():
        emit("fit   %-34s %s" % (c["name"], fit_digest(c)))
    for nbin in WAVE_NBINS:
        for dtype in (np.float32, np.float64):
            for name, fn in wave_routes(nbin, dtype):
                emit("%-5s %5d %-7s %s" % (name, nbin, np.dtype(dtype).name,
                                          fn()))
    print("all %s" % hashlib.sha256("\n".join(lines).encode()).hexdigest())


if __name__ == "__main__":
    main()
