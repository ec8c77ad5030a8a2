#!/usr/bin/env python
"""SHA-256 of what the block row kernels return on fixed seeded inputs, to
compare two builds of the library (env PPFIT_LIB) bit for bit, as
tools/unpack_bench.py does for the unpack routes.  Through the engine's public
functions, three rows (or channels) per call, float32 and float64 input where
the function takes both:

  rotate, rotate_ref   engine.rotate_rows, ref_len False / True   (k_rotate)
  resid_chi2           engine.resid_chi2_rows                      (k_resid_chi2)
  inst_resp            engine.inst_response_rows, with a table     (k_inst_resp)
  align                engine.align_accum, 5 sub-ints, one weight 0
                                                  (k_align_part / k_align_fin)
  gport, gport_tau, gport_join, gport_join_tau
                       engine.gauss_portraits                 (k_gauss_port[_join])
  glsq, glsq_join      engine.gauss_lsq, tau != 0        (k_gauss_rows[_join])

at the smallest lengths that reach each class of the launchers' dispatch
(tests/fftplans.py): 64 and 34 (KMAX 1, butterflies / mixed radix), 33 (odd,
the nbin - 1 inverse at 16 points), 770 (KMAX 2), 1025 (KMAX 4, odd), 2050
(KMAX 8), 8192 and 8190 (KMAX 16).  A length a function refuses
(NotImplementedError: odd nbin for inst_resp and the joined model) prints
"refused".  One line per (route, nbin, dtype), then the digest of all lines.
Needs a HIP device.

  python tools/rowcore_hash.py
  PPFIT_LIB=/other/build/libppfit.so python tools/rowcore_hash.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from pulseportraiture_amd import engine  # noqa: E402

NBINS = (64, 34, 33, 770, 1025, 2050, 8192, 8190)
FREQS = np.array([[1200.0, 1400.0, 1650.0]])
# DC, tau [bin], two components (loc, m_loc, wid, m_wid, amp, m_amp)
PARAMS = np.array([0.1, 0.0, 0.31, 0.02, 0.05, -0.3, 1.0, -1.2,
                   0.62, -0.01, 0.11, 0.4, 0.4, 0.7])
JOIN_ID = np.array([[0, 1, -1]], dtype=np.int32)
JOIN_PARAMS = np.array([[0.0123, 1.5e-3, -0.0311, -2.5e-3]])
PERIOD = np.array([0.0031])


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def routes(nbin, dtype, rng):
    rows = rng.normal(size=(3, nbin)).astype(dtype)
    phases = np.array([0.137, -0.4021, 2.25])
    model = rng.normal(size=(2, nbin))
    yield "rotate", lambda: digest(engine.rotate_rows(rows, phases))
    yield "rotate_ref", lambda: digest(
        engine.rotate_rows(rows, phases, ref_len=True))
    yield "resid_chi2", lambda: digest(engine.resid_chi2_rows(
        rows, phases, model, [1, 0, 1], [0.9, 1.1, 1.3], [1.0, 2.0, 0.5],
        nbin - 3))
    if dtype == np.float64:
        table = 1.0 / (1.0 + 0.01 * np.arange(nbin // 2 + 1))
        yield "inst_resp", lambda: digest(engine.inst_response_rows(
            rows, [2, 0, 1], table, [0.0, 3e-3, 0.02]))
    data = rng.normal(size=(5, 3, nbin)).astype(dtype)
    aph = rng.uniform(-0.5, 0.5, size=(5, 3))
    aw = rng.uniform(0.5, 2.0, size=(5, 3))
    aw[3, 1] = 0.0

    def align():
        dev = engine.device()
        out = torch.zeros((3, nbin), dtype=torch.float64, device=dev)
        wsum = torch.zeros(3, dtype=torch.float64, device=dev)
        engine.align_accum(data, aph, aw, out, wsum)
        return digest(out, wsum)
    yield "align", align
    prm_tau = PARAMS.copy()
    prm_tau[1] = 0.004 * nbin
    join = dict(join_id=JOIN_ID, join_params=JOIN_PARAMS, P=PERIOD)
    if dtype == np.float64:
        for name, prm, kw in (("gport", PARAMS, {}), ("gport_tau", prm_tau, {}),
                              ("gport_join", PARAMS, join),
                              ("gport_join_tau", prm_tau, join)):
            yield name, lambda prm=prm, kw=kw: digest(engine.gauss_portraits(
                "010", prm, -4.0, FREQS, 1400.0, nbin, **kw))
    gdata = rng.normal(size=(1, 3, nbin)).astype(dtype)
    errs = np.full((1, 3, nbin), 0.5)
    # DC, tau, a location, a width, (the DM of archive 0,) the scattering index
    for name, free, kw in (("glsq", [0, 1, 2, 4, 14], {}),
                           ("glsq_join", [0, 1, 2, 4, 15, 18], join)):
        yield name, lambda free=free, kw=kw: digest(engine.gauss_lsq(
            "010", prm_tau, -4.0, FREQS, 1400.0, free, [1e-6] * len(free),
            gdata, errs, **kw))


def main():
    lines = []
    for nbin in NBINS:
        for dtype in (np.float32, np.float64):
            rng = np.random.default_rng(nbin)
            for name, fn in routes(nbin, dtype, rng):
                try:
                    sha = fn()
                except NotImplementedError:
                    sha = "refused"
                lines.append("%-14s %5d %s %s" % (name, nbin,
                                                  np.dtype(dtype).name, sha))
                print(lines[-1], flush=True)
    print("all %s" % hashlib.sha256("\n".join(lines).encode()).hexdigest())


if __name__ == "__main__":
    main()
