#!/usr/bin/env python
"""Time the PSRFITS unpack on the device (k_unpack, k_base_window,
k_row_stats) on 16-bit samples, as tools/pack_bench.py does for the pack
kernel, by the three routes load_data takes:

  npol1   engine.unpack_psrfits, total intensity from one block (pol_mode 0)
  aabb    engine.unpack_psrfits, total intensity = AA + BB (npol 2, pol_mode 1)
  pol     engine.unpack_psrfits_pol, Coherence -> Stokes (conv 2)

Per shape (nsub x nchan x nbin) and route: the device-event time of one call,
the median and all of --runs calls after one warm-up, for the samples as
stored (4 bins per lane: 8-byte loads, 16-byte stores) and for the same
samples behind a sub_stride padded by 2 bytes (element-wide accesses), with
the outputs of the two compared bitwise.  GB/s counts the bytes k_unpack
itself reads and writes per sample (2 per block read, 4 per row written) over
the whole call's time (the statistics pass reads the rows again, and writes
them with rm_baseline: not counted), beside the share of the HBM peak (8 TB/s
nominal).  The inputs are seeded: sha256 is the digest of the bytes of rows,
stats, total and wstart of one call with rm_baseline and one without, for
both layouts, to compare two builds of the library (env PPFIT_LIB) bit for
bit.  For the polarised route the alternative without the kernel is timed too
(--no-host skips it): psrfits.unpack_host_pol of the same bytes on the host
plus the upload of its float32 rows (no baseline, no statistics).  Needs a
HIP device.

  python tools/unpack_bench.py --out unpack.json
  PPFIT_LIB=/other/build/libppfit.so python tools/unpack_bench.py --no-host

profiles/unpack.json holds such runs in fresh processes, alternating this
library and its parent commit's: per-round medians, spreads and digests.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from pulseportraiture_amd import engine, psrfits  # noqa: E402

HBM_PEAK_GBS = 8000.0
CONV = 2
KEYS = ("rows", "stats", "total", "wstart")
# route -> (polarisation blocks read, rows written per channel)
ROUTES = {"npol1": (1, 1), "aabb": (2, 1), "pol": (4, 4)}


def _call(route, raw, nchan, nbin, scl, offs, wts, rm):
    if route == "pol":
        return engine.unpack_psrfits_pol(raw, 0, nchan, nbin, scl, offs,
                                         wts=wts, conv=CONV, rm_baseline=rm)
    npol = ROUTES[route][0]
    return engine.unpack_psrfits(raw, 0, npol, nchan, nbin, scl, offs,
                                 wts=wts, pol_mode=npol - 1, rm_baseline=rm)


def _digest(res):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(res[k].cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x512x2048,1x512x2048")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true",
                    help="skip the host unpack + upload comparison")
    ap.add_argument("--out", default=None, help="JSON result file")
    a = ap.parse_args()
    dev = engine.device(None)
    out = []
    for shape in a.shapes.split(","):
        nsub, nchan, nbin = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        raw4 = torch.randint(0, 256, (nsub, 4 * nchan * nbin * 2),
                             generator=g, device=dev, dtype=torch.uint8)
        scl4 = torch.rand((nsub, 4 * nchan), generator=g, device=dev) + 0.5
        offs4 = torch.rand((nsub, 4 * nchan), generator=g, device=dev) * 40
        wts = torch.ones((nsub, nchan), device=dev)
        routes = {}
        for route, (nread, nrows) in ROUTES.items():
            n = nread * nchan * nbin * 2
            raw = raw4[:, :n].contiguous()
            padded = torch.empty((nsub, n + 2), dtype=torch.uint8, device=dev)
            padded[:, :n] = raw
            padded = padded[:, :n]            # stride n + 2: no 8-byte loads
            scl = scl4[:, :nread * nchan].contiguous()
            offs = offs4[:, :nread * nchan].contiguous()

            def events(r):
                ev, res = [], None
                for _ in range(a.runs + 1):          # run 0 warms up
                    e0, e1 = torch.cuda.Event(enable_timing=True), \
                        torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = _call(route, r, nchan, nbin, scl, offs, wts, True)
                    e1.record()
                    e1.synchronize()
                    ev.append(e0.elapsed_time(e1))
                return ev[1:], res

            sha = {}
            t_vec, r_vec = events(raw)
            t_sca, r_sca = events(padded)
            same = all(bool(torch.equal(r_vec[k], r_sca[k])) for k in KEYS)
            sha["as_stored"] = dict(rm_baseline=_digest(r_vec))
            sha["padded"] = dict(rm_baseline=_digest(r_sca))
            del r_vec, r_sca
            # (the rows above had their baseline removed: fresh calls)
            keep = _call(route, raw, nchan, nbin, scl, offs, wts, False)
            sha["as_stored"]["keep_baseline"] = _digest(keep)
            sha["padded"]["keep_baseline"] = _digest(
                _call(route, padded, nchan, nbin, scl, offs, wts, False))
            samples = nsub * nchan * nbin
            nbytes = samples * (2 * nread + 4 * nrows)
            ms_v, ms_s = float(np.median(t_vec)), float(np.median(t_sca))
            routes[route] = res = dict(
                unpack_ms=dict(median=ms_v, runs=t_vec),
                unpack_gbytes_per_s=nbytes / ms_v / 1e6,
                share_of_hbm_peak=nbytes / ms_v / 1e6 / HBM_PEAK_GBS,
                element_wide_ms=dict(median=ms_s, runs=t_sca),
                element_wide_gbytes_per_s=nbytes / ms_s / 1e6,
                vector_over_element_wide=ms_s / ms_v,
                outputs_identical=same, sha256=sha)
            if route != "pol" or a.no_host:
                continue
            # the route without the kernel: unpack on the host, upload the rows
            raw_h = raw.cpu().numpy()
            scl_h, offs_h = scl.cpu().numpy(), offs.cpu().numpy()
            t_host, rows_h = [], None
            for _ in range(2 if nsub > 8 else a.runs + 1):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                rows_h = psrfits.unpack_host_pol(raw_h, ">i2", scl_h, offs_h,
                                                 nchan, nbin, CONV)
                up = torch.from_numpy(rows_h).to(dev)
                torch.cuda.synchronize(dev)
                t_host.append(time.perf_counter() - t0)
            t_host = t_host[1:]
            res.update(
                host_unpack_upload_s=dict(median=float(np.median(t_host)),
                                          runs=t_host),
                host_rows_identical=bool(torch.equal(
                    keep["rows"].view(torch.int32), up.view(torch.int32))),
                host_over_device=float(np.median(t_host)) / (ms_v / 1e3))
            del up, keep
        out.append(dict(shape=dict(nsub=nsub, nchan=nchan, nbin=nbin,
                                   elem="int16", conv=CONV), routes=routes))
    res = dict(device=torch.cuda.get_device_name(dev), runs=a.runs,
               hbm_peak_gbytes_per_s=HBM_PEAK_GBS, shapes=out)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
