#!/usr/bin/env python
"""Time the full-polarisation PSRFITS unpack on the device:
engine.unpack_psrfits_pol (k_unpack_pol, k_base_window, k_row_stats over four
polarisations) on 16-bit samples, Coherence -> Stokes (conv 2), as
tools/pack_bench.py does for the pack kernel.

Per shape (nsub x 4 x nchan x nbin): the device-event time of one call, the
median and all of --runs calls after one warm-up, for the shape as it is (4
bins per lane: 8-byte loads, 16-byte stores) and for the same samples behind a
sub_stride padded by 2 bytes (element-wide accesses), with the outputs of the
two compared bitwise.  GB/s counts the 8 bytes read and 16 written per sample
of k_unpack_pol's own traffic over the whole call's time (the statistics pass
reads the rows again, and writes them with rm_baseline: not counted), beside
the share of the HBM peak (8 TB/s nominal).  The alternative without the
kernel is timed too: psrfits.unpack_host_pol of the same bytes on the host
plus the upload of its float32 rows (no baseline, no statistics).  Needs a
HIP device.

  python tools/unpack_pol_bench.py --out profiles/unpack_pol.json
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x512x2048,1x512x2048")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="JSON result file")
    a = ap.parse_args()
    dev = engine.device(None)
    out = []
    for shape in a.shapes.split(","):
        nsub, nchan, nbin = (int(v) for v in shape.split("x"))
        n = 4 * nchan * nbin * 2
        g = torch.Generator(device=dev).manual_seed(1)
        raw = torch.randint(0, 256, (nsub, n), generator=g, device=dev,
                            dtype=torch.uint8)
        padded = torch.empty((nsub, n + 2), dtype=torch.uint8, device=dev)
        padded[:, :n] = raw
        padded = padded[:, :n]                # stride n + 2: no 8-byte loads
        scl = torch.rand((nsub, 4 * nchan), generator=g, device=dev) + 0.5
        offs = torch.rand((nsub, 4 * nchan), generator=g, device=dev) * 40
        wts = torch.ones((nsub, nchan), device=dev)

        def events(r):
            ev, res = [], None
            for _ in range(a.runs + 1):          # run 0 warms up
                e0, e1 = torch.cuda.Event(enable_timing=True), \
                    torch.cuda.Event(enable_timing=True)
                e0.record()
                res = engine.unpack_psrfits_pol(r, 0, nchan, nbin, scl, offs,
                                                wts=wts, conv=CONV,
                                                rm_baseline=True)
                e1.record()
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
            return ev[1:], res

        t_vec, r_vec = events(raw)
        t_sca, r_sca = events(padded)
        same = all(bool(torch.equal(r_vec[k], r_sca[k]))
                   for k in ("rows", "stats", "total", "wstart"))
        del r_sca
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
        # (the device rows had their baseline removed: compare a fresh call)
        keep = engine.unpack_psrfits_pol(raw, 0, nchan, nbin, scl, offs,
                                         wts=wts, conv=CONV,
                                         rm_baseline=False)["rows"]
        host_same = bool(torch.equal(keep.view(torch.int32),
                                     up.view(torch.int32)))
        del up, keep, r_vec
        samples = nsub * nchan * nbin            # per polarisation block: x 4
        nbytes = 4 * samples * (2 + 4)           # 8 B read + 16 B written
        ms_v, ms_s = float(np.median(t_vec)), float(np.median(t_sca))
        out.append(dict(
            shape=dict(nsub=nsub, npol=4, nchan=nchan, nbin=nbin,
                       elem="int16", conv=CONV),
            unpack_pol_ms=dict(median=ms_v, runs=t_vec),
            unpack_pol_gbytes_per_s=nbytes / ms_v / 1e6,
            share_of_hbm_peak=nbytes / ms_v / 1e6 / HBM_PEAK_GBS,
            element_wide_ms=dict(median=ms_s, runs=t_sca),
            element_wide_gbytes_per_s=nbytes / ms_s / 1e6,
            vector_over_element_wide=ms_s / ms_v,
            outputs_identical=same,
            host_unpack_upload_s=dict(median=float(np.median(t_host)),
                                      runs=t_host),
            host_rows_identical=host_same,
            host_over_device=float(np.median(t_host)) / (ms_v / 1e3)))
    res = dict(device=torch.cuda.get_device_name(dev), runs=a.runs,
               hbm_peak_gbytes_per_s=HBM_PEAK_GBS, shapes=out)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
