#!/usr/bin/env python
"""Time digitising device rows for a PSRFITS file: engine.pack_rows (16-bit
samples made on the device, 2 bytes per sample over PCIe) against the route
that preceded it (download the float rows, psrfits.quantize on the host), as
tools/fake_bench.py does for k_fake.

Both routes start from the same float rows in device memory (--dtype) and
end with the file's DATA bytes, DAT_SCL and DAT_OFFS in host memory; the
figure of a route is the median of --runs calls after one warm-up call, each
ending in a device synchronise.  The kernels' own time is taken with events
around engine.pack_rows.  --shapes lists nsub x nchan x nbin archives: a large
one and a single portrait by default.  Needs a HIP device.

  python tools/pack_bench.py --out profiles/pack.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x512x2048,1x512x2048,1x64x256")
    ap.add_argument("--dtype", default="float64",
                    choices=["float32", "float64"])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="JSON result file")
    a = ap.parse_args()
    dev = engine.device(None)
    dt = getattr(torch, a.dtype)
    out = []
    for shape in a.shapes.split(","):
        nsub, nchan, nbin = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        rows = torch.randn((nsub, 1, nchan, nbin), generator=g, device=dev,
                           dtype=dt) * 3.0 + 7.0

        def device_route():
            raw, scl, offs = engine.pack_rows(rows)
            s, o = engine.dev_to_host(scl), engine.dev_to_host(offs)
            return engine.dev_to_host_view(raw), s, o

        def host_route():
            q, s, o = psrfits.quantize(engine.dev_to_host(rows))
            return q.astype(">i2").view(np.uint8), s, o

        def timed(fn):
            t = []
            for r in range(a.runs + 1):          # run 0 warms up
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = fn()
                torch.cuda.synchronize(dev)
                t.append(time.perf_counter() - t0)
            return t[1:], res

        t_dev, rd = timed(device_route)
        rd = tuple(np.array(v) for v in rd)      # (the view is reused)
        t_host, rh = timed(host_route)
        same = bool(np.array_equal(rd[0].reshape(-1), rh[0].reshape(-1)) and
                    np.array_equal(rd[1].reshape(-1), rh[1].reshape(-1)) and
                    np.array_equal(rd[2].reshape(-1), rh[2].reshape(-1)))
        ev = []
        for r in range(a.runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), \
                torch.cuda.Event(enable_timing=True)
            e0.record()
            res = engine.pack_rows(rows)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
            del res
        samples = nsub * nchan * nbin
        k_ms = float(np.median(ev[1:]))
        # the kernel reads every row twice and writes 2 bytes per sample
        nbytes = samples * (2 * rows.element_size() + 2)
        out.append(dict(
            shape=dict(nsub=nsub, nchan=nchan, nbin=nbin, dtype=a.dtype),
            pack_rows_download_s=dict(median=float(np.median(t_dev)),
                                      runs=t_dev),
            download_quantize_s=dict(median=float(np.median(t_host)),
                                     runs=t_host),
            speedup=float(np.median(t_host) / np.median(t_dev)),
            outputs_identical=same,
            pack_rows_ms=dict(median=k_ms, runs=ev[1:]),
            pack_rows_gsamples_per_s=float(samples / k_ms / 1e6),
            pack_rows_gbytes_per_s=float(nbytes / k_ms / 1e6),
            bytes_over_pcie_per_sample=dict(pack_rows=2,
                                            download_quantize=rows.element_size())))
    res = dict(device=torch.cuda.get_device_name(dev), runs=a.runs,
               shapes=out)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
