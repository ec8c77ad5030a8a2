"""Time pplib.smart_smooth on cuda:0 with search="brute" (the reference's
road: scipy.optimize.brute per (profile, level), its fmin finish one
evaluator call per evaluation) and search="batched" (k_swt_search: every
finish in one launch) at 64 x 512 and 512 x 2048, by the wall clock around
the call after one warm-up call on four rows.  The brute road is timed on
the first BRUTE_ROWS rows only and scaled by nrow / BRUTE_ROWS (it is a
serial loop over rows; `brute_rows_timed` says how many were run).  Recorded
per shape: wall seconds, evaluator calls (analyse, score, search), the
nfev of the finishes (min / median / max) and whether the two roads gave the
same rows.  Written to profiles/smart_smooth.json.
usage: python tools/smooth_time.py [--out FILE] [--no-write]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pulseportraiture_amd import engine, pplib  # noqa: E402

SHAPES = [(64, 512), (512, 2048)]
BRUTE_ROWS = 32


def portrait(nrow, nbin, seed=1):
    """A two-component pulse whose S/N falls from ~200 to ~5 down the rows."""
    rng = np.random.default_rng(seed)
    x = (np.arange(nbin) + 0.5) / nbin
    prof = np.exp(-0.5 * ((x - 0.4) / 0.01) ** 2) + \
        0.3 * np.exp(-0.5 * ((x - 0.55) / 0.04) ** 2)
    noise = np.geomspace(0.005, 0.2, nrow)[:, None]
    return prof + noise * rng.standard_normal((nrow, nbin))


class Counting(engine.SwtEvaluator):
    """The device evaluator, its calls counted."""

    def __init__(self):
        engine.SwtEvaluator.__init__(self)
        self.calls = dict(analyse=0, score=0, search=0)
        self.nfev = None

    def analyse(self, *a, **k):
        self.calls["analyse"] += 1
        return engine.SwtEvaluator.analyse(self, *a, **k)

    def score(self, *a, **k):
        self.calls["score"] += 1
        return engine.SwtEvaluator.score(self, *a, **k)

    def search(self, *a, **k):
        self.calls["search"] += 1
        out = engine.SwtEvaluator.search(self, *a, **k)
        self.nfev = out[2]
        return out


def run(port, search):
    ev = Counting()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pplib.smart_smooth(port, search=search, evaluator=ev)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ev, out


def main():
    out = dict(device=torch.cuda.get_device_name(engine.device()),
               brute_rows=BRUTE_ROWS, shapes=[])
    for nrow, nbin in SHAPES:
        port = portrait(nrow, nbin)
        for search in ("brute", "batched"):
            run(port[:4], search)                       # warm-up
        tb, evb, sb = run(port, "batched")
        nb = min(nrow, BRUTE_ROWS)
        tr, evr, sr = run(port[:nb], "brute")
        nfev = evb.nfev
        out["shapes"].append(dict(
            nrow=nrow, nbin=nbin, nlevel=int(nfev.shape[1]),
            batched_s=tb, batched_calls=evb.calls,
            brute_rows_timed=nb, brute_timed_s=tr,
            brute_s=tr * nrow / nb, brute_scaled=nb != nrow,
            brute_calls_timed=evr.calls,
            brute_over_batched=tr * nrow / nb / tb,
            nfev=dict(min=int(nfev.min()), median=float(np.median(nfev)),
                      max=int(nfev.max())),
            same_rows=bool(np.array_equal(sb[:nb], sr)),
            rows_kept=int(sb.any(axis=1).sum())))
        print(json.dumps(out["shapes"][-1]), flush=True)
    if "--no-write" not in sys.argv:
        fn = os.path.join(ROOT, "profiles", "smart_smooth.json")
        if "--out" in sys.argv:
            fn = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(fn)), exist_ok=True)
        with open(fn, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
