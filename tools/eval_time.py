"""Time the many-point likelihood evaluator (engine.eval_points,
ppf_eval_batch) on cuda:0 and measure its accuracy against the goldens.

Times, by HIP events around the call on device-resident inputs (one warm-up,
then the median of 5 with min-max), at 64 x 512 spectra (nharm 257) and
512 x 2048 (nharm 1025), K = 1, 64 and 4096 points, order 0 and order 2; the
same K = 4096 as 4096 one-point calls (the only other route to the result on
the device) and the ratio; the fp64 operations per (point, channel, harmonic)
counted from k_eval's source (an fma as 2) over the time, against the fp64
vector peak bench.py's solver_fp64 line uses.
Accuracy: the largest error / (eps * scale) over every case and point of
tests/golden/eval.npz, for the oracle (host) and for the device.
Writes profiles/eval.json and prints it as one JSON line.
usage: python tools/eval_time.py [--small] [--out FILE]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pulseportraiture_amd import engine, pptoaslib  # noqa: E402

FP64_PEAK_TF = 78.6          # bench.py FP64_PEAK_TF
# k_eval's harmonic loop body, counted from the source (fma = 2): X E 6, u
# u^2 1 + u^2 3, 1 / den 9 (rcp + two Newton steps), u d 1, z1 6, a0 1, s0 2,
# phasor step 6 = 34 at order 0; order 2 adds z2 6, tp 3, a1 2, q1 2, t1 1,
# z3 3, a2 3, q1p 3, q2 2, t2 4 = 63
FLOPS = {0: 34, 2: 63}


def stats(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()),
                max=float(v.max()))


def problem(nchan, nharm, K, dev):
    rng = np.random.default_rng(nchan + K)
    c128 = torch.complex128
    D = torch.as_tensor(rng.normal(size=(1, nchan, nharm)) +
                        1j * rng.normal(size=(1, nchan, nharm)),
                        dtype=c128).to(dev)
    M = torch.as_tensor(rng.normal(size=(1, nchan, nharm)) +
                        1j * rng.normal(size=(1, nchan, nharm)),
                        dtype=c128).to(dev)
    cw = 800.0 / nchan
    freqs = torch.as_tensor(np.linspace(1100 + cw / 2, 1900 - cw / 2, nchan),
                            dtype=torch.float64).to(dev)
    errs = torch.ones(nchan, dtype=torch.float64, device=dev)
    th = np.zeros((1, K, 5))
    th[0, :, 0] = rng.uniform(-0.5, 0.5, K)
    th[0, :, 1] = rng.normal(0, 1e-2, K)
    th[0, :, 3] = rng.uniform(-3, -1.5, K)
    th[0, :, 4] = rng.uniform(-5, -3, K)
    th = torch.as_tensor(th).to(dev)
    P = torch.tensor([2.9e-3], dtype=torch.float64, device=dev)
    nus = torch.tensor([1480.3, 1455.7, 1437.9], dtype=torch.float64,
                       device=dev)
    return th, D, M, errs, P, freqs, nus


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def times(small):
    dev = engine.device()
    rows = []
    shapes = [(64, 257)] if small else [(64, 257), (512, 1025)]
    for nchan, nharm in shapes:
        for order in (0, 2):
            for K in (1, 64, 4096):
                a = problem(nchan, nharm, K, dev)
                t = timed(lambda: engine.eval_points(*a, order=order))
                fl = FLOPS[order] * K * nchan * nharm
                tf = fl / (t["median"] * 1e-3) / 1e12
                row = dict(nchan=nchan, nharm=nharm, K=K, order=order, ms=t,
                           flops_per_point_channel_harmonic=FLOPS[order],
                           achieved_tflops=round(tf, 3),
                           fp64_frac=round(tf / FP64_PEAK_TF, 4))
                if K == 4096:
                    th = a[0]
                    one = [th[:, i:i + 1].contiguous() for i in range(K)]

                    def loop():
                        for x in one:
                            engine.eval_points(x, *a[1:], order=order)
                    t1 = timed(loop, reps=3)
                    row["one_point_calls_ms"] = t1
                    row["batched_speedup"] = round(t1["median"] / t["median"],
                                                   1)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
    return rows


def accuracy():
    import evalcases as E
    import oracle as O
    G = E.golden()
    out = dict(oracle=dict(terms=0.0, fgH=0.0), device=dict(terms=0.0,
                                                            fgH=0.0))
    for shape in E.SHAPES:
        p = E.inputs(*shape)
        a = (p["D"], p["M"], p["errs_FT"], p["P"], p["freqs"]) + \
            tuple(p["nus"])
        name = E.case_name(*shape)
        for mode, lt in (("log", True), ("lin", False)):
            pre = "%s/%s/" % (name, mode)
            th = G[pre + "theta"]
            d = pptoaslib.eval_portrait_full(th, *a, log10_tau=lt,
                                             per_channel=True)
            for i, x in enumerate(th):
                to = O.channel_terms(x, *a, lt)
                td = {k: v[i] for k, v in d.terms.items()}
                for who, t, f, g, H in (
                        ("oracle", to, O.objective(to),
                         O.gradient(to, E.FLAGS_A), O.hessian(to, E.FLAGS_A)),
                        ("device", td, d.f[i], d.grad[i], d.hess[i])):
                    o = out[who]
                    o["terms"] = max(o["terms"], E.terms_ratio(
                        t, G[pre + "terms"][i], G[pre + "hat"][i]))
                    o["fgH"] = max(o["fgH"],
                                   E.ratio(f, G[pre + "f"][i], G[pre + "sf"][i]),
                                   E.ratio(g, G[pre + "g"][i], G[pre + "sg"][i]),
                                   E.ratio(H, G[pre + "H"][i], G[pre + "sH"][i]))
    for o in out.values():
        for k in o:
            o[k] = round(o[k], 1)
    out["unit"] = "largest error / (eps * scale); bar 256"
    return out


def main():
    small = "--small" in sys.argv
    res = dict(device=torch.cuda.get_device_name(0), note="one MI355X, one run",
               point_block=engine.eval_point_block(), accuracy=accuracy(),
               times=times(small))
    if not small:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "eval.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if "--out" in sys.argv:                 # a second copy, e.g. off the box
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
