"""Cases, inputs and error bars of the likelihood-evaluator tests (TEST
INFRASTRUCTURE; no reference import): tests/golden/make_golden_eval.py builds
the inputs here, hands them to the REFERENCE and stores its outputs in
tests/golden/eval.npz with a SHA-256 of the inputs; tests/test_eval_host.py
and tests/test_gpu_eval.py rebuild the same inputs here and check the hash
(tests/golden/synth_np.py explains the scheme).

Error bars.  Every per-channel term of the likelihood is a harmonic sum; its
"absolute companion" is the same sum with the modulus of each harmonic's term
(C^ = sum_k |X_k conj(B_k)| / sigma^2, ...): the modulus of the COMPLEX
product whose real part the reference sums, for the S family as for the C
family (dS^ = sum_k 2 |B_k| |dB_k| |M_k|^2 / sigma^2, not the modulus of
Re(B conj(dB)), which cancels to O(u^2) of it at small u = 2 pi k tau_n: the
rounding of a real part is that of the product).  A term may differ from the
reference's by BAR_EPS * eps * companion: the device's phasor recurrence adds
up to 64 complex multiplications' rounding per harmonic, which NumPy's direct
exp does not have.  f, g and H are sums over channels of products
T = coef * prod_j r_j^p_j of those terms; first-order propagation gives them
the scale sum |T| sum_j |p_j| r^_j / |r_j| (net powers, the form without a
division by C), and the bar BAR_EPS * eps * scale.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import synth_np as S  # noqa: E402

EPS = np.finfo(np.float64).eps
BAR_EPS = 256.0
LN10 = np.log(10.0)
DCONST = S.DCONST
GOLDEN = os.path.join(HERE, "golden", "eval.npz")

# (nchan, nharm): 64-harmonic groups (17, 33, 65, 130), the 1024-harmonic LDS
# tile (1024 exactly, 1025 straddling it, 4100 over five tiles), one channel,
# channel counts around 64
SHAPES = [(1, 17), (3, 17), (64, 33), (65, 33), (67, 65), (5, 130), (16, 1025),
          (2, 4100), (4, 1024)]
KEEP_DC = {(3, 17)}          # harmonic 0 summed as given (not zeroed)
PER_CHANNEL_H = {(1, 17), (3, 17), (5, 130), (2, 4100)}   # H_n stored
WITH_SCALES = (3, 17)
FLAGS_A = (1, 1, 1, 1, 1)
FLAGS_B = (1, 1, 0, 1, 0)
# the three problems of the batched case (6 channels, 65 harmonics): their
# own P, bands and reference frequencies; problems 0 and 2 share model 0;
# problem 1 keeps one channel, problem 2 loses two
BATCH = dict(nchan=6, nharm=65, model_index=[0, 1, 0],
             mask=[[1, 1, 1, 1, 1, 1], [0, 0, 0, 1, 0, 0], [1, 0, 1, 1, 0, 1]],
             lo=[1100.0, 1150.0, 1210.0], bw=[800.0, 700.0, 500.0],
             nus=[[1480.3, 1455.7, 1437.9], [1391.2, 1502.6, 1377.1],
                  [1462.9, 1411.3, 1530.4]],
             Pfac=[1.0, 1.37, 0.81])


def case_name(nchan, nharm):
    return "c%dx%d" % (nchan, nharm)


def _problem(seed, nchan, nharm, lo, bw, nus, Pfac, keep_dc, model=None):
    nbin = 2 * (nharm - 1)
    rng = np.random.default_rng(20261021 + seed)
    phi = rng.uniform(-0.3, 0.3)
    # a dedispersed sub-integration: k phi_n multiplies every rounding of
    # phi_n, the reference's own included, so phi_n stays within a turn at
    # the near points
    DM = 0.05 + rng.normal(3e-4, 2e-4)
    tau, alpha = 0.012, -4.0
    P = S.P0 * Pfac
    tmpl, freqs = S.template(nchan, nbin, lo=lo, bw=bw)
    if model is None:
        model = tmpl
    data = S.subint(seed, model, freqs, phi, DM, P, tau=tau, alpha=alpha)
    D = np.fft.rfft(data, axis=-1)
    M = np.fft.rfft(model, axis=-1)
    if not keep_dc:
        D[:, 0] = 0.0
        M[:, 0] = 0.0
    F = np.fft.rfft(data, axis=-1)
    pows = (F.real ** 2 + F.imag ** 2) / nbin
    kc = int(0.75 * pows.shape[-1])
    errs_FT = np.sqrt(pows[:, kc:].mean(axis=-1)) * np.sqrt(nbin / 2.0)
    nu_DM, nu_GM, nu_tau = nus
    # the generating parameters in the frame of the reference frequencies
    truth = np.array([
        phi + DCONST * DM * (nu_DM ** -2 - 1500.0 ** -2) / P, DM, 0.0,
        tau * (nu_tau / 1500.0) ** alpha, alpha])
    return dict(D=D, M=M, errs_FT=errs_FT, P=P, freqs=freqs,
                nus=np.array(nus, dtype=float), truth=truth, model=model)


def inputs(nchan, nharm):
    """One problem of a shape: spectra [nchan, nharm], errs_FT, P, freqs,
    nus = (nu_DM, nu_GM, nu_tau) (off every channel frequency), truth."""
    return _problem(1000 * nchan + nharm, nchan, nharm, 1100.0, 800.0,
                    (1480.3, 1455.7, 1437.9), 1.0,
                    (nchan, nharm) in KEEP_DC)


def batch_inputs():
    """The three problems of BATCH; problem 2 is built on problem 0's model
    (their shared model 0).  Returns (list of problems, models [2, ...])."""
    b = BATCH
    probs = []
    for s in range(3):
        shared = probs[0]["model"] if b["model_index"][s] == 0 and s else None
        probs.append(_problem(7000 + s, b["nchan"], b["nharm"], b["lo"][s],
                              b["bw"][s], b["nus"][s], b["Pfac"][s], False,
                              model=shared))
    models = np.array([probs[0]["M"], probs[1]["M"]])
    return probs, models


def input_sha(p):
    return S.sha(p["D"], p["M"], p["errs_FT"], p["freqs"], p["nus"],
                 np.float64(p["P"]))


def make_points(truth, sig, seed):
    """theta of the log10-tau points [7, 5] (three near: within 2 sigma of
    the generating parameters; four far) and of the linear-tau points
    [4, 5] (near, far, and two with tau = 0)."""
    rng = np.random.default_rng(555 + seed)
    cap = np.array([0.01, 1e-3, 5.0, 0.1, 0.3])
    lt = truth.copy()
    lt[3] = np.log10(truth[3])
    near = [lt + np.clip(rng.normal(size=5) * 2.0 * sig, -cap, cap)
            for _ in range(3)]
    far = [lt + np.array([0.45, 4.0, 0.0, 0.0, -0.4]),
           lt + np.array([-0.45, -3.0, 30.0, 0.0, 2.0]),
           lt + np.array([0.2, 0.5, -20.0, 0.0, -1.0]),
           lt + np.array([-0.31, -5.0, 0.0, 0.0, 0.9])]
    for p, tau in zip(far, (1e-4, 0.3, 0.03, 3e-3)):
        p[3] = np.log10(tau)
    log_pts = np.array(near + far)
    lin = log_pts[[0, 4, 1, 6]].copy()
    lin[:2, 3] = 10.0 ** lin[:2, 3]
    lin[2:, 3] = 0.0
    return log_pts, lin


# ---------------------------------------------------------------------------
# the 27 distinct per-channel terms, packed [27, nchan]
# ---------------------------------------------------------------------------
UPPER = [(i, j) for i in range(5) for j in range(i, 5)]
PACK = ([("C",)] + [("dC", i) for i in range(5)] +
        [("d2C", i, j) for i, j in UPPER] + [("S",), ("dS", 3), ("dS", 4),
                                            ("d2S", 3, 3), ("d2S", 3, 4),
                                            ("d2S", 4, 4)])
assert len(PACK) == 27


def pack_terms(t):
    return np.array([t[k[0]][k[1:]] if len(k) > 1 else t[k[0]] for k in PACK])


def unpack_terms(a):
    """[27, nchan] -> dict in oracle.channel_terms' layout."""
    n = a.shape[-1]
    t = dict(C=a[0], S=a[21], dC=np.zeros((5, n)), dS=np.zeros((5, n)),
             d2C=np.zeros((5, 5, n)), d2S=np.zeros((5, 5, n)))
    for row, k in zip(a, PACK):
        if len(k) == 2:
            t[k[0]][k[1]] = row
        elif len(k) == 3:
            t[k[0]][k[1], k[2]] = t[k[0]][k[2], k[1]] = row
    return t


def companions(theta, D, M, errs_FT, P, freqs, nu_DM, nu_GM, nu_tau,
               log10_tau):
    """The absolute companions of oracle.channel_terms' outputs (same
    layout): every harmonic sum with the modulus of each harmonic's term."""
    phi, DM, GM, tau, alpha = theta
    if log10_tau:
        tau = 10 ** tau
    nchan, nharm = D.shape
    k = np.arange(nharm)
    e2 = errs_FT ** 2
    dphi = np.array([np.ones(nchan), DCONST * (freqs ** -2 - nu_DM ** -2) / P,
                     DCONST ** 2 * (freqs ** -4 - nu_GM ** -4) / P])
    taus = tau * (freqs / nu_tau) ** alpha
    lnf = np.log(freqs / nu_tau)
    B = 1.0 / (1.0 + 2j * np.pi * np.outer(taus, k))
    if tau == 0.0:
        c = np.zeros((2, nchan))
        e = np.zeros((2, 2, nchan))
    elif log10_tau:
        c = np.array([np.full(nchan, LN10), lnf])
        e = np.array([[np.full(nchan, LN10 ** 2), LN10 * lnf],
                      [LN10 * lnf, lnf ** 2]])
    else:
        c = np.array([np.full(nchan, 1.0 / tau), lnf])
        e = np.array([[np.zeros(nchan), lnf / tau], [lnf / tau, lnf ** 2]])
    BB1 = B * (B - 1.0)
    dB = [BB1 * c[j][:, None] for j in range(2)]
    d2B = [[BB1 * (2.0 * (c[i] * c[j])[:, None] * (B - 1.0) +
                   e[i, j][:, None]) for j in range(2)] for i in range(2)]
    X = D * np.conj(M)
    M2 = np.abs(M) ** 2
    w1 = 2.0 * np.pi * k

    def asum(a):
        return np.abs(a).sum(axis=-1) / e2

    t = dict(C=asum(X * np.conj(B)), S=asum(np.abs(B) ** 2 * M2),
             dC=np.zeros((5, nchan)), dS=np.zeros((5, nchan)),
             d2C=np.zeros((5, 5, nchan)), d2S=np.zeros((5, 5, nchan)))
    Cp, Cpp = asum(w1 * X * np.conj(B)), asum(w1 ** 2 * X * np.conj(B))
    for i in range(3):
        t["dC"][i] = Cp * np.abs(dphi[i])
        for j in range(3):
            t["d2C"][i, j] = Cpp * np.abs(dphi[i] * dphi[j])
    for j in range(2):
        t["dC"][3 + j] = asum(X * np.conj(dB[j]))
        t["dS"][3 + j] = asum(2 * np.abs(B) * np.abs(dB[j]) * M2)
        cross = asum(w1 * X * np.conj(dB[j]))
        for i in range(3):
            t["d2C"][i, 3 + j] = t["d2C"][3 + j, i] = np.abs(dphi[i]) * cross
        for i in range(2):
            t["d2C"][3 + i, 3 + j] = asum(X * np.conj(d2B[i][j]))
            t["d2S"][3 + i, 3 + j] = asum(
                2 * (np.abs(dB[i]) * np.abs(dB[j]) +
                     np.abs(B) * np.abs(d2B[i][j])) * M2)
    return t


def _prop(coef, factors):
    """First-order scale of coef * prod r^p per channel: factors is a list
    of (r, rhat, p); sum_j |p_j| rhat_j |T / r_j| without dividing by r_j."""
    out = 0.0
    for j, (_, rh, p) in enumerate(factors):
        prod = abs(coef) * abs(p) * rh
        for l, (r, _, q) in enumerate(factors):
            prod = prod * np.abs(r) ** (q - 1 if l == j else q)
        out = out + prod
    return out


def scales(t, h, flags=FLAGS_A, per_channel=False):
    """Scales of f, g [5] and H [5, 5] (summed over channels unless
    per_channel) from the terms t and their companions h."""
    fl = np.asarray(flags, dtype=float)
    C, S = (t["C"], h["C"]), (t["S"], h["S"])
    red = (lambda x: x) if per_channel else (lambda x: np.sum(x, axis=-1))
    sf = red(_prop(1.0, [C + (2,), S + (-1,)]))
    sg, sH = [], np.zeros((5, 5) + (np.shape(t["C"]) if per_channel else ()))
    dC = [(t["dC"][i], h["dC"][i]) for i in range(5)]
    dS = [(t["dS"][i], h["dS"][i]) for i in range(5)]
    for i in range(5):
        sg.append(red(_prop(2.0, [C + (1,), dC[i] + (1,), S + (-1,)]) +
                      _prop(1.0, [C + (2,), dS[i] + (1,), S + (-2,)])) *
                  abs(fl[i]))
        for j in range(5):
            d2C = (t["d2C"][i, j], h["d2C"][i, j])
            d2S = (t["d2S"][i, j], h["d2S"][i, j])
            s = (_prop(1.0, [C + (1,), d2C + (1,), S + (-1,)]) +
                 _prop(0.5, [C + (2,), d2S + (1,), S + (-2,)]) +
                 _prop(1.0, [dC[i] + (1,), dC[j] + (1,), S + (-1,)]) +
                 _prop(1.0, [C + (2,), dS[i] + (1,), dS[j] + (1,),
                             S + (-3,)]) +
                 _prop(1.0, [C + (1,), dC[i] + (1,), dS[j] + (1,),
                             S + (-2,)]) +
                 _prop(1.0, [C + (1,), dS[i] + (1,), dC[j] + (1,),
                             S + (-2,)]))
            sH[i, j] = red(2.0 * s) * abs(fl[i] * fl[j])
    return sf, np.array(sg), sH


def ratio(got, ref, scale):
    """max |got - ref| / (eps * scale); a zero scale demands equality."""
    got, ref, scale = np.broadcast_arrays(np.asarray(got, dtype=float),
                                          np.asarray(ref, dtype=float),
                                          np.asarray(scale, dtype=float))
    err = np.abs(got - ref)
    if not np.all(np.isfinite(got)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / (EPS * scale),
                     np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def terms_ratio(got, ref_packed, hat_packed):
    """The largest error / (eps * companion) over the 27 packed terms of a
    channel-terms dict `got` against the golden's packed arrays."""
    return ratio(pack_terms(got), ref_packed, hat_packed)


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN
