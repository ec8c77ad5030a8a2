"""Degenerate sub-integrations and poisoned masked channels for every fit
kernel family (TEST INFRASTRUCTURE; no pytest hooks).

include/ppfit.h promises that a per-sub-int numerical outcome is reported in
ppf_result.status and never aborts the batch, that a masked channel's values
reach no result, and (engine.fit_batch) that a sub-int's result does not
depend on the batch it is in.  The inputs here put those promises in front
of each family of tests/ragged.py:

  poisoned(c, v)    the case's batch of four with NaN / +-Inf / a huge finite
                    constant in every masked channel's data row, errs and
                    guess weight: the tables must be bitwise the clean call's;
  degenerate(c)     the case's four sub-ints between five degenerate copies
                    of the first: no usable channel (E, E2: also all-NaN
                    data), nothing to fit (F), one NaN sample (N), a channel
                    of zero noise (Z);
  minimal(name)     one usable channel fitted for the phase, two for phase
                    and DM, against the oracle.

Inputs are built on the host only, as in tests/ragged.py;
tests/test_degenerate_inputs.py checks them there,
tests/test_gpu_degenerate.py runs them on the device."""
import functools

import numpy as np

import ragged as R

TABLES = ("results", "scales", "scale_errs", "channel_snrs", "covariance")
PER_CHANNEL = ("scales", "scale_errs", "channel_snrs")

# ---------------------------------------------------------------------------
# A. poisoned masked channels
# ---------------------------------------------------------------------------
VARIANTS = (1, 2, 3)


def huge(c):
    """Variant 3's finite constant: near the top of the rows' number
    format, so that a sum over every row that subtracts the masked ones
    afterwards overflows or loses every digit."""
    return 3e38 if c["dtype"] == "f32" else 1e300


def poisoned(c, variant):
    """The override (ragged.device_fit's `over`) that poisons every masked
    channel of the case's batch: the data row (1: all NaN; 2: +Inf in the
    first bin, -Inf in the last, NaN at nbin // 2; 3: huge(c) everywhere),
    errs where the case gives them (NaN; 0.0 in variants 2 and 3) and the
    guess weight where the case has a guess (NaN in variant 1, else the 0
    it has anyway)."""
    b = R.inputs(c)
    keep = b["keep"]
    data = b["data"].copy()
    for i in range(b["nsub"]):
        rows = data[i][~keep[i]]
        if variant == 1:
            rows[:] = np.nan
        elif variant == 2:
            rows[:, 0], rows[:, -1] = np.inf, -np.inf
            rows[:, c["nbin"] // 2] = np.nan
        else:
            rows[:] = huge(c)
        data[i][~keep[i]] = rows
    over = dict(data=data)
    if b["errs"] is not None:
        errs = b["errs"].copy()
        errs[~keep] = np.nan if variant == 1 else 0.0
        over["errs"] = errs
    if c["guess"]:
        gw = keep.astype(float)
        if variant == 1:
            gw[~keep] = np.nan
        over["guess_weights"] = gw
    return over


def block_last_masked(keep, block):
    """True if some sub-int masks the last row of a block-channel block (a
    multiple of block minus one, or the band's last channel) while another
    row of that block is kept: the spectrum pass's prefetch then replaces a
    masked row by the block's last row, which is itself masked."""
    nchan = keep.shape[1]
    for k in keep:
        for n in np.flatnonzero(~k):
            if n % block == block - 1 or n == nchan - 1:
                lo = n // block * block
                if k[lo:lo + block].any():
                    return True
    return False


# ---------------------------------------------------------------------------
# B. degenerate sub-ints inside a batch
# ---------------------------------------------------------------------------
FAMILIES = ("w2_guess-250x2048-pd-cut-f32", "w2_guess-250x2048-pd-cut-f64",
            "w2_dsum-100x2048-pd-full-f32", "xmom-100x1024-pd-cut-f32",
            "momx-100x512-pd-cut-f32", "pass-97x512-pdta-cut-f32",
            "warm-257x256-pdta-cut-f32", "wm-45x1000-pd-cut-f32",
            "wo-37x1001-pdta-cut-f32", "blk-17x512-pd-cut-f32",
            "blk-45x4096-pd-cut-f32", "long-5x8194-pd-cut-f32")
ORDER = ("E", "s0", "F", "s1", "N", "s2", "Z", "s3", "E2")
ONLY_DEGENERATE = ("E", "F", "E2")
SCIPY = ("xmom-100x1024-pd-cut-f32", "pass-97x512-pdta-cut-f32")
NO_X = "w2_guess-33x2048-pd-cut-f32"
NO_X_ORDER = ("E", "s0", "F", "s1", "N", "s2", "Z", "s3")
ONLY = ("xmom-37x512-pd-cut-f32", "blk-17x512-pdt-cut-f32")
NAN_BIN = 7


def nan_channel(c):
    """N's channel: the band's last, in the last (partial) channel block."""
    return c["nchan"] - 1


def zero_channel(c):
    return c["nchan"] // 2


def degenerate(c, order=ORDER):
    """(subs, over) for ragged.device_fit: the sub-ints of order, "s<i>"
    the case's own sub-int i with its own mask, the others copies of sub-int
    0 (whose mask keeps every channel) made degenerate:
      E   mask all zero;
      F   fit_flags all zero (flags go in as [nsub, 5]);
      N   one NaN sample, bin NAN_BIN of nan_channel(c);
      Z   a channel of zero noise: zero_channel(c)'s row all zeros where the
          errors are estimated from the data, its errs 0 where given;
      E2  mask all zero and data all NaN."""
    b = R.inputs(c)
    assert b["keep"][0].all()
    subs = [int(k[1:]) if k[0] == "s" else 0 for k in order]
    data = b["data"][subs].copy()
    keep = b["keep"][subs].copy()
    flags = np.tile(np.array(c["flags"], dtype=np.int32), (len(order), 1))
    errs = None if b["errs"] is None else b["errs"][subs].copy()
    for j, k in enumerate(order):
        if k in ("E", "E2"):
            keep[j] = False
        if k == "E2":
            data[j] = np.nan
        if k == "F":
            flags[j] = 0
        if k == "N":
            data[j, nan_channel(c), NAN_BIN] = np.nan
        if k == "Z":
            if errs is None:
                data[j, zero_channel(c)] = 0.0
            else:
                errs[j, zero_channel(c)] = 0.0
    over = dict(data=data, mask=keep, flags=flags)
    if errs is not None:
        over["errs"] = errs
    return subs, over


def oracle_degenerate(c, kind):
    """The oracle's fit of the N or the Z sub-int of degenerate(c) (all
    channels kept), from the case's start."""
    import oracle as O
    b = R.inputs(c)
    subs, over = degenerate(c, (kind,))
    return O.fit_portrait_full(
        over["data"][0], b["model"], list(b["init"][0]), b["P"], b["freqs"],
        [b["nu_fit"][0]] * 3, [None] * 3,
        over["errs"][0] if "errs" in over else None, list(c["flags"]),
        log10_tau=b["scat"])


# ---------------------------------------------------------------------------
# C. minimal channel counts
# ---------------------------------------------------------------------------
ONE_CHANNEL = R._case("blk", 512, 1, R.PD)
MINIMAL = {"w2_guess-33x2048": R.case("w2_guess-33x2048-pd-cut-f32"),
           "xmom-37x512": R.case("xmom-37x512-pd-cut-f32"),
           "wm-45x1000": R.case("wm-45x1000-pd-cut-f32"),
           "wo-33x1001": R.case("wo-33x1001-pd-cut-f32"),
           "blk-3x512": R.case("blk-3x512-pd-cut-f32"),
           "one-1x512": ONE_CHANNEL}
MINIMAL_NAMES = list(MINIMAL)
P_ONLY = (1, 0, 0, 0, 0)


def placements(nchan):
    """[(kept channels, fit flags)]: one survivor fitted for the phase, two
    for phase and DM; the survivors first in the band, last (a partial
    tile), and apart (no shape here has two 64-channel groups: the band's
    two ends, in different 32-channel blocks from 33 channels on)."""
    if nchan == 1:
        return [((0,), P_ONLY)] * 2
    mid = nchan // 2
    return [((0,), P_ONLY), ((nchan - 1,), P_ONLY), ((mid,), P_ONLY),
            ((0, 1), R.PD), ((nchan - 2, nchan - 1), R.PD),
            ((0, nchan - 1), R.PD)]


@functools.lru_cache(maxsize=None)
def minimal(name):
    """The batch of a minimal-channel case: sub-int j is the case's sub-int
    j % 4 (its data, phase and DM) under placement j's mask and flags, with
    the fit frequency and the start ragged.inputs would give that mask."""
    import oracle as O
    import synth_np as S
    c = MINIMAL[name]
    b = R.inputs(c)
    pl = placements(c["nchan"])
    n = len(pl)
    src = np.arange(n) % b["nsub"]
    keep = np.zeros((n, c["nchan"]), dtype=bool)
    flags = np.zeros((n, 5), dtype=np.int32)
    init = np.zeros((n, 5))
    nu_fit = np.zeros(n)
    for j, (chans, fl) in enumerate(pl):
        keep[j, list(chans)] = True
        flags[j] = fl
        nu_fit[j] = O.guess_fit_freq(b["freqs"][keep[j]])
        phi, DM = b["truth"][src[j], :2]
        init[j, 0] = O.phase_transform(phi + 2e-3, DM, 1500.0, nu_fit[j],
                                       b["P"], mod=True)
        init[j, 1] = S.DM0
    out = dict(c=c, src=src, keep=keep, flags=flags, init=init, nu_fit=nu_fit,
               data=b["data"][src], errs=None if b["errs"] is None else
               b["errs"][src], model=b["model"], freqs=b["freqs"], P=b["P"],
               nsub=n)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def minimal_oracle(name, j):
    """The oracle's fit of sub-int j's surviving channels: the GetTOAs loop
    with zero weights where masked for the guess case, fit_portrait_full from
    the batch's start otherwise (as ragged.oracle_fit)."""
    import oracle as O
    m = minimal(name)
    c, k = m["c"], m["keep"][j]
    flags = [int(f) for f in m["flags"][j]]
    errs = None if m["errs"] is None else m["errs"][j]
    if c["guess"]:
        o = O.get_toas_archive(
            m["data"][j:j + 1], m["model"], m["freqs"][None],
            k.astype(float)[None], np.ones((1, c["nchan"])),
            np.array([m["P"]]), m["init"][j, 1], np.ones(1),
            noise_stds=None if errs is None else errs[None],
            fit_flags=flags, log10_tau=True)
        assert o["nu_fits"][0, 0] == m["nu_fit"][j]
        return o["fits"][0]
    return O.fit_portrait_full(
        m["data"][j][k], m["model"][k], list(m["init"][j]), m["P"],
        m["freqs"][k], [m["nu_fit"][j]] * 3, [None] * 3,
        None if errs is None else errs[k], flags, log10_tau=False)


def minimal_refit(name, j, first):
    """ragged.oracle_refit on a minimal sub-int: the oracle restarted from
    its own x_fit plus 1e-2 sigma in each fitted parameter."""
    import oracle as O
    m = minimal(name)
    k = m["keep"][j]
    errs = None if m["errs"] is None else m["errs"][j][k]
    x0 = np.asarray(first["x_fit"]) + 1e-2 * np.asarray(first["param_errs"])
    return O.fit_portrait_full(
        m["data"][j][k], m["model"][k], list(x0), m["P"], m["freqs"][k],
        [m["nu_fit"][j]] * 3, [None] * 3, errs,
        [int(f) for f in m["flags"][j]], log10_tau=False)


def minimal_device_fit(name):
    """engine.fit_batch on the whole minimal batch -> dict of numpy arrays."""
    from pulseportraiture_amd import engine
    m = minimal(name)
    c, n = m["c"], m["nsub"]
    data = m["data"].astype(np.float32) if c["dtype"] == "f32" else \
        m["data"].copy()
    kw = {}
    if c["guess"]:
        kw = dict(guess=True, guess_weights=m["keep"].astype(float),
                  guess_DM=m["init"][:, 1].copy(), guess_Ns=100)
    return engine.results_numpy(engine.fit_batch(
        data, m["model"], np.tile(m["freqs"], (n, 1)), np.full(n, m["P"]),
        m["init"].copy(), m["flags"].copy(),
        nu_fits=np.repeat(m["nu_fit"][:, None], 3, axis=1),
        nu_outs=np.full((n, 3), np.nan),
        errs=None if m["errs"] is None else m["errs"].copy(),
        chan_mask=m["keep"].astype(np.uint8), log10_tau=False,
        mom_x=c["mom_x"], **kw))


# ---------------------------------------------------------------------------
# 0. termination of the shared host / device routines on non-finite input
# ---------------------------------------------------------------------------
NONFINITE = (np.nan, np.inf, -np.inf)


def _put(a, where, v):
    a = np.array(a, dtype=float)
    if where == "first":
        a.flat[0] = v
    elif where == "last":
        a.flat[-1] = v
    else:
        a[...] = v
    return a


def termination_calls():
    """[(label, callable -> return code)]: ppf_poly_real_roots_host for
    degrees 1..8 and ppf_tr_subproblem_host for n 1..5, a NaN, +Inf or -Inf
    in the leading entry, in the trailing one, or in all of them; for the
    subproblem in H, in g, and in R."""
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    calls = []
    for deg in range(1, 9):
        base = rng.normal(size=deg + 1)
        for v in NONFINITE:
            for where in ("first", "last", "all"):
                co = _put(base, where, v)

                def roots(co=co, deg=deg):
                    out = np.zeros(8)
                    return lib.ppf_poly_real_roots_host(
                        co.ctypes.data, deg, out.ctypes.data)
                calls.append(("roots deg %d %s %s" % (deg, where, v), roots))
    for n in range(1, 6):
        A = rng.normal(size=(n, n))
        H0, g0 = A + A.T + 2 * n * np.eye(n), rng.normal(size=n)
        for v in NONFINITE:
            for what in ("H", "g", "R"):
                for where in ("first", "last", "all"):
                    if what == "R" and where != "all":
                        continue
                    H = _put(H0, where, v) if what == "H" else H0.copy()
                    g = _put(g0, where, v) if what == "g" else g0.copy()
                    Rr = float(v) if what == "R" else 0.5

                    def sub(H=H, g=g, n=n, Rr=Rr):
                        p = np.zeros(n)
                        return lib.ppf_tr_subproblem_host(
                            H.ctypes.data, g.ctypes.data, n, Rr,
                            p.ctypes.data)
                    calls.append(("subproblem n %d %s %s %s" %
                                  (n, what, where, v), sub))
    return calls
