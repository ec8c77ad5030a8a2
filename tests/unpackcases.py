"""Cases for ppf_unpack_psrfits_batch (k_unpack, k_base_window, k_row_stats)
and their NumPy reference: every sample type and polarisation layout, the
sample values at the edges of each type, the two float32 roundings of DATA *
DAT_SCL + DAT_OFFS, baseline windows placed exactly (integer arithmetic),
profile lengths across every thread partition of the window search, weights
and degenerate rows.  Seeded, no file I/O.  The host side of the cases:
tests/test_unpack_inputs.py; the device side: tests/test_gpu_unpack.py.

A case is a dict: raw uint8 [nsub, sub_stride] (the DATA bytes as the entry
takes them, holding npol_raw polarisation blocks), elem, npol, pol_mode,
nchan, nbin, scl / offs float32 [nsub, npol * nchan], wts float32 [nsub,
nchan] or None.  reference(name) restates the entry in float64 on
psrfits.unpack_host's rows.

No case has a baseline mean near zero (DAT_OFFS is 20 to 60, or the samples
carry their own offset; test_unpack_inputs asserts |mean| > 1e-3 max|row|
for every compared row), so the mean is compared relatively everywhere.
The same-thread tie (tie-near-1000) is one dip of W + 2 bins shaped so that
exactly two starts, two bins apart, tie: two separate W-bin dips cannot sit
within one thread's four starts."""
import functools

import numpy as np

from pulseportraiture_amd import psrfits as PF

DT = {0: ">i2", 1: "u1", 2: ">f4", 3: "<f4"}
NSUB, NCHAN, NBIN = 3, 17, 64           # one full 16-channel block + one of 1
THREADS = 256                            # k_base_window's workgroup

# nbin edges: 30, 50, 70 make 0.15 nbin a half-integer; 257 is the first
# length with two start bins per thread; 8192 is the first whose total
# profile is past 64 KB of LDS; 32768 does not fit the LDS at all
NBINS = (2, 3, 10, 30, 50, 70, 255, 256, 257, 1000, 8192, 16384, 32768)
BIG = 8192                               # from here: nsub 2, nchan 3


def window(nbin):
    return min(nbin - 1, max(1, int(np.rint(0.15 * nbin))))


def per(nbin):
    """Start bins per thread of k_base_window."""
    return (nbin + THREADS - 1) // THREADS


# ------------------------------------------------------------- builders --
def _case(name, x, elem, npol, pol_mode, scl, offs, wts=None, pad=0, **kw):
    """x: [nsub, npol_raw, nchan, nbin] samples of the polarisations raw
    holds; pad: bytes after each sub-int's block."""
    nsub, npol_raw, nchan, nbin = x.shape
    raw = np.ascontiguousarray(x.astype(DT[elem])).view(np.uint8)
    raw = raw.reshape(nsub, -1)
    if pad:
        raw = np.concatenate([raw, np.full((nsub, pad), 0xA5, np.uint8)],
                             axis=1)
    assert scl.shape == offs.shape == (nsub, npol * nchan)
    c = dict(name=name, raw=np.ascontiguousarray(raw), elem=elem, npol=npol,
             npol_raw=npol_raw, pol_mode=pol_mode, nsub=nsub, nchan=nchan,
             nbin=nbin, scl=scl.astype(np.float32),
             offs=offs.astype(np.float32),
             wts=None if wts is None else np.asarray(wts, np.float32))
    c.update(kw)
    return c


def _pulse(rng, nsub, npol, nchan, nbin):
    """A pulse near 0.3 turn (amplitude in [0.5, 1.5] per profile) and unit
    noise: [nsub, npol, nchan, nbin] float64, and the pulse alone."""
    b = np.arange(nbin)
    wid = max(0.03 * nbin, 0.6)
    prof = np.exp(-0.5 * ((b - int(0.3 * nbin)) / wid) ** 2)
    amp = rng.uniform(0.5, 1.5, (nsub, npol, nchan, 1))
    return prof * amp, rng.normal(size=(nsub, npol, nchan, nbin))


def _samples(rng, elem, nsub, npol, nchan, nbin):
    """Random samples of the type: a pulse on noise, in the type's range."""
    p, n = _pulse(rng, nsub, npol, nchan, nbin)
    if elem == 0:
        return np.clip(np.rint(3000.0 * n + 20000.0 * p), -32768,
                       32767).astype(np.int16)
    if elem == 1:
        return np.clip(np.rint(60.0 + 12.0 * n + 150.0 * p), 0,
                       255).astype(np.uint8)
    return (n + 20.0 * p + 7.0).astype(np.float32)


def _scales(rng, x, npol):
    """The issue's DAT_SCL = U(0.5, 1.5) 100 / max|x| and DAT_OFFS = U(20,
    60) per profile (products and sums that round: a fused multiply-add
    shows), for all npol polarisations whichever of them x holds."""
    nsub, npol_raw, nchan, nbin = x.shape
    mx = np.abs(x.astype(np.float64)).max(axis=-1)
    mx = np.concatenate([mx] + [mx[:, :1]] * (npol - npol_raw), axis=1)
    scl = rng.uniform(0.5, 1.5, (nsub, npol, nchan)) * 100.0 / mx
    offs = rng.uniform(20.0, 60.0, (nsub, npol, nchan))
    return (scl.reshape(nsub, -1).astype(np.float32),
            offs.reshape(nsub, -1).astype(np.float32))


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


def _random(name, elem, npol=1, pol_mode=0, npol_raw=None, pad=0,
            nsub=NSUB, nchan=NCHAN, nbin=NBIN, **kw):
    rng = np.random.default_rng(_seed(name))
    used = 2 if pol_mode == 1 else 1
    npol_raw = used if npol_raw is None else npol_raw
    x = _samples(rng, elem, nsub, npol_raw, nchan, nbin)
    scl, offs = _scales(rng, x, npol)
    return _case(name, x, elem, npol, pol_mode, scl, offs, pad=pad, **kw)


LAYOUTS = {"p1": dict(npol=1, pol_mode=0),
           "p2aabb": dict(npol=2, pol_mode=1),
           "p4iquv": dict(npol=4, pol_mode=0),          # raw: pol 0 only
           "p4aabb": dict(npol=4, pol_mode=1),          # raw: pols 0, 1
           "p4full": dict(npol=4, pol_mode=1, npol_raw=4, pad=64)}
ELEMS = {"i16": 0, "u8": 1, "f32": 2, "nat": 3}


def _values(name, elem):
    """The type's edge values planted in random rows."""
    c = _random(name, elem)
    rng = np.random.default_rng(_seed(name) + 1)
    x = np.ascontiguousarray(c["raw"]).view(DT[elem]).reshape(
        NSUB, 1, NCHAN, NBIN).astype(np.dtype(DT[elem]).newbyteorder("="))
    k = 40
    free = np.array([b for b in range(NBIN) if b not in (k - 1, k)])
    if elem == 0:
        special = np.array([-32768, 32767, -1, 0x00FF, -256], np.int16)
        assert special[-1].astype(np.uint16) == 0xFF00
    elif elem == 1:
        special = np.array([0, 127, 128, 255], np.uint8)
    else:
        special = np.array([-1.5, -0.0, 1e-40, -2.5e-41], np.float32)
    for s in range(NSUB):
        for n in range(NCHAN):
            at = rng.choice(free, size=special.size, replace=False)
            x[s, 0, n, at] = special
    scl, offs = c["scl"], c["offs"]
    if elem == 2:
        # +3e38 then -3e38 in neighbouring bins of every channel: the one
        # window that holds the second without the first starts on it
        x[:, 0, :, k - 1] = 3e38
        x[:, 0, :, k] = -3e38
        scl, offs = np.ones_like(scl), np.zeros_like(offs)
    return _case(name, x, elem, 1, 0, scl, offs, special=special)


def dip_value(n):
    return 100 + n % 3, 200 + n % 5


def _dips(name, nbin, starts, nchan=NCHAN, noise=True, wts=None):
    """uint8 profiles, DAT_SCL 1, DAT_OFFS 0: about 200 everywhere but a
    dip of W bins of about 100 at starts[s] in sub-int s (integers: every
    window sum is exact in float64)."""
    rng = np.random.default_rng(_seed(name))
    nsub, W = len(starts), window(nbin)
    x = np.empty((nsub, 1, nchan, nbin), np.uint8)
    for n in range(nchan):
        lo, hi = dip_value(n)
        x[:, 0, n] = hi
        for s, p in enumerate(starts):
            x[s, 0, n, (p + np.arange(W)) % nbin] = lo
    if noise:
        x += rng.integers(0, 4, x.shape, dtype=np.uint8)
    one = np.ones((nsub, nchan), np.float32)
    return _case(name, x, 1, 1, 0, one, 0 * one, wts=wts, exact=True,
                 starts=[p % nbin for p in starts])


def dip_starts(nbin):
    """The dip positions of the issue: the first bins, the window that ends
    on the last bin, the first that wraps, the last bin; at 1000 bins (four
    starts per thread) the last start of one thread and the first of the
    next as well."""
    W = window(nbin)
    ps = [0, 1, nbin - W, nbin - W + 1, nbin - 1]
    if nbin == 1000:
        ps += [3, 4, 996, 999]
    out = []
    for p in ps:
        if p % nbin not in out:
            out.append(p % nbin)
    return out


def _flat(name, nbin):
    x = np.full((1, 1, NCHAN, nbin), 200, np.uint8)
    one = np.ones((1, NCHAN), np.float32)
    return _case(name, x, 1, 1, 0, one, 0 * one, exact=True, tie=(0, None))


def _tie_far(name, nbin, a, b):
    """Two equal W-bin dips at a and b >= a + W: two equal minima."""
    W = window(nbin)
    assert a + W <= b and b + W <= nbin
    x = np.full((1, 1, NCHAN, nbin), 200, np.uint8)
    x[..., a:a + W] = 100
    x[..., b:b + W] = 100
    one = np.ones((1, NCHAN), np.float32)
    return _case(name, x, 1, 1, 0, one, 0 * one, exact=True, tie=(a, b))


def _tie_near(name, nbin, a):
    """Two equal minima at a and a + 2, starts of one thread (a a multiple
    of per(nbin) >= 3), the start between them 10 per channel above: one
    dip of W + 2 bins whose bins a + 1 and a + W are 110."""
    W = window(nbin)
    assert per(nbin) >= 3 and a % per(nbin) == 0 and W > 3
    x = np.full((1, 1, NCHAN, nbin), 200, np.uint8)
    x[..., a:a + W + 2] = 100
    x[..., a + 1] = 110
    x[..., a + W] = 110
    one = np.ones((1, NCHAN), np.float32)
    return _case(name, x, 1, 1, 0, one, 0 * one, exact=True, tie=(a, a + 2))


def _heavy(name):
    """Every channel dips at bin 5 but channel 3, of weight 100, which dips
    at bin 40: the window goes there (unweighted it stays at 5)."""
    W = window(NBIN)
    c = _dips(name, NBIN, [5, 5, 5])
    x = c["raw"].reshape(NSUB, 1, NCHAN, NBIN).copy()
    lo, hi = dip_value(3)
    x[:, 0, 3] = hi
    x[:, 0, 3, 40:40 + W] = lo
    wts = np.ones((NSUB, NCHAN), np.float32)
    wts[:, 3] = 100.0
    return _case(name, x, 1, 1, 0, c["scl"], c["offs"], wts=wts, exact=True,
                 starts=[40] * NSUB, unweighted=[5] * NSUB)


def _constant(name):
    """Channel 2 of every sub-int is constant (sigma 0, S/N 0)."""
    c = _random(name, 0)
    x = np.ascontiguousarray(c["raw"]).view(">i2").reshape(
        NSUB, 1, NCHAN, NBIN).astype(np.int16)
    x[:, 0, 2] = 1234
    return _case(name, x, 0, 1, 0, c["scl"], c["offs"], constant=2)


def _zero_weight(name):
    """elem 2, channels 4 and 16 (the block of one) of weight 0: `poison`
    holds the same bytes with NaN and +-Inf samples in those channels."""
    c = _random(name, 2)
    wts = np.ones((NSUB, NCHAN), np.float32)
    wts[:, [4, 16]] = 0.0
    x = np.ascontiguousarray(c["raw"]).view(">f4").reshape(
        NSUB, 1, NCHAN, NBIN).astype(np.float32)
    bad = x.copy()
    bad[:, 0, 4, ::3] = np.nan
    bad[:, 0, 4, 1::3] = np.inf
    bad[:, 0, 16, ::2] = -np.inf
    bad[:, 0, 16, 1::2] = np.nan
    poison = np.ascontiguousarray(bad.astype(">f4")).view(np.uint8)
    return _case(name, x, 2, 1, 0, c["scl"], c["offs"], wts=wts,
                 poison=poison.reshape(NSUB, -1), zero=[4, 16])


def _shape(nbin):
    return dict(nsub=2, nchan=3) if nbin >= BIG else {}


def _big_dip_cases(nbin):
    """Two sub-ints per case at the long lengths: the starts in pairs."""
    ps = dip_starts(nbin)
    ps += ps[:len(ps) % 2]
    return [ps[i:i + 2] for i in range(0, len(ps), 2)]


def _table():
    t = {}
    for en, e in ELEMS.items():
        for ln, kw in LAYOUTS.items():
            if e == 3 and ln != "p1":
                continue                 # load_data's use of elem 3
            t["layout-%s-%s" % (en, ln)] = functools.partial(
                _random, elem=e, **kw)
    for en in ("i16", "u8", "f32"):
        t["values-%s" % en] = functools.partial(_values, elem=ELEMS[en])
        t["round-%s" % en] = functools.partial(_random, elem=ELEMS[en])
    for nbin in (NBIN, 1000):
        t["dip-%d" % nbin] = functools.partial(
            _dips, nbin=nbin, starts=dip_starts(nbin))
        t["flat-%d" % nbin] = functools.partial(_flat, nbin=nbin)
    t["tie-far-64"] = functools.partial(_tie_far, nbin=64, a=7, b=30)
    t["tie-far-1000"] = functools.partial(_tie_far, nbin=1000, a=100, b=500)
    t["tie-near-1000"] = functools.partial(_tie_near, nbin=1000, a=4)
    for nbin in NBINS:
        t["edge-rand-%d" % nbin] = functools.partial(
            _random, elem=0, nbin=nbin, **_shape(nbin))
        if nbin >= BIG:
            for i, ps in enumerate(_big_dip_cases(nbin)):
                t["edge-dip-%d-%d" % (nbin, i)] = functools.partial(
                    _dips, nbin=nbin, starts=ps, nchan=3)
        elif nbin not in (NBIN, 1000):
            t["edge-dip-%d" % nbin] = functools.partial(
                _dips, nbin=nbin, starts=dip_starts(nbin))
    t["edge-one-row"] = functools.partial(_random, elem=0, nsub=1, nchan=1)
    t["heavy"] = _heavy
    t["constant"] = _constant
    t["zero-weight"] = _zero_weight
    return t


_TABLE = _table()
CASE_NAMES = list(_TABLE)
ROUND_MIN_SHARE = 0.05


@functools.lru_cache(maxsize=None)
def case(name):
    c = _TABLE[name](name)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ------------------------------------------------------------ reference --
def used_pols(c):
    return 2 if c["pol_mode"] == 1 else 1


def samples(c, raw=None):
    """The samples of the polarisations the entry reads, as float64
    [nsub, used, nchan, nbin], and their scales and offsets."""
    u, n = used_pols(c), c["nchan"] * c["nbin"]
    dt = np.dtype(DT[c["elem"]])
    raw = c["raw"] if raw is None else raw
    x = np.ascontiguousarray(raw[:, :u * n * dt.itemsize]).view(dt)
    x = x.reshape(c["nsub"], u, c["nchan"], c["nbin"])
    so = [v.reshape(c["nsub"], c["npol"], c["nchan"])[:, :u]
          for v in (c["scl"], c["offs"])]
    return x, so[0], so[1]


def unpacked(c, raw=None):
    """psrfits.unpack_host on the polarisations the entry reads: float32
    [nsub, nchan, nbin], two roundings per sample."""
    x, scl, offs = samples(c, raw)
    u = used_pols(c)
    with np.errstate(invalid="ignore", over="ignore"):
        return PF.unpack_host(x.reshape(c["nsub"], -1).view(np.uint8),
                              x.dtype, scl.reshape(c["nsub"], -1),
                              offs.reshape(c["nsub"], -1), u, c["nchan"],
                              c["nbin"])


def single_rounding(c):
    """DATA * DAT_SCL + DAT_OFFS formed in float64 and rounded once (what
    a fused multiply-add returns), pol 0."""
    x, scl, offs = samples(c)
    v = x[:, 0].astype(np.float64) * scl[:, 0, :, None].astype(np.float64) \
        + offs[:, 0, :, None].astype(np.float64)
    return v.astype(np.float32)


def window_sums(tot, W):
    """Sum of the circular W-bin window at every start (extended
    precision running sum: exact for integer profiles)."""
    ext = np.concatenate([tot, tot[:W]]).astype(np.longdouble)
    cs = np.concatenate([[np.longdouble(0)], np.cumsum(ext)])
    return (cs[W:W + tot.size] - cs[:tot.size]).astype(np.float64)


def baseline(u, wts):
    """k_base_window + k_row_stats restated in float64 on float32 rows u
    [nsub, nchan, nbin]: dict(W, total, sums, wstart, stats [nsub, nchan,
    3] = off-pulse mean, sigma, S/N, removed = float32(u - mean), cond =
    sum |v| / |sum v| over the on-pulse bins)."""
    nsub, nchan, nbin = u.shape
    W = window(nbin)
    w = np.ones((nsub, nchan)) if wts is None else wts.astype(np.float64)
    total, sums = np.empty((nsub, nbin)), np.empty((nsub, nbin))
    stats, cond = np.empty((nsub, nchan, 3)), np.empty((nsub, nchan))
    removed, wstart = np.empty_like(u), np.empty(nsub, np.int32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(nsub):
            sel = w[s] != 0.0            # the entry skips zero weights
            total[s] = (w[s][sel, None] * u[s][sel].astype(np.float64)
                        ).sum(axis=0)
            sums[s] = window_sums(total[s], W)
            wstart[s] = k = int(np.argmin(sums[s]))   # the first minimum
            idx = (k + np.arange(W)) % nbin
            on = np.ones(nbin, bool)
            on[idx] = False
            x = u[s].astype(np.float64)
            mean, sig = x[:, idx].mean(axis=1), x[:, idx].std(axis=1)
            v = x[:, on] - mean[:, None]
            osum = v.sum(axis=1)
            stats[s, :, 0], stats[s, :, 1] = mean, sig
            stats[s, :, 2] = np.where(sig > 0, osum / (sig * np.sqrt(
                on.sum())), 0.0)
            cond[s] = np.abs(v).sum(axis=1) / np.abs(osum)
            removed[s] = (x - mean[:, None]).astype(np.float32)
    return dict(W=W, total=total, sums=sums, wstart=wstart, stats=stats,
                removed=removed, cond=cond)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    u = unpacked(c)
    r = baseline(u, c["wts"])
    r["rows"] = u
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def margin(sums):
    """(second smallest - smallest window sum) / max |sum| of one sub-int."""
    two = np.partition(sums, 1)[:2]
    return (two[1] - two[0]) / np.abs(sums).max()


def live_rows(c):
    """[nsub, nchan] bool: the rows a comparison takes (all but the
    zero-weight channels of the case that poisons them)."""
    ok = np.ones((c["nsub"], c["nchan"]), bool)
    ok[:, c.get("zero", [])] = False
    return ok


def poison_unused(c):
    """scl, offs with NaN in the polarisations the entry does not read."""
    out = []
    for v in (c["scl"], c["offs"]):
        v = v.reshape(c["nsub"], c["npol"], c["nchan"]).copy()
        v[:, used_pols(c):] = np.nan
        out.append(v.reshape(c["nsub"], -1))
    return out


# files for psrfits.load_data: (sample type, NPOL, POL_TYPE, pol_mode), all
# NPOL blocks in the file; 3 x 17 x 64 but the long int16 one
FILES = {"file-u8": ("B", 1, "AA+BB", 0), "file-f32": ("E", 1, "AA+BB", 0),
         "file-iquv": ("I", 4, "IQUV", 0), "file-aabbcrci": ("I", 4, "AABBCRCI", 1),
         "file-i16-8192": ("I", 1, "AA+BB", 0)}


@functools.lru_cache(maxsize=None)
def file_case(name):
    code, npol, _, pol_mode = FILES[name]
    shape = dict(nsub=2, nchan=3, nbin=8192) if name.endswith("8192") else {}
    c = _random(name, {"I": 0, "B": 1, "E": 2}[code], npol=npol,
                pol_mode=pol_mode, npol_raw=npol, **shape)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def write_file(name, path):
    """The file of file_case(name), unit weights."""
    c = file_case(name)
    code, npol, pol_type, _ = FILES[name]
    nsub, nchan = c["nsub"], c["nchan"]
    PF.write_psrfits_rows(
        path, c["raw"], c["scl"], c["offs"],
        np.tile(np.linspace(1100.0, 1900.0, nchan), (nsub, 1)),
        np.ones((nsub, nchan)), np.full(nsub, 0.00289),
        5.0 + 10.0 * np.arange(nsub), np.full(nsub, 10.0), c["nbin"],
        npol=npol, pol_type=pol_type, dm=12.5, elem=code)
    return path
