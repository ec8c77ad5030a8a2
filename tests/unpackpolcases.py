"""Cases for ppf_unpack_psrfits_pol_batch (k_unpack on four blocks, then
k_base_window and k_row_stats over all four polarisations) and their NumPy
reference, in
the manner of tests/unpackcases.py, whose builders and baseline restatement
they use.  Seeded, no file I/O.  The host side: tests/test_unpack_pol_host.py;
the device side: tests/test_gpu_unpack_pol.py.

A case is a dict: raw uint8 [nsub, sub_stride] holding the four polarisation
blocks of every sub-int (and `pad` bytes after them), elem, conv, nchan, nbin,
scl / offs float32 [nsub, 4 * nchan], wts float32 [nsub, nchan] or None.

The four polarisations have distinct baselines (14, 6, 4, -3) and pulse
amplitudes (20, 12, 6, -4, times one factor per profile) under unit noise, so
every row of every converted state has an off-pulse mean well away from zero
(reference() asserts |mean| >= sigma for every row): the relative bars of
test_gpu_unpack._check apply to all of them."""
import functools

import numpy as np

import unpackcases as U
from pulseportraiture_amd import psrfits as PF

NSUB, NCHAN = 3, 17                      # one full 16-channel block + one of 1
BASE = np.array([14.0, 6.0, 4.0, -3.0])
AMP = np.array([20.0, 12.0, 6.0, -4.0])
# 30 and 257 are no multiple of 4 (element-wide accesses), 64 and 1000 are
# (4 bins per lane); 257 and 1000 take a second trip of the 256-thread loop
NBINS = (2, 30, 64, 257, 1000)
ZERO = (4, 16)                           # the zero-weight channels


def _values(rng, nsub, nchan, nbin):
    """[nsub, 4, nchan, nbin] float64: baseline + pulse + unit noise."""
    b = np.arange(nbin)
    wid = max(0.03 * nbin, 0.6)
    prof = np.exp(-0.5 * ((b - int(0.3 * nbin)) / wid) ** 2)
    u = rng.uniform(0.5, 1.5, (nsub, 1, nchan, 1))
    return BASE[None, :, None, None] + AMP[None, :, None, None] * u * prof \
        + rng.normal(size=(nsub, 4, nchan, nbin))


def _digitise(rng, v, elem):
    """Samples of the type and per-profile DAT_SCL / DAT_OFFS that give v
    back (to the type's resolution): products and sums that round."""
    lo, hi = v.min(axis=-1, keepdims=True), v.max(axis=-1, keepdims=True)
    if elem == 0:
        offs, scl = (lo + hi) / 2, (hi - lo) / 2 / 32767.0
        x = np.clip(np.rint((v - offs) / scl), -32768, 32767).astype(np.int16)
    elif elem == 1:
        offs, scl = lo, (hi - lo) / 255.0
        x = np.clip(np.rint((v - offs) / scl), 0, 255).astype(np.uint8)
    else:
        scl = rng.uniform(0.5, 1.5, lo.shape)
        offs = rng.uniform(-1.0, 1.0, lo.shape)
        x = ((v - offs) / scl).astype(np.float32)
    nsub = v.shape[0]
    return x, scl.reshape(nsub, -1).astype(np.float32), \
        offs.reshape(nsub, -1).astype(np.float32)


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


def _build(name, elem, conv, nbin, nchan=NCHAN, nsub=NSUB, pad=0,
           zero_weight=False):
    rng = np.random.default_rng(_seed(name))
    x, scl, offs = _digitise(rng, _values(rng, nsub, nchan, nbin), elem)
    raw = np.ascontiguousarray(x.astype(U.DT[elem])).view(np.uint8)
    raw = raw.reshape(nsub, -1)
    c = dict(name=name, elem=elem, conv=conv, nsub=nsub, nchan=nchan,
             nbin=nbin, scl=scl, offs=offs, wts=None, pad=pad)
    if zero_weight:
        # NaN and +-Inf samples in every polarisation of the zero-weight
        # channels: `poison` holds the same bytes with them
        assert elem == 2
        wts = np.ones((nsub, nchan), np.float32)
        wts[:, list(ZERO)] = 0.0
        bad = x.copy()
        bad[:, :, ZERO[0], ::3] = np.nan
        bad[:, :, ZERO[0], 1::3] = np.inf
        bad[:, :, ZERO[1], ::2] = -np.inf
        bad[:, :, ZERO[1], 1::2] = np.nan
        c["wts"] = wts
        c["poison"] = np.ascontiguousarray(bad.astype(">f4")).view(
            np.uint8).reshape(nsub, -1)
        c["zero"] = list(ZERO)
    if pad:
        fill = np.full((nsub, pad), 0xA5, np.uint8)
        raw = np.concatenate([raw, fill], axis=1)
    c["raw"] = np.ascontiguousarray(raw)
    return c


def _table():
    t = {}
    for en, e in U.ELEMS.items():
        for conv in range(6):            # every conv meets every elem
            t["conv%d-%s" % (conv, en)] = dict(elem=e, conv=conv, nbin=64)
    for i, nbin in enumerate(NBINS):     # every nbin meets int16 and float32
        for en in ("i16", "f32"):
            t["nbin%d-%s" % (nbin, en)] = dict(
                elem=U.ELEMS[en], conv=(2, 5, 3, 4, 1)[i], nbin=nbin)
    # one channel: a single, ragged channel block
    t["one-chan-i16"] = dict(elem=0, conv=2, nbin=64, nchan=1)
    t["one-chan-f32"] = dict(elem=2, conv=5, nbin=30, nchan=1)
    t["one-chan-u8"] = dict(elem=1, conv=4, nbin=1000, nchan=1)
    t["one-chan-nat"] = dict(elem=3, conv=1, nbin=257, nchan=1)
    # a sub_stride that is whole elements but no multiple of the vector
    # width: element-wide accesses on a shape that otherwise takes 4 bins
    # per lane (the same samples as conv2-i16 / conv3-nat: same seed below)
    t["pad-i16"] = dict(elem=0, conv=2, nbin=64, pad=2, like="conv2-i16")
    t["pad-nat"] = dict(elem=3, conv=3, nbin=64, pad=4, like="conv3-nat")
    t["zero-weight"] = dict(elem=2, conv=2, nbin=64, zero_weight=True)
    return t


_TABLE = _table()
CASE_NAMES = list(_TABLE)


@functools.lru_cache(maxsize=None)
def case(name):
    kw = dict(_TABLE[name])
    c = _build(kw.pop("like", name), **kw)
    c["name"] = name
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def unpacked(c, raw=None):
    """psrfits.unpack_host_pol on the case: float32 [nsub, 4, nchan, nbin]."""
    raw = c["raw"] if raw is None else raw
    n = 4 * c["nchan"] * c["nbin"] * np.dtype(U.DT[c["elem"]]).itemsize
    with np.errstate(invalid="ignore", over="ignore"):
        return PF.unpack_host_pol(np.ascontiguousarray(raw[:, :n]),
                                  U.DT[c["elem"]], c["scl"], c["offs"],
                                  c["nchan"], c["nbin"], c["conv"])


def row_stats(u, wstart, W):
    """k_row_stats restated in float64 on float32 rows u [nsub, nrow, nbin]
    with the window start of each sub-int given: (stats [nsub, nrow, 3],
    removed float32)."""
    nsub, nrow, nbin = u.shape
    stats, removed = np.empty((nsub, nrow, 3)), np.empty_like(u)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(nsub):
            idx = (int(wstart[s]) + np.arange(W)) % nbin
            on = np.ones(nbin, bool)
            on[idx] = False
            x = u[s].astype(np.float64)
            mean, sig = x[:, idx].mean(axis=1), x[:, idx].std(axis=1)
            osum = (x[:, on] - mean[:, None]).sum(axis=1)
            stats[s, :, 0], stats[s, :, 1] = mean, sig
            stats[s, :, 2] = np.where(sig > 0, osum / (sig * np.sqrt(
                on.sum())), 0.0)
            removed[s] = (x - mean[:, None]).astype(np.float32)
    return stats, removed


def restate(rows, conv, wts):
    """The entry restated on unpacked rows [nsub, 4, nchan, nbin]: the
    window of unpackcases.baseline on the total intensity, the statistics of
    every polarisation's rows with it.  dict(rows, total, sums, wstart,
    stats [nsub, 4, nchan, 3], removed)."""
    nsub, _, nchan, nbin = rows.shape
    with np.errstate(invalid="ignore", over="ignore"):
        tot = np.ascontiguousarray(PF.total_intensity_host(rows, conv))
    b = U.baseline(tot, wts)
    stats, removed = row_stats(rows.reshape(nsub, 4 * nchan, nbin),
                               b["wstart"], b["W"])
    return dict(rows=rows, total=b["total"], sums=b["sums"],
                wstart=b["wstart"], W=b["W"],
                stats=stats.reshape(nsub, 4, nchan, 3),
                removed=removed.reshape(rows.shape))


def live(c):
    """[nsub, 4, nchan] bool: the rows a comparison takes (all but the
    zero-weight channels of the case that poisons them)."""
    ok = np.ones((c["nsub"], 4, c["nchan"]), bool)
    ok[:, :, c.get("zero", [])] = False
    return ok


@functools.lru_cache(maxsize=None)
def reference(name):
    """restate() of the case, with what the bars need asserted: a window
    minimum clear of rounding, and every compared row's off-pulse mean at
    least one off-pulse sigma from zero."""
    c = case(name)
    r = restate(unpacked(c), c["conv"], c["wts"])
    for s in range(c["nsub"]):
        assert U.margin(r["sums"][s]) > 1e-9, (name, s)
    st = r["stats"][live(c)]
    assert (np.abs(st[:, 0]) >= st[:, 1]).all(), name
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def flat(c):
    """The case as test_gpu_unpack._check reads it: the four polarisations
    of a channel as 4 nchan rows of the sub-int."""
    n = c["nchan"]
    return dict(nsub=c["nsub"], nchan=4 * n,
                zero=[p * n + z for p in range(4) for z in c.get("zero", [])])


def flatten(r):
    """Outputs [nsub, 4, nchan, ...] as [nsub, 4 nchan, ...]."""
    out = dict(r)
    for k in ("rows", "removed", "stats"):
        if k in r:
            a = r[k]
            out[k] = a.reshape((a.shape[0], a.shape[1] * a.shape[2]) +
                               a.shape[3:])
    return out
