"""The 2048-bin spectrum pass with a channel block of its own (k_xspec_w2: 64
channels per workgroup, the sub-int's scalars from k_classify's record) and
the launches bounded by k_classify's lists (the harmonic-major k_xspec_w2
instantiation and k_dsum_w when the caller passes n_x=0, PPF_OPT_NO_X).

Every case is at nbin = 2048 (the only shape that reaches k_xspec_w2), 3-5
sub-ints, GetTOAs guess on, float32 rows.  Inputs come from
tests/golden/synth_np.py and tests/ragged.py's templates; each sub-int is
held to the oracle's GetTOAs loop on the same inputs at ragged.compare_row's
bars (parameters within 0.01 sigma, chi2_red 1e-8 relative, the per-channel
tables).  n_x=0 takes the list-strided launches, n_x=1 (fewer slots than
sub-ints: no PPF_OPT_NO_X) the full grids; both must give the same tables bit
for bit, because a list changes which workgroup does a block, never a sum.

Channel counts: 40 (one block shorter than 64), 72 (a ragged last block of
8), 136 (two whole blocks and a tail of 8).  Masks, one per sub-int: a whole
round of four rows (channels 8-11); the whole second 64-channel block (at 72
channels: all of the ragged last block; at 40: nothing); only the last
channel."""
import functools
import os

import numpy as np
import pytest

import goldens as G
import ragged as R
from ragged import S

pytestmark = pytest.mark.gpu

NBIN = 2048
NCHANS = (40, 72, 136)
TAU = 3e-3                       # injected scattering time [rot] at 1500 MHz
PD, PDT, PDTA = (1, 1, 0, 0, 0), (1, 1, 0, 1, 0), (1, 1, 0, 1, 1)
TABLES = ("results", "scales", "scale_errs", "channel_snrs", "covariance")

# key -> (nchan, template, fit kinds)
CALLS = dict(
    [("pd-%d" % n, (n, "cut", (PD, PD, PD))) for n in NCHANS] +
    # phase + DM sub-ints around a scattering one: tiled and harmonic-major
    # slots, both lists short
    [("mixed", (72, "cut", (PD, PD, PDTA, PD, PD))),
     # every sub-int on the harmonic-major list
     ("scat", (72, "cut", (PDT, PDTA, PDT))),
     # a template too sharp for the fused guess: every sub-int through k_dsum_w
     ("narrow", (72, "narrow", (PD, PD, PD)))])


def masks(nchan, nsub):
    """[nsub, nchan] bool, True = kept; the three masks of the module text
    in turn."""
    m = np.ones((3, nchan), dtype=bool)
    m[0, 8:12] = False
    m[1, 64:128] = False
    m[2, -1] = False
    assert (m.sum(axis=1) >= 2).all()
    return m[np.arange(nsub) % 3]


@functools.lru_cache(maxsize=None)
def model(kind, nchan):
    import oracle as O
    if kind == "cut":
        return R.template("cut", nchan, NBIN)
    code, nu_ref, params, alpha = S.read_gmodel(
        os.path.join(G.GOLDEN, "narrow.gmodel"))
    freqs = S.channel_freqs(nchan)
    m = O.gen_gaussian_portrait(code, params, alpha, O.get_bin_centers(NBIN),
                                freqs, nu_ref)
    m.setflags(write=False)
    return m, freqs


@functools.lru_cache(maxsize=None)
def inputs(key):
    import oracle as O
    nchan, kind, kinds = CALLS[key]
    mod, freqs = model(kind, nchan)
    nsub = len(kinds)
    keep = masks(nchan, nsub)
    seed = 8100 + 37 * nchan + 1009 * list(CALLS).index(key)
    rng = np.random.default_rng(seed)
    data = np.empty((nsub, nchan, NBIN))
    gtau = np.zeros(nsub)
    for i, fl in enumerate(kinds):
        scat = bool(fl[3] or fl[4])
        data[i] = S.subint(seed + 1 + i, mod, freqs, rng.uniform(-0.5, 0.5),
                           S.DM0 + rng.normal(3e-4, 2e-4), S.P0,
                           noise=0.5 if scat else 1.5, tau=TAU if scat else 0.0)
        if scat:
            nu_fit = O.guess_fit_freq(freqs[keep[i]])
            gtau[i] = 0.8 * TAU * (nu_fit / 1500.0) ** -4.0
    out = dict(data=data, model=mod, freqs=freqs, keep=keep,
               flags=np.array(kinds, dtype=np.int32), gtau=gtau)
    for a in out.values():
        a.setflags(write=False)
    out["nsub"] = nsub
    return out


@functools.lru_cache(maxsize=None)
def oracle_fit(key, i):
    """The oracle's GetTOAs loop on sub-int i alone (its kept channels and
    flags)."""
    import oracle as O
    b = inputs(key)
    nchan = b["data"].shape[1]
    o = O.get_toas_archive(
        b["data"][i:i + 1], b["model"], b["freqs"][None],
        b["keep"][i].astype(float)[None], np.ones((1, nchan)),
        np.array([S.P0]), S.DM0, np.ones(1),
        fit_flags=tuple(int(f) for f in b["flags"][i]),
        tau_guess=b["gtau"][i], alpha_guess=-4.0, log10_tau=False)
    return o["fits"][0], float(o["nu_fits"][0, 0])


@functools.lru_cache(maxsize=None)
def device_fit(key, n_x, run=0):
    """engine.fit_batch on the call (numpy tables, read-only, shared); run
    tells repeated calls apart."""
    from pulseportraiture_amd import engine
    b = inputs(key)
    n = b["nsub"]
    nu_fit = np.array([oracle_fit(key, i)[1] for i in range(n)])
    init = np.zeros((n, 5))
    init[:, 1] = S.DM0
    scat = b["gtau"] != 0.0
    init[scat, 3] = b["gtau"][scat]
    init[scat, 4] = -4.0
    r = engine.results_numpy(engine.fit_batch(
        b["data"].astype(np.float32), b["model"], np.tile(b["freqs"], (n, 1)),
        np.full(n, S.P0), init, b["flags"].copy(),
        nu_fits=np.repeat(nu_fit[:, None], 3, axis=1),
        nu_outs=np.full((n, 3), np.nan), chan_mask=b["keep"].astype(np.uint8),
        log10_tau=False, guess=True, guess_weights=b["keep"].astype(float),
        guess_DM=np.full(n, S.DM0), guess_Ns=100, guess_tau=b["gtau"].copy(),
        n_x=n_x))
    for a in r.values():
        a.setflags(write=False)
    return r


def _same(a, b, msg):
    for t in TABLES:
        np.testing.assert_array_equal(a[t], b[t], err_msg="%s %s" % (t, msg))


def _check(key):
    """Both launch shapes against each other, the bounded one against the
    oracle."""
    from pulseportraiture_amd import _lib
    b = inputs(key)
    r = device_fit(key, 0)
    st = r["results"][:, _lib.RESULT_INDEX["status"]].astype(int)
    assert not (st & _lib.ST_NOSPACE).any(), st
    _same(r, device_fit(key, 1), "%s: n_x=0 against the full grids" % key)
    for i in range(b["nsub"]):
        o, _ = oracle_fit(key, i)
        R.compare_row("BLOCKS %s sub-int %d" % (key, i), (key, i), r, i, o,
                      b["keep"][i], S.P0, False)


def test_templates_are_what_the_cases_need():
    """The cut template's cutoffs stay inside the fused guess (448
    harmonics); the narrow one's do not (R.kc restates k_model_cut)."""
    for nchan in NCHANS:
        assert R.kc(model("cut", nchan)[0]).max() <= R.GUESS_HARMONICS
    assert R.kc(model("narrow", 72)[0]).max() > R.GUESS_HARMONICS


@pytest.mark.parametrize("nchan", NCHANS)
def test_channel_counts_and_masks(nchan):
    """One block shorter than 64, a ragged last block of 8, two whole blocks
    and a tail; a zapped round, a zapped block (the whole ragged block at 72
    channels), a zapped last channel (the clamped prefetch address)."""
    _check("pd-%d" % nchan)


def test_mixed_call():
    """Phase + DM sub-ints (tiled slots, k_moments) around a scattering one
    (harmonic-major slot, k_pass): with n_x=0 the scattering sub-int is the
    one entry of the harmonic-major list."""
    from pulseportraiture_amd import engine
    b = inputs("mixed")
    init = np.zeros((b["nsub"], 5))
    init[:, 3] = b["gtau"]
    assert engine.x_subints(b["flags"], init, False, b["nsub"]) == 1
    _check("mixed")


def test_all_scattering_call():
    """Every sub-int on the harmonic-major list, the guess fused there."""
    _check("scat")


def test_guess_fallback_through_dsum():
    """A template too sharp for the fused guess: with n_x=0 k_dsum_w strides
    over the list of all three sub-ints."""
    _check("narrow")


def test_same_call_twice_is_bitwise_equal():
    for key in ("mixed", "narrow"):
        _same(device_fit(key, 0), device_fit(key, 0, run=1), "%s repeated" % key)
