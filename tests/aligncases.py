"""Shapes, weights and references that put more than one sub-int in front of
a wave of the ppalign accumulation (TEST INFRASTRUCTURE; no pytest hooks).

ppf_align_accum splits the sub-ints of a channel into align_groups(nsub,
nchan) groups (ppf_kernels.hip); inside a group, wave w of kXW (ppf_xspec.hip,
k_align_part_w) takes rows s0 + w, s0 + w + kXW, ...: it prefetches the next
live row during the current row's FFT, steps over rows of weight 0 inside its
stride and the waves' sums are then added in wave order.  A wave gets a second
row only when nsub > kXW * ceil(2048 / nchan); partition() restates the split
so that the cases below can be shown to reach it (tests/
test_align_inputs.py) before the device is compared with NumPy on them
(tests/test_gpu_align_groups.py).  phases_reference is the plain formula of
ppalign.py:236-241 that k_align_phases evaluates."""
import functools

import numpy as np

MIN_BLOCKS = 2048        # ppf_kernels.hip align_groups: workgroups wanted
WAVES = 8                # ppf_xspec.hip kXW: waves per k_align_part_w block
K_BLOCK = 256            # ppf_device.hpp kBlock: threads of k_align_phases
U = 2.0 ** -53           # unit roundoff of float64


# ----------------------------------------------------------- the row split ---
def partition(nsub, nchan):
    """align_groups and the row split of k_align_part / k_align_part_w:
    dict(ngroup, per, groups=[(s0, s1)], waves=[[rows of wave 0], ...] per
    group)."""
    ngroup = max(1, min(nsub, -(-MIN_BLOCKS // nchan)))
    per = -(-nsub // ngroup)
    groups = [(g * per, min(nsub, g * per + per)) for g in range(ngroup)]
    waves = [[list(range(s0 + w, s1, WAVES)) for w in range(WAVES)]
             for s0, s1 in groups]
    return dict(ngroup=ngroup, per=per, groups=groups, waves=waves)


def rows_per_wave(nsub, nchan):
    """The most rows any wave of any group takes."""
    return max(len(r) for g in partition(nsub, nchan)["waves"] for r in g)


# (nsub, nchan): what the shape exercises
CASES = (
    (18, 1024),   # groups 9, 9: wave 0 two rows, the smallest second trip
    (37, 1024),   # groups 19, 18: three or two rows, a ragged last group
    (50, 700),    # groups 17, 17, 16: a channel count off the powers of two
    (19, 2048),   # one group: the psradd Stokes shape
)
# the shapes the suite ran before these cases: parity, plan sweep, C4
OLD_SHAPES = ((37, 12), (37, 37), (37, 100), (5, 12), (5, 37), (3, 5),
              (16, 256), (24, 256))
WAVE_NBINS = (256, 512, 1024, 2048)      # k_align_part_w<7..10>
BLOCK_NBINS = (128, 242, 243)            # k_align_part: pow2, generic, odd


def case_id(case):
    return "%dx%d" % case


# ------------------------------------------------------------ zero weights ---
WAVE_PATTERNS = ("first", "first2", "middle", "last", "wave")
ALL_PATTERNS = WAVE_PATTERNS + ("group", "channel", "random")


def _target_waves(nsub, nchan):
    """(group, wave) pairs the per-wave patterns are applied to: wave 0 of
    group 0 and, in the last group, the highest wave that still has as many
    rows as any (the ragged group's own split)."""
    p = partition(nsub, nchan)
    out = [(0, 0)]
    if p["ngroup"] > 1:
        g = p["ngroup"] - 1
        most = max(len(r) for r in p["waves"][g])
        out.append((g, max(w for w in range(WAVES)
                           if len(p["waves"][g][w]) == most)))
    return out


def zero_patterns(nsub, nchan, only=ALL_PATTERNS):
    """[dict(name, chan, rows, group, wave, live)]: the sub-ints whose weight
    is 0 in one channel each, the channels distinct and spread over
    [0, nchan - 1] with both ends taken.  live is the number of rows of
    non-zero weight the pattern leaves its wave (per-wave patterns), its
    group ("group") or its channel ("channel", "random").

    first   the first row of a wave's stride (s0 + w)
    first2  the first two (s0 + w, s0 + w + WAVES)
    middle  rows[len // 2] of the stride
    last    the last row of the stride: the walk to the next live row ends
            at s1 and nothing is fetched
    wave    every row of the wave
    group   every row of one group (shapes with more than one group)
    channel every row of the channel
    random  each row with probability 0.4, one row kept"""
    p = partition(nsub, nchan)
    pats = []
    for g, w in _target_waves(nsub, nchan):
        rows = p["waves"][g][w]
        assert len(rows) >= 2, (nsub, nchan, g, w)
        pick = dict(first=rows[:1], first2=rows[:2],
                    middle=[rows[len(rows) // 2]], last=rows[-1:], wave=rows)
        for name in WAVE_PATTERNS:
            if name in only:
                pats.append(dict(name=name, rows=pick[name], group=g, wave=w,
                                 live=len(rows) - len(pick[name])))
    if "group" in only and p["ngroup"] > 1:
        for g in sorted({0, p["ngroup"] - 1}):
            s0, s1 = p["groups"][g]
            pats.append(dict(name="group", rows=list(range(s0, s1)), group=g,
                             wave=None, live=0))
    if "channel" in only:
        pats.append(dict(name="channel", rows=list(range(nsub)), group=None,
                         wave=None, live=0))
    if "random" in only:
        rng = np.random.default_rng([nsub, nchan, 11])
        z = rng.random(nsub) < 0.4
        z[rng.integers(nsub)] = False
        pats.append(dict(name="random", rows=list(np.flatnonzero(z)),
                         group=None, wave=None, live=int((~z).sum())))
    assert len(pats) <= nchan
    chans = np.round(np.linspace(0, nchan - 1, len(pats))).astype(int)
    assert len(set(chans)) == len(pats)
    for q, c in zip(pats, chans):
        q["chan"] = int(c)
    return pats


REDUCED = ("first", "wave")      # the instantiation sweep's pattern set


def weights(nsub, nchan, only=ALL_PATTERNS):
    """Uniform (0.1, 2.0) weights with the zero patterns applied."""
    w = np.random.default_rng([nsub, nchan, 7]).uniform(
        0.1, 2.0, size=(nsub, nchan))
    for q in zero_patterns(nsub, nchan, only):
        w[q["rows"], q["chan"]] = 0.0
    return w


@functools.lru_cache(maxsize=2)
def inputs(case, nbin, dtype="f32", only=ALL_PATTERNS):
    """(x, ph, w) of a case, read-only: unit normal rows (float32, or
    float64 values that float32 does not hold), phases in (-0.5, 0.5)."""
    nsub, nchan = case
    rng = np.random.default_rng([nsub, nchan, nbin, int(dtype == "f64")])
    x = rng.standard_normal(
        (nsub, nchan, nbin),
        dtype=np.float32 if dtype == "f32" else np.float64)
    ph = rng.uniform(-0.5, 0.5, size=(nsub, nchan))
    w = weights(nsub, nchan, only)
    for a in (x, ph, w):
        a.setflags(write=False)
    return x, ph, w


def align_reference(x, ph, w, chunk=256):
    """sum_s w[s, n] rotate(x[s, n], ph[s, n]) in float64 (the oracle's
    rotate_rows, as tests/test_gpu_parity.py): rows of weight 0 are left
    out, not multiplied by 0; a chunk of channels at a time."""
    import oracle as O
    nsub, nchan, nbin = x.shape
    ref = np.zeros((nchan, nbin))
    for c0 in range(0, nchan, chunk):
        c1 = min(nchan, c0 + chunk)
        for s in range(nsub):
            live = np.flatnonzero(w[s, c0:c1] != 0.0) + c0
            if live.size:
                ref[live] += w[s, live][:, None] * O.rotate_rows(
                    x[s, live].astype(np.float64), ph[s, live])
    return ref


@functools.lru_cache(maxsize=None)
def reference(case, nbin, dtype="f32", only=ALL_PATTERNS):
    """align_reference of inputs(...), shared and read-only."""
    ref = align_reference(*inputs(case, nbin, dtype, only))
    ref.setflags(write=False)
    return ref


def poisoned(x, w):
    """x with NaN in every row of weight 0."""
    bad = np.array(x)
    bad[w == 0.0] = np.nan
    return bad


# ------------------------------------------------------ phases and weights ---
# (1, 255 | 256 | 257): either side of one K_BLOCK-thread block; (3, 171):
# 513 entries, a block boundary inside a sub-int
PHASE_SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (3, 171), (7, 37))


def phases_reference(phi, DM, P, nu_ref, freqs, scales, errs, mask=None):
    """ppalign.py:236-241 in np.longdouble: phase = phi + Dconst DM / P
    (nu^-2 - nu_ref^-2), weight = scale / err^2 per (sub-int, channel), 0
    where mask is false.  phi, DM, P, nu_ref [nsub]; the rest [nsub, nchan]."""
    from pulseportraiture_amd import pplib
    L = np.longdouble
    phi, DM, P, nu_ref = (np.asarray(a, dtype=L)[:, None]
                          for a in (phi, DM, P, nu_ref))
    freqs, scales, errs = (np.asarray(a, dtype=L)
                           for a in (freqs, scales, errs))
    with np.errstate(invalid="ignore"):      # masked entries may hold NaN
        ph = phi + L(pplib.Dconst) * DM / P * (freqs ** -2 - nu_ref ** -2)
        wt = scales / errs ** 2
    if mask is not None:
        ph = np.where(mask, ph, L(0))
        wt = np.where(mask, wt, L(0))
    return ph, wt


def phase_bound(phi, DM, P, nu_ref, freqs):
    """8 u (|phi| + A (nu^-2 + nu_ref^-2)), A = Dconst |DM| / P: two pow
    calls of about 1 ulp, three roundings in A, one subtraction, one product
    and one sum."""
    from pulseportraiture_amd import pplib
    A = (pplib.Dconst * np.abs(DM) / P)[:, None]
    return 8 * U * (np.abs(phi)[:, None] +
                    A * (freqs ** -2.0 + nu_ref[:, None] ** -2.0))


def phase_case(nsub, nchan, slow=False):
    """One set of fit results per sub-int: DM positive, negative or exactly 0
    (s % 3), nu_ref inside the band (even s) or below / above it (odd s), a
    band of its own per sub-int.  slow: a 0.1-s period and |DM| of a few, so
    that the dispersive term stays below a rotation."""
    rng = np.random.default_rng([nsub, nchan, 3, int(slow)])
    s = np.arange(nsub)
    phi = rng.uniform(-0.5, 0.5, nsub)
    big = rng.uniform(2.0, 6.0, nsub) if slow else \
        34.5 + rng.normal(0, 1e-2, nsub)
    DM = np.where(s % 3 == 0, big, np.where(s % 3 == 1, -0.37 * big, 0.0))
    P = rng.uniform(0.09, 0.11, nsub) if slow else \
        rng.uniform(1.5e-3, 6e-3, nsub)
    lo = 1100.0 + rng.uniform(-5, 5, nsub)
    hi = 1900.0 + rng.uniform(-5, 5, nsub)
    freqs = lo[:, None] + (hi - lo)[:, None] * \
        ((np.arange(nchan) + 0.5) / nchan)[None, :]
    inside = rng.uniform(1200.0, 1800.0, nsub)
    outside = np.where(s % 4 == 1, rng.uniform(400.0, 900.0, nsub),
                       rng.uniform(2100.0, 3000.0, nsub))
    nu_ref = np.where(s % 2 == 0, inside, outside)
    scales = rng.uniform(0.5, 2.0, (nsub, nchan))
    errs = rng.uniform(0.5, 1.5, (nsub, nchan))
    mask = rng.random((nsub, nchan)) > 0.3
    mask.flat[0] = mask.flat[-1] = False
    return dict(phi=phi, DM=DM, P=P, nu_ref=nu_ref, freqs=freqs,
                scales=scales, errs=errs, mask=mask)


def results_rows(phi, DM, nu_ref):
    """ppf_result rows [nsub, RESULT_DOUBLES]: NaN but for params[0],
    params[1] and nu_out[0], so a read at a wrong offset poisons the
    output."""
    from pulseportraiture_amd import _lib
    I = _lib.RESULT_INDEX
    res = np.full((len(phi), _lib.RESULT_DOUBLES), np.nan)
    res[:, I["params"].start] = phi
    res[:, I["params"].start + 1] = DM
    res[:, I["nu_out"].start] = nu_ref
    return res


def float64_phases(c):
    """The direct float64 evaluation, in the order k_align_phases takes."""
    from pulseportraiture_amd import pplib
    ph = c["phi"][:, None] + (pplib.Dconst * c["DM"] / c["P"])[:, None] * (
        c["freqs"] ** -2.0 - c["nu_ref"][:, None] ** -2.0)
    return ph, c["scales"] / (c["errs"] * c["errs"])
