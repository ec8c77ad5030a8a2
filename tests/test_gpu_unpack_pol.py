"""ppf_unpack_psrfits_pol_batch (k_unpack on four blocks, then k_base_window
and k_row_stats over all four polarisations) against the NumPy restatement of
tests/unpackpolcases.py (psrfits.unpack_host_pol + unpackcases.baseline):
every conv on every sample type, profile lengths on both sides of the
4-bins-per-lane path and of the 256-thread bin loop, one full and one ragged
channel block, a padded sub_stride, zero-weight channels holding NaN.

The bars are test_gpu_unpack._check's: rows bitwise without baseline removal,
within 2 float32 spacings of the row maximum with it; wstart equal; total
rtol 1e-12 / atol 1e-9; mean 1e-12, sigma 1e-10, S/N 1e-9 relative (every
compared row has an off-pulse mean at least one sigma from zero:
unpackpolcases.reference asserts it)."""
import ctypes

import numpy as np
import pytest

import unpackcases as U
import unpackpolcases as UP
from test_gpu_unpack import KEYS, _bits, _check, _same

pytestmark = pytest.mark.gpu


def _run(c, rm, raw=None, wts="case", conv=None):
    import torch
    from pulseportraiture_amd import engine
    raw_d = torch.from_numpy(np.array(c["raw"] if raw is None else raw)).cuda()
    res = engine.unpack_psrfits_pol(
        raw_d, c["elem"], c["nchan"], c["nbin"], np.array(c["scl"]),
        np.array(c["offs"]), wts=c["wts"] if isinstance(wts, str) else wts,
        conv=c["conv"] if conv is None else conv, rm_baseline=rm)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}


def _check_pol(c, r, got, rm):
    assert got["rows"].shape == (c["nsub"], 4, c["nchan"], c["nbin"])
    assert got["stats"].shape == (c["nsub"], 4, c["nchan"], 3)
    _check(UP.flat(c), UP.flatten(r), UP.flatten(got), rm)


@pytest.mark.parametrize("name", UP.CASE_NAMES)
def test_unpack_pol_matches_restatement(name):
    """Every case with and without baseline removal; the statistics are
    formed before the subtraction, so they do not change with it."""
    c, r = UP.case(name), UP.reference(name)
    keep, gone = _run(c, False), _run(c, True)
    _check_pol(c, r, keep, False)
    _check_pol(c, r, gone, True)
    for k in ("stats", "total", "wstart"):
        np.testing.assert_array_equal(_bits(keep[k]), _bits(gone[k]),
                                      err_msg=k)


@pytest.mark.parametrize("name,like", [("pad-i16", "conv2-i16"),
                                       ("pad-nat", "conv3-nat")])
def test_padded_stride_takes_element_accesses_bitwise(name, like):
    """A sub_stride of whole elements that is no multiple of 8 bytes: the
    element-wide form on the samples the 4-bins-per-lane form just took,
    every output the same bits."""
    c, v = UP.case(name), UP.case(like)
    assert c["raw"].shape[1] % 8 and v["raw"].shape[1] % 16 == 0
    np.testing.assert_array_equal(c["raw"][:, :v["raw"].shape[1]], v["raw"])
    for rm in (False, True):
        _same(_run(c, rm), _run(v, rm), name)


def test_pol0_is_the_intensity_entry():
    """Stokes from Coherence: pol 0 (AA + BB), the total profile and the
    window are those of ppf_unpack_psrfits_batch on the same bytes, bitwise;
    so are pol 0's statistics."""
    import torch
    from pulseportraiture_amd import engine
    for name in ("conv2-i16", "conv3-f32", "conv0-u8", "nbin30-i16"):
        c = UP.case(name)
        if c["conv"] not in (0, 2, 3):
            c = dict(c, conv=2)
        raw_d = torch.from_numpy(np.array(c["raw"])).cuda()
        for rm in (False, True):
            got = _run(c, rm, conv=c["conv"])
            res = engine.unpack_psrfits(
                raw_d, c["elem"], 4, c["nchan"], c["nbin"],
                np.array(c["scl"]), np.array(c["offs"]),
                pol_mode=0 if c["conv"] == 0 else 1, rm_baseline=rm)
            torch.cuda.synchronize()
            one = {k: res[k].cpu().numpy() for k in KEYS}
            np.testing.assert_array_equal(_bits(got["rows"][:, 0]),
                                          _bits(one["rows"]), err_msg=name)
            np.testing.assert_array_equal(_bits(got["stats"][:, 0]),
                                          _bits(one["stats"]), err_msg=name)
            for k in ("total", "wstart"):
                np.testing.assert_array_equal(_bits(got[k]), _bits(one[k]),
                                              err_msg=name + " " + k)


def test_no_weights_is_unit_weights():
    c = UP.case("conv4-i16")
    one = np.ones((c["nsub"], c["nchan"]), np.float32)
    for rm in (False, True):
        _same(_run(c, rm, wts=None), _run(c, rm, wts=one))


def test_zero_weight_channels_are_skipped():
    """NaN and +-Inf samples in all four polarisations of the zero-weight
    channels: total and wstart as without them, the other channels' rows and
    stats bitwise the same."""
    c = UP.case("zero-weight")
    ok = UP.live(c)
    for rm in (False, True):
        clean, bad = _run(c, rm), _run(c, rm, raw=c["poison"])
        for k in ("total", "wstart"):
            np.testing.assert_array_equal(_bits(bad[k]), _bits(clean[k]))
        assert np.isfinite(bad["total"]).all()
        assert not np.isfinite(bad["rows"][~ok]).all()
        for k in ("rows", "stats"):
            np.testing.assert_array_equal(_bits(bad[k][ok]),
                                          _bits(clean[k][ok]))
        _check_pol(c, UP.reference("zero-weight"), bad, rm)


def test_same_call_twice_is_bitwise():
    for name in ("nbin1000-i16", "nbin257-f32"):
        c = UP.case(name)
        _same(_run(c, True), _run(c, True), name)


# -------------------------------------------------------------- validation --
def _call(c, raw_d, stride, nsub=None, nchan=None, nbin=None, elem=None,
          conv=None, short_ws=False):
    """The entry called with sentinel outputs: (return code, outputs
    untouched)."""
    import torch
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    dev = raw_d.device
    n, ch, nb = c["nsub"], c["nchan"], c["nbin"]
    scl = torch.from_numpy(np.array(c["scl"])).to(dev)
    offs = torch.from_numpy(np.array(c["offs"])).to(dev)
    rows = torch.full((n, 4, ch, nb), -7.0, dtype=torch.float32, device=dev)
    stats = torch.full((n, 4, ch, 3), -7.0, dtype=torch.float64, device=dev)
    total = torch.full((n, nb), -7.0, dtype=torch.float64, device=dev)
    wstart = torch.full((n,), -7, dtype=torch.int32, device=dev)
    wsb = int(lib.ppf_unpack_workspace_bytes(n, ch, nb))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ctx = _lib.context(dev.index)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ppf_unpack_psrfits_pol_batch(
        ctx, n if nsub is None else nsub, ch if nchan is None else nchan,
        nb if nbin is None else nbin, c["elem"] if elem is None else elem,
        p(raw_d), stride, p(scl), p(offs), None,
        c["conv"] if conv is None else conv, 1, p(rows), p(stats), p(total),
        p(wstart), p(ws), wsb - 8 if short_ws else wsb,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    clean = all(bool((t == -7).all()) for t in (rows, stats, total, wstart))
    return rc, clean


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from pulseportraiture_amd import _lib
    EINVAL, ENOMEM, OK = _lib.PPF_EINVAL, _lib.PPF_ENOMEM, _lib.PPF_OK
    c = UP.case("conv2-i16")
    n = c["raw"].shape[1]
    raw = torch.from_numpy(np.array(c["raw"])).cuda()
    for kw in (dict(conv=-1), dict(conv=6), dict(elem=-1), dict(elem=4),
               dict(nbin=1), dict(nchan=0), dict(nsub=-1)):
        assert _call(c, raw, n, **kw) == (EINVAL, True), kw
    # a sub_stride below the four polarisation blocks (three of them)
    assert _call(c, raw, n // 4 * 3) == (EINVAL, True)
    # an odd sub_stride under 2-byte samples
    wide = torch.zeros((c["nsub"], n + 1), dtype=torch.uint8).cuda()
    wide[:, :n] = raw
    assert _call(c, wide, n + 1) == (EINVAL, True)
    # raw 2 bytes off a 4-byte boundary under float32 samples
    f = UP.case("conv2-f32")
    m = f["raw"].shape[1]
    buf = torch.zeros(f["nsub"] * m + 8, dtype=torch.uint8).cuda()
    off = buf[2:2 + f["nsub"] * m].view(f["nsub"], m)
    off.copy_(torch.from_numpy(np.array(f["raw"])).cuda())
    assert off.data_ptr() % 4 == 2
    assert _call(f, off, m) == (EINVAL, True)
    # a short workspace
    assert _call(c, raw, n, short_ws=True) == (ENOMEM, True)
    # no sub-ints: nothing to do
    assert _call(c, raw, n, nsub=0) == (OK, True)
    # and the same arguments unspoilt pass
    assert _call(c, raw, n) == (OK, False)
