"""ppf_unpack_psrfits_batch (k_unpack, k_base_window, k_row_stats) on every
sample type, polarisation layout and edge, against the NumPy reference of
tests/unpackcases.py (the host side of the same cases:
tests/test_unpack_inputs.py).

Bars, from test_psrfits.test_device_unpack_matches_restatement: rows bitwise
psrfits.unpack_host's without baseline removal, within 2 float32 spacings of
the row maximum with it; total rtol 1e-12 / atol 1e-9; mean 1e-12, sigma
1e-10, S/N 1e-9 relative.  The window start is the reference's first
minimum, exactly: test_unpack_inputs asserts that every case has a unique
minimum clear of rounding, or an exact tie."""
import ctypes

import numpy as np
import pytest

import unpackcases as U

pytestmark = pytest.mark.gpu

KEYS = ("rows", "stats", "total", "wstart")


def _run(c, rm, raw=None, scl=None, offs=None, wts="case"):
    import torch
    from pulseportraiture_amd import engine
    raw_d = torch.from_numpy(np.array(c["raw"] if raw is None else raw)).cuda()
    res = engine.unpack_psrfits(
        raw_d, c["elem"], c["npol"], c["nchan"], c["nbin"],
        np.array(c["scl"] if scl is None else scl),
        np.array(c["offs"] if offs is None else offs),
        wts=c["wts"] if isinstance(wts, str) else wts,
        pol_mode=c["pol_mode"], rm_baseline=rm)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}


def _bits(a):
    return np.ascontiguousarray(a).view(
        {4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, msg=""):
    """Bitwise equality of every output."""
    for k in KEYS:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]),
                                      err_msg="%s %s" % (msg, k))


def _check(c, r, raw, rm):
    """One call's outputs against the reference r of case c."""
    ok = U.live_rows(c)
    np.testing.assert_array_equal(raw["wstart"], r["wstart"])
    np.testing.assert_allclose(raw["total"], r["total"], rtol=1e-12,
                               atol=1e-9)
    if rm:
        for s in range(c["nsub"]):
            want = r["removed"][s][ok[s]]
            np.testing.assert_allclose(
                raw["rows"][s][ok[s]], want, rtol=0,
                atol=2 * np.spacing(np.float32(np.abs(want).max())))
    else:
        np.testing.assert_array_equal(_bits(raw["rows"][ok]),
                                      _bits(r["rows"][ok]))
    st, ref = raw["stats"][ok], r["stats"][ok]
    assert np.isfinite(st).all()
    np.testing.assert_allclose(st[:, 0], ref[:, 0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(st[:, 1], ref[:, 1], rtol=1e-10, atol=0)
    np.testing.assert_allclose(st[:, 2], ref[:, 2], rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_unpack_matches_reference(name):
    """Every case with and without baseline removal; the statistics are
    formed before the subtraction, so they do not change with it."""
    c, r = U.case(name), U.reference(name)
    keep, gone = _run(c, False), _run(c, True)
    _check(c, r, keep, False)
    _check(c, r, gone, True)
    for k in ("stats", "total", "wstart"):
        np.testing.assert_array_equal(_bits(keep[k]), _bits(gone[k]),
                                      err_msg=k)


@pytest.mark.parametrize("name", [n for n in U.CASE_NAMES
                                  if U.case(n)["npol"] > U.used_pols(U.case(n))])
def test_unused_polarisations_are_not_read(name):
    """DAT_SCL / DAT_OFFS of the polarisations total intensity leaves out
    (IQUV's QUV, AABBCRCI's CR CI) are NaN: nothing changes."""
    c = U.case(name)
    scl, offs = U.poison_unused(c)
    for rm in (False, True):
        _same(_run(c, rm, scl=scl, offs=offs), _run(c, rm), name)


def test_two_roundings_bitwise():
    """DATA * DAT_SCL + DAT_OFFS is no fused multiply-add: rows whose single
    rounding differs in a sixth of the samples (test_unpack_inputs) are
    bitwise the twice-rounded ones."""
    for en in ("i16", "u8", "f32"):
        name = "round-" + en
        got = _run(U.case(name), False)
        ref = U.reference(name)["rows"]
        assert np.mean(U.single_rounding(U.case(name)) != ref) >= \
            U.ROUND_MIN_SHARE
        np.testing.assert_array_equal(_bits(got["rows"]), _bits(ref),
                                      err_msg=name)


def test_no_weights_is_unit_weights():
    for name in ("layout-i16-p2aabb", "dip-1000"):
        c = U.case(name)
        one = np.ones((c["nsub"], c["nchan"]), np.float32)
        for rm in (False, True):
            _same(_run(c, rm, wts=None), _run(c, rm, wts=one), name)


def test_heavy_channel_moves_the_window():
    c = U.case("heavy")
    assert list(_run(c, True)["wstart"]) == c["starts"]
    assert list(_run(c, True, wts=None)["wstart"]) == c["unweighted"]


def test_zero_weight_channels_are_skipped():
    """NaN and +-Inf samples in zero-weight channels: total and wstart as
    without them, the other channels' rows and stats bitwise the same."""
    c = U.case("zero-weight")
    ok = U.live_rows(c)
    for rm in (False, True):
        clean, bad = _run(c, rm), _run(c, rm, raw=c["poison"])
        for k in ("total", "wstart"):
            np.testing.assert_array_equal(_bits(bad[k]), _bits(clean[k]))
        assert np.isfinite(bad["total"]).all()
        for k in ("rows", "stats"):
            np.testing.assert_array_equal(_bits(bad[k][ok]),
                                          _bits(clean[k][ok]))
        _check(c, U.reference("zero-weight"), bad, rm)


def test_constant_row_and_two_bins():
    c = U.case("constant")
    got = _run(c, True)
    st = got["stats"][:, c["constant"]]
    assert (st[:, 1:] == 0).all() and np.isfinite(got["stats"]).all()
    assert (got["rows"][:, c["constant"]] == 0).all()
    for name in ("edge-rand-2", "edge-dip-2"):
        got = _run(U.case(name), False)
        assert (got["stats"][..., 1:] == 0).all()      # W = 1: sigma 0
        assert np.isfinite(got["stats"]).all()


def test_same_call_twice_is_bitwise():
    c = U.case("edge-rand-1000")
    _same(_run(c, True), _run(c, True))


@pytest.mark.parametrize("npol,pol_mode", [(1, 0), (2, 1)])
@pytest.mark.parametrize("en,pad", [("i16", 2), ("nat", 4)])
def test_padded_stride_takes_element_accesses_bitwise(en, pad, npol, pol_mode):
    """Total intensity from one block and from AA + BB, on samples whose
    layout admits the 4-bins-per-lane form and on the same samples behind a
    sub_stride of whole elements that is no multiple of 8 bytes (the
    element-wide form): every output the same bits."""
    name = "pad-%s-p%d" % (en, npol)
    kw = dict(npol=npol, pol_mode=pol_mode, nsub=3, nchan=17, nbin=64)
    v = U._random(name, U.ELEMS[en], **kw)
    c = U._random(name, U.ELEMS[en], pad=pad, **kw)
    assert c["raw"].shape[1] % 8 and v["raw"].shape[1] % 8 == 0
    np.testing.assert_array_equal(c["raw"][:, :v["raw"].shape[1]], v["raw"])
    for rm in (False, True):
        _same(_run(c, rm), _run(v, rm), name)


def test_profile_past_the_lds():
    """32768 bins (256 KB of float64): k_base_window reads the total
    profile back from `total`; the window is exact, wrapped ones too."""
    names = [n for n in U.CASE_NAMES if n.startswith("edge-dip-32768-")]
    assert names
    for name in names:
        c, r = U.case(name), U.reference(name)
        got = _run(c, True)
        assert list(got["wstart"]) == c["starts"]
        np.testing.assert_array_equal(got["total"], r["total"])


def _refused(c, raw_d, stride):
    """The entry called with sentinel outputs: (return code, outputs
    untouched)."""
    import torch
    from pulseportraiture_amd import _lib
    lib = _lib.load()
    nsub, nchan, nbin = c["nsub"], c["nchan"], c["nbin"]
    dev = raw_d.device
    scl = torch.from_numpy(np.array(c["scl"])).to(dev)
    offs = torch.from_numpy(np.array(c["offs"])).to(dev)
    rows = torch.full((nsub, nchan, nbin), -7.0, dtype=torch.float32,
                      device=dev)
    stats = torch.full((nsub, nchan, 3), -7.0, dtype=torch.float64,
                       device=dev)
    total = torch.full((nsub, nbin), -7.0, dtype=torch.float64, device=dev)
    wstart = torch.full((nsub,), -7, dtype=torch.int32, device=dev)
    wsb = int(lib.ppf_unpack_workspace_bytes(nsub, nchan, nbin))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    ctx = _lib.context(dev.index)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ppf_unpack_psrfits_batch(
        ctx, nsub, c["npol"], nchan, nbin, c["elem"], p(raw_d), stride,
        p(scl), p(offs), None, c["pol_mode"], 1, p(rows), p(stats), p(total),
        p(wstart), p(ws), wsb,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    clean = all(bool((t == -7).all()) for t in (rows, stats, total, wstart))
    return rc, clean


def test_misaligned_input_is_refused_before_any_launch():
    import torch
    from pulseportraiture_amd import _lib
    # an odd sub_stride under 2-byte samples
    c = U.case("layout-i16-p1")
    n = c["raw"].shape[1]
    raw = torch.zeros((c["nsub"], n + 1), dtype=torch.uint8).cuda()
    raw[:, :n] = torch.from_numpy(np.array(c["raw"])).cuda()
    assert _refused(c, raw, n + 1) == (_lib.PPF_EINVAL, True)
    # (and a sub_stride short of one sub-int's samples, as before)
    assert _refused(c, raw, n - 2) == (_lib.PPF_EINVAL, True)
    # raw 2 bytes off a 4-byte boundary under float32 samples
    c = U.case("layout-f32-p1")
    n = c["raw"].shape[1]
    buf = torch.zeros(c["nsub"] * n + 8, dtype=torch.uint8).cuda()
    off = buf[2:2 + c["nsub"] * n].view(c["nsub"], n)
    off.copy_(torch.from_numpy(np.array(c["raw"])).cuda())
    assert off.data_ptr() % 4 == 2
    assert _refused(c, off, n) == (_lib.PPF_EINVAL, True)
    # the same bytes on the boundary pass
    good = buf[4:4 + c["nsub"] * n].view(c["nsub"], n)
    good.copy_(off.clone())
    assert _refused(c, good, n) == (_lib.PPF_OK, False)


# ------------------------------------------------------------ load_data --
def _loaded(tmp_path, name):
    from pulseportraiture_amd import psrfits as PF
    fn = U.write_file(name, str(tmp_path / (name + ".fits")))
    return PF.load_data(fn, pscrunch=True, rm_baseline=False, quiet=True)


@pytest.mark.parametrize("name", list(U.FILES))
def test_load_data_sample_types_and_layouts(tmp_path, name):
    """psrfits.load_data on uint8 and float32 files, IQUV and AABBCRCI
    files of four polarisations (it uploads one or two of the blocks) and
    an 8192-bin file: subints bitwise the restatement, S/N and noise as
    test_psrfits._check_dedisperse_tscrunch checks them."""
    from pulseportraiture_amd import pplib
    c = U.file_case(name)
    u = U.unpacked(c)
    ref = U.baseline(u, None)
    d = _loaded(tmp_path, name)
    assert (d.nsub, d.nchan, d.nbin) == (c["nsub"], c["nchan"], c["nbin"])
    got = np.asarray(d.subints)[:, 0]
    np.testing.assert_array_equal(_bits(got), _bits(u))
    np.testing.assert_allclose(d.SNRs[:, 0], ref["stats"][..., 2], rtol=1e-6)
    for s in range(c["nsub"]):
        np.testing.assert_allclose(
            d.noise_stds[s, 0],
            pplib.get_noise(got[s].astype(float), chans=True), rtol=1e-9)


def test_load_data_upload_meets_the_alignment(tmp_path, monkeypatch):
    """What load_data hands the entry: raw on an element boundary, sub-int
    blocks of whole elements (the condition the entry checks)."""
    from pulseportraiture_amd import engine
    seen = []
    real = engine.unpack_psrfits

    def spy(raw, elem, *a, **k):
        seen.append((elem, raw.data_ptr(), raw.stride(0)))
        return real(raw, elem, *a, **k)

    monkeypatch.setattr(engine, "unpack_psrfits", spy)
    for name in ("file-u8", "file-f32", "file-iquv", "file-aabbcrci"):
        _loaded(tmp_path, name)
    assert [e for e, _, _ in seen] == [1, 2, 0, 0]
    for elem, ptr, stride in seen:
        es = np.dtype(U.DT[elem]).itemsize
        assert ptr % es == 0 and stride % es == 0
        assert ptr % 256 == 0              # a fresh device allocation
