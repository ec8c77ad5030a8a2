"""Host checks of the PSRFITS unpack cases (tests/unpackcases.py): the inputs
have the properties tests/test_gpu_unpack.py relies on, every compared
quantity is well conditioned against the bars, and the cases tell the
kernels' likely mistakes apart on the reference alone, so that a device
deviation there is the device's.  No GPU."""
import numpy as np
import pytest

import unpackcases as U


def test_case_table_is_complete():
    names = set(U.CASE_NAMES)
    assert len(names) == len(U.CASE_NAMES)
    for en, e in U.ELEMS.items():
        for ln in U.LAYOUTS:
            assert ("layout-%s-%s" % (en, ln) in names) == \
                (e != 3 or ln == "p1")
    for en in ("i16", "u8", "f32"):
        assert {"values-" + en, "round-" + en} <= names
    assert U.NBINS == (2, 3, 10, 30, 50, 70, 255, 256, 257, 1000, 8192,
                       16384, 32768)
    for nbin in U.NBINS:
        assert "edge-rand-%d" % nbin in names
        dips = [n for n in names if n.startswith("edge-dip-%d-" % nbin) or
                n in ("dip-%d" % nbin, "edge-dip-%d" % nbin)]
        got = set()
        for n in dips:
            got |= set(U.case(n)["starts"])
        assert got == set(U.dip_starts(nbin)), nbin
        shape = (2, 3) if nbin >= 8192 else (U.NSUB, U.NCHAN)
        c = U.case("edge-rand-%d" % nbin)
        assert (c["nsub"], c["nchan"]) == shape
    assert [0.15 * n % 1 for n in (30, 50, 70)] == [0.5] * 3
    assert U.per(256) == 1 and U.per(257) == 2 and U.per(1000) == 4
    # past 64 KB of LDS, and past the LDS altogether
    assert 8192 * 8 + 3072 > 64 * 1024 and 32768 * 8 > 160 * 1024
    c = U.case("edge-one-row")
    assert (c["nsub"], c["nchan"]) == (1, 1)


def test_layouts_hold_what_the_entry_reads():
    for en, e in U.ELEMS.items():
        es = np.dtype(U.DT[e]).itemsize
        n = U.NCHAN * U.NBIN * es
        for ln, used, stride in (("p1", 1, n), ("p2aabb", 2, 2 * n),
                                 ("p4iquv", 1, n), ("p4aabb", 2, 2 * n),
                                 ("p4full", 2, 4 * n + 64)):
            if e == 3 and ln != "p1":
                continue
            c = U.case("layout-%s-%s" % (en, ln))
            assert c["raw"].shape == (U.NSUB, stride) and U.used_pols(c) == used
            assert c["scl"].shape == (U.NSUB, c["npol"] * U.NCHAN)
            assert stride % es == 0
            # scales differ between sub-ints and polarisations: a wrong row
            # stride reads another profile's
            s = c["scl"].reshape(U.NSUB, c["npol"], U.NCHAN)
            assert len(np.unique(s)) == s.size
            if c["npol"] > used:
                ps, po = U.poison_unused(c)
                bad = np.isnan(ps.reshape(s.shape))
                assert bad[:, used:].all() and not bad[:, :used].any()
                assert np.isnan(po.reshape(s.shape)[:, used:]).all()


def test_planted_sample_values():
    for en in ("i16", "u8", "f32"):
        c = U.case("values-" + en)
        x = U.samples(c)[0][:, 0]
        for row in x.reshape(-1, U.NBIN):
            for v in c["special"]:
                hit = row == v
                if v == 0 and c["elem"] == 2:
                    hit &= np.signbit(row)            # -0.0 itself
                assert hit.any(), (en, v)
    c = U.case("values-i16")
    b = c["raw"].reshape(-1, U.NBIN, 2)
    for pair in ((0x80, 0x00), (0x7F, 0xFF), (0xFF, 0xFF), (0x00, 0xFF),
                 (0xFF, 0x00)):
        assert ((b == pair).all(axis=-1)).any(axis=-1).all()
    c = U.case("values-f32")
    x = U.samples(c)[0][:, 0].astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(x) < tiny) & (x != 0)).any(axis=-1).all()    # subnormal
    assert (x == np.float32(3e38)).any(axis=-1).all()
    assert (x == np.float32(-3e38)).any(axis=-1).all()
    assert (c["scl"] == 1).all() and (c["offs"] == 0).all()
    r = U.reference("values-f32")
    assert (r["wstart"] == 40).all() and np.isfinite(r["removed"]).all()
    # uint8 above 127: a signed read differs
    x = U.samples(U.case("values-u8"))[0]
    assert (x > 127).any(axis=-1).all()
    x = U.samples(U.case("round-u8"))[0]
    assert (x > 127).any(axis=-1).all()


@pytest.mark.parametrize("en", ["i16", "u8", "f32"])
def test_one_rounding_differs_from_two(en):
    """The share of samples where DATA * DAT_SCL + DAT_OFFS rounded once
    (a fused multiply-add) differs from unpack_host's two roundings."""
    c = U.case("round-" + en)
    share = np.mean(U.single_rounding(c) != U.reference("round-" + en)["rows"])
    print("round-%s: %.1f %% of samples differ" % (en, 100 * share))
    assert share >= U.ROUND_MIN_SHARE


def kernel_window(tot, W, lt_thread=np.less, lt_reduce=np.less, wrap=True):
    """k_base_window's search as the kernel orders it: per(nbin) starts per
    thread, a direct sum at the first and the sliding update after it, the
    threads' minima reduced in thread order.  lt_*, wrap: the kernel's
    comparisons and the sliding update's modulo, to be broken."""
    nbin = tot.size
    per = U.per(nbin)
    ext = np.concatenate([tot, np.zeros(nbin)])       # past the row: not tot
    best, bi = [], []
    for t in range(U.THREADS):
        b0, b1 = t * per, min(nbin, (t + 1) * per)
        m, mi = np.inf, nbin
        if b0 < b1:
            w = sum(tot[(b0 + j) % nbin] for j in range(W))
            for b in range(b0, b1):
                if b > b0:
                    k = b - 1 + W
                    w += (tot[k % nbin] if wrap else ext[k]) - tot[b - 1]
                if lt_thread(w, m):
                    m, mi = w, b
        best.append(m)
        bi.append(mi)
    m, mi = best[0], bi[0]
    for t in range(1, U.THREADS):
        if lt_reduce(best[t], m):
            m, mi = best[t], bi[t]
    return mi if mi < nbin else 0


SMALL = [n for n in U.CASE_NAMES if U.case(n)["nbin"] <= 1000]


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_reference_is_well_posed(name):
    c, r = U.case(name), U.reference(name)
    ok = U.live_rows(c)
    assert r["W"] == U.window(c["nbin"]) and 1 <= r["W"] < c["nbin"]
    assert np.isfinite(r["total"]).all() and np.isfinite(r["sums"]).all()
    assert np.isfinite(r["stats"][ok]).all()
    # means are far from zero against the row, so a relative bar is sound
    scale = np.abs(r["rows"]).max(axis=-1)
    assert (np.abs(r["stats"][..., 0])[ok] > 1e-3 * scale[ok]).all()
    # the on-pulse sum is no cancellation where the S/N is compared
    sn = ok & (r["stats"][..., 1] > 0)
    assert (r["cond"][sn] < 1e3).all()
    if c.get("exact"):
        assert (r["total"] == np.rint(r["total"])).all()
        assert (r["sums"] == np.rint(r["sums"])).all()
        assert np.abs(r["sums"]).max() < 2.0 ** 52
    for s in range(c["nsub"]):
        if "tie" in c:
            a, b = c["tie"]
            mins = np.flatnonzero(r["sums"][s] == r["sums"][s].min())
            if b is None:
                assert mins.size == c["nbin"]
            else:
                assert list(mins) == [a, b]
                assert r["sums"][s][a] == r["sums"][s][b]
            assert r["wstart"][s] == a
        else:
            # a unique minimum, clear of the rounding of any order of sums
            assert U.margin(r["sums"][s]) > 1e-9, U.margin(r["sums"][s])
        if "starts" in c:
            assert r["wstart"][s] == c["starts"][s]


@pytest.mark.parametrize("name", SMALL)
def test_kernel_order_gives_the_reference_window(name):
    """The kernel's own order of sums, restated, lands on the reference's
    first minimum in every case; at the cases built for it, each broken
    variant does not."""
    c, r = U.case(name), U.reference(name)
    for s in range(c["nsub"]):
        assert kernel_window(r["total"][s], r["W"]) == r["wstart"][s]


def _wrong(name, **kw):
    r = U.reference(name)
    return [s for s in range(len(r["wstart"]))
            if kernel_window(r["total"][s], r["W"], **kw) != r["wstart"][s]]


def test_cases_discriminate_window_mistakes():
    # <= within a thread's share: the later of two equal starts of a thread
    assert _wrong("tie-near-1000", lt_thread=np.less_equal)
    assert _wrong("flat-1000", lt_thread=np.less_equal)
    # <= in the reduction: the later of two threads
    assert _wrong("tie-far-64", lt_reduce=np.less_equal)
    assert _wrong("tie-far-1000", lt_reduce=np.less_equal)
    assert _wrong("flat-64", lt_reduce=np.less_equal)
    # no modulo in the sliding update: a window that wraps, reached by a
    # thread's second or later start
    c = U.case("dip-1000")
    first_wrap = 1000 - U.window(1000) + 1
    assert first_wrap % U.per(1000)
    assert c["starts"].index(first_wrap) in _wrong("dip-1000", wrap=False)
    # the tie cases sit where they are meant to
    a, b = U.case("tie-near-1000")["tie"]
    assert a // U.per(1000) == b // U.per(1000)
    a, b = U.case("tie-far-1000")["tie"]
    assert a // U.per(1000) != b // U.per(1000)


def test_weight_cases():
    c, r = U.case("heavy"), U.reference("heavy")
    assert (r["wstart"] == 40).all()
    free = U.baseline(r["rows"], None)
    assert list(free["wstart"]) == c["unweighted"]
    c, r = U.case("zero-weight"), U.reference("zero-weight")
    bad = U.unpacked(c, c["poison"])
    for n in c["zero"]:
        assert np.isnan(bad[:, n]).any() and np.isinf(bad[:, n]).any()
    ok = U.live_rows(c)
    np.testing.assert_array_equal(bad[ok], r["rows"][ok])
    # the reference skips zero weights as the entry does
    rb = U.baseline(bad, c["wts"])
    np.testing.assert_array_equal(rb["total"], r["total"])
    np.testing.assert_array_equal(rb["wstart"], r["wstart"])


def test_degenerate_cases():
    c, r = U.case("constant"), U.reference("constant")
    n = c["constant"]
    assert (r["stats"][:, n, 1:] == 0).all()
    assert (r["removed"][:, n] == 0).all()
    assert (np.ptp(r["rows"][:, n], axis=-1) == 0).all()
    for name in ("edge-rand-2", "edge-dip-2"):
        r = U.reference(name)
        assert r["W"] == 1 and U.case(name)["nbin"] - r["W"] == 1
        assert (r["stats"][..., 1:] == 0).all()       # one bin: sigma 0


@pytest.mark.parametrize("name", list(U.FILES))
def test_written_files_read_back(tmp_path, name):
    """write_psrfits_rows with each sample type: the reader returns the
    bytes, the element type load_data maps to elem, and the layout."""
    from pulseportraiture_amd import psrfits as PF
    c = U.file_case(name)
    code, npol, pol_type, pol_mode = U.FILES[name]
    f = PF.PSRFITS(U.write_file(name, str(tmp_path / "f.fits")))
    try:
        assert (f.nsub, f.npol, f.nchan, f.nbin) == \
            (c["nsub"], npol, c["nchan"], c["nbin"])
        assert f.pol_type == pol_type
        raw, dt = f.data_bytes()
        assert dt == np.dtype(U.DT[c["elem"]])
        assert f.subint.columns["DATA"][3] == code
        np.testing.assert_array_equal(np.asarray(raw), c["raw"])
        s, o = f.scales_offsets()
        np.testing.assert_array_equal(s, c["scl"])
        np.testing.assert_array_equal(o, c["offs"])
        # what load_data uploads: the first one or two polarisation blocks
        assert c["npol_raw"] == npol and U.used_pols(c) == 1 + pol_mode
    finally:
        f.close()
    with pytest.raises(ValueError):
        PF.write_psrfits_rows(str(tmp_path / "g.fits"), c["raw"], c["scl"],
                              c["offs"], np.ones((c["nsub"], c["nchan"])),
                              None, None, None, None, c["nbin"], npol=npol,
                              elem="J")
