"""Batched device engine: torch tensors in, libppfit kernels, torch tensors out.

PyTorch supplies device memory, the current HIP stream and (in dist.py) the
RCCL communicator; all arithmetic happens in libppfit's HIP kernels.  Every
function here accepts numpy arrays or torch tensors (host or device) and
returns device tensors; the drop-in modules (pplib / pptoaslib / pptoas)
convert to the reference's numpy/DataBunch forms.
"""
import ctypes
import functools
import os
import threading
import warnings

import numpy as np
import torch

from . import _lib
from .timeline import span

DEVICE_TYPE = "cuda"   # torch's name for HIP devices on ROCm


def device(dev=None):
    if not torch.cuda.is_available():
        raise RuntimeError("pulseportraiture_amd needs a HIP device "
                           "(torch.cuda.is_available() is False); there is "
                           "no CPU fallback")
    if dev is None:
        return torch.device(DEVICE_TYPE, torch.cuda.current_device())
    dev = torch.device(dev)
    if dev.type != DEVICE_TYPE:
        raise ValueError("device must be a HIP device, got %s" % dev)
    return dev if dev.index is not None else torch.device(
        DEVICE_TYPE, torch.cuda.current_device())


def to_dev(x, dev, dtype):
    """Contiguous device tensor of dtype (None passes through)."""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    a = np.ascontiguousarray(x)
    if not a.flags.writeable:
        # the host array is only read (copied to the device): torch's
        # warning about non-writable NumPy memory does not apply
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return torch.as_tensor(a, dtype=dtype).to(dev)
    return torch.as_tensor(a, dtype=dtype).to(dev)


_PIN = {}
_PIN_LOCK = threading.Lock()


def _pinned(tag, nbytes):
    """A page-locked staging buffer of at least nbytes, one per (thread,
    tag), grown on demand and reused: the single-call APIs copy their host
    arrays through it instead of torch's pageable path (whose per-call
    staging made a 512 x 2048 rotate_data take 1.6-25 ms)."""
    key = (threading.get_ident(), tag)
    with _PIN_LOCK:
        buf = _PIN.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8,
                              pin_memory=True)
            _PIN[key] = buf
    return buf


_STAGE = threading.local()
# fit inputs staged by ppf_copy_from_pinned's kernel (1) or a copy-engine
# transfer (0); env PPF_STAGE_KERNEL
_STAGE_KERNEL = os.environ.get("PPF_STAGE_KERNEL", "1") != "0"
_NPD = {torch.float64: np.float64, torch.float32: np.float32,
        torch.int32: np.int32, torch.uint8: np.uint8}


def _stage_host(items, dev):
    """[(host array, torch dtype)] -> device tensors of the same shapes:
    the arrays are packed (256-B aligned) into one of the calling thread's
    two page-locked buffers and copied with ONE non-blocking copy on the
    current stream; a buffer is refilled only after the copy that last
    read it has completed (its event)."""
    arrs = [np.ascontiguousarray(x, dtype=_NPD[dt]) for x, dt in items]
    offs, o = [], 0
    for a in arrs:
        offs.append(o)
        o += -(-a.nbytes // 256) * 256
    total = max(o, 256)
    ring = getattr(_STAGE, "ring", None)
    if ring is None:
        ring = _STAGE.ring = [[[None, None], [None, None]], 0]
    slot = ring[0][ring[1] % 2]
    ring[1] += 1
    if slot[1] is not None:
        slot[1].synchronize()
    if slot[0] is None or slot[0].numel() < total:
        slot[0] = torch.empty(max(total, 1 << 20), dtype=torch.uint8,
                              pin_memory=True)
    hb = slot[0].numpy()
    for a, off in zip(arrs, offs):
        hb[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
    d = torch.empty(total, dtype=torch.uint8, device=dev)
    global _STAGE_KERNEL
    staged = False
    if _STAGE_KERNEL:
        # read by a kernel over PCIe: no copy-engine transfer, so it never
        # queues behind an archive upload (ppf_copy_from_pinned).  A pinned
        # buffer the device cannot map (host-registered without the mapped
        # flag, another allocator) makes the call return an error: then the
        # copy engine takes this and every later staging of the process
        ctx = _lib.context(dev.index)
        rc = _lib.load().ppf_copy_from_pinned(
            ctx, _p(d), ctypes.c_void_p(slot[0].data_ptr()), total,
            _stream(dev))
        if rc == 0:
            staged = True
        else:
            _STAGE_KERNEL = False
    if not staged:
        d.copy_(slot[0][:total], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    slot[1] = ev
    return [d[off:off + a.nbytes].view(dt).view(a.shape)
            for a, (_, dt), off in zip(arrs, items, offs)]


def host_to_dev(x, dev, dtype):
    """to_dev through the caller's pinned staging buffer (the copy is
    ordered on the current stream; the buffer is reused only by the same
    thread's next call, which comes after this call's own synchronising
    read-back)."""
    a = np.ascontiguousarray(x)
    t = torch.as_tensor(a) if a.flags.writeable else torch.from_numpy(a.copy())
    t = t.to(dtype)
    buf = _pinned("in", t.numel() * t.element_size())
    h = buf[:t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    h.copy_(t)
    return h.to(dev, non_blocking=True)


def dev_to_host(t):
    """A NumPy copy of device tensor t, read back through the caller's
    pinned staging buffer (synchronises the current stream)."""
    n = t.numel() * t.element_size()
    buf = _pinned("out", n)
    h = buf[:n].view(t.dtype).view(t.shape)
    h.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return h.numpy().copy()


def dev_to_host_view(t):
    """dev_to_host without the final copy: a NumPy view of the caller's
    page-locked "view" buffer holding device tensor t (synchronises the
    current stream).  Valid until the same thread's next call."""
    n = t.numel() * t.element_size()
    buf = _pinned("view", n)
    h = buf[:n].view(t.dtype).view(t.shape)
    h.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return h.numpy()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _data_dtype(x):
    if isinstance(x, torch.Tensor):
        return torch.float32 if x.dtype == torch.float32 else torch.float64
    return torch.float32 if np.asarray(x).dtype == np.float32 else \
        torch.float64


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def x_subints(fit_flags, init, log10_tau, nsub):
    """Sub-ints whose fit streams the cross spectrum X (k_classify's test,
    restated on the host): scattering flags set, or a nonzero initial tau
    (10**tau with log10_tau, pptoaslib.py:271-276)."""
    fl = _host(fit_flags).reshape(-1, 5)
    if fl.shape[0] == 1:
        fl = np.repeat(fl, nsub, axis=0)
    x3 = _host(init).reshape(nsub, 5)[:, 3]
    with np.errstate(over="ignore"):
        tau0 = 10.0 ** x3 if log10_tau else x3
    return int(np.count_nonzero((fl[:, 3] != 0) | (fl[:, 4] != 0) |
                                (tau0 != 0.0)))


SOLVER = os.environ.get("PPF_SOLVER", "newton")
# phase/DM/GM moments: None = the library's choice (from the stored cross
# spectrum where the GetTOAs guess rides along in the spectrum pass), True /
# False = always from X / always from the fused k_xmom_g pass (env PPF_MOM_X
# = 1 / 0)
MOM_X = {"1": True, "0": False}.get(os.environ.get("PPF_MOM_X", ""), None)


def _solver(name):
    name = SOLVER if name is None else name
    if name not in ("newton", "scipy"):
        raise ValueError("solver must be 'newton' or 'scipy', not %r" % name)
    return name


def fit_batch(data, model, freqs, P, init, fit_flags, nu_fits=None,
              nu_outs=None, errs=None, chan_mask=None, model_index=None,
              log10_tau=False, option=0, is_toa=True, mode=_lib.PPF_MODE_FULL,
              max_iter=0, guess=False, guess_weights=None, guess_DM=None,
              guess_Ns=100, guess_tau=None, dev=None, workspace=None,
              n_x=None, no_hcut=False, max_workspace=None, guess_ref=0,
              bounds=None, solver=None, mom_x=None, spin_wait=False):
    """Fit nsub sub-integrations: data [nsub, nchan, nbin] (f32 or f64),
    model [nmodel, nchan, nbin] (or [nchan, nbin]), freqs [nsub, nchan],
    P [nsub], init [nsub, 5], fit_flags [nsub, 5] (or [5]).

    n_x: cross-spectrum slots (sub-ints whose fit streams X); None computes
    it from fit_flags / init (x_subints).  no_hcut: sum every harmonic
    (PPF_OPT_NO_HCUT).  guess_ref: frame of the guess profile (0: mean
    frequency then phase_transform to nu_fit, GetTOAs; 1: nu_fit, ppalign).
    bounds: method='TNC' box, [5, 2] or [nsub, 5, 2] (lower, upper; None or
    NaN = unbounded), or None for an unbounded fit.
    solver: minimiser of the unbounded fits, "newton" (scaled Newton trust
    region with an exact subproblem: the same stationary point, in 3x fewer
    passes over the cross spectrum for scattering fits and half the data
    passes for ppalign's) or "scipy" (scipy trust-ncg's own path,
    PPF_OPT_SCIPY_TR); None = SOLVER (env PPF_SOLVER, default "newton").
    mom_x: take the moments of the phase/DM/GM fits from the stored cross
    spectrum (True, PPF_OPT_MOM_X) or from the fused pass (False,
    PPF_OPT_FUSED_MOM); None = MOM_X (env PPF_MOM_X; unset: the library
    chooses).
    spin_wait: poll the read-backs of the iteration loop on the host
    (PPF_OPT_SPIN_WAIT) -- for callers with no host threads of their own.
    max_workspace: workspace budget in bytes (default
    half the free device memory); a batch needing more is fitted in
    consecutive chunks of sub-ints (a sub-int's result does not depend on
    the batch it is in).

    Returns a dict of device tensors: results [nsub, 32] (see
    _lib.RESULT_INDEX), scales/scale_errs/channel_snrs [nsub, nchan],
    covariance [nsub, 5, 5], and the workspace (reusable)."""
    dev = device(dev)
    f64 = torch.float64
    if n_x is None and not isinstance(init, torch.Tensor) and \
            not isinstance(fit_flags, torch.Tensor):
        # counted from the host arrays before the upload (no device
        # round trip)
        n_x = x_subints(fit_flags, init, log10_tau,
                        int(np.asarray(init).size // 5))
    data_t = to_dev(data, dev, _data_dtype(data))
    if data_t.dim() != 3:
        raise ValueError("data must be [nsub, nchan, nbin]")
    nsub, nchan, nbin = data_t.shape
    # the per-sub-int inputs that arrive as host arrays travel in ONE pinned
    # buffer and ONE asynchronous copy on the current stream (a pageable
    # copy per input synchronises the host each time and queues behind any
    # archive upload on the copy engine: GetTOAs' fit worker measured
    # ~7.7 ms per 64-sub-int archive that way)
    specs = [("freqs", freqs, f64), ("P", P, f64), ("init", init, f64),
             ("flags", fit_flags, torch.int32), ("nu_fits", nu_fits, f64),
             ("nu_outs", nu_outs, f64), ("errs", errs, f64),
             ("mask", chan_mask, torch.uint8), ("mi", model_index, torch.int32)]
    if guess:
        specs += [("gtau", guess_tau, f64), ("gw", guess_weights, f64),
                  ("gdm", guess_DM, f64)]
    host = [(k, x, dt) for k, x, dt in specs
            if x is not None and not isinstance(x, torch.Tensor)]
    if host:
        with span("fit.stage"):
            up = dict(zip([k for k, _, _ in host], _stage_host(
                [(x, dt) for _, x, dt in host], dev)))
        freqs, P, init = up.get("freqs", freqs), up.get("P", P), \
            up.get("init", init)
        fit_flags, nu_fits = up.get("flags", fit_flags), \
            up.get("nu_fits", nu_fits)
        nu_outs, errs = up.get("nu_outs", nu_outs), up.get("errs", errs)
        chan_mask, model_index = up.get("mask", chan_mask), \
            up.get("mi", model_index)
        guess_tau, guess_weights = up.get("gtau", guess_tau), \
            up.get("gw", guess_weights)
        guess_DM = up.get("gdm", guess_DM)
    model_t = to_dev(model, dev, f64)
    if model_t.dim() == 2:
        model_t = model_t.unsqueeze(0)
    if model_t.shape[1:] != (nchan, nbin):
        raise ValueError("model shape %s != [*, %d, %d]" %
                         (tuple(model_t.shape), nchan, nbin))
    freqs_t = to_dev(freqs, dev, f64).reshape(-1)
    if freqs_t.numel() == nchan:
        freqs_t = freqs_t.repeat(nsub)
    freqs_t = freqs_t.reshape(nsub, nchan).contiguous()
    P_t = to_dev(P, dev, f64).reshape(-1)
    if P_t.numel() == 1:
        P_t = P_t.repeat(nsub)
    init_t = to_dev(init, dev, f64).reshape(nsub, 5).contiguous()
    flags_t = to_dev(fit_flags, dev, torch.int32).reshape(-1)
    if flags_t.numel() == 5:
        flags_t = flags_t.repeat(nsub)
    flags_t = flags_t.reshape(nsub, 5).contiguous()
    def nan3():
        return torch.full((nsub, 3), float("nan"), dtype=f64, device=dev)
    nu_fits_t = nan3() if nu_fits is None else \
        to_dev(nu_fits, dev, f64).reshape(nsub, 3).contiguous()
    nu_outs_t = nan3() if nu_outs is None else \
        to_dev(nu_outs, dev, f64).reshape(nsub, 3).contiguous()
    errs_t = None if errs is None else \
        to_dev(errs, dev, f64).reshape(nsub, nchan).contiguous()
    mask_t = None if chan_mask is None else \
        to_dev(chan_mask, dev, torch.uint8).reshape(nsub, nchan).contiguous()
    mi_t = None if model_index is None else \
        to_dev(model_index, dev, torch.int32).reshape(nsub).contiguous()
    gw_t = gdm_t = gtau_t = None
    if guess:
        if guess_tau is not None:
            gtau_t = to_dev(guess_tau, dev, f64).reshape(-1)
            if gtau_t.numel() == 1:
                gtau_t = gtau_t.repeat(nsub)
        gw_t = to_dev(guess_weights, dev, f64).reshape(nsub, nchan).contiguous()
        gdm_t = to_dev(guess_DM, dev, f64).reshape(-1)
        if gdm_t.numel() == 1:
            gdm_t = gdm_t.repeat(nsub)
    bnd_t = None
    if bounds is not None:
        b = np.array([[np.nan if v is None else float(v) for v in lu]
                      for lu in np.asarray(bounds, dtype=object).reshape(-1, 2)
                      ], dtype=float).reshape(-1, 5, 2)
        if b.shape[0] == 1:
            b = np.repeat(b, nsub, axis=0)
        bnd_t = to_dev(b.reshape(nsub, 5, 2), dev, f64)
    per_sub = dict(data=data_t, freqs=freqs_t, P=P_t, init=init_t,
                   flags=flags_t, nu_fits=nu_fits_t, nu_outs=nu_outs_t,
                   errs=errs_t, mask=mask_t, mi=mi_t, gw=gw_t, gdm=gdm_t,
                   gtau=gtau_t, bounds=bnd_t)
    if n_x is None:
        n_x = x_subints(flags_t, init_t, log10_tau, nsub)
    xsel = None
    cfg = dict(model=model_t, log10_tau=log10_tau, option=option,
               is_toa=is_toa, mode=mode, max_iter=max_iter, guess=guess,
               guess_Ns=guess_Ns, no_hcut=no_hcut, guess_ref=guess_ref,
               solver=_solver(solver),
               mom_x=MOM_X if mom_x is None else bool(mom_x),
               spin_wait=bool(spin_wait))
    lib = _lib.load()
    d0 = _desc(per_sub, 0, nsub, n_x, cfg)
    need = _desc_workspace_bytes(lib, d0)
    if max_workspace is None and (need <= (64 << 20) or nsub == 1):
        # small batches (the single-call APIs) skip the free-memory query
        return _fit_slice(lib, dev, per_sub, 0, nsub, n_x, cfg, workspace,
                          d0, need)
    if max_workspace is None:
        free, _ = torch.cuda.mem_get_info(dev)
        max_workspace = free // 2
    if need <= max_workspace:
        return _fit_slice(lib, dev, per_sub, 0, nsub, n_x, cfg, workspace,
                          d0, need)
    # chunks of equal size whose workspace fits the budget
    per = max(1, int(nsub * max_workspace // max(need, 1)))
    while per > 1 and _workspace_bytes(lib, per_sub, 0, per, per, cfg) > \
            max_workspace:
        per //= 2
    if xsel is None:
        fl = _host(flags_t)
        x3 = _host(init_t)[:, 3]
        with np.errstate(over="ignore"):
            tau0 = 10.0 ** x3 if log10_tau else x3
        xsel = (fl[:, 3] != 0) | (fl[:, 4] != 0) | (tau0 != 0.0)
    outs, ws = [], None
    for c0 in range(0, nsub, per):
        c1 = min(nsub, c0 + per)
        r = _fit_slice(lib, dev, per_sub, c0, c1,
                       int(np.count_nonzero(xsel[c0:c1])), cfg, ws)
        ws = r["workspace"]
        outs.append(r)
    out = {k: torch.cat([o[k] for o in outs], 0)
           for k in ("results", "scales", "scale_errs", "channel_snrs",
                     "covariance")}
    out["workspace"] = ws
    out["_keep"] = tuple(o["_keep"] for o in outs)
    return out


def _desc(per_sub, c0, c1, n_x, cfg):
    """ppf_fit_desc of sub-ints [c0, c1) (pointers into the device tensors;
    outputs left NULL)."""
    sl = slice(c0, c1)

    def pp(t):
        return None if t is None else _p(t[sl])
    data_t = per_sub["data"]
    nchan, nbin = data_t.shape[1:]
    model_t = cfg["model"]
    d = _lib.FitDesc()
    d.nsub, d.nchan, d.nbin = c1 - c0, nchan, nbin
    d.data_dtype = _lib.PPF_F32 if data_t.dtype == torch.float32 else \
        _lib.PPF_F64
    d.data, d.model, d.nmodel = pp(data_t), _p(model_t), model_t.shape[0]
    d.model_index, d.chan_mask = pp(per_sub["mi"]), pp(per_sub["mask"])
    d.freqs, d.P, d.errs = pp(per_sub["freqs"]), pp(per_sub["P"]), \
        pp(per_sub["errs"])
    d.init, d.fit_flags = pp(per_sub["init"]), pp(per_sub["flags"])
    d.nu_fits, d.nu_outs = pp(per_sub["nu_fits"]), pp(per_sub["nu_outs"])
    d.log10_tau, d.option = int(bool(cfg["log10_tau"])), int(cfg["option"])
    d.is_toa = int(bool(cfg["is_toa"]))
    d.mode, d.max_iter = int(cfg["mode"]), int(cfg["max_iter"])
    d.guess, d.guess_Ns = int(bool(cfg["guess"])), int(cfg["guess_Ns"])
    d.guess_weights, d.guess_DM = pp(per_sub["gw"]), pp(per_sub["gdm"])
    d.guess_tau = pp(per_sub["gtau"])
    d.x_subints = int(max(n_x, 1)) if n_x < (c1 - c0) else 0
    d.options = (_lib.OPT_NO_HCUT if cfg["no_hcut"] else 0) | \
        (_lib.OPT_NO_X if n_x == 0 else 0) | \
        (_lib.OPT_SCIPY_TR if cfg.get("solver") == "scipy" else 0) | \
        (_lib.OPT_MOM_X if cfg.get("mom_x") is True else 0) | \
        (_lib.OPT_FUSED_MOM if cfg.get("mom_x") is False else 0) | \
        (_lib.OPT_SPIN_WAIT if cfg.get("spin_wait") else 0)
    d.guess_ref = int(cfg["guess_ref"])
    d.bounds = pp(per_sub["bounds"])
    return d


def _workspace_bytes(lib, per_sub, c0, c1, n_x, cfg):
    return _desc_workspace_bytes(lib, _desc(per_sub, c0, c1, n_x, cfg))


def _desc_workspace_bytes(lib, d):
    nbytes = lib.ppf_fit_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise NotImplementedError(
            "unsupported shape nsub=%d nchan=%d nbin=%d (nbin must be even in"
            " [32, 8192] or odd in [33, 4095]; longer rows fit without the"
            " GetTOAs guess, up to 2^23 transform points)" %
            (d.nsub, d.nchan, d.nbin))
    return nbytes


def _fit_slice(lib, dev, per_sub, c0, c1, n_x, cfg, workspace, d=None,
               nbytes=None):
    """ppf_fit_batch over sub-ints [c0, c1) (d / nbytes: their descriptor
    and workspace size when the caller has them).  The outputs are views of
    ONE zeroed float64 buffer ("_flat": results | scales | scale_errs |
    channel_snrs | covariance), which a caller may download in one copy."""
    nsub = c1 - c0
    nchan = per_sub["data"].shape[1]
    R = _lib.RESULT_DOUBLES
    sizes = (nsub * R, nsub * nchan, nsub * nchan, nsub * nchan, nsub * 25)
    flat = torch.zeros(sum(sizes), dtype=torch.float64, device=dev)
    views, o = [], 0
    for n in sizes:
        views.append(flat[o:o + n])
        o += n
    results = views[0].view(nsub, R)
    scales, scale_errs, channel_snrs = (v.view(nsub, nchan)
                                        for v in views[1:4])
    cov = views[4].view(nsub, 5, 5)
    if d is None:
        d = _desc(per_sub, c0, c1, n_x, cfg)
    if nbytes is None:
        nbytes = _desc_workspace_bytes(lib, d)
    d.results, d.scales, d.scale_errs = _p(results), _p(scales), \
        _p(scale_errs)
    d.channel_snrs, d.covariance = _p(channel_snrs), _p(cov)
    if workspace is None or workspace.numel() < nbytes or \
            workspace.device != dev:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = _p(workspace), workspace.numel()
    ctx = _lib.context(dev.index)
    with span("fit.lib"):
        rc = lib.ppf_fit_batch(ctx, ctypes.byref(d), _stream(dev))
    _lib.check(rc, ctx)
    # keep inputs alive until the stream has consumed them
    keep = (cfg["model"],) + tuple(v for v in per_sub.values()
                                   if v is not None)
    return dict(results=results, scales=scales, scale_errs=scale_errs,
                channel_snrs=channel_snrs, covariance=cov,
                workspace=workspace, _keep=keep, _flat=flat)


def rotate_rows(rows, phases, dev=None, ref_len=False):
    """irfft(rfft(row) * exp(2 pi i k phase)) for each row of rows [..., nbin]
    (float64 output, same leading shape).  ref_len: the reference's public
    rotate routines' length-less irfft (ppf_rotate_batch_ref): nbin - 1
    samples per row at odd nbin; otherwise (internal callers) nbin."""
    dev = device(dev)
    r = to_dev(rows, dev, _data_dtype(rows)) if isinstance(rows, torch.Tensor) \
        else host_to_dev(rows, dev, _data_dtype(rows))
    shape = r.shape
    nbin = shape[-1]
    r2 = r.reshape(-1, nbin).contiguous()
    ph = to_dev(phases, dev, torch.float64).reshape(-1).contiguous()
    if ph.numel() != r2.shape[0]:
        raise ValueError("need one phase per row")
    nout = nbin - 1 if (ref_len and nbin % 2) else nbin
    out = torch.empty((r2.shape[0], nout), dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    lib = _lib.load()
    if not _noise_batch_len_ok(nbin):
        # past the LDS transforms (even > 8192, odd > 4095; the same rule as
        # ppf_noise_batch): Bluestein transforms both ways (ppf_rotate_long)
        nb = lib.ppf_rotate_long_workspace_bytes(r2.shape[0], nbin,
                                                 int(bool(ref_len)))
        if nb == 0:
            raise NotImplementedError(
                "rotation of %d-sample rows: past the 2^23-point transform"
                % nbin)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        rc = lib.ppf_rotate_long(
            ctx, r2.shape[0], nbin,
            _lib.PPF_F32 if r2.dtype == torch.float32 else _lib.PPF_F64,
            _p(r2), _p(ph), _p(out), int(bool(ref_len)), _p(ws), nb,
            _stream(dev))
        _lib.check(rc, ctx)
        return out.reshape(tuple(shape[:-1]) + (nout,))
    fn = lib.ppf_rotate_batch_ref if ref_len else lib.ppf_rotate_batch
    rc = fn(ctx, r2.shape[0], nbin,
            _lib.PPF_F32 if r2.dtype == torch.float32 else _lib.PPF_F64,
            _p(r2), _p(ph), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out.reshape(tuple(shape[:-1]) + (nout,))


def inst_response_len_ok(nbin):
    """Row lengths ppf_inst_response_batch takes: even, 32..8192."""
    return nbin % 2 == 0 and 32 <= nbin <= 8192


def inst_response_rows(src, src_row, table, widths, dev=None):
    """out[r] = irfft(rfft(src[src_row[r]]) * table * sinc(k widths[r])) on the
    device (ppf_inst_response_batch, k_inst_resp): the instrumental response
    of pptoaslib.instrumental_response_port_FT on template rows.  src
    [nsrc, nbin] (array or device tensor, taken as float64); src_row [nrows]
    indices into src (checked here: the kernel trusts them); table
    [nbin // 2 + 1] or None (all ones); widths [nrows] in rotations.  Returns
    a float64 device tensor [nrows, nbin].  Odd nbin and nbin > 8192 raise
    NotImplementedError."""
    dev = device(dev)
    s = to_dev(src, dev, torch.float64)
    if s.dim() != 2:
        raise ValueError("src must be [nsrc, nbin]")
    nsrc, nbin = s.shape
    idx = np.ascontiguousarray(src_row, dtype=np.int32).reshape(-1)
    w = np.ascontiguousarray(widths, dtype=np.float64).reshape(-1)
    if w.size != idx.size:
        raise ValueError("need one width per output row")
    if idx.size and (idx.min() < 0 or idx.max() >= nsrc):
        raise ValueError("src_row out of range")
    if table is not None:
        table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        if table.size != nbin // 2 + 1:
            raise ValueError("table must hold nbin // 2 + 1 harmonics")
    if not inst_response_len_ok(nbin):
        raise NotImplementedError(
            "instrumental response at nbin = %d: even nbin from 32 to 8192 "
            "only" % nbin)
    out = torch.empty((idx.size, nbin), dtype=torch.float64, device=dev)
    if not idx.size:
        return out
    # the small arrays in one staged upload
    items = [(idx, torch.int32), (w, torch.float64)]
    if table is not None:
        items.append((table, torch.float64))
    staged = _stage_host(items, dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_inst_response_batch(
        ctx, idx.size, nbin, _p(s), _p(staged[0]),
        None if table is None else _p(staged[2]), _p(staged[1]), _p(out),
        _stream(dev))
    _lib.check(rc, ctx)
    return out


def align_accum(data, phases, weights, out, wsum, dev=None):
    """ppalign accumulation on the device (ppf_align_accum):
    out[n] += sum_s w[s,n] rotate(data[s,n], phases[s,n]); wsum[n] += sum_s
    w[s,n].  data [nsub, nchan, nbin]; out [nchan, nbin] and wsum [nchan] are
    float64 device tensors updated in place."""
    dev = device(dev)
    d = to_dev(data, dev, _data_dtype(data))
    if d.dim() != 3:
        raise ValueError("data must be [nsub, nchan, nbin]")
    nsub, nchan, nbin = d.shape
    ph = to_dev(phases, dev, torch.float64).reshape(nsub, nchan).contiguous()
    w = to_dev(weights, dev, torch.float64).reshape(nsub, nchan).contiguous()
    if out.shape != (nchan, nbin) or out.dtype != torch.float64 or \
            wsum.shape != (nchan,) or wsum.dtype != torch.float64:
        raise ValueError("out must be float64 [nchan, nbin], wsum [nchan]")
    lib = _lib.load()
    if not _noise_batch_len_ok(nbin):
        # rows past the LDS transforms: the rotations on the long transforms
        # (ppf_rotate_long), the weighted sum over sub-ints on the stream;
        # rows of weight 0 contribute nothing whatever they hold
        rot = rotate_rows(d, ph, dev).reshape(nsub, nchan, nbin)
        wr = w.unsqueeze(-1)
        out += torch.where(wr != 0.0, wr * rot, 0.0).sum(dim=0)
        wsum += w.sum(dim=0)
        return out, wsum
    nbytes = lib.ppf_align_workspace_bytes(nsub, nchan, nbin)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    ctx = _lib.context(dev.index)
    rc = lib.ppf_align_accum(
        ctx, nsub, nchan, nbin,
        _lib.PPF_F32 if d.dtype == torch.float32 else _lib.PPF_F64,
        _p(d), _p(ph), _p(w), _p(out), _p(wsum), _p(ws), int(nbytes),
        _stream(dev))
    _lib.check(rc, ctx)
    return out, wsum


def align_phases(results, freqs, P, mask, scales, errs, dev=None):
    """ppalign's per-row rotation phases and weights from fit results
    (ppf_align_phases, ppalign.py:222-247): device tensors results [nsub,
    32], freqs / scales / errs [nsub, nchan] float64, P [nsub], mask [nsub,
    nchan] uint8 (or None) -> (phases, weights) [nsub, nchan] float64."""
    dev = device(dev)
    nsub, nchan = freqs.shape
    for t in (results, freqs, P, scales, errs):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("align_phases takes contiguous float64 tensors")
    ph = torch.empty((nsub, nchan), dtype=torch.float64, device=dev)
    wt = torch.empty((nsub, nchan), dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_align_phases(
        ctx, nsub, nchan, _p(results), _p(freqs), _p(P),
        None if mask is None else _p(mask), _p(scales), _p(errs), _p(ph),
        _p(wt), _stream(dev))
    _lib.check(rc, ctx)
    return ph, wt


def resid_chi2_rows(rows, phases, model_rows, model_index, scales, errs, dof,
                    dev=None):
    """Per row: sum_t (rotate(row, phase) - scale * model_rows[index])^2 /
    err^2 / dof (ppf_resid_chi2_batch) -> float64 [nrows]."""
    dev = device(dev)
    r = to_dev(rows, dev, _data_dtype(rows))
    nbin = r.shape[-1]
    r2 = r.reshape(-1, nbin).contiguous()
    n = r2.shape[0]
    ph = to_dev(phases, dev, torch.float64).reshape(-1).contiguous()
    m = to_dev(model_rows, dev, torch.float64).reshape(-1, nbin).contiguous()
    mi = to_dev(model_index, dev, torch.int32).reshape(-1).contiguous()
    sc = to_dev(scales, dev, torch.float64).reshape(-1).contiguous()
    er = to_dev(errs, dev, torch.float64).reshape(-1).contiguous()
    if not (ph.numel() == mi.numel() == sc.numel() == er.numel() == n):
        raise ValueError("need one phase / model index / scale / err per row")
    if n and (int(mi.min()) < 0 or int(mi.max()) >= m.shape[0]):
        raise ValueError("model index out of range")
    if not _noise_batch_len_ok(nbin):
        # rows past the LDS transforms (round 6): the rotation on the long
        # transforms (ppf_rotate_long, full nbin as k_resid_chi2's), the
        # residual sum of squares on the stream
        rot = rotate_rows(r2, ph, dev)
        res = (rot - sc.unsqueeze(-1) * m[mi.long()]) / er.unsqueeze(-1)
        return (res * res).sum(dim=-1) / float(dof)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_resid_chi2_batch(
        ctx, n, nbin, _lib.PPF_F32 if r2.dtype == torch.float32 else
        _lib.PPF_F64, _p(r2), _p(ph), _p(m), _p(mi), _p(sc), _p(er),
        float(dof), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out


def pinned_host_array(shape, dtype=np.float32):
    """A NumPy array in page-locked host memory (a torch pinned buffer; the
    array keeps it alive).  An archive loaded into one is uploaded by
    GetTOAs' stager straight from it, without the copy into its own pinned
    buffers."""
    t = torch.empty(tuple(shape), dtype=torch.from_numpy(
        np.zeros(0, dtype=dtype)).dtype, pin_memory=True)
    return t.numpy()


def _noise_batch_len_ok(nbin):
    """Row lengths ppf_noise_batch's LDS transforms take (nbin_supported)."""
    return 32 <= nbin <= 8192 and (nbin % 2 == 0 or nbin <= 4095)


def noise_rows(rows, frac=4, dev=None):
    """get_noise_PS per row of rows [..., nbin] -> [...] float64 (rows past
    the LDS transforms: ppf_noise_long)."""
    dev = device(dev)
    r = to_dev(rows, dev, _data_dtype(rows))
    shape = r.shape
    r2 = r.reshape(-1, shape[-1]).contiguous()
    if not _noise_batch_len_ok(shape[-1]):
        return noise_rows_long(r2, frac, dev).reshape(shape[:-1])
    out = torch.empty(r2.shape[0], dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_noise_batch(
        ctx, r2.shape[0], shape[-1],
        _lib.PPF_F32 if r2.dtype == torch.float32 else _lib.PPF_F64,
        _p(r2), int(frac), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out.reshape(shape[:-1])


# largest prime factor of the transform length the LDS path takes for
# get_noise_PS of a single flattened row: the generic-radix stage costs
# O(N R) per row (R the prime), so a length like 8186 = 2 x 4093 would be a
# 4093-point direct DFT inside one workgroup; ppf_noise_long's Bluestein
# transform is faster
NOISE_MAX_PRIME = 61


def _max_prime_factor(n):
    p, m, f = 2, n, 1
    while p * p <= m:
        while m % p == 0:
            f, m = p, m // p
        p += 1
    return max(f, m) if m > 1 else f


def noise_len_supported(n):
    """Row lengths get_noise_PS(chans=False) sends to ppf_noise_batch (its LDS
    FFT): even 32..8192 or odd 33..4095 (every length ppf_noise_batch
    accepts) whose transform length -- n / 2 complex points at even n, n at
    odd n -- has no prime factor above NOISE_MAX_PRIME; the rest go to
    ppf_noise_long (noise_long)."""
    if not 32 <= n <= (8192 if n % 2 == 0 else 4095):
        return False
    return _max_prime_factor(n // 2 if n % 2 == 0 else n) <= NOISE_MAX_PRIME


def noise_rows_long(rows, frac=4, dev=None):
    """get_noise_PS of rows [nrows, nbin] of any length (pplib.py:2312-2338)
    on ppf_noise_long: a four-step rFFT of block LDS transforms, or
    Bluestein's chirp z-transform on one, up to 2^24 complex points ->
    [nrows] float64 on the device."""
    dev = device(dev)
    r = to_dev(rows, dev, _data_dtype(rows))
    r2 = r.reshape(-1, r.shape[-1]).contiguous()
    nrows, nbin = r2.shape
    lib = _lib.load()
    nb = lib.ppf_noise_long_workspace_bytes(nrows, nbin)
    if nb == 0:
        raise NotImplementedError(
            "get_noise_PS of %d-sample rows: past the 2^24-point transform"
            % nbin)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.empty(nrows, dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = lib.ppf_noise_long(
        ctx, nrows, nbin,
        _lib.PPF_F32 if r2.dtype == torch.float32 else _lib.PPF_F64,
        _p(r2), int(frac), _p(out), _p(ws), nb, _stream(dev))
    _lib.check(rc, ctx)
    return out


def noise_long(row, frac=4, dev=None):
    """get_noise_PS of ONE row of any length (pplib.py:2334-2338: the
    flattened portrait of get_noise(chans=False)): the mean power of the top
    1/frac of the rFFT, float64 (ppf_noise_long)."""
    x = to_dev(row, device(dev), None if isinstance(row, torch.Tensor)
               else torch.float64)
    return float(noise_rows_long(x.reshape(1, -1), frac, dev).cpu()[0])


FIND_KC_FN = {"exp_dc": 0, "half_tri": 1}


@functools.lru_cache(maxsize=64)
def find_kc_tables(nharm, fn="exp_dc"):
    """The width grid of find_kc (pplib.py:1541-1551) for a power spectrum of
    nharm harmonics, and the kc each of its 20 values stands for
    (pplib.py:1553-1559): (a_grid float64 [20], kc_table int32 [20]).  Both
    depend on nharm alone, so they are formed here (once per nharm: cached,
    read-only) with NumPy as the reference forms them -- scipy.optimize.brute's grid is
    np.mgrid[lo:hi:20j] -- and no device exp decides a kc."""
    n = int(nharm)
    if fn == "exp_dc":
        a = np.mgrid[slice(n ** -1, 1.0, complex(20))]
        kc = np.empty(20, dtype=np.int32)
        for i, ai in enumerate(a):
            below = np.where(np.exp(-ai * np.arange(n)) < 0.005)[0]
            kc[i] = below.min() if len(below) else n - 1
    elif fn == "half_tri":
        a = np.mgrid[slice(1, n, complex(20))]
        kc = np.floor(a).astype(np.int32)
    else:
        raise KeyError(fn)
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)                # cached: shared by every caller
    kc.setflags(write=False)
    return a, kc


def noise_fit_rows(rows, fact=1.1, dev=None):
    """get_noise_fit per row of rows [..., nbin] (pplib.py:2341-2364) ->
    (noise float64 [...], kc int32 [...]) on the device: ppf_noise_fit_batch
    at the lengths of its LDS transforms, ppf_noise_fit_long past them."""
    dev = device(dev)
    r = to_dev(rows, dev, _data_dtype(rows))
    shape = r.shape
    r2 = r.reshape(-1, shape[-1]).contiguous()
    nrows, nbin = r2.shape
    lib = _lib.load()
    long_rows = not _noise_batch_len_ok(nbin)
    if long_rows:
        nb = lib.ppf_noise_fit_long_workspace_bytes(nrows, nbin)
        if nb == 0:
            raise NotImplementedError(
                "get_noise_fit of %d-sample rows: fewer than 2 harmonics, or "
                "past the 2^24-point transform" % nbin)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    a_grid, kc_table = find_kc_tables(nbin // 2 + 1)
    noise = torch.empty(nrows, dtype=torch.float64, device=dev)
    kc = torch.empty(nrows, dtype=torch.int32, device=dev)
    dt = _lib.PPF_F32 if r2.dtype == torch.float32 else _lib.PPF_F64
    ctx = _lib.context(dev.index)
    if long_rows:
        rc = lib.ppf_noise_fit_long(
            ctx, nrows, nbin, dt, _p(r2), float(fact), a_grid.ctypes.data,
            kc_table.ctypes.data, _p(noise), _p(kc), _p(ws), nb, _stream(dev))
    else:
        rc = lib.ppf_noise_fit_batch(
            ctx, nrows, nbin, dt, _p(r2), float(fact), a_grid.ctypes.data,
            kc_table.ctypes.data, _p(noise), _p(kc), _stream(dev))
    _lib.check(rc, ctx)
    return noise.reshape(shape[:-1]), kc.reshape(shape[:-1])


def find_kc_rows(pows, errs=1.0, fn="exp_dc", dev=None):
    """find_kc (pplib.py:1530-1561) of each power spectrum in pows
    [..., nharm] -> kc int32 [...] on the device (ppf_find_kc_batch).  errs:
    a scalar or [nharm] uncertainties of log10(pows), shared by the rows."""
    dev = device(dev)
    p = to_dev(pows, dev, torch.float64)
    shape = p.shape
    p2 = p.reshape(-1, shape[-1]).contiguous()
    nrows, nharm = p2.shape
    a_grid, kc_table = find_kc_tables(nharm, fn)
    e = to_dev(np.atleast_1d(np.asarray(errs, dtype=np.float64)), dev,
               torch.float64).contiguous()
    kc = torch.empty(nrows, dtype=torch.int32, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_find_kc_batch(
        ctx, nrows, nharm, _p(p2), _p(e), e.numel(), FIND_KC_FN[fn],
        a_grid.ctypes.data, kc_table.ctypes.data, _p(kc), _stream(dev))
    _lib.check(rc, ctx)
    return kc.reshape(shape[:-1])


def _unpack(entry, npol_in, npol_out, raw, elem, nchan, nbin, scl, offs, wts,
            mode, rm_baseline, dev):
    """The body of unpack_psrfits (npol_out 1, mode = pol_mode) and
    unpack_psrfits_pol (npol_out 4, mode = conv): npol_in blocks of scl /
    offs per sub-int; entry is the library function to call."""
    dev = device(dev)
    nsub = raw.shape[0]
    f32 = torch.float32
    scl_t = to_dev(scl, dev, f32).reshape(nsub, npol_in * nchan).contiguous()
    offs_t = to_dev(offs, dev, f32).reshape(nsub, npol_in * nchan).contiguous()
    wts_t = None if wts is None else \
        to_dev(wts, dev, f32).reshape(nsub, nchan).contiguous()
    shape = (nsub, nchan) if npol_out == 1 else (nsub, npol_out, nchan)
    rows = torch.empty(shape + (nbin,), dtype=f32, device=dev)
    stats = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
    total = torch.empty((nsub, nbin), dtype=torch.float64, device=dev)
    wstart = torch.empty(nsub, dtype=torch.int32, device=dev)
    lib = _lib.load()
    wsb = int(lib.ppf_unpack_workspace_bytes(nsub, nchan, nbin))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    ctx = _lib.context(dev.index)
    # (the intensity entry takes the file's npol; the polarised one has 4)
    dims = (npol_in, nchan, nbin) if npol_out == 1 else (nchan, nbin)
    rc = getattr(lib, entry)(
        ctx, nsub, *dims, int(elem), _p(raw), int(raw.stride(0)), _p(scl_t),
        _p(offs_t), None if wts_t is None else _p(wts_t), int(mode),
        int(bool(rm_baseline)), _p(rows), _p(stats), _p(total), _p(wstart),
        _p(ws), wsb, _stream(dev))
    _lib.check(rc, ctx)
    return dict(rows=rows, stats=stats, total=total, wstart=wstart,
                _keep=(scl_t, offs_t, wts_t, ws, raw))


def unpack_psrfits(raw, elem, npol, nchan, nbin, scl, offs, wts=None,
                   pol_mode=0, rm_baseline=True, dev=None):
    """ppf_unpack_psrfits_batch: raw DATA bytes [nsub, >= npol nchan nbin
    esize] (device uint8 tensor, one row per sub-int, as stored in the
    file) -> dict(rows float32 [nsub, nchan, nbin], stats float64
    [nsub, nchan, 3] (off-pulse mean, sigma, S/N), total float64
    [nsub, nbin], wstart int32 [nsub]), all on the device."""
    return _unpack("ppf_unpack_psrfits_batch", npol, 1, raw, elem, nchan, nbin,
                   scl, offs, wts, pol_mode, rm_baseline, dev)


def unpack_psrfits_pol(raw, elem, nchan, nbin, scl, offs, wts=None, conv=0,
                       rm_baseline=True, dev=None):
    """ppf_unpack_psrfits_pol_batch: raw DATA bytes [nsub, >= 4 nchan nbin
    esize] of a four-polarisation file (device uint8 tensor, one row per
    sub-int) -> dict(rows float32 [nsub, 4, nchan, nbin] in the state conv
    asks for (0 / 1: as stored, Stokes / Coherence; 2 / 3: Coherence ->
    Stokes for linear / circular feeds; 4 / 5: Stokes -> Coherence), stats
    float64 [nsub, 4, nchan, 3] (off-pulse mean, sigma, S/N; the window of
    the sub-int's total intensity), total float64 [nsub, nbin], wstart int32
    [nsub]), all on the device."""
    return _unpack("ppf_unpack_psrfits_pol_batch", 4, 4, raw, elem, nchan,
                   nbin, scl, offs, wts, conv, rm_baseline, dev)


def pack_rows(rows, elem="I", dev=None):
    """ppf_pack_psrfits_batch, the inverse of unpack_psrfits: float rows ->
    (raw, scl, offs), all on the device.  rows: a NumPy array or a device
    tensor, float32 or float64 (anything else is converted to float64), of
    any leading shape [..., nbin], flattened to nrow rows.  elem "I": raw
    uint8 [nrow, nbin * 2] of big-endian int16 with psrfits.quantize's
    per-row scl / offs (float32 [nrow]), bit for bit; "E": raw uint8 [nrow,
    nbin * 4] of big-endian float32, scl = 1, offs = 0."""
    if elem not in ("I", "E"):
        raise ValueError("elem must be 'I' or 'E'")
    dev = device(dev)
    x = to_dev(rows, dev, _data_dtype(rows))
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError("rows must be [..., nbin] with nbin >= 1")
    nbin = int(x.shape[-1])
    x = x.reshape(-1, nbin)
    nrow = int(x.shape[0])
    esize = 2 if elem == "I" else 4
    raw = torch.empty((nrow, nbin * esize), dtype=torch.uint8, device=dev)
    scl = torch.empty(nrow, dtype=torch.float32, device=dev)
    offs = torch.empty_like(scl)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_pack_psrfits_batch(
        ctx, nrow, nbin,
        _lib.PPF_F32 if x.dtype == torch.float32 else _lib.PPF_F64, _p(x),
        0 if elem == "I" else 2, _p(raw), _p(scl), _p(offs), _stream(dev))
    _lib.check(rc, ctx)
    return raw, scl, offs


def scales_batch(D, M, params, P, freqs, nus, log10_tau, errs_FT=None,
                 model_index=None, dev=None):
    """get_scales_full (pptoaslib.py:953-971) per sub-int: D [nsub, nchan,
    nharm] complex data spectra, M [nmodel, nchan, nharm] complex model
    spectra (or [nchan, nharm]), params [nsub, 5], P [nsub], freqs
    [nsub, nchan], nus [nsub, 3]; returns a_n [nsub, nchan] float64."""
    dev = device(dev)
    c128 = torch.complex128
    D_t = to_dev(D, dev, c128)
    if D_t.dim() == 2:
        D_t = D_t.unsqueeze(0)
    nsub, nchan, nharm = D_t.shape
    M_t = to_dev(M, dev, c128)
    if M_t.dim() == 2:
        M_t = M_t.unsqueeze(0)
    if M_t.shape[1:] != (nchan, nharm):
        raise ValueError("model spectra %s != [*, %d, %d]" %
                         (tuple(M_t.shape), nchan, nharm))
    f64 = torch.float64
    pr = to_dev(params, dev, f64).reshape(nsub, 5).contiguous()
    P_t = to_dev(np.broadcast_to(np.asarray(P, dtype=float), (nsub,)).copy()
                 if not isinstance(P, torch.Tensor) else P, dev, f64)
    fr = to_dev(freqs, dev, f64).reshape(-1)
    if fr.numel() == nchan:
        fr = fr.repeat(nsub)
    fr = fr.reshape(nsub, nchan).contiguous()
    nu = to_dev(nus, dev, f64).reshape(-1)
    if nu.numel() == 3:
        nu = nu.repeat(nsub)
    nu = nu.reshape(nsub, 3).contiguous()
    e_t = None if errs_FT is None else \
        to_dev(errs_FT, dev, f64).reshape(-1)
    if e_t is not None and e_t.numel() == nchan:
        e_t = e_t.repeat(nsub)
    mi = None if model_index is None else \
        to_dev(model_index, dev, torch.int32).reshape(nsub).contiguous()
    out = torch.empty((nsub, nchan), dtype=f64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_scales_batch(
        ctx, nsub, nchan, nharm, _p(D_t), _p(M_t), _p(mi), _p(e_t), _p(pr),
        _p(P_t), _p(fr), _p(nu), int(bool(log10_tau)), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out


EVAL_TERMS = 62      # C, S, dC[5], dS[5], d2C[5][5], d2S[5][5] per channel


def eval_point_block():
    """Points that share one load of a channel's spectra in ppf_eval_batch."""
    return int(_lib.load().ppf_eval_point_block())


def _shape(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)


def _eval_shapes(theta, data_FT, model_FT, errs_FT, P, freqs, nus, fit_flags,
                 order, mask, model_index):
    """Shape checks of eval_points, on the host arrays' shapes alone (no
    device needed): returns (nprob, npoint, nchan, nharm, nmodel)."""
    ds = _shape(data_FT)
    if len(ds) == 2:
        ds = (1,) + ds
    if len(ds) != 3:
        raise ValueError("data_FT must be [nchan, nharm] or [nprob, nchan, "
                         "nharm], got %s" % (ds,))
    nprob, nchan, nharm = ds
    if nprob < 1 or nchan < 1 or nharm < 2:
        raise ValueError("data_FT %s: need nprob >= 1, nchan >= 1, nharm >= 2"
                         % (ds,))
    ms = _shape(model_FT)
    if len(ms) == 2:
        ms = (1,) + ms
    if len(ms) != 3 or ms[1:] != (nchan, nharm) or ms[0] < 1:
        raise ValueError("model_FT %s != [*, %d, %d]" % (ms, nchan, nharm))
    nmodel = ms[0]
    ts = _shape(theta)
    if len(ts) == 2:
        ts = (1,) + ts
    if len(ts) != 3 or ts[2] != 5 or ts[0] != nprob or ts[1] < 1:
        raise ValueError("theta %s != [%d, K >= 1, 5]" % (ts, nprob))
    for name, x, inner in (("errs_FT", errs_FT, nchan),
                           ("freqs", freqs, nchan), ("nus", nus, 3)):
        n = int(np.prod(_shape(x), dtype=np.int64))
        if n not in (inner, nprob * inner):
            raise ValueError("%s has %d elements, not %d or %d" %
                             (name, n, inner, nprob * inner))
    n = int(np.prod(_shape(P), dtype=np.int64))
    if n not in (1, nprob):
        raise ValueError("P has %d elements, not 1 or %d" % (n, nprob))
    if mask is not None:
        n = int(np.prod(_shape(mask), dtype=np.int64))
        if n not in (nchan, nprob * nchan):
            raise ValueError("mask has %d elements, not %d or %d" %
                             (n, nchan, nprob * nchan))
    if fit_flags is not None and \
            int(np.prod(_shape(fit_flags), dtype=np.int64)) != 5:
        raise ValueError("fit_flags must have 5 entries")
    if order not in (0, 1, 2):
        raise ValueError("order must be 0, 1 or 2, not %r" % (order,))
    if model_index is None:
        if nmodel not in (1, nprob):
            raise ValueError("%d models for %d problems need a model_index"
                             % (nmodel, nprob))
    else:
        mi = _host(model_index).reshape(-1)
        if mi.size != nprob or mi.min() < 0 or mi.max() >= nmodel:
            raise ValueError("model_index must be [%d] in [0, %d)" %
                             (nprob, nmodel))
    return nprob, ts[1], nchan, nharm, nmodel


def eval_points(theta, data_FT, model_FT, errs_FT, P, freqs, nus,
                fit_flags=None, log10_tau=True, order=2, per_channel=False,
                mask=None, model_index=None, max_bytes=None, dev=None):
    """The portrait likelihood of fit_portrait_full_function
    (pptoaslib.py:564-684) at many parameter points (ppf_eval_batch).

    theta [nprob, K, 5] (or [K, 5]); data_FT [nprob, nchan, nharm] and
    model_FT [nmodel, nchan, nharm] complex128 (or [nchan, nharm]); errs_FT,
    freqs [nprob, nchan]; P [nprob]; nus [nprob, 3] = nu_DM, nu_GM, nu_tau
    (each may be given once for all problems); mask [nprob, nchan] (0 drops
    a channel); model_index [nprob]; fit_flags [5].

    Returns device tensors (f [nprob, K], grad [nprob, K, 5] or None, hess
    [nprob, K, 5, 5] or None, terms [nprob, K, 62, nchan] or None): terms
    (per_channel) holds C, S, dC[5], dS[5], d2C[5, 5], d2S[5, 5] per
    channel.  The points are evaluated in consecutive chunks when the
    per-channel arrays of all of them would pass max_bytes (default half
    the free device memory); a point's result does not depend on the
    chunking."""
    nprob, K, nchan, nharm, nmodel = _eval_shapes(
        theta, data_FT, model_FT, errs_FT, P, freqs, nus, fit_flags, order,
        mask, model_index)
    dev = device(dev)
    c128, f64 = torch.complex128, torch.float64
    D_t = to_dev(data_FT, dev, c128).reshape(nprob, nchan, nharm)
    M_t = to_dev(model_FT, dev, c128).reshape(nmodel, nchan, nharm)
    th = to_dev(theta, dev, f64).reshape(nprob, K, 5)

    def per_prob(x, inner, dtype=f64):
        t = to_dev(x, dev, dtype).reshape(-1)
        if t.numel() == inner and nprob > 1:
            t = t.repeat(nprob)
        return t.reshape(nprob, inner).contiguous()

    e_t = per_prob(errs_FT, nchan)
    fr = per_prob(freqs, nchan)
    nu = per_prob(nus, 3)
    P_t = per_prob(P if isinstance(P, torch.Tensor) else
                   np.asarray(P, dtype=float), 1)
    mk = None if mask is None else per_prob(
        mask if isinstance(mask, torch.Tensor) else
        (np.asarray(mask) != 0).astype(np.uint8), nchan, torch.uint8)
    mi = None if model_index is None else \
        to_dev(model_index, dev, torch.int32).reshape(nprob).contiguous()
    fl = None if fit_flags is None else \
        to_dev(np.asarray(_host(fit_flags), dtype=float).reshape(5), dev, f64)
    ncomp = (1, 6, 21)[order]
    per_point = nprob * nchan * 8 * (ncomp +
                                     (EVAL_TERMS if per_channel else 0))
    if max_bytes is None:
        if K * per_point <= (64 << 20):
            max_bytes = 64 << 20
        else:
            free, _ = torch.cuda.mem_get_info(dev)
            max_bytes = free // 2
    # also within the 2^31 - 1 workgroups of one launch
    pb = eval_point_block()
    kmax = max(pb, ((2 ** 31 - 1) // (nprob * nchan) - 1) * pb)
    step = int(min(K, kmax, max(1, max_bytes // per_point)))
    f = torch.empty((nprob, K), dtype=f64, device=dev)
    g = torch.empty((nprob, K, 5), dtype=f64, device=dev) if order >= 1 \
        else None
    H = torch.empty((nprob, K, 5, 5), dtype=f64, device=dev) if order >= 2 \
        else None
    terms = torch.empty((nprob, K, EVAL_TERMS, nchan), dtype=f64,
                        device=dev) if per_channel else None
    lib = _lib.load()
    ctx = _lib.context(dev.index)
    ws = None
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        whole = k0 == 0 and k1 == K
        n = k1 - k0
        need = lib.ppf_eval_workspace_bytes(nprob, nchan, n, order)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        th_c = th if whole else th[:, k0:k1].contiguous()
        f_c = f if whole else torch.empty((nprob, n), dtype=f64, device=dev)
        g_c = g if whole or g is None else \
            torch.empty((nprob, n, 5), dtype=f64, device=dev)
        H_c = H if whole or H is None else \
            torch.empty((nprob, n, 5, 5), dtype=f64, device=dev)
        t_c = terms if whole or terms is None else \
            torch.empty((nprob, n, EVAL_TERMS, nchan), dtype=f64, device=dev)
        rc = lib.ppf_eval_batch(
            ctx, nprob, nchan, nharm, n, _p(D_t), _p(M_t), nmodel, _p(mi),
            _p(e_t), _p(P_t), _p(fr), _p(nu), _p(mk), _p(th_c), _p(fl),
            int(bool(log10_tau)), int(order), _p(f_c), _p(g_c), _p(H_c),
            _p(t_c), _p(ws), ws.numel(), _stream(dev))
        _lib.check(rc, ctx)
        if not whole:
            f[:, k0:k1] = f_c
            if g is not None:
                g[:, k0:k1] = g_c
            if H is not None:
                H[:, k0:k1] = H_c
            if terms is not None:
                terms[:, k0:k1] = t_c
    return f, g, H, terms


def phase_shift_batch(data, model, noise=None, Ns=100, bounds=(-0.5, 0.5),
                      model_index=None, dev=None):
    """Batched pplib.fit_phase_shift: data [nprof, nbin], model
    [nmodel, nbin] -> [nprof, 8] (phase, phase_err, scale, scale_err, snr,
    red_chi2, nfev, status)."""
    dev = device(dev)
    d = to_dev(data, dev, _data_dtype(data))
    if d.dim() == 1:
        d = d.unsqueeze(0)
    m = to_dev(model, dev, torch.float64)
    if m.dim() == 1:
        m = m.unsqueeze(0)
    nz = None if noise is None else \
        to_dev(noise, dev, torch.float64).reshape(-1).contiguous()
    mi = None if model_index is None else \
        to_dev(model_index, dev, torch.int32).reshape(-1).contiguous()
    out = torch.zeros((d.shape[0], 8), dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_phase_shift_batch(
        ctx, d.shape[0], d.shape[1],
        _lib.PPF_F32 if d.dtype == torch.float32 else _lib.PPF_F64,
        _p(d), _p(m), _p(mi), _p(nz), int(Ns), float(bounds[0]),
        float(bounds[1]), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out


def _join_args(join_id, join_params, P, n, nchan, dev):
    """The join arguments of the joined Gaussian entry points: join_id
    [n, nchan] int32 on the HOST (the archive of each channel, -1: none),
    join_params [n, 2 njoin] (phase [rot], DM per archive) and P [n] [s] on
    the device."""
    if join_params is None or P is None:
        raise ValueError("join_id needs join_params and P")
    ji = np.ascontiguousarray(np.broadcast_to(
        np.asarray(join_id, dtype=np.int32).reshape(-1, nchan), (n, nchan)))
    jp = to_dev(join_params, dev, torch.float64).reshape(n, -1).contiguous()
    if jp.shape[1] % 2:
        raise ValueError("join_params must hold (phase, DM) per archive")
    Pd = to_dev(np.broadcast_to(np.asarray(P, dtype=float), (n,)), dev,
                torch.float64).contiguous()
    return ji, jp, Pd, jp.shape[1] // 2


def gauss_portraits(model_code, params, scattering_index, freqs, nu_ref, nbin,
                    dev=None, join_id=None, join_params=None, P=None):
    """Gaussian-component model portraits (pplib.gen_gaussian_portrait,
    pplib.py:886-963) on the device: params [nport, 2 + 6 ngauss] (DC, tau
    [bin], per component loc, m_loc, wid, m_wid, amp, m_amp),
    scattering_index [nport], freqs [nport, nchan], nu_ref [nport] ->
    float64 [nport, nchan, nbin] (odd nbin with tau != 0: nbin - 1 bins, as
    the reference's length-less irfft gives, then a zero column).
    join_id [nport, nchan] (the archive of each channel, -1: none) with
    join_params [nport, 2 njoin] (phase [rot], DM per archive) and P [nport]
    [s] rotates each archive's rows as gen_gaussian_portrait(join_ichans=...)
    does (ppf_gauss_portrait_join_batch; even nbin in [32, 8192])."""
    code = str(model_code)
    if len(code) != 3 or any(c not in "01" for c in code):
        raise KeyError(code)     # evolve_parameter's dictionary lookup
    dev = device(dev)
    prm = to_dev(params, dev, torch.float64)
    if prm.dim() == 1:
        prm = prm.unsqueeze(0)
    nport, npar = prm.shape
    if npar < 2 or (npar - 2) % 6:
        raise ValueError("params must hold 2 + 6*ngauss values per portrait")
    f = to_dev(freqs, dev, torch.float64).reshape(nport, -1).contiguous()
    nchan = f.shape[1]
    si = to_dev(np.broadcast_to(np.asarray(scattering_index, dtype=float),
                                (nport,)), dev, torch.float64).contiguous()
    nr = to_dev(np.broadcast_to(np.asarray(nu_ref, dtype=float), (nport,)),
                dev, torch.float64).contiguous()
    out = torch.empty((nport, nchan, int(nbin)), dtype=torch.float64,
                      device=dev)
    ctx = _lib.context(dev.index)
    if join_id is not None:
        ji, jp, Pd, njoin = _join_args(join_id, join_params, P, nport, nchan,
                                       dev)
        rc = _lib.load().ppf_gauss_portrait_join_batch(
            ctx, nport, nchan, int(nbin), (npar - 2) // 6, code.encode(),
            _p(prm), _p(si), _p(f), _p(nr), njoin, ji.ctypes.data, _p(jp),
            _p(Pd), _p(out), _stream(dev))
        _lib.check(rc, ctx)
        return out
    rc = _lib.load().ppf_gauss_portrait_batch(
        ctx, nport, nchan, int(nbin), (npar - 2) // 6, code.encode(),
        _p(prm), _p(si), _p(f), _p(nr), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out


def gauss_lsq(model_code, params, scattering_index, freqs, nu_ref, free_idx,
              delta, data, inv_errs, dev=None, workspace=None, join_id=None,
              join_params=None, P=None):
    """Normal equations of the Gaussian portrait model on the device
    (ppf_gauss_lsq_batch): for each of nfit fits the Gram matrix C C^T of
    the forward-difference Jacobian columns ((m(p + delta_j e_j) - m(p)) /
    delta_j) * inv_errs and the residual (data - m(p)) * inv_errs, m the
    portrait gauss_portraits builds.  params [nfit, 2 + 6 ngauss],
    scattering_index / nu_ref [nfit], freqs [nfit, nchan], free_idx [nfree]
    (strictly increasing indices into params, npar = the scattering index),
    delta [nfit, nfree], data [nfit, nchan, nbin] (float32 or float64),
    inv_errs [nfit, nchan, nbin] -> float64 [nfit, nfree + 1, nfree + 1]
    on the device: J^T J, J^T r in the last column, chi^2 in the corner.
    workspace: a uint8 device tensor to reuse between calls (any size; a
    larger one is allocated when it is too small).
    join_id / join_params / P as for gauss_portraits
    (ppf_gauss_lsq_join_batch): free_idx then indexes [params, join_params,
    scattering index], the index at npar + 2 njoin."""
    code = str(model_code)
    if len(code) != 3 or any(c not in "01" for c in code):
        raise KeyError(code)     # evolve_parameter's dictionary lookup
    dev = device(dev)
    prm = to_dev(params, dev, torch.float64)
    if prm.dim() == 1:
        prm = prm.unsqueeze(0)
    nfit, npar = prm.shape
    if npar < 2 or (npar - 2) % 6:
        raise ValueError("params must hold 2 + 6*ngauss values per fit")
    f = to_dev(freqs, dev, torch.float64).reshape(nfit, -1).contiguous()
    nchan = f.shape[1]
    si = to_dev(np.broadcast_to(np.asarray(scattering_index, dtype=float),
                                (nfit,)), dev, torch.float64).contiguous()
    nr = to_dev(np.broadcast_to(np.asarray(nu_ref, dtype=float), (nfit,)),
                dev, torch.float64).contiguous()
    if not isinstance(data, torch.Tensor):
        data = np.asarray(data)
    ddt = torch.float32 if data.dtype in (torch.float32, np.float32) \
        else torch.float64
    d = to_dev(data, dev, ddt)
    if d.dim() == 2:
        d = d.unsqueeze(0)
    if d.shape[:2] != (nfit, nchan):
        raise ValueError("data must be [nfit, nchan, nbin]")
    nbin = d.shape[2]
    w = to_dev(inv_errs, dev, torch.float64).reshape(d.shape).contiguous()
    fi = np.ascontiguousarray(free_idx, dtype=np.int32).reshape(-1)
    nfree = fi.size
    dl = np.zeros((nfit, 0))
    if nfree:
        dl = np.ascontiguousarray(np.broadcast_to(
            np.asarray(delta, dtype=np.float64).reshape((-1, nfree)),
            (nfit, nfree)))
    lib = _lib.load()
    need = lib.ppf_gauss_lsq_workspace_bytes(nfit, nchan, nbin, nfree)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    gram = torch.empty((nfit, nfree + 1, nfree + 1), dtype=torch.float64,
                       device=dev)
    ctx = _lib.context(dev.index)
    if join_id is not None:
        ji, jp, Pd, njoin = _join_args(join_id, join_params, P, nfit, nchan,
                                       dev)
        rc = lib.ppf_gauss_lsq_join_batch(
            ctx, nfit, nchan, nbin, (npar - 2) // 6, code.encode(), _p(prm),
            _p(si), _p(f), _p(nr), njoin, ji.ctypes.data, _p(jp), _p(Pd),
            nfree, fi.ctypes.data, dl.ctypes.data,
            _lib.PPF_F32 if ddt == torch.float32 else _lib.PPF_F64, _p(d),
            _p(w), _p(gram), _p(workspace), workspace.numel(), _stream(dev))
    else:
        rc = lib.ppf_gauss_lsq_batch(
            ctx, nfit, nchan, nbin, (npar - 2) // 6, code.encode(), _p(prm),
            _p(si), _p(f), _p(nr), nfree, fi.ctypes.data, dl.ctypes.data,
            _lib.PPF_F32 if ddt == torch.float32 else _lib.PPF_F64, _p(d),
            _p(w), _p(gram), _p(workspace), workspace.numel(), _stream(dev))
    _lib.check(rc, ctx)
    # free_idx / delta are host arrays the stream still reads
    torch.cuda.current_stream(dev).synchronize()
    return gram


class GaussLsqEvaluator:
    """The device evaluator of _gaussfit.levenberg_marquardt for ONE fit:
    (p_ext, free_idx, delta) -> Gram matrix (numpy), p_ext the parameters
    with the scattering index appended; with join_id [nchan] (the archive
    of each channel, -1: none) and P [s], p_ext is [params, 2 njoin join
    parameters, scattering index].  The data, weights and workspace
    stay on the device between calls.  time_kernels=True brackets each call
    with HIP events; kernel_ms then lists the device time of every call."""

    def __init__(self, model_code, data, inv_errs, freqs, nu_ref, dev=None,
                 time_kernels=False, join_id=None, P=None, njoin=None):
        self.dev = device(dev)
        self.code = model_code
        data = np.asarray(data) if not isinstance(data, torch.Tensor) else data
        ddt = torch.float32 if data.dtype in (torch.float32, np.float32) \
            else torch.float64
        self.data = to_dev(data, self.dev, ddt).unsqueeze(0)
        self.w = to_dev(inv_errs, self.dev, torch.float64).unsqueeze(0)
        self.freqs = to_dev(freqs, self.dev, torch.float64).reshape(1, -1)
        self.nu_ref = float(nu_ref)
        self.join_id = None
        self.njoin = 0
        if join_id is not None:
            if P is None:
                raise ValueError("join_id needs P")
            self.join_id = np.ascontiguousarray(join_id, dtype=np.int32)
            self.njoin = int(self.join_id.max()) + 1 if njoin is None \
                else int(njoin)
            self.P = float(P)
        self.ws = None
        self.time_kernels = time_kernels
        self.kernel_ms = []

    def __call__(self, p_ext, free_idx, delta):
        p_ext = np.asarray(p_ext, dtype=np.float64)
        nchan, nbin = self.data.shape[1:]
        need = _lib.load().ppf_gauss_lsq_workspace_bytes(1, nchan, nbin,
                                                         len(free_idx))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(max(need, 256), dtype=torch.uint8,
                                  device=self.dev)
        if self.time_kernels:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
        if self.join_id is not None:
            npar = len(p_ext) - 1 - 2 * self.njoin
            g = gauss_lsq(self.code, p_ext[None, :npar], [p_ext[-1]],
                          self.freqs, [self.nu_ref], free_idx, delta,
                          self.data, self.w, dev=self.dev, workspace=self.ws,
                          join_id=self.join_id[None, :],
                          join_params=p_ext[None, npar:-1], P=[self.P])
        else:
            g = gauss_lsq(self.code, p_ext[None, :-1], [p_ext[-1]],
                          self.freqs, [self.nu_ref], free_idx, delta,
                          self.data, self.w, dev=self.dev, workspace=self.ws)
        if self.time_kernels:
            e1.record()
            e1.synchronize()
            self.kernel_ms.append(e0.elapsed_time(e1))
        return g[0].cpu().numpy()


class SwtHandle(object):
    """One analysed batch of profiles (swt_analyse): the device arrays
    swt_score reads.  medians [nprof, nlevel] and noise [nprof] are NumPy
    copies."""


def swt_analyse(profs, nlevel, max_ncase=0, dev=None):
    """The stationary db8 transform of profs [nprof, nbin] (float64) to
    nlevel levels on the device (ppf_swt_analyse_batch): the coefficient
    rows stay in the handle's workspace, which has room for max_ncase cases
    per swt_score call (it grows on demand)."""
    dev = device(dev)
    p = to_dev(profs, dev, torch.float64)
    if p.dim() == 1:
        p = p.unsqueeze(0)
    nprof, nbin = p.shape
    nlevel = int(nlevel)
    lib = _lib.load()
    h = SwtHandle()
    h.dev, h.prof, h.nprof, h.nbin, h.nlevel = dev, p, nprof, nbin, nlevel
    h.ncase = max(int(max_ncase), 1)
    need = lib.ppf_swt_workspace_bytes(nprof, nbin, nlevel, h.ncase)
    h.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    h.med = torch.empty((nprof, max(nlevel, 1)), dtype=torch.float64,
                        device=dev)
    h.sig = torch.empty(nprof, dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = lib.ppf_swt_analyse_batch(ctx, nprof, nbin, nlevel, _p(p), _p(h.med),
                                   _p(h.sig), _p(h.ws), h.ws.numel(),
                                   _stream(dev))
    _lib.check(rc, ctx)
    h.medians = h.med.cpu().numpy()
    h.noise = h.sig.cpu().numpy()
    return h


def _swt_grow(h, ncase):
    """Room for ncase cases in the handle's workspace: the coefficients sit
    at its front, a longer case list needs a larger one and the rows are
    copied over."""
    if ncase > h.ncase:
        lib = _lib.load()
        need = lib.ppf_swt_workspace_bytes(h.nprof, h.nbin, h.nlevel, ncase)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=h.dev)
        ncoef = h.nprof * h.nlevel * 2 * h.nbin * 8
        ws[:ncoef].copy_(h.ws[:ncoef])
        h.ws, h.ncase = ws, ncase


def swt_score(h, cases, facts, smooth=False, on_device=False):
    """Denoise-and-score cases on an analysed batch (ppf_swt_score_batch):
    cases [ncase, 3] = (profile, level, 0 hard / 1 soft), facts [ncase] ->
    (out [ncase, 3] = (signal, noise, red_chi2), the smoothed rows [ncase,
    nbin] or None), NumPy, or with on_device the device tensors."""
    cs = np.ascontiguousarray(cases, dtype=np.int32).reshape(-1, 3)
    fs = np.ascontiguousarray(facts, dtype=np.float64).reshape(-1)
    ncase = len(cs)
    if len(fs) != ncase:
        raise ValueError("one factor per case")
    lib = _lib.load()
    dev = h.dev
    _swt_grow(h, ncase)
    out = torch.empty((ncase, 3), dtype=torch.float64, device=dev)
    rows = torch.empty((ncase, h.nbin), dtype=torch.float64, device=dev) \
        if smooth else None
    ctx = _lib.context(dev.index)
    rc = lib.ppf_swt_score_batch(
        ctx, h.nprof, h.nbin, h.nlevel, _p(h.prof), _p(h.med), _p(h.sig),
        ncase, cs.ctypes.data, fs.ctypes.data, _p(out), _p(rows), _p(h.ws),
        h.ws.numel(), _stream(dev))
    _lib.check(rc, ctx)
    # cases / facts are host arrays the stream still reads
    torch.cuda.current_stream(dev).synchronize()
    if on_device:
        return out, rows
    return out.cpu().numpy(), (rows.cpu().numpy() if smooth else None)


def swt_search(h, soft, rchi2_tol, grid, table):
    """The fmin finish of scipy.optimize.brute for every (profile, level) of
    an analysed batch in one launch (ppf_swt_search_batch): grid [ngrid]
    the factors brute tabulates, table the device out of the swt_score call
    over _swt.grid_cases -> fact_min, fun_min (float64), nfev (int32), each
    [nprof, nlevel], NumPy, from one download."""
    gs = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
    lib = _lib.load()
    dev = h.dev
    m = h.nprof * h.nlevel
    if table.shape != (m * len(gs), 3) or table.dtype != torch.float64 or \
            not table.is_contiguous():
        raise ValueError("table: the [nprof * nlevel * ngrid, 3] float64 out "
                         "of swt_score over the grid")
    _swt_grow(h, len(gs))
    # fact_min, fun_min and (two int32 to a double) nfev, one buffer
    res = torch.empty(2 * m + (m + 1) // 2, dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = lib.ppf_swt_search_batch(
        ctx, h.nprof, h.nbin, h.nlevel, _p(h.prof), _p(h.med), _p(h.sig),
        int(soft), float(rchi2_tol), len(gs), gs.ctypes.data, _p(table),
        _p(res[:m]), _p(res[m:2 * m]), _p(res[2 * m:]), _p(h.ws),
        h.ws.numel(), _stream(dev))
    _lib.check(rc, ctx)
    # the download waits for the stream, which still reads the host grid
    r = res.cpu().numpy()
    shape = (h.nprof, h.nlevel)
    return (r[:m].reshape(shape), r[m:2 * m].reshape(shape),
            r[2 * m:].view(np.int32)[:m].reshape(shape))


class SwtEvaluator(object):
    """The device evaluator of pplib.wavelet_smooth / smart_smooth (see
    _swt.py for the interface)."""

    def __init__(self, dev=None):
        self.dev = dev

    def noise(self, rows):
        return noise_rows(np.atleast_2d(np.asarray(rows, dtype=np.float64)),
                          4, self.dev).cpu().numpy()

    def analyse(self, profs, nlevel, max_ncase=0):
        return swt_analyse(profs, nlevel, max_ncase, self.dev)

    def score(self, h, cases, facts, smooth=False):
        return swt_score(h, cases, facts, smooth)

    def search(self, h, soft, rchi2_tol, grid):
        from . import _swt
        cases, facts = _swt.grid_cases(h.nprof, h.nlevel, soft, grid)
        table = swt_score(h, cases, facts, on_device=True)[0]
        return swt_search(h, soft, rchi2_tol, grid, table)


def spline_portraits(mean_prof, eigvec, tck, freqs, nbin=None, dev=None):
    """PCA + B-spline model portraits (pplib.gen_spline_portrait,
    pplib.py:966-990) on the device (ppf_spline_portrait_batch): mean_prof
    [nbin_model], eigvec [nbin_model, ncomp], tck = (knots, [coefs per
    component], degree) as si.splprep returns it, freqs [nport, nchan] (or
    [nchan]) -> float64 [nport, nchan, nbin]."""
    dev = device(dev)
    mean_prof = np.asarray(mean_prof, dtype=np.float64)
    eigvec = np.asarray(eigvec, dtype=np.float64)
    nbin0 = len(mean_prof)
    nbin = nbin0 if nbin is None else int(nbin)
    ncomp = eigvec.shape[1] if eigvec.ndim == 2 else 0
    f = np.atleast_2d(np.asarray(freqs, dtype=np.float64))
    nport, nchan = f.shape
    if ncomp:
        t = np.asarray(tck[0], dtype=np.float64)
        cs = [np.asarray(c, dtype=np.float64) for c in tck[1]]
        if len(cs) != ncomp:
            raise ValueError("tck has %d coefficient arrays, eigvec %d "
                             "columns" % (len(cs), ncomp))
        coefs = np.zeros((ncomp, len(t)))
        for i, c in enumerate(cs):
            coefs[i, :len(c)] = c
        degree, nknots = int(tck[2]), len(t)
    else:
        t, coefs, degree, nknots = np.zeros(1), np.zeros((1, 1)), 0, 1
    ev = eigvec if ncomp else np.zeros((nbin0, 1))
    mp_t = to_dev(mean_prof, dev, torch.float64)
    ev_t = to_dev(np.ascontiguousarray(ev), dev, torch.float64)
    t_t = to_dev(t, dev, torch.float64)
    c_t = to_dev(coefs, dev, torch.float64)
    f_t = to_dev(f, dev, torch.float64)
    out = torch.empty((nport, nchan, nbin), dtype=torch.float64, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_spline_portrait_batch(
        ctx, nport, nchan, nbin0, nbin, ncomp, nknots, degree, _p(mp_t),
        _p(ev_t), _p(t_t), _p(c_t), _p(f_t), _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out


def synth(model, freqs, phi, DM, P, nu_ref, noise, seed, out_dtype=torch.float32,
          dev=None, first=0):
    """Synthetic sub-integrations [nsub, nchan, nbin] on the device."""
    dev = device(dev)
    m = to_dev(model, dev, torch.float64)
    nchan, nbin = m.shape
    f = to_dev(freqs, dev, torch.float64).reshape(-1).contiguous()
    ph = to_dev(phi, dev, torch.float64).reshape(-1).contiguous()
    dm = to_dev(DM, dev, torch.float64).reshape(-1).contiguous()
    Pt = to_dev(P, dev, torch.float64).reshape(-1).contiguous()
    nsub = ph.numel()
    out = torch.empty((nsub, nchan, nbin), dtype=out_dtype, device=dev)
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_synth_batch(
        ctx, nsub, nchan, nbin, _p(m), _p(f), _p(ph), _p(dm), _p(Pt),
        float(nu_ref), float(noise), ctypes.c_uint64(int(seed)), int(first),
        _lib.PPF_F32 if out_dtype == torch.float32 else _lib.PPF_F64,
        _p(out), _stream(dev))
    _lib.check(rc, ctx)
    return out


def fake_subints(model, model_of, phase, tau_n, gain, noise, seed, first_sub=0,
                 quantized=False, dev=None):
    """Simulated archive rows on the device (ppf_fake_batch, k_fake): per
    (sub-int s, polarisation p, channel n) the template model[model_of[s]][n]
    rotated by phase[s][n] turns, scattered by tau_n[s][n] turns (0: not),
    scaled by gain[s][p][n], plus N(0, noise[n]) per bin (noise[n] = 0: no
    noise at all) from the counter RNG keyed by (seed, first_sub + s, p, n,
    bin): sub-int s of a call with first_sub = f is sub-int f + s of the
    whole job, however it is split.

    model [nmodel, nchan, nbin] (or [nchan, nbin]), model_of [nsub], phase and
    tau_n [nsub, nchan], gain [nsub, npol, nchan], noise [nchan].

    quantized=False: float64 rows [nsub, npol, nchan, nbin].
    quantized=True: (data, scl, offs): the same rows as psrfits.quantize
    digitises them, data a uint8 tensor [nsub, npol * nchan * nbin * 2] of
    big-endian int16 in the SUBINT DATA layout (the bytes of the file), scl /
    offs float32 [nsub, npol * nchan]."""
    dev = device(dev)
    m = to_dev(model, dev, torch.float64)
    if m.dim() == 2:
        m = m.unsqueeze(0)
    nmodel, nchan, nbin = m.shape
    g = to_dev(gain, dev, torch.float64)
    if g.dim() != 3 or g.shape[2] != nchan:
        raise ValueError("gain must be [nsub, npol, nchan]")
    nsub, npol = int(g.shape[0]), int(g.shape[1])
    mo = np.asarray(_host(model_of), dtype=np.int64).reshape(-1)
    if mo.size != nsub or (nsub and (mo.min() < 0 or mo.max() >= nmodel)):
        raise ValueError("model_of must hold nsub indices in [0, nmodel)")
    mo_t = to_dev(mo.astype(np.int32), dev, torch.int32)
    ph = to_dev(phase, dev, torch.float64)
    tn = to_dev(tau_n, dev, torch.float64)
    nz = to_dev(noise, dev, torch.float64).reshape(-1).contiguous()
    if tuple(ph.shape) != (nsub, nchan) or tuple(tn.shape) != (nsub, nchan) \
            or nz.numel() != nchan:
        raise ValueError("phase, tau_n must be [nsub, nchan], noise [nchan]")
    if quantized:
        out = torch.empty((nsub, npol * nchan * nbin * 2), dtype=torch.uint8,
                          device=dev)
        scl = torch.empty((nsub, npol * nchan), dtype=torch.float32,
                          device=dev)
        offs = torch.empty_like(scl)
    else:
        out = torch.empty((nsub, npol, nchan, nbin), dtype=torch.float64,
                          device=dev)
        scl = offs = None
    ctx = _lib.context(dev.index)
    rc = _lib.load().ppf_fake_batch(
        ctx, nsub, npol, nchan, nbin, nmodel, _p(m), _p(mo_t), _p(ph), _p(tn),
        _p(g), _p(nz), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
        int(first_sub), _lib.PPF_FAKE_I16 if quantized else _lib.PPF_FAKE_F64,
        _p(out), _p(scl), _p(offs), _stream(dev))
    _lib.check(rc, ctx)
    return (out, scl, offs) if quantized else out


def results_numpy(res):
    """Device fit_batch output -> dict of numpy arrays (synchronises)."""
    out = {k: v.detach().cpu().numpy() for k, v in res.items()
           if isinstance(v, torch.Tensor) and k != "workspace"}
    return out
