"""Drop-in mirror of PulsePortraiture's ``ppgauss``: Gaussian-component
portrait models fitted on the device.

``DataPortrait(datafile).make_gaussian_model(...)`` is the reference's
workflow (ppgauss.py:62-245): the evolving-Gaussian model is fitted to the
dedispersed, time-averaged portrait with pplib.fit_gaussian_portrait
(ppf_gauss_lsq_batch under a Levenberg-Marquardt driver), the residual phase
/ DM offset between data and model is measured with fit_phase_shift +
fit_portrait, the data are rotated by it and the fit is repeated until the
offset is within its errors.  The written .gmodel is what pptoas.GetTOAs
reads.

A metafile of several archives of one pulsar (or a list of DataBunches) is
fitted with ONE model: every archive gets a phase and a DM offset of its own
(the join parameters), fitted with the model on the device
(ppf_gauss_lsq_join_batch).  The data are then not rotated between
iterations; the join parameters are appended to the join file after every
fit, and port, portx and model are de-rotated by them at the end.

Outside the accelerated path (NotImplementedError): the interactive
GaussianSelector, rotate_stuff and every plot.
"""
import time

import numpy as np

from .pplib import DataPortrait as _DataPortrait
from .pplib import (DataBunch, default_model, file_is_type, fit_gaussian_portrait,
                    fit_gaussian_profile, fit_phase_shift, fit_portrait,
                    gaussian_profile, gen_gaussian_portrait, get_noise,
                    guess_fit_freq, load_data, read_model, rotate_data,
                    scattering_alpha, write_model)

_OUTSIDE = "%s is outside the accelerated path"


class DataPortrait(_DataPortrait):
    """The data a Gaussian model is fitted to (pplib.py:155-349, with
    ppgauss.py's methods).  datafile: a fold-mode PSRFITS file (loaded with
    dedisperse=True, tscrunch=True on the PSRFITS fast path) or an in-memory
    DataBunch with load_data's keys (subints [nsub, npol, nchan, nbin],
    masks, freqs [nsub, nchan], ok_ichans, noise_stds, SNRs [nsub, npol,
    nchan], Ps, phases, nu0, bw, source); its first sub-integration is the
    portrait.  A metafile, or a list of DataBunches, joins several archives
    (see pplib.DataPortrait)."""

    def __init__(self, datafile=None, joinfile=None, quiet=False,
                 **load_data_kwargs):
        self.init_params = []
        _DataPortrait.__init__(self, datafile, joinfile, quiet,
                               **load_data_kwargs)
        self.init_params = []

    def fit_profile(self, profile, tau=0.0, fixscat=True, auto_gauss=0.0,
                    profile_fit_flags=None, show=True):
        """ppgauss.py:35-60 for auto_gauss != 0 and show=False: one Gaussian
        of initial width auto_gauss [rot] placed with fit_phase_shift and
        fitted with fit_gaussian_profile (GaussianSelector's automatic
        branch, ppgauss.py:450-467, without its figure).  Hand-placed
        components (auto_gauss == 0) and show=True need the interactive
        window.  Whether the reference's own fit_profile(show=False) runs
        without a display was not checked: it opens a matplotlib figure and
        connects canvas events first."""
        if not auto_gauss or show:
            raise NotImplementedError(
                _OUTSIDE % "the interactive GaussianSelector (use auto_gauss "
                "!= 0 with show=False, or a modelfile)")
        profile = np.asarray(profile, dtype=float)
        nbin = len(profile)
        errs = get_noise(profile)
        fit_scattering = not fixscat
        if fit_scattering and tau == 0.0:
            tau = 0.1                                # ppgauss.py:423-424
        dc = sorted(profile)[nbin // 10 + 1]
        amp, wid = profile.max(), auto_gauss
        first = amp * gaussian_profile(nbin, 0.5, wid)
        loc = 0.5 + fit_phase_shift(profile, first, errs).phase
        fgp = fit_gaussian_profile(profile, [dc, tau, loc, wid, amp],
                                   np.zeros(nbin) + errs, profile_fit_flags,
                                   fit_scattering, quiet=True)
        self.init_params = fgp.fitted_params
        self.init_param_errs = fgp.fit_errs
        self.ngauss = (len(self.init_params) - 2) // 3

    def make_gaussian_model(self, modelfile=None, ref_prof=(None, None),
                            tau=0.0, fixloc=False, fixwid=False, fixamp=False,
                            fixscat=True, fixalpha=True,
                            scattering_index=scattering_alpha,
                            model_code=default_model, niter=0,
                            fiducial_gaussian=False, auto_gauss=0.0,
                            writemodel=False, outfile=None, writeerrfile=False,
                            errfile=None, model_name=None, residplot=None,
                            quiet=False):
        """ppgauss.py:62-245: fit the evolving-Gaussian model, iterating up
        to niter times on the residual phase / DM offset.  The starting
        point is a modelfile, self.init_params set beforehand, or one
        automatically fitted component (auto_gauss != 0).  residplot needs
        matplotlib and is outside the accelerated path."""
        if residplot:
            raise NotImplementedError(_OUTSIDE % "residplot")
        if modelfile:
            if outfile is None:
                outfile = modelfile
            if errfile is None:
                errfile = outfile + "_errs"
            (self.model_name, self.model_code, self.nu_ref, self.ngauss,
             self.init_model_params, self.fit_flags, self.scattering_index,
             self.fitalpha) = read_model(modelfile)
            self.fixalpha = not self.fitalpha
            if model_name is not None:
                self.model_name = model_name
            self.init_model_params[1] *= self.nbin / self.Ps[0]
        else:
            self.model_code = model_code
            self.scattering_index = scattering_index
            self.fixalpha = fixalpha
            self.fitalpha = int(not self.fixalpha)
            if errfile is None and outfile is not None:
                errfile = outfile + "_errs"
            self.model_name = self.source if model_name is None else model_name
            if not len(self.init_params):
                self.nu_ref, self.bw_ref = ref_prof
                if self.nu_ref is None:
                    self.nu_ref = self.nu0
                if self.bw_ref is None:
                    self.bw_ref = abs(self.bw)
                inband = (self.nu_ref - self.bw_ref / 2 < self.freqs[0]) & \
                    (self.nu_ref + self.bw_ref / 2 > self.freqs[0]) & \
                    (np.asarray(self.masks[0, 0]).mean(axis=1) != 0)
                profile = self.port[inband].mean(axis=0)
                self.fit_profile(profile, tau=tau, fixscat=fixscat,
                                 auto_gauss=auto_gauss, profile_fit_flags=None,
                                 show=False)
            elif getattr(self, "nu_ref", None) is None:
                self.nu_ref = self.nu0 if ref_prof[0] is None else ref_prof[0]
            ip = np.asarray(self.init_params, dtype=float)
            self.ngauss = (len(ip) - 2) // 3
            # all slopes and spectral indices start at 0
            comps = np.zeros((self.ngauss, 6))
            comps[:, 0], comps[:, 2], comps[:, 4] = ip[2::3], ip[3::3], ip[4::3]
            self.init_model_params = np.r_[ip[:2], comps.ravel()]
            self.fit_flags = np.ones(len(self.init_model_params))
            self.fit_flags[1] *= not fixscat
            self.fit_flags[3::6] *= not fixloc
            self.fit_flags[5::6] *= not fixwid
            self.fit_flags[7::6] *= not fixamp
            if fiducial_gaussian:
                self.fit_flags[3::6] = 1
                self.fit_flags[3] = 0
        self.portx_noise = np.outer(self.noise_stdsxs, np.ones(self.nbin))
        self.nu_fit = guess_fit_freq(self.freqsxs[0], self.SNRsxs)
        niter = max(int(niter), 0)
        self.niter = self.itern = niter
        self.model_params = np.copy(self.init_model_params)
        self.total_time = 0.0
        self.start = time.time()
        if not quiet:
            print("Fitting Gaussian model portrait...")
        iterator = self.model_iteration(quiet)
        next(iterator)
        self.cnvrgnc = self.check_convergence(efac=1.0, quiet=quiet)
        if writemodel:
            self.write_model(outfile=outfile, quiet=quiet)
        if writeerrfile:
            self.write_errfile(errfile=errfile, quiet=quiet)
        while self.niter and not self.cnvrgnc:
            if not quiet:
                print("\n...iteration %d..." % (self.itern - self.niter + 1))
            if not self.njoin:
                self.port = rotate_data(self.port, self.phi, self.DM,
                                        self.Ps[0], self.freqs[0], self.nu_fit)
                self.portx = rotate_data(self.portx, self.phi, self.DM,
                                         self.Ps[0], self.freqsxs[0],
                                         self.nu_fit)
            next(iterator)
            self.niter -= 1
            self.cnvrgnc = self.check_convergence(efac=1.0, quiet=quiet)
            # for safety, the model is written after each iteration
            if writemodel:
                self.write_model(outfile=outfile, quiet=quiet)
            if writeerrfile:
                self.write_errfile(errfile=errfile, quiet=quiet)
        # ppgauss.py:213-231: the archives aligned with the fitted model
        for ii in range(self.njoin):
            phi, DM = -self.join_params[0::2][ii], -self.join_params[1::2][ii]
            jic, jicx = self.join_ichans[ii], self.join_ichanxs[ii]
            self.port[jic] = rotate_data(self.port[jic], phi, DM, self.Ps[0],
                                         self.freqs[0, jic], self.nu_ref)
            self.portx[jicx] = rotate_data(self.portx[jicx], phi, DM,
                                           self.Ps[0], self.freqsxs[0][jicx],
                                           self.nu_ref)
            self.model[jic] = rotate_data(self.model[jic], phi, DM,
                                          self.Ps[0], self.freqs[0, jic],
                                          self.nu_ref)
        if self.njoin:
            mask = np.asarray(self.masks[0, 0])
            self.model_masked = self.model * mask
            self.modelx = self.model[mask.mean(axis=1) != 0]
        if not quiet:
            print("Residuals std:  %.2e" % (self.portx - self.modelx).std())
            print("Data std:       %.2e" % np.median(self.noise_stdsxs))
            print("Total fit time: %.2f min" % (self.total_time / 60.0))

    def model_iteration(self, quiet=False):
        """ppgauss.py:247-283: one fit_gaussian_portrait per next()."""
        while True:
            start = time.time()
            fgp = fit_gaussian_portrait(
                self.model_code, self.portx, self.model_params,
                self.scattering_index, self.portx_noise, self.fit_flags,
                not self.fixalpha, self.phases, self.freqsxs[0], self.nu_ref,
                self.all_join_params, self.Ps[0], quiet=quiet)
            self.fitted_params, self.fit_errs, self.chi2, self.dof = \
                fgp.fitted_params, fgp.fit_errs, fgp.chi2, fgp.dof
            self.scattering_index = fgp.scattering_index
            self.scattering_index_err = fgp.scattering_index_err
            self.fgp = fgp
            if self.njoin:
                nj = 2 * self.njoin
                self.model_params = self.fitted_params[:-nj]
                self.model_param_errs = self.fit_errs[:-nj]
                self.join_params = self.fitted_params[-nj:]
                self.join_param_errs = self.fit_errs[-nj:]
                self.all_join_params[1] = self.join_params
                self.write_join_parameters()
            else:
                self.model_params = self.fitted_params[:]
                self.model_param_errs = self.fit_errs[:]
            self.model = gen_gaussian_portrait(
                self.model_code, self.fitted_params, self.scattering_index,
                self.phases, self.freqs[0], self.nu_ref, self.join_ichans,
                self.Ps[0])
            mask = np.asarray(self.masks[0, 0])
            self.model_masked = self.model * mask
            self.modelx = self.model[mask.mean(axis=1) != 0]
            self.duration = time.time() - start
            self.total_time += self.duration
            yield

    def check_convergence(self, efac=1.0, quiet=False):
        """ppgauss.py:285-341: the phase and DM of the data against the
        fitted model (fit_phase_shift for the guess, fit_portrait for both);
        converged (1) when each is within efac of its error, else 0."""
        portx, modelx = self.portx, self.modelx
        if self.njoin:
            # data and model with every archive's join rotation taken out
            portx, modelx = np.zeros(portx.shape), np.zeros(modelx.shape)
            for ii in range(self.njoin):
                jicx = self.join_ichanxs[ii]
                phi = -self.join_params[0::2][ii]
                DM = -self.join_params[1::2][ii]
                portx[jicx] = rotate_data(self.portx[jicx], phi, DM,
                                          self.Ps[0], self.freqsxs[0][jicx],
                                          self.nu_ref)
                modelx[jicx] = rotate_data(self.modelx[jicx], phi, DM,
                                           self.Ps[0], self.freqsxs[0][jicx],
                                           self.nu_ref)
        phase_guess = fit_phase_shift(portx.mean(axis=0),
                                      modelx.mean(axis=0)).phase
        phase_guess %= 1
        if phase_guess >= 0.5:
            phase_guess -= 1.0
        fp = fit_portrait(portx, modelx,
                          np.array([phase_guess, 0.0]), self.Ps[0],
                          self.freqsxs[0], self.nu_fit, None, None,
                          bounds=[(None, None), (None, None)], id=None,
                          quiet=True)
        self.fp_results = fp
        self.phi, self.phierr, self.DM, self.DMerr, self.red_chi2 = \
            fp.phase, fp.phase_err, fp.DM, fp.DM_err, fp.red_chi2
        if not quiet:
            print("Iter %d:" % (self.itern - self.niter))
            print(" phase offset of %.2e +/- %.2e [rot]" % (self.phi,
                                                            self.phierr))
            print(" DM of %.6e +/- %.2e [cm**-3 pc]" % (self.DM, self.DMerr))
            print(" red. chi**2 of %.2f." % self.red_chi2)
        if min(abs(self.phi), abs(1 - self.phi)) < abs(self.phierr) * efac \
                and abs(self.DM) < abs(self.DMerr) * efac:
            if not quiet:
                print("\nIteration converged.\n")
            return 1
        return 0

    def write_model(self, outfile=None, append=False, quiet=False):
        """ppgauss.py:343-361: locs wrapped into [0, 1), tau in seconds."""
        if outfile is None:
            outfile = self.datafile + ".gmodel"
        model_params = np.copy(self.model_params)
        model_params[2::6] = np.where(model_params[2::6] >= 1.0,
                                      model_params[2::6] % 1,
                                      model_params[2::6])
        model_params[1] *= self.Ps[0] / self.nbin
        write_model(outfile, self.model_name, self.model_code, self.nu_ref,
                    model_params, self.fit_flags, self.scattering_index,
                    self.fitalpha, append=append, quiet=quiet)

    def write_errfile(self, errfile=None, append=False, quiet=False):
        """ppgauss.py:363-379: the parameter uncertainties in write_model's
        format (a fixed parameter's is 0)."""
        if errfile is None:
            errfile = self.datafile + ".gmodel_errs"
        model_param_errs = np.copy(self.model_param_errs)
        model_param_errs[1] *= self.Ps[0] / self.nbin
        write_model(errfile, self.model_name + "_errors", self.model_code,
                    self.nu_ref, model_param_errs, self.fit_flags,
                    self.scattering_index_err, self.fitalpha, append=append,
                    quiet=quiet)


class GaussianSelector(object):
    """The reference's interactive window for hand-placing components
    (ppgauss.py:382-663): outside the accelerated path."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(_OUTSIDE % "the interactive "
                                  "GaussianSelector")
