"""Drop-in mirror of PulsePortraiture's ``ppspline``: PCA + B-spline portrait
models, the wavelet search on the device.

``DataPortrait(datafile).make_spline_model(...)`` is the reference's workflow
(ppspline.py:39-217) for ONE archive: the profiles of the aligned average
portrait are decomposed with pplib.pca (host, float64), the significant
eigenvectors are picked and, with smooth=True, wavelet-smoothed together with
the mean profile by pplib.find_significant_eigvec / smart_smooth
(ppf_swt_analyse_batch / ppf_swt_score_batch under scipy.optimize.brute), and
the curve the projected profiles trace with frequency is fitted with
scipy.interpolate.splprep (host).  The written .spl file is what
pptoas.GetTOAs and pplib.read_spline_model read.

The wavelet transform is written from its definition (_swt.py); agreement
with PyWavelets itself has not been checked.

Outside the accelerated path (NotImplementedError): metafiles (several
archives joined), write_model_archive and every plot.
"""
import pickle

import numpy as np
import scipy.interpolate as si

from .pplib import DataPortrait as _DataPortrait
from .pplib import (find_significant_eigvec, gen_spline_portrait, pca,
                    reconstruct_portrait, smart_smooth)

_OUTSIDE = "%s is outside the accelerated path"


class DataPortrait(_DataPortrait):
    """The data a spline model is made from: pplib.DataPortrait (a fold-mode
    PSRFITS file or a DataBunch) with ppspline.py's methods."""

    def __init__(self, datafile=None, joinfile=None, quiet=False,
                 **load_data_kwargs):
        from .pplib import file_is_type
        if isinstance(datafile, (list, tuple)) or (
                not isinstance(datafile, dict) and
                file_is_type(datafile, "ASCII")):
            raise NotImplementedError(
                _OUTSIDE % "ppspline.DataPortrait(metafile): joining several "
                "archives")
        _DataPortrait.__init__(self, datafile, joinfile, quiet,
                               **load_data_kwargs)

    def make_spline_model(self, max_ncomp=10, smooth=True, snr_cutoff=150.0,
                          rchi2_tol=0.1, k=3, sfac=1.0, max_nbreak=None,
                          model_name=None, quiet=False, **kwargs):
        """ppspline.py:39-217: a model from PCA and B-spline interpolation.

        max_ncomp (<= 10) caps the eigenvectors kept; smooth=True smooths
        them and the mean profile (smart_smooth); snr_cutoff is the S/N an
        eigenvector needs to be significant; rchi2_tol the smoothing
        tolerance; k the spline degree; sfac scales splprep's smoothing
        condition; max_nbreak, when the fit returns more unique knots, refits
        with at most that many (2: s = inf).  kwargs go to
        find_significant_eigvec (evaluator=... selects the wavelet evaluator
        for the mean profile too, see _swt)."""
        port = self.portx
        SNRs = np.asarray(self.SNRsxs, dtype=float)
        pca_weights = SNRs / np.sum(SNRs)
        mean_prof = (port.T * pca_weights).T.sum(axis=0) / pca_weights.sum()
        freqs = self.freqsxs[0]
        nu_lo, nu_hi = freqs.min(), freqs.max()
        nchan_all = len(self.freqs[0])
        nbin = port.shape[1]
        if nbin % 2 != 0:
            print("nbin = %d is odd; cannot wavelet_smooth.\n" % nbin)
            smooth = False
        elif np.modf(np.log2(nbin))[0] != 0.0:
            print("nbin = %d is not a power of two; can only try "
                  "wavelet_smooth to one level; recommend resampling to a "
                  "power-of-two number of phase bins.\n" % nbin)
        eigval, eigvec = pca(port, mean_prof, pca_weights, quiet=quiet)
        return_max = 10 if max_ncomp is None else min(max_ncomp, 10)
        found = find_significant_eigvec(
            eigvec, check_max=10, return_max=return_max,
            snr_cutoff=snr_cutoff, return_smooth=bool(smooth),
            rchi2_tol=rchi2_tol, **kwargs)
        if smooth:
            ieig, smooth_eigvec = found
            smooth_mean_prof = smart_smooth(
                mean_prof, rchi2_tol=rchi2_tol,
                evaluator=kwargs.get("evaluator"))
            use_prof, use_vec = smooth_mean_prof, smooth_eigvec
        else:
            ieig = found
            use_prof, use_vec = mean_prof, eigvec
        ncomp = len(ieig)
        tck, u = [np.array([]), np.array([]), 0], np.array([])
        fp = ier = msg = None
        if ncomp == 0:
            # a constant portrait: the (smoothed) mean profile
            proj_port = port[:, :ncomp]
            modelx = reconst_port = np.tile(use_prof, len(freqs)).reshape(
                len(freqs), nbin)
            model = np.tile(use_prof, nchan_all).reshape(nchan_all, nbin)
        else:
            basis = use_vec[:, ieig]
            reconst_port = reconstruct_portrait(port, mean_prof, basis)
            proj_port = np.dot(port - mean_prof, basis)
            s = sfac * len(proj_port) * \
                np.sum((SNRs * self.noise_stdsxs) ** 2) / sum(SNRs) ** 2
            flip = -1 if self.bw < 0 else 1     # splprep wants increasing u
            fit = dict(w=pca_weights[::flip], u=freqs[::flip], ub=nu_lo,
                       ue=nu_hi, k=k, task=0, t=None, full_output=1, per=0,
                       quiet=int(quiet))
            (tck, u), fp, ier, msg = si.splprep(proj_port[::flip].T, s=s,
                                                nest=None, **fit)
            if max_nbreak is not None and len(np.unique(tck[0])) > max_nbreak:
                if max_nbreak < 2:
                    print("max_nbreak not >= 2; setting max_nbreak = 2...")
                    max_nbreak = 2
                if max_nbreak == 2:
                    s = np.inf
                (tck, u), fp, ier, msg = si.splprep(
                    proj_port[::flip].T, s=s, nest=max_nbreak + (k * 2),
                    **fit)
            if ier > 1:
                print("Something went wrong in si.splprep for %s:\n%s" %
                      (self.source, msg))
            modelx = gen_spline_portrait(use_prof, freqs, basis, tck)
            model = gen_spline_portrait(use_prof, self.freqs[0], basis, tck)
        self.ieig, self.ncomp = ieig, ncomp
        self.eigvec, self.eigval = eigvec, eigval
        self.mean_prof = mean_prof
        if smooth:
            self.smooth_mean_prof = smooth_mean_prof
            self.smooth_eigvec = smooth_eigvec
        self.proj_port, self.reconst_port = proj_port, reconst_port
        self.tck, self.u, self.fp, self.ier, self.msg = tck, u, fp, ier, msg
        self.model_name = self.datafile + ".spl" if model_name is None \
            else model_name
        self.model, self.modelx = model, modelx
        self.model_masked = self.model * np.asarray(self.masks[0, 0])
        if not quiet:
            if proj_port.sum():
                print("B-spline interpolation model %s uses %d basis profile "
                      "components and %d breakpoints (%d B-splines with "
                      "k=%d)." % (self.model_name, ncomp,
                                  len(np.unique(tck[0])),
                                  len(tck[0]) - tck[2] - 1, tck[2]))
            else:
                print("B-spline interpolation model %s uses 0 basis profile "
                      "components; it returns the average profile." %
                      self.model_name)

    def write_model(self, outfile, quiet=False):
        """ppspline.py:219-244: the pickled (protocol 2) list [model name,
        source, datafile, mean profile, eigenvectors, tck], smoothed
        versions when the model has them."""
        if hasattr(self, "smooth_eigvec"):
            prof, vec = self.smooth_mean_prof, self.smooth_eigvec
        else:
            prof, vec = self.mean_prof, self.eigvec
        cols = self.ieig if len(self.ieig) else []
        with open(outfile, "wb") as of:
            pickle.dump([self.model_name, self.source, self.datafile, prof,
                         vec[:, cols], self.tck], of, protocol=2)
        if not quiet:
            print("Wrote modelfile %s." % outfile)

    def write_model_archive(self, *args, **kwargs):
        raise NotImplementedError(_OUTSIDE % "write_model_archive (PSRCHIVE)")

    def show_eigenprofiles(self, *args, **kwargs):
        raise NotImplementedError(_OUTSIDE % "show_eigenprofiles (plots)")

    def show_spline_curve_projections(self, *args, **kwargs):
        raise NotImplementedError(
            _OUTSIDE % "show_spline_curve_projections (plots)")

    def show_model_fit(self, *args, **kwargs):
        raise NotImplementedError(_OUTSIDE % "show_model_fit (plots)")


def main(argv=None):
    """The reference's command line (ppspline.py:291-397)."""
    from optparse import OptionParser
    parser = OptionParser("Usage: %prog -d <datafile> [options]")
    parser.add_option("-d", "--datafile", action="store", metavar="archive",
                      dest="datafile",
                      help="Fold-mode PSRFITS archive of aligned, averaged "
                      "profiles from which to make the model.")
    parser.add_option("-o", "--modelfile", action="store",
                      metavar="modelfile", dest="modelfile",
                      help="Name for output model (pickle) file. "
                      "[default=datafile.spl].")
    parser.add_option("-l", "--model_name", action="store",
                      metavar="model_name", dest="model_name", default=None,
                      help="Optional name for model [default=datafile.spl].")
    parser.add_option("-a", "--archive", action="store", metavar="archive",
                      dest="archive", default=None,
                      help="Name for optional output archive (not built: "
                      "needs PSRCHIVE).")
    parser.add_option("-N", "--norm", action="store",
                      metavar="normalization", dest="norm", default="prof",
                      help="Normalize the input data by channel ('None', "
                      "'mean', 'max', 'rms', 'prof' [default], or 'abs').")
    parser.add_option("-s", "--smooth", action="store_true", dest="smooth",
                      default=False,
                      help="Smooth the eigenvectors and mean profile "
                      "[recommended] with smart_smooth.")
    parser.add_option("-n", "--max_ncomp", action="store",
                      metavar="max_ncomp", dest="max_ncomp", default=10,
                      help="Maximum number of principal components (at most "
                      "10) [default=10].")
    parser.add_option("-S", "--snr", action="store", metavar="snr_cutoff",
                      dest="snr_cutoff", default=150.0,
                      help="S/N ratio cutoff for 'significant' "
                      "eigenprofiles [default=150.0].")
    parser.add_option("-T", "--rchi2_tol", action="store",
                      metavar="tolerance", dest="rchi2_tol", default=0.1,
                      help="Smoothing tolerance between 0.0 and 0.1 "
                      "[default].")
    parser.add_option("-k", "--degree", action="store", metavar="degree",
                      dest="k", default=3,
                      help="Degree of the spline, 1 <= k <= 5 [default=3].")
    parser.add_option("-f", "--sfac", action="store",
                      metavar="smooth_factor", dest="sfac", default=1.0,
                      help="Multiplies the B-spline smoothing condition; 0.0 "
                      "interpolates [default=1.0].")
    parser.add_option("-t", "--knots", action="store", metavar="max_knots",
                      dest="max_nbreak", default=None,
                      help="The maximum number of unique knots.")
    parser.add_option("--plots", action="store_true", dest="make_plots",
                      default=False, help="Plots (not built).")
    parser.add_option("--quiet", action="store_true", dest="quiet",
                      default=False, help="Suppresses output.")
    options, _ = parser.parse_args(argv)
    if options.datafile is None:
        print("\nppspline.py - make a pulse portrait model using PCA & "
              "B-spline interpolation\n")
        parser.print_help()
        print("")
        parser.exit()
    max_nbreak = None if options.max_nbreak is None else \
        int(options.max_nbreak)
    dp = DataPortrait(options.datafile, quiet=options.quiet)
    if options.norm in ("mean", "max", "prof", "rms", "abs"):
        dp.normalize_portrait(options.norm)
    dp.make_spline_model(max_ncomp=int(options.max_ncomp),
                         smooth=options.smooth,
                         snr_cutoff=float(options.snr_cutoff),
                         rchi2_tol=float(options.rchi2_tol), k=int(options.k),
                         sfac=float(options.sfac), max_nbreak=max_nbreak,
                         model_name=options.model_name, quiet=options.quiet)
    modelfile = options.modelfile
    if modelfile is None:
        modelfile = options.datafile + ".spl"
    dp.write_model(modelfile, quiet=options.quiet)
    if options.archive is not None:
        dp.write_model_archive(options.archive, quiet=options.quiet)
    if options.make_plots:
        dp.show_eigenprofiles(title=dp.model_name, savefig=dp.model_name)


if __name__ == "__main__":
    main()
