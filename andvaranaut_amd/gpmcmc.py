"""GPMCMC: the reference's GP-surrogate facade (andvaranaut/gpmcmc.py:30) with its hot path -- the
GP log marginal likelihood, its hyper-parameter gradient and the posterior conditional -- running on
an MI355X through libmi_gp.so instead of PyMC / PyTensor / SciPy-LAPACK.

Same constructor, ``set_data`` / ``sample`` / ``fit`` / ``predict`` / ``change_model`` signatures and the
same ``hypers`` dictionary keys as the reference (gpmcmc.py:31-32,122,158,175-177,472,522-523;
keys recorded at tutorial/tutorial.ipynb:529), including the warped fits ``fit(iwgp=True)`` /
``fit(cwgp=True)`` whose warp parameters are optimised / sampled with the hyper-parameters
(gpmcmc.py:211-279,319): the device supplies dLML/dX and dLML/dy, torch.autograd carries them through the
warps.  ``BO`` and ``inverse_opt`` live in consumers.py.  Out of scope here:
dask-parallel target execution, plots."""
import copy
import os
import re
import threading
from time import time as stopwatch

import numpy as np

from .backend import MiGP, parse_kernel
from .deriv import KERNELS as DERIV_KERNELS, MAX_D as DERIV_MAX_D, MiDerivGP
from .sparse import MAX_INDUCING, MiSparseGP, select_inducing
from .consumers import ConsumersMixin
from .lhc import latin_sample
from .nuts import Trace, sample_chain
from .optimize import find_MAP
from .priors import HyperModel
from .transform import _none_conrev, wgp

# handles that may evaluate at once per device with in-kernel polls on their cross-stream edges (include/mi_gp.h, option 26)
MAX_POLLING_HANDLES = 6


def save_object(obj, fname):
    """core.py:21-23: whole-object checkpoint with cloudpickle (a GPMCMC drops its device handle, see __getstate__)."""
    import cloudpickle

    with open(fname, "wb") as f:
        cloudpickle.dump(obj, f)


def load_object(fname):
    """core.py:24-27."""
    import cloudpickle

    with open(fname, "rb") as f:
        return cloudpickle.load(f)


class PosteriorPaths:
    """What GPMCMC.sample_paths returns: npaths posterior function draws (a paths.PathDraw of the converted-space GP) behind
    predict_mean's conversions."""

    def __init__(self, model, draw):
        self.model, self.draw = model, draw
        self.npaths = draw.npaths

    def __call__(self, x, convert=True, revert=True, return_grad=False):
        """The draws at x (M, nx): values (npaths, M), and with ``return_grad`` (values, gradients (npaths, M, nx)) w.r.t. x as
        passed.  The conversions are predict_mean's, applied per draw, point by point: ``revert=True`` yconrevs[0].rev(f) + mean
        function, the chain rule through rev' and con' for the gradient; a non-zero mean function with ``return_grad`` raises."""
        from .consumers import _con_and_der

        g = self.model
        if return_grad and g.mean != g.zero_mean:
            raise ValueError("sample_paths(...)(return_grad=True) has no form under a non-zero mean function")
        xarg, x = g._converted_x(np.asarray(x, dtype=np.float64), convert)
        if return_grad:
            f, df = self.draw.evaluate(xarg, grad=True)
        else:
            f = self.draw.evaluate(xarg)
        cr0 = g.yconrevs[0]
        y = np.stack([cr0.rev(fs) for fs in f]) + g._mean_at(x) if revert else f
        if not return_grad:
            return y
        if revert:
            for s in range(f.shape[0]):
                df[s] /= np.reshape(cr0.der(cr0.rev(f[s])), (-1, 1))
        if convert:
            for i in range(g.nx):
                cr = g.xconrevs[i]
                if hasattr(cr, "der"):
                    df[:, :, i] *= np.asarray(cr.der(x[:, i]), dtype=np.float64).reshape(1, -1)
                else:
                    df[:, :, i] *= np.array([_con_and_der(cr, v)[1] for v in x[:, i]])[None, :]
        return y, df

    def close(self):
        self.draw.close()


class GPMCMC(ConsumersMixin):
    def __init__(self, xconrevs=None, yconrevs=None, kernel="RBF", noise=True, mean=0, nx=None, ny=None,
                 priors=None, target=None, parallel=False, nproc=1, constraints=None, rundir=None, verbose=True,
                 pulse=1, device=0):
        # argument checks of _core.__init__ (core.py:57-86)
        if (not isinstance(nx, int)) or (nx < 1):
            raise Exception("Error: must specify an integer number of input dimensions > 0")
        if (not isinstance(ny, int)) or (ny < 1):
            raise Exception("Error: must specify an integer number of output dimensions > 0")
        if (not isinstance(priors, list)) or (len(priors) != nx):
            raise Exception("Error: must provide list of scipy.stats univariate priors of length nx")
        if any(getattr(p, "__module__", None) != "scipy.stats._distn_infrastructure" for p in priors):
            raise Exception("Error: must provide list of scipy.stats univariate priors of length nx")
        if not callable(target):
            raise Exception("Error: must provide target function which produces output from specified inputs")
        if not isinstance(parallel, bool):
            raise Exception("Error: parallel must be type bool.")
        if parallel:
            raise NotImplementedError("dask-parallel target evaluation (core.py:105-134) is outside this backend")
        keys = ["constraints", "lower_bounds", "upper_bounds"]
        if (constraints is not None) and ((not isinstance(constraints, dict)) or not all(k in constraints for k in keys)):
            raise Exception(f"Error: provided constraints must be a dictionary with keys {keys} and list items.")
        self.nx, self.ny, self.priors, self.target = nx, ny, priors, target
        self.parallel, self.nproc, self.pulse = parallel, nproc, pulse
        self.constraints, self.verbose = constraints, verbose
        self.rundir = "runs" if rundir is None else rundir
        self.device = int(device)
        self.nsamp = 0
        self.x = np.empty((0, nx))
        self.y = np.empty((0, ny))
        self.dy = None
        self.xc = copy.deepcopy(self.x)
        self.yc = copy.deepcopy(self.y)
        self.__conrev_check(xconrevs, yconrevs)
        self.ym = copy.deepcopy(self.y)
        self.change_model(kernel, noise, mean)
        self.train = None
        self.test = None

    # ------------------------------------------------------------------ data plumbing
    def zero_mean(self, x):
        return np.zeros(self.ny)

    def __conrev_check(self, xconrevs, yconrevs):
        """gpmcmc.py:98-119."""
        xconrevs = [None] * self.nx if xconrevs is None else xconrevs
        yconrevs = [None] * self.ny if yconrevs is None else yconrevs
        if not isinstance(xconrevs, list) or len(xconrevs) != self.nx:
            raise Exception("Error: xconrevs must be None or list of conversion/reversion classes of size nx")
        if not isinstance(yconrevs, list) or len(yconrevs) != self.ny:
            raise Exception("Error: yconrevs must be None or list of conversion/reversion classes of size ny")
        for lst in (xconrevs, yconrevs):
            for j, c in enumerate(lst):
                if c is None:
                    lst[j] = _none_conrev()
                elif (not callable(c.con)) or (not callable(c.rev)):
                    raise Exception("Error: Provided data conversion/reversion function not callable.")
        self.xconrevs, self.yconrevs = xconrevs, yconrevs

    def __evaluate(self, xsamps, fun):
        """Serial branch of _core.__vector_solver (core.py:137-215): failed / non-finite rows are dropped."""
        keep_x, ys = [], []
        for i in range(len(xsamps)):
            try:
                yout = np.atleast_1d(np.asarray(fun(xsamps[i, :]), dtype=np.float64))
            except Exception as e:
                print(f"Warning: Target function evaluation failed at sample {i} with x values: {xsamps[i, :]}; "
                      f"error message: {e}")
                continue
            if yout.shape != (self.ny,):
                raise Exception("Error: number of target function outputs is not equal to ny")
            if np.any(np.isnan(yout)) or np.any(np.abs(yout) == np.inf):
                print(f"Warning: Target function evaluation returned inf/nan at sample with x values: {xsamps[i, :]}")
                continue
            keep_x.append(xsamps[i, :])
            ys.append(yout)
        if not ys:
            return np.empty((0, self.nx)), np.empty((0, self.ny))
        return np.array(keep_x), np.array(ys)

    def __check_constraints(self, xsamps):
        """core.py:218-246, applied to proposed samples before the target runs (lhc.py:30-31).  As in the reference the
        mask entry of a sample is overwritten by every constraint in turn, so the LAST constraint decides (quirk kept)."""
        n0 = len(xsamps)
        mask = np.ones(n0, dtype=bool)
        for i, xj in enumerate(xsamps):
            for e, f in enumerate(self.constraints["constraints"]):
                flag = True
                res = f(xj)
                lo, hi = self.constraints["lower_bounds"][e], self.constraints["upper_bounds"][e]
                if isinstance(lo, list):
                    for k, b in enumerate(lo):
                        if res[k] < b:
                            flag = False
                    for k, b in enumerate(hi):
                        if res[k] > b:
                            flag = False
                elif res < lo or res > hi:
                    flag = False
                mask[i] = flag
                if not flag:
                    print(f"Sample {i + 1} with x values {xj} removed due to invalidaing constraint {e + 1}.")
        xsamps = xsamps[mask]
        if len(xsamps) < n0:
            print(f"{n0 - len(xsamps)} samples removed due to violating constraints.")
        return xsamps

    def __reconvert(self):
        self.xc = np.empty_like(self.x)
        self.yc = np.empty_like(self.y)
        for i in range(self.nx):
            self.xc[:, i] = self.xconrevs[i].con(self.x[:, i])
        for i in range(self.ny):
            self.yc[:, i] = self.yconrevs[i].con(self.y[:, i] - self.ym[:, i])

    def __mean_eval(self):
        xm, ym = self.__evaluate(self.x, self.mean)
        if len(xm) != len(self.x):
            raise Exception("Mean function not valid at every x point in dataset")
        self.ym = ym.reshape(len(self.x), self.ny)

    def sample(self, nsamps, seed=None):
        """gpmcmc.py:158-172 + lhc.py:24-37."""
        if not isinstance(nsamps, int) or (nsamps < 1):
            raise Exception("Error: nsamps argument must be an integer > 0")
        if self.verbose:
            print(f"Evaluating {nsamps} latin hypercube samples...")
        xs = latin_sample(self.priors, nsamps, seed)
        if self.constraints is not None:
            xs = self.__check_constraints(xs)
        xs, ys = self.__evaluate(xs, self.target)
        self.x = np.r_[self.x, xs]
        self.y = np.r_[self.y, ys]
        self.dy = None  # (the target returns values alone: gradients come with set_data)
        self.nsamp = len(self.x)
        self.__mean_eval()
        self.__reconvert()
        self.train = self.test = None

    def _design_ready(self, what):
        """Raised, before any device call, by the adaptive sampler where it has no form or no fit to work from."""
        self._no_sparse(what)
        self._no_trend(what)
        self._no_all_outputs(what)
        if getattr(self, "hypers", None) is None or self.m is None:
            raise Exception(f"Error: fit the GP before {what}")

    def propose_samples(self, nsamps, criterion="alc", ncand=None, nref=None, seed=None, jitter=1e-6):
        """Where to run the target next: ``nsamps`` points chosen greedily among ``ncand`` Latin-hypercube candidates of the
        priors (default max(1024, 16 nsamps)) at the fitted hyper-parameters.  ``criterion="alc"``: each point is the candidate
        whose observation lowers the latent posterior variance, averaged over ``nref`` (default 512) further Latin-hypercube
        points, the most, given the points chosen before it (integrated variance reduction: Cohn 1996, Gramacy & Lee 2009).
        ``criterion="var"``: the candidate of the largest posterior variance.  Neither reads an output, so the whole set is
        chosen before the target runs once.  Candidates and reference points come from ``latin_sample`` under ``seed`` and
        ``seed + 1``, pass the constraints as ``sample``'s points do and are converted with the current ``xconrevs``.  Points are
        chosen in batches of at most 128 (MiGP.design); between batches the chosen ones are appended to the resident
        factorisation with placeholder outputs, and afterwards the handle is rebuilt from the data, so the object is left as it
        was found.  Returns (x, gains): the raw-space points (k, nx), k <= nsamps, and their gains in converted output units."""
        what = "propose_samples"
        self._design_ready(what)
        if not isinstance(nsamps, (int, np.integer)) or isinstance(nsamps, bool) or nsamps < 1:
            raise Exception("Error: nsamps argument must be an integer > 0")
        if criterion not in ("alc", "var"):
            raise ValueError(f"criterion must be 'alc' or 'var' (got {criterion!r})")
        ncand = max(1024, 16 * int(nsamps)) if ncand is None else int(ncand)
        nref = 512 if nref is None else int(nref)
        if ncand < 1 or (criterion == "alc" and nref < 1):
            raise ValueError("ncand and nref must be >= 1")
        xcand = latin_sample(self.priors, ncand, seed)
        xref = latin_sample(self.priors, nref, None if seed is None else seed + 1) if criterion == "alc" else None
        if self.constraints is not None:
            xcand = self.__check_constraints(xcand)
            xref = self.__check_constraints(xref) if xref is not None else None
        if len(xcand) < 1 or (xref is not None and len(xref) < 1):
            raise ValueError("the constraints leave no candidate or no reference point")
        ccand, _ = self._converted_x(xcand, True)
        cref = self._converted_x(xref, True)[0] if xref is not None else None
        gp = self._ensure_gp()
        theta = self._theta_from_hypers(self.hypers, jitter)
        left = np.arange(len(xcand))
        chosen, gains, appended = [], [], False
        try:
            while len(chosen) < nsamps and len(left) > 0:
                k = min(MiGP.DESIGN_MAX_BATCH, int(nsamps) - len(chosen))
                idx, gn, _ = gp.design(theta, ccand[left], cref, batch=k)
                chosen.extend(left[idx])
                gains.extend(gn)
                if len(idx) < k or len(chosen) >= nsamps:
                    break
                gp.append(ccand[left[idx]], np.zeros(len(idx)))  # (placeholders: the criterion never reads an output)
                appended = True
                left = np.delete(left, idx)
        finally:
            if appended:  # the handle holds the placeholders: the next use builds it again from the data
                self.__release()
        return xcand[np.array(chosen, dtype=np.int64)], np.array(gains)

    def adaptive_sample(self, nsamps, batch=None, refit=True, **propose_kwargs):
        """Sequential design: propose ``batch`` points (default: all ``nsamps`` at once) with ``propose_samples(**propose_kwargs)``,
        run the target there, extend the data exactly as ``sample`` does, fit again with the last fit's arguments
        (``refit=False``: keep the hyper-parameters and only rebuild the factorisation on the extended data), and repeat until
        ``nsamps`` points have been proposed.  A ``seed`` among the keyword arguments advances by 2 per round."""
        self._design_ready("adaptive_sample")
        if not isinstance(nsamps, (int, np.integer)) or isinstance(nsamps, bool) or nsamps < 1:
            raise Exception("Error: nsamps argument must be an integer > 0")
        batch = int(nsamps) if batch is None else int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        seed = propose_kwargs.pop("seed", None)
        done, rnd = 0, 0
        while done < nsamps:
            k = min(batch, int(nsamps) - done)
            xs, _ = self.propose_samples(k, seed=None if seed is None else seed + 2 * rnd, **propose_kwargs)
            if len(xs) == 0:
                break
            done += len(xs)
            rnd += 1
            if self.verbose:
                print(f"Evaluating {len(xs)} adaptively chosen samples...")
            xs, ys = self.__evaluate(xs, self.target)
            self.x = np.r_[self.x, xs]
            self.y = np.r_[self.y, ys]
            self.nsamp = len(self.x)
            self.__mean_eval()
            self.__reconvert()
            self.train = self.test = None
            if refit and getattr(self, "_fit_args", None) is not None:
                self.fit(**self._fit_args)
            else:
                self.__release()  # (same hyper-parameters: _ensure_gp builds the handle on the extended data)

    def set_data(self, x, y, dy=None):
        """gpmcmc.py:122-137 + lhc.py:113-131.  ``dy`` (optional): the (n, nx) raw gradients d y[:, 0] / d x of an adjoint solver,
        for ``fit(gradients=True)``; without it the object behaves as it always has."""
        if dy is not None and (not isinstance(dy, np.ndarray) or dy.dtype != "float64" or dy.shape != (len(x), self.nx)
                               or not np.isfinite(dy).all()):
            raise Exception("Error: Setting gradient data requires a finite 2d numpy array of float64 of shape (n, nx)")
        if not isinstance(x, np.ndarray) or len(x.shape) != 2 or x.dtype != "float64" or x.shape[1] != self.nx:
            raise Exception("Error: Setting data requires a 2d numpy array of float64 inputs")
        if not isinstance(y, np.ndarray) or len(y.shape) != 2 or y.dtype != "float64" or y.shape[1] != self.ny:
            raise Exception("Error: Setting data requires a 2d numpy array of float64 outputs")
        for i in range(self.nx):
            intv = self.priors[i].interval(1.0)
            if not all(x[:, i] >= intv[0]) or not all(x[:, i] <= intv[1]):
                raise Exception("Error: provided x data must fit within provided input distribution ranges.")
        self.x, self.y, self.nsamp = x, y, len(x)
        self.dy = dy
        self.__mean_eval()
        self.__reconvert()
        self.train = self.test = None

    def converted_gradients(self, x=None, y=None, dy=None):
        """d yc / d xc at the data (default: the stored x, y[:, 0], dy) by the chain rule through the installed transforms' own
        derivatives: ``yconrevs[0].der`` at y over ``xconrevs[m].der`` at x[:, m], per point and input dimension."""
        x = self.x if x is None else x
        y = self.y[:, 0] if y is None else y
        dy = self.dy if dy is None else dy
        out = np.empty_like(dy)
        dyc = np.asarray(self.yconrevs[0].der(y), dtype=np.float64)
        for m in range(self.nx):
            out[:, m] = dyc * dy[:, m] / np.asarray(self.xconrevs[m].der(x[:, m]), dtype=np.float64)
        return np.ascontiguousarray(out)

    def _gradient_fit_check(self, method, iwgp, cwgp, objective, trend, outputs, inducing):
        """Every refusal of fit(gradients=True), raised before any device call."""
        if getattr(self, "dy", None) is None:
            raise ValueError("gradients=True needs gradient data: call set_data(x, y, dy) first")
        if self.mean != self.zero_mean:
            raise ValueError("gradients=True needs a zero mean function: the gradients of a non-zero mean are not known here")
        if iwgp or cwgp:
            raise ValueError("gradients=True has no form under iwgp / cwgp: the chain rule runs through fixed transforms")
        if method not in ("map", "none"):
            raise ValueError(f"gradients=True needs method='map' or 'none' (got {method!r}): there is no sampler on the gradient binding")
        if objective != "lml":
            raise ValueError(f"gradients=True needs objective='lml' (got {objective!r})")
        if trend is not None:
            raise ValueError(f"gradients=True has no form under trend={trend!r}")
        if outputs != "first":
            raise ValueError("gradients=True has no form under outputs='all': the gradients are those of y[:, 0]")
        if inducing is not None:
            raise ValueError("gradients=True has no form under inducing points: the sparse bound takes values alone")
        if self.nkern != 1 or self.kernel not in DERIV_KERNELS:
            raise ValueError(f"gradients=True needs one kernel out of {DERIV_KERNELS} (got {self.kernel!r}): no composite kernel, and "
                             "a kernel that is twice differentiable")
        if self.nx > DERIV_MAX_D:
            raise ValueError(f"gradients=True needs nx <= {DERIV_MAX_D} (got {self.nx})")

    def del_samples(self, ndels=None, method="coarse_lhc", idx=None):
        """Drop samples (gpmcmc.py:57-72 + lhc.py:50-97): the ndels points nearest to a fresh Latin-hypercube
        sample ('coarse_lhc'), ndels at random, or the given indexes ('specific'); converted copies follow."""
        if method == "coarse_lhc":
            if not isinstance(ndels, int) or ndels < 1:
                raise Exception("Error: must specify positive int for ndels")
            xsamps = latin_sample(self.priors, ndels)
            for i in range(ndels):
                k = int(np.argmin(np.linalg.norm(self.x - xsamps[i], axis=1)))
                self.x, self.y = np.delete(self.x, k, axis=0), np.delete(self.y, k, axis=0)
                self.xc, self.yc = np.delete(self.xc, k, axis=0), np.delete(self.yc, k, axis=0)
                self.ym = np.delete(self.ym, k, axis=0)
        elif method == "random":
            if not isinstance(ndels, int) or ndels < 1:
                raise Exception("Error: must specify positive int for ndels")
            keep = np.random.choice(np.arange(len(self.x)), size=len(self.x) - ndels, replace=False)
            self.x, self.y, self.xc, self.yc, self.ym = (a[keep] for a in (self.x, self.y, self.xc, self.yc, self.ym))
        elif method == "specific":
            if not isinstance(idx, (int, list)):
                raise Exception("Error: must specify int or list of ints for idx")
            mask = np.ones(len(self.x), dtype=bool)
            mask[idx] = False
            self.x, self.y, self.xc, self.yc, self.ym = (a[mask] for a in (self.x, self.y, self.xc, self.yc, self.ym))
        else:
            raise Exception("Error: method must be one of 'coarse_lhc','random','specific'")
        if getattr(self, "dy", None) is not None and len(self.dy) != len(self.x):
            self.dy = None  # (the gradients no longer belong to the rows that are left)
        self.nsamp = len(self.x)
        self.train = self.test = None

    def change_conrevs(self, xconrevs=None, yconrevs=None):
        self.__conrev_check(xconrevs, yconrevs)
        self.__reconvert()

    def change_xconrevs(self, xconrevs=None):
        self.__conrev_check(xconrevs, self.yconrevs)
        self.__reconvert()

    def change_yconrevs(self, yconrevs=None):
        self.__conrev_check(self.xconrevs, yconrevs)
        self.__reconvert()

    def train_test(self, training_frac=0.9):
        from sklearn.model_selection import train_test_split

        self.nsamp = len(self.x)
        self.train, self.test = train_test_split(np.arange(self.nsamp), train_size=training_frac)

    def test_stats(self, revert=True, iwgp=False, cwgp=False, method="none", jitter=1e-6):
        """The numeric half of ``test_plots`` (gpmcmc.py:933-976; the plots are out of scope): condition the model on the
        training split (``train_test``; refitted there with ``method``, 'none' = the stored hypers), predict the held-out
        points and return RMSE, mean absolute / percentage error and R^2 with the arrays ``returndat`` hands back."""
        self._no_all_outputs("test_stats")
        grads = getattr(self, "gradients", False)  # (an object fitted on gradient observations is tested with them)
        if grads:
            self._gradient_fit_check(method, iwgp, cwgp, "lml", None, "first", None)
        trend = getattr(self, "trend", None)  # (an object fitted with a trend is tested with it)
        if trend is not None and (method not in ("none", "map") or iwgp or cwgp):
            raise ValueError(f"test_stats under trend={trend!r} needs method='none' or 'map' and neither iwgp nor cwgp")
        if getattr(self, "train", None) is None:
            self.train_test()
        xtrain, xtest = self.x[self.train, :], self.x[self.test, :]
        ytrain, ytest = self.y[self.train, :], self.y[self.test, :]
        ymtrain, ymtest = self.ym[self.train, :], self.ym[self.test, :]
        m, gp, hypers, _ = self.__fit(xtrain, ytrain - ymtrain, method, iwgp, cwgp, jitter, trend=trend,
                                      dy=self.dy[self.train, :] if grads else None, grad_noise=getattr(self, "grad_noise", None))
        try:
            xctest = np.column_stack([self.xconrevs[i].con(xtest[:, i]) for i in range(self.nx)])
            saved = self.m, self.hypers
            self.m, self.hypers = m, hypers
            try:
                mu, var = gp.predict(self._theta_from_hypers(hypers, jitter), xctest, pred_noise=True)
            finally:
                self.m, self.hypers = saved
        finally:
            gp.close()  # (self.gp was released by __fit: the next predict rebuilds it on the full data)
        ypred, yvars = mu.reshape((-1, 1)), var.reshape((-1, 1))
        if revert:
            yt = ytest[:, 0]
            ypred, yvars = self.__gh_stats(xtest, ypred, yvars, normvar=False)
            meany = np.mean(self.y)
        else:
            yt = self.yconrevs[0].con(ytest[:, 0] - ymtest[:, 0])
            meany = np.mean(self.yconrevs[0].con((self.y - self.ym)[:, 0]))
        ypred, yvars = ypred[:, 0], yvars[:, 0]
        out = {"rmse": float(np.sqrt(np.mean((ypred - yt) ** 2))), "mea": float(np.mean(np.abs(ypred - yt))),
               "mpe": float(np.mean(np.abs(ypred - yt) / np.abs(yt))),
               "r2": float(1 - np.sum((ypred - yt) ** 2) / np.sum((yt - meany) ** 2)),
               "xtest": xtest if revert else xctest, "ytest": yt, "ypred": ypred, "yvars": yvars}
        if self.verbose:
            print(f"RMSE for y is: {out['rmse']:0.5e}")
            print(f"Mean absoulte error for y is: {out['mea']:0.5e}")
            print(f"Mean percentage error for y is: {out['mpe']:0.5%}")
            print(f"R^2 for y is: {out['r2']:0.5f}")
        return out

    def cv_stats(self, nfolds=10, seed=None, folds=None, revert=True, jitter=1e-6):
        """Exact k-fold cross-validation of the fitted model on its own data: every point is predicted from all points outside
        its fold, and the figures of ``test_stats`` are formed over all held-out points (``rmse``, ``mea``, ``mpe``, ``r2``,
        ``ytest``, ``ypred``, ``yvars``, ``xtest``; Gauss-Hermite reversion with ``revert``).  All folds come out of ONE gradient
        evaluation on the full data (MiGP.kfold) instead of a factorisation per fold.  It works at the stored ``self.hypers``:
        NO hyper-parameter is refitted per fold, so the figures measure the model at these hyper-parameters (what
        ``test_stats(method='none')`` measures on one split) and are optimistic where the hyper-parameters were fitted to the
        same data.  ``nfolds``: an integer >= 2 or 'loo' (leave-one-out); the folds are a random partition --
        ``np.random.default_rng(seed).permutation`` cut by ``np.array_split`` -- unless ``folds``, a list of index arrays, is
        given.  A fold holds at most 128 points.  Also returned: ``lpd``, the sum of the folds' joint log predictive densities
        in the original output units (with the Jacobian sum log|d y_con / d y| when the output conversion has ``der``, as in
        ``log_predictive``), ``lpd_folds`` (per fold, its Jacobian included), ``folds`` and ``info`` (0 per fold, or the
        pivot at which the fold's block of K^-1 was not positive definite)."""
        self._no_trend("cv_stats")
        self._no_sparse("cv_stats")
        self._no_all_outputs("cv_stats")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before cross-validating")
        n = len(self.x)
        if folds is None:
            if isinstance(nfolds, str):
                if nfolds != "loo":
                    raise ValueError("nfolds must be an integer or 'loo'")
                folds = [np.array([i]) for i in range(n)]
            else:
                k, kmin = int(nfolds), max(2, -(-n // 128))
                if k < kmin:
                    raise ValueError(f"{k} folds of {n} points: a fold holds at most 128 points and there are at least two "
                                     f"folds, so the smallest admissible nfolds is {kmin}")
                if k > n:
                    raise ValueError(f"nfolds = {k} exceeds the {n} points")
                folds = np.array_split(np.random.default_rng(seed).permutation(n), k)
        folds = [np.asarray(f, dtype=np.int64).reshape(-1) for f in folds]
        equal = len({len(f) for f in folds}) == 1
        logp, mu, var, info = self.gp.kfold(self._theta_from_hypers(self.hypers, jitter), np.stack(folds) if equal else folds)
        idx = np.concatenate(folds)
        xtest, ytest, ymtest = self.x[idx, :], self.y[idx, :], self.ym[idx, :]
        ypred, yvars = np.concatenate(mu).reshape((-1, 1)), np.concatenate(var).reshape((-1, 1))
        if revert:
            yt = ytest[:, 0]
            ypred, yvars = self.__gh_stats(xtest, ypred, yvars, normvar=False)
            meany = np.mean(self.y)
        else:
            yt = self.yconrevs[0].con(ytest[:, 0] - ymtest[:, 0])
            meany = np.mean(self.yconrevs[0].con((self.y - self.ym)[:, 0]))
        ypred, yvars = ypred[:, 0], yvars[:, 0]
        lpd_folds = np.array(logp, dtype=np.float64)
        if hasattr(self.yconrevs[0], "der"):
            jac = np.log(np.abs(self.yconrevs[0].der(ytest[:, 0] - ymtest[:, 0])))
            lpd_folds = lpd_folds + np.add.reduceat(jac, np.cumsum([0] + [len(f) for f in folds[:-1]]))
        out = {"rmse": float(np.sqrt(np.mean((ypred - yt) ** 2))), "mea": float(np.mean(np.abs(ypred - yt))),
               "mpe": float(np.mean(np.abs(ypred - yt) / np.abs(yt))),
               "r2": float(1 - np.sum((ypred - yt) ** 2) / np.sum((yt - meany) ** 2)),
               "xtest": xtest if revert else self._converted(xtest, ytest - ymtest)[0], "ytest": yt, "ypred": ypred,
               "yvars": yvars, "lpd": float(np.sum(lpd_folds)), "lpd_folds": lpd_folds, "folds": folds, "info": info}
        if self.verbose:
            print(f"RMSE for y is: {out['rmse']:0.5e}")
            print(f"Mean absoulte error for y is: {out['mea']:0.5e}")
            print(f"Mean percentage error for y is: {out['mpe']:0.5%}")
            print(f"R^2 for y is: {out['r2']:0.5f}")
            print(f"Log predictive density is: {out['lpd']:0.5e}")
        return out

    def y_dist(self, mode="hist_kde", nsamps=None, return_data=False, surrogate=True, seed=None, mean_only=False, npaths=0,
               nfeatures=4096, path_seed=None):
        """Uncertainty propagation through the surrogate (gpmcmc.py:140-151; tutorial.ipynb cell 34): a Latin-hypercube sample of the
        input priors is pushed through ``predict`` (one device sweep via U = L^-T for large ``nsamps``), or with ``mean_only=True``
        through ``predict_mean``, the matrix-free sweep (samples large enough for a tail).  The density plots of
        LHC.__y_dist (lhc.py:100-110) are outside this backend's scope: ``mode`` is validated as there and otherwise ignored.
        ``surrogate=False``: the underlying data set.  ``return_data=True`` returns (x, y) as the reference does.
        ``npaths > 0``: the same sample goes through one ``sample_paths`` draw instead, and y is (npaths, nsamps): one output
        distribution per posterior function draw, whose spread is the surrogate's uncertainty about the distribution."""
        modes = ["hist", "kde", "ecdf", "hist_kde"]
        if mode not in modes:
            raise Exception(f"Error: selected mode must be one of {modes}")
        if not isinstance(surrogate, bool):
            raise Exception("Error: surrogate argument must be of type bool")
        if not surrogate:
            return (self.x, self.y) if return_data else None
        xsamps = latin_sample(self.priors, nsamps, seed)
        if npaths > 0:
            ypreds = self.sample_paths(npaths, nfeatures, path_seed)(xsamps)
        else:
            ypreds = self.predict_mean(xsamps) if mean_only else self.predict(xsamps)
        if return_data:
            return xsamps, ypreds

    def relative_importances(self, logscale=False):
        """Inverse length scales of the fitted model (gpmcmc.py:1030-1037 draws them as a bar chart; here the values are returned)."""
        if self.hypers is None:
            raise Exception("Error: fit the GP before asking for relative importances")
        ri = 1.0 / np.asarray(self.hypers["l"], dtype=np.float64)
        return np.log(ri) if logscale else ri

    # ------------------------------------------------------------------ mean-only sweeps and sensitivity analysis
    def predict_mean(self, x, convert=True, revert=True, return_grad=False, jitter=1e-6):
        """The posterior mean at x (M, nx) by the matrix-free sweep (MiGP.mean_sweep: O(n d) per point, no variance), an (M, 1)
        array -- the route of sweeps of 1e5 .. 1e7 points.  ``revert=False``: the converted-space mean mu.  ``revert=True``: the
        plug-in surrogate yconrevs[0].rev(mu) + mean function.  That is NOT the Gauss-Hermite mean of ``predict``, which averages
        the reverted variable over the predictive normal: the two agree for an affine output conversion and differ by the
        conversion's curvature times the predictive variance otherwise.  ``return_grad=True`` returns (mean, grad (M, nx)), the
        gradient w.r.t. the inputs x as they are passed: rev'(mu) d mu / d xc_m con'_m(x_m), without rev' under ``revert=False``
        and without con' under ``convert=False``; a non-zero mean function has no derivative here and raises ValueError."""
        from .consumers import _con_and_der

        self._no_trend("predict_mean")
        self._no_sparse("predict_mean")
        self._no_all_outputs("predict_mean")
        if return_grad and self.mean != self.zero_mean:
            raise ValueError("predict_mean(return_grad=True) has no form under a non-zero mean function")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before predicting")
        xarg, x = self._converted_x(np.asarray(x, dtype=np.float64), convert)
        theta = self._theta_from_hypers(self.hypers, jitter)
        if return_grad:
            mu, g = self.gp.mean_sweep(theta, xarg, grad=True)
        else:
            mu = self.gp.mean_sweep(theta, xarg)
        y = self.yconrevs[0].rev(mu) + self._mean_at(x) if revert else mu
        if not return_grad:
            return np.reshape(y, (-1, 1))
        if revert:
            g = g / np.reshape(self.yconrevs[0].der(self.yconrevs[0].rev(mu)), (-1, 1))
        if convert:
            for i in range(self.nx):
                cr = self.xconrevs[i]
                if hasattr(cr, "der"):  # (the whole column at once: the sweeps this serves hold 1e5 .. 1e7 points)
                    g[:, i] *= np.asarray(cr.der(x[:, i]), dtype=np.float64).reshape(-1)
                else:
                    g[:, i] *= np.array([_con_and_der(cr, v)[1] for v in x[:, i]])
        return np.reshape(y, (-1, 1)), g

    def sample_paths(self, npaths=16, nfeatures=4096, seed=None, jitter=1e-6):
        """``npaths`` (1..128) posterior function draws of the fitted GP by pathwise conditioning (MiGP.draw_paths: a prior draw
        from ``nfeatures`` random Fourier features plus a kernel-weighted update; O((n + nfeatures) d) per point and draw, no
        M x M matrix).  Returns a PosteriorPaths: call it like ``predict_mean`` -- ``paths(x, convert=True, revert=True,
        return_grad=False)`` -- for values (npaths, M), and with ``return_grad`` the gradients (npaths, M, nx) w.r.t. x as passed.
        Each draw is one consistent function over any number of calls; it is of the latent f (no observation noise).  The
        object goes stale (RuntimeError) once the GP is factorised again at other hyper-parameters or given other data."""
        self._no_trend("sample_paths")
        self._no_sparse("sample_paths")
        self._no_all_outputs("sample_paths")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before sampling paths")
        theta = self._theta_from_hypers(self.hypers, jitter)
        return PosteriorPaths(self, self.gp.draw_paths(theta, npaths, nfeatures, seed))

    def active_subspace(self, nsamps=10000, seed=None, x=None, space="converted", revert=False, npaths=0, nfeatures=4096,
                        path_seed=None):
        """The active subspace of the posterior mean (sensitivity.active_subspace_from_gradients) from its gradients at a
        Latin-hypercube sample of the input priors, or at the rows of ``x`` (original inputs).  ``space="converted"`` (default):
        gradients w.r.t. the converted inputs, which are comparable across dimensions; ``"original"``: w.r.t. x.  ``revert``: of the
        plug-in surrogate in the original output space instead of the converted-space mean.  Returns a dict: eigenvalues,
        eigenvectors (columns), C, dgsm (diag C), x, grads.  ``npaths > 0``: the same points also go through one
        ``sample_paths`` draw, and the dict carries the per-draw estimates eigenvalues_paths (npaths, nx) and dgsm_paths
        (npaths, nx) beside the mean-based ones."""
        from . import sensitivity

        if space not in ("converted", "original"):
            raise ValueError("space must be 'converted' or 'original'")
        x = latin_sample(self.priors, nsamps, seed) if x is None else np.asarray(x, dtype=np.float64)
        if space == "converted":
            xc, _ = self._converted_x(x, True)
            _, g = self.predict_mean(xc, convert=False, revert=revert, return_grad=True)
        else:
            _, g = self.predict_mean(x, convert=True, revert=revert, return_grad=True)
        lam, V, C, dgsm = sensitivity.active_subspace_from_gradients(g)
        out = {"eigenvalues": lam, "eigenvectors": V, "C": C, "dgsm": dgsm, "x": x, "grads": g}
        if npaths > 0:
            draws = self.sample_paths(npaths, nfeatures, path_seed)
            if space == "converted":
                _, gp_ = draws(xc, convert=False, revert=revert, return_grad=True)
            else:
                _, gp_ = draws(x, convert=True, revert=revert, return_grad=True)
            per = [sensitivity.active_subspace_from_gradients(gs) for gs in gp_]
            out["eigenvalues_paths"] = np.array([r[0] for r in per])
            out["dgsm_paths"] = np.array([r[3] for r in per])
        return out

    def sobol_indices(self, nsamps=10000, seed=None, revert=True, npaths=0, nfeatures=4096, path_seed=None):
        """First-order (Saltelli 2010) and total (Jansen) Sobol indices of the posterior mean over the input priors: two
        Latin-hypercube base samples of ``nsamps`` points from SeedSequence(seed).spawn(2), the (nx + 2) nsamps points of
        sensitivity.saltelli_design through ``predict_mean``.  Returns a dict: first, total, mean, var.  ``npaths > 0``: the same
        design also goes through one ``sample_paths`` draw, and the dict carries the per-draw estimates first_paths (npaths, nx),
        total_paths, mean_paths and var_paths (npaths,) beside the mean-based ones: their spread is the surrogate's uncertainty."""
        from . import sensitivity

        sa, sb = np.random.SeedSequence(seed).spawn(2)
        A = latin_sample(self.priors, nsamps, np.random.default_rng(sa))
        B = latin_sample(self.priors, nsamps, np.random.default_rng(sb))
        design = sensitivity.saltelli_design(A, B)
        f = self.predict_mean(design, revert=revert)[:, 0]
        first, total, mean, var = sensitivity.sobol_from_evaluations(*sensitivity.split_saltelli(f, self.nx))
        out = {"first": first, "total": total, "mean": mean, "var": var}
        if npaths > 0:
            fp = self.sample_paths(npaths, nfeatures, path_seed)(design, revert=revert)
            per = [sensitivity.sobol_from_evaluations(*sensitivity.split_saltelli(fs, self.nx)) for fs in fp]
            out["first_paths"] = np.array([r[0] for r in per])
            out["total_paths"] = np.array([r[1] for r in per])
            out["mean_paths"] = np.array([r[2] for r in per])
            out["var_paths"] = np.array([r[3] for r in per])
        return out

    def test_plots(self, revert=True, yplots=True, xplots=True, logscale=False, iwgp=False, cwgp=False, method="none",
                   errorbars=True, saveyfig=None, xlab=None, ylab=None, returndat=False):
        """Signature of the reference's ``test_plots`` (gpmcmc.py:933-1026) for drop-in callers: the train / test fit and the
        four printed figures are ``test_stats``; the matplotlib figures themselves are outside this backend's scope, so the
        plotting arguments are accepted and ignored.  ``returndat=True`` returns (xtest, ytest, ypred, yvars) as there."""
        st_ = self.test_stats(revert=revert, iwgp=iwgp, cwgp=cwgp, method=method)
        if returndat:
            return st_["xtest"], st_["ytest"], st_["ypred"], st_["yvars"]

    def change_model(self, kernel=None, noise=None, mean=None):
        """gpmcmc.py:472-519: kernel string grammar, noise flag, mean function; scrubs the fitted model."""
        kernel = self.kernel if kernel is None else kernel
        noise = self.noise if noise is None else noise
        if mean is not None:
            self.mean = self.zero_mean if (not callable(mean) and mean == 0) else mean
            if len(self.x) > 0:
                self.__mean_eval()
                self.__reconvert()
        kerns, ops = parse_kernel(kernel)
        if not isinstance(noise, bool):
            raise Exception("Error: noise must be of type bool")
        self.kernel, self.kerns, self.ops, self.nkern, self.noise = kernel, kerns, ops, len(kerns), noise
        self.__release()
        self.m = None
        self.hypers = None
        self.trend = None
        self.outputs = "first"
        self.output_cov = "shared"
        self.inducing = None
        self.inducing_raw = None
        self.gradients = False
        self.grad_noise = None

    def __release(self):
        gp = getattr(self, "gp", None)
        if gp is not None:
            gp.close()
        self.gp = None

    # -- checkpoint / resume: the reference pickles the whole object (core.py:21-27 save_object / load_object).  Here
    # x, y, the conrevs, `m` (the HyperModel) and `hypers` are the state; the device handle is dropped on pickling
    # and rebuilt from them on the next predict / BO / inverse_opt.
    def __getstate__(self):
        state = dict(self.__dict__)
        state["gp"] = None
        return state

    def _ensure_gp(self):
        if self.gp is None and self.hypers is not None and self.m is not None:
            xin, yin = self._converted(self.x, self.y - self.ym)
            if getattr(self, "gradients", False):  # a fit on gradient observations: the handle under its binding
                self.gp = MiDerivGP(xin, yin, self.converted_gradients(), self.kernel, device=self.device,
                                    grad_noise=getattr(self, "grad_noise", None))
                return self.gp
            if getattr(self, "inducing", None) is not None:  # a sparse fit: the bound's object on the stored inducing points
                self.gp = MiSparseGP(xin, yin, self.inducing, self.kernel, device=self.device)
                return self.gp
            self.gp = MiGP(xin, yin, self.kernel, device=self.device)
            if getattr(self, "trend", None) is not None:
                self.gp.set_trend(self.trend)
            if getattr(self, "outputs", "first") == "all":
                self.gp.set_outputs(self._converted_outputs(self.y - self.ym))
                self.gp.set_output_cov(getattr(self, "output_cov", "shared"))
        return self.gp

    def _no_trend(self, what):
        """Raised, before any device call, by what has no form under a fitted trend."""
        if getattr(self, "trend", None) is not None:
            raise ValueError(f"{what} has no form under trend={self.trend!r}: fit without a trend to use it")

    def _no_sparse(self, what):
        """Raised, before any device call, by what needs the dense factorisation after a fit on inducing points -- or the plain
        handle after a fit on gradient observations, whose binding serves fit, predict and test_stats alone."""
        if getattr(self, "gradients", False):
            raise ValueError(f"{what} has no form under a fit on gradient observations (gradients=True): fit with "
                             "gradients=False to use it")
        if getattr(self, "inducing", None) is not None:
            raise ValueError(f"{what} has no form under a sparse fit (inducing={len(self.inducing)} points): it needs the dense "
                             "factorisation; fit with inducing=None to use it")

    def _inducing_points(self, inducing, inducing_seed, method, iwgp, cwgp, objective, trend, outputs, optimize_inducing=False):
        """(Z, Zraw) of fit(inducing=...): the inducing points converted by the installed xconrevs and as raw inputs, or
        (None, None).  Every refusal is raised here, before any device call."""
        if optimize_inducing and (inducing is None or method != "map"):
            raise ValueError("optimize_inducing=True needs inducing points to move and method='map': give inducing=m or an array, "
                             "and fit with method='map'")
        if inducing is None:
            return None, None
        warps = bool(iwgp or cwgp)
        if (method not in ("map", "none") or (warps and method != "map") or objective != "lml" or trend is not None
                or outputs != "first"):
            raise ValueError("inducing needs method='map' or 'none', objective='lml', trend=None, outputs='first' and neither iwgp "
                             "nor cwgp: the sparse bound has no sampler, no cross-validation objective, no trend, no warps and one output")
        if warps and optimize_inducing:
            raise ValueError("inducing: iwgp / cwgp and optimize_inducing=True do not combine -- under warps the inducing points "
                             "are raw inputs that move with the input warp, not free parameters")
        if iwgp and not any(isinstance(c, wgp) for c in self.xconrevs):
            raise ValueError("inducing with iwgp=True needs at least one wgp among xconrevs: there is no input warp to fit")
        if cwgp and (not isinstance(self.yconrevs[0], wgp) or self.yconrevs[0].np == 0):
            raise ValueError("inducing with cwgp=True needs yconrevs[0] to be a wgp with tunable parameters: there is no output "
                             "warp to fit")
        xin, _ = self._converted(self.x, self.y - self.ym)
        if isinstance(inducing, (int, np.integer)) and not isinstance(inducing, bool):
            if not 1 <= inducing <= min(len(xin), MAX_INDUCING):
                raise ValueError(f"inducing = {inducing} points: 1 <= inducing <= min(n, {MAX_INDUCING}) is required (n = {len(xin)})")
            Z, idx = select_inducing(xin, int(inducing), seed=inducing_seed, return_index=True)
            return Z, np.ascontiguousarray(self.x[idx], dtype=np.float64)
        Z = np.array(inducing, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != self.nx or not 1 <= Z.shape[0] <= min(len(xin), MAX_INDUCING) or not np.isfinite(Z).all():
            raise ValueError(f"inducing must be an int or a finite (m, nx = {self.nx}) array of raw inputs with 1 <= m <= "
                             f"min(n, {MAX_INDUCING})")
        Zraw = np.ascontiguousarray(Z.copy())
        for i in range(self.nx):
            Z[:, i] = self.xconrevs[i].con(Z[:, i])
        return np.ascontiguousarray(Z), Zraw

    def _no_all_outputs(self, what):
        """Raised, before any device call, by what has no form once every output is modelled (fit(outputs="all"))."""
        if getattr(self, "outputs", "first") == "all":
            raise ValueError(f"{what} has no form under outputs='all': fit with outputs='first' to use it")

    def _converted_outputs(self, y):
        """Every column of y through its own yconrevs[i]: the (n, ny) outputs of a fit with outputs="all"."""
        return np.ascontiguousarray(np.column_stack([self.yconrevs[i].con(y[:, i]) for i in range(self.ny)]))

    # ------------------------------------------------------------------ fit
    def fit(self, method="map", return_data=False, iwgp=False, cwgp=False, jitter=1e-6, truncate=False,
            restarts=1, objective="lml", nfolds=10, fold_seed=None, trend=None, outputs="first", output_cov="shared",
            inducing=None, inducing_seed=None, optimize_inducing=False, gradients=False, grad_noise=None, **kwargs):
        """gpmcmc.py:175-182.  ``gradients=True`` (with ``set_data(x, y, dy)``, ``method="map"`` or ``"none"``) conditions on the
        gradients as well as the values: the n (1 + nx) observations of a joint GP over f and grad f (gradient-enhanced kriging),
        the raw gradients converted by the chain rule through the installed transforms (``converted_gradients``).  It needs a
        zero mean function, one RBF or Matern52 kernel, ``objective="lml"``, no trend, ``outputs="first"``, no inducing points
        and neither iwgp nor cwgp; ``grad_noise`` is a fixed noise variance of the converted gradients (scalar or (n, nx); None:
        the jitter alone).  The choice is part of the object's state (``self.gradients``): ``predict`` and ``test_stats`` follow
        it, what needs the plain handle raises ValueError.
        ``objective="loo"`` (with ``method="map"``) maximises the leave-one-out log predictive density
        sum_i log p(y_i | y_-i) plus the priors instead of the log marginal likelihood (Rasmussen & Williams section 5.4.2: the
        criterion for a misspecified kernel family); the hyper-parameters are stored as a MAP fit stores them.  It has no
        sampler (a pseudo-likelihood) and no warps (their data-side gradients are the marginal likelihood's).
        ``objective="kfold"`` maximises the k-fold log predictive density sum_f log p(y_I_f | y_-I_f) plus the priors under the
        same conditions: the remedy where points cluster and every left-out point is predicted by its twin.  The folds are a
        random partition, ``np.random.default_rng(fold_seed).permutation`` cut into blocks of b = ceil(n / nfolds) points (the
        last fold may be smaller; a fold holds at most 128 points); ``return_data`` carries them as ``data["folds"]``, index
        arrays into the data as given, for ``cv_stats(folds=...)``.
        ``trend="constant"`` or ``"linear"`` (with ``method="map"``, ``objective="lml"``, no warps) gives the GP a prior mean
        h(x)^T beta with h = [1] or [1, x_1 .. x_nx] in the converted inputs, whose coefficients carry a vague prior and are
        integrated out (Rasmussen & Williams section 2.7): the hyper-parameters are those of a zero-mean fit, the fit maximises
        the trend's marginal likelihood, and ``predict`` returns the trend's conditional.  The choice is part of the object's
        state (``self.trend``).  Restarts run one after the other.
        ``outputs="first"`` (default) models y[:, 0] alone, whatever ``ny`` is.  ``outputs="all"`` (``ny >= 2``, with
        ``method="map"``, ``objective="lml"``, no trend, no warps) models every column under ONE shared kernel and one noise,
        column i converted by ``yconrevs[i]``, the outputs independent given the hyper-parameters: the fit maximises the sum of
        the columns' log marginal likelihoods plus the priors on one factorisation per evaluation, and ``predict`` returns
        (M, ny) arrays.  The choice is part of the object's state (``self.outputs``).
        ``output_cov="shared"`` (default) is that model: one variance for every output, in converted units.
        ``output_cov="integrated"`` (with ``outputs="all"``, at least ny + 2 points) gives the outputs a ny x ny covariance Sigma,
        vec(Y) ~ N(0, Sigma (x) K_y), under the Jeffreys prior |Sigma|^-(ny+1)/2 and integrates it out in closed form (the
        separable emulator of Conti & O'Hagan 2010): the fit no longer depends on how the columns are scaled or mixed, and
        ``predict(return_var=True)`` returns a variance per output, column i reverted through ``yconrevs[i]``.  That marginal
        likelihood does not change under K_y -> c K_y, so only their priors identify the overall scale of kv, gv and the
        jitter.  The choice is part of the object's state (``self.output_cov``).
        ``inducing=m`` (an int) or an (m, nx) array of raw inputs (with ``method="map"`` or ``"none"``, ``objective="lml"``, no
        trend, ``outputs="first"``) fits on m << n inducing points instead of the n x n covariance, for data sets one
        card cannot factorise: the fit maximises Titsias' collapsed variational bound (a lower bound of the log marginal
        likelihood, exact theta gradient, the data streamed in chunks) plus the priors, and ``predict`` returns the sparse
        predictive.  An int chooses the points by k-means++ seeding among the converted inputs (``select_inducing``,
        ``inducing_seed``); an array goes through ``xconrevs``.  At most 2048 points.  With ``optimize_inducing=False``
        (default) the locations stay where they are.  ``optimize_inducing=True`` (``method="map"``) trains them jointly with the
        hyper-parameters, as the bound -- variational in Z -- allows: L-BFGS-B runs over [q | vec(Z)] with the exact dF/dZ of the
        device, Z in converted input space without prior or bounds, started at the points ``inducing`` gives;
        ``data["inducing_start"]`` keeps those.  The choice is part of the object's state (``self.inducing``, the converted --
        with ``optimize_inducing`` the optimised -- points) and survives pickling;
        ``iwgp`` / ``cwgp`` combine with ``inducing`` under ``method="map"`` (not with ``optimize_inducing``): the inducing points
        are then raw inputs (``self.inducing_raw``, ``data["inducing_raw"]``; an int picks data rows by k-means++ over the
        inputs as the installed warps convert them), every evaluation warps them along with the data and pulls the bound's exact
        dF/dy, dF/dX and dF/dZ back onto the warp parameters, and ``self.inducing`` ends as those points under the fitted warps;
        what needs the dense factorisation (predict_joint, sample_posterior, log_predictive, cv_stats, predict_mean,
        sample_paths, predict_posterior, the resident paths of BO and inverse_opt) then raises ValueError."""
        if gradients:
            self._gradient_fit_check(method, iwgp, cwgp, objective, trend, outputs, inducing)
        Z, Zraw = self._inducing_points(inducing, inducing_seed, method, iwgp, cwgp, objective, trend, outputs, optimize_inducing)
        sparse_warps = Z is not None and bool(iwgp or cwgp)
        if outputs not in ("first", "all"):
            raise ValueError(f"outputs must be 'first' or 'all' (got {outputs!r})")
        if output_cov not in MiGP.OUTPUT_COVS:
            raise ValueError(f"output_cov must be one of {list(MiGP.OUTPUT_COVS)} (got {output_cov!r})")
        if output_cov != "shared" and outputs != "all":
            raise ValueError(f"output_cov={output_cov!r} needs outputs='all'")
        if outputs == "all":
            if self.ny < 2:
                raise ValueError("outputs='all' needs ny >= 2")
            if method != "map" or objective != "lml" or trend is not None or iwgp or cwgp:
                raise ValueError("outputs='all' needs method='map', objective='lml', trend=None and neither iwgp nor cwgp")
            if output_cov != "shared" and self.x is not None and len(self.x) < self.ny + 2:
                raise ValueError(f"output_cov={output_cov!r} needs at least ny + 2 = {self.ny + 2} points, got {len(self.x)}")
        if trend is not None:
            if trend not in ("constant", "linear"):
                raise ValueError(f"trend must be None, 'constant' or 'linear' (got {trend!r})")
            if method != "map" or objective != "lml" or iwgp or cwgp:
                raise ValueError("trend needs method='map', objective='lml' and neither iwgp nor cwgp")
        cv = None
        if objective == "kfold":
            cv = self._kfold_plan(method, iwgp, cwgp, nfolds, fold_seed)
        elif objective not in MiGP.OBJECTIVES:
            raise ValueError(f"objective must be one of {list(MiGP.OBJECTIVES) + ['kfold']}")
        if objective == "loo" and (method != "map" or iwgp or cwgp):
            raise ValueError("objective='loo' needs method='map' and neither iwgp nor cwgp")
        self.m, self.gp, self.hypers, data = self.__fit(self.x, self.y - self.ym, method, iwgp, cwgp, jitter,
                                                        truncate, restarts, objective=objective, cv=cv, trend=trend, outputs=outputs,
                                                        output_cov=output_cov, inducing=Z, optimize_inducing=optimize_inducing,
                                                        inducing_raw=Zraw if sparse_warps else None,
                                                        dy=self.dy if gradients else None, grad_noise=grad_noise, **kwargs)
        # (under warps the stored points are the raw ones converted by the FITTED warps: what predict and a rebuilt object need)
        self.inducing = data["inducing"] if (optimize_inducing or sparse_warps) else Z
        self.inducing_raw = Zraw
        # what adaptive_sample(refit=True) fits again with
        self._fit_args = dict(method=method, iwgp=iwgp, cwgp=cwgp, jitter=jitter, truncate=truncate, restarts=restarts, objective=objective,
                              nfolds=nfolds, fold_seed=fold_seed, trend=trend, outputs=outputs, output_cov=output_cov, inducing=inducing,
                              inducing_seed=inducing_seed, optimize_inducing=optimize_inducing, gradients=gradients,
                              grad_noise=grad_noise, **kwargs)
        self.gradients = bool(gradients)
        self.grad_noise = grad_noise if gradients else None
        self.trend = trend
        self.outputs = outputs
        self.output_cov = output_cov
        if return_data:
            return data

    def _kfold_plan(self, method, iwgp, cwgp, nfolds, fold_seed):
        """(b, permutation) of a fit on the k-fold objective: the fit's handle holds the data in the order of the permutation,
        where the folds are the contiguous blocks of b points.  Every refusal is raised here, before any device call."""
        if method != "map" or iwgp or cwgp:
            raise ValueError("objective='kfold' needs method='map' and neither iwgp nor cwgp")
        n = len(self.x)
        if isinstance(nfolds, bool) or not isinstance(nfolds, (int, np.integer)) or nfolds < 2:
            raise ValueError(f"objective='kfold' needs an integer nfolds >= 2 (got {nfolds!r})")
        if nfolds > n:
            raise ValueError(f"objective='kfold': nfolds = {nfolds} exceeds the {n} points")
        b = -(-n // int(nfolds))
        if b > 128:
            raise ValueError(f"objective='kfold': {nfolds} folds of {n} points hold {b} points each and a fold holds at most 128, "
                             f"so the smallest admissible nfolds is {-(-n // 128)}")
        return b, np.random.default_rng(fold_seed).permutation(n)

    def _converted(self, x, y):
        xin = np.zeros_like(x)
        for i in range(self.nx):
            xin[:, i] = self.xconrevs[i].con(x[:, i])
        yin = self.yconrevs[0].con(y[:, 0])  # only y[:,0] is modelled (gpmcmc.py:279)
        return np.ascontiguousarray(xin), np.ascontiguousarray(yin)

    # -- warps whose parameters are model variables (gpmcmc.py:211-279, 433-462)
    def cwgp_set(self, params, mode="numpy", y=None):
        """Set (mode='numpy') or build (otherwise) the output warp with new parameters (gpmcmc.py:433-441)."""
        if y is None:
            y = self.y - self.ym
        warper = wgp(self.yconrevs[0].warping_names, params, y[:, 0], mode=mode)
        if mode == "numpy":
            self.change_yconrevs([warper])
        else:
            return warper

    def iwgp_set(self, params, mode="numpy", x=None):
        """Set / build the input warps with new parameters (gpmcmc.py:443-462)."""
        if x is None:
            x = self.x
        xconrevs, rc = [], 0
        for i in range(self.nx):
            if isinstance(self.xconrevs[i], wgp):
                ran = len(self.xconrevs[i].params)
                xconrevs.append(wgp(self.xconrevs[i].warping_names, params[rc : rc + ran], y=x[:, i],
                                    xdist=self.priors[i], mode=mode))
                rc += ran
            else:
                xconrevs.append(self.xconrevs[i])
        if mode == "numpy":
            self.change_xconrevs(xconrevs=xconrevs)
        else:
            return xconrevs

    def _warp_sizes(self, iwgp, cwgp):
        n_i = n_pos = n_free = 0
        if iwgp:
            n_i = sum(c.np for c in self.xconrevs if isinstance(c, wgp))
            if n_i == 0:
                raise Exception("Error: iwgp set to true but none of xconrevs are wgp classes")
        if cwgp:
            if not isinstance(self.yconrevs[0], wgp):
                raise Exception("Error: cwgp set to true but yconrevs class is not wgp")
            if self.yconrevs[0].np == 0:
                raise Exception("Error: cwgp set to true but wgp class has no tuneable parameters")
            n_pos = int(np.sum(self.yconrevs[0].pos[: self.yconrevs[0].np]))
            n_free = self.yconrevs[0].np - n_pos
        return n_i, n_pos, n_free

    def _cwgp_params(self, pos_vals, free_vals):
        """Interleave the positive and unconstrained output-warp parameters in warp order (gpmcmc.py:263-275)."""
        out, rc, rcpos = [], 0, 0
        for i in range(self.yconrevs[0].np):
            if self.yconrevs[0].pos[i]:
                out.append(pos_vals[rcpos])
                rcpos += 1
            else:
                out.append(free_vals[rc])
                rc += 1
        return out

    def _warp_likelihood(self, gp, x, y, xin0, iwgp, cwgp, zraw=None):
        """likelihood(values, theta) for HyperModel.logp_dlogp with warp variables: warp the data with the
        current parameters (torch, host), evaluate LML + its theta / X / y gradients on the device, add the
        warp Jacobian sum(log y') (gpmcmc.py:319) and pull the data gradients back onto the warp parameters.
        ``zraw`` (a sparse fit: gp is the bound's object) are the inducing points as raw inputs: under iwgp they go through the
        warpers that warp x, the object is moved onto them and dF/dZ joins the pull-back."""
        import torch

        xt = torch.from_numpy(np.ascontiguousarray(x))
        yt = torch.from_numpy(np.ascontiguousarray(y))
        if zraw is not None:
            zt = torch.from_numpy(np.ascontiguousarray(zraw, dtype=np.float64))
            zin0 = np.column_stack([self.xconrevs[i].con(np.asarray(zraw, dtype=np.float64)[:, i]) for i in range(self.nx)])

        def likelihood(values, theta):
            leaves = {}
            xin_t = yin_t = yder_t = zin_t = None
            if iwgp:
                leaves["iwgp"] = torch.tensor(values["iwgp"], dtype=torch.float64, requires_grad=True)
                warpers = self.iwgp_set(leaves["iwgp"], mode="torch", x=xt)
                cols = [warpers[i].conmc(xt[:, i]) if isinstance(warpers[i], wgp) else torch.from_numpy(xin0[:, i])
                        for i in range(self.nx)]
                xin_t = torch.stack(cols, dim=1)
                if zraw is not None:
                    zin_t = torch.stack([warpers[i].conmc(zt[:, i]) if isinstance(warpers[i], wgp) else torch.from_numpy(zin0[:, i])
                                         for i in range(self.nx)], dim=1)
                    if not bool(torch.all(torch.isfinite(zin_t))):
                        return -np.inf, None, {}
            if cwgp:
                for nm in ("cwgp_pos", "cwgp"):
                    if nm in values:
                        leaves[nm] = torch.tensor(values[nm], dtype=torch.float64, requires_grad=True)
                rvs = self._cwgp_params(leaves.get("cwgp_pos"), leaves.get("cwgp"))
                warper = self.cwgp_set(torch.stack(list(rvs)), mode="torch", y=yt)
                yin_t = warper.conmc(yt[:, 0])
                yder_t = warper.dermc(yt[:, 0])
                if not bool(torch.all(torch.isfinite(yin_t))) or not bool(torch.all(yder_t > 0)):
                    return -np.inf, None, {}
            gp.update_data(X=None if xin_t is None else xin_t.detach().numpy(),
                           y=None if yin_t is None else yin_t.detach().numpy())
            gz = None
            if zraw is None:
                val, gth, gy, gx = gp.lml_grad_data(theta, want_x=iwgp)
            elif iwgp:
                gp.set_inducing(zin_t.detach().numpy())
                val, gth, gy, gx, gz = gp.lml_grad_data(theta, want_x=True, want_z=True)
            else:  # the output warp alone moves nothing but y
                val, gth, gy, gx = gp.lml_grad_data(theta, want_x=False, want_z=False)
            if not np.isfinite(val):
                return -np.inf, None, {}
            s = torch.zeros((), dtype=torch.float64)
            if cwgp:
                s = s + (torch.from_numpy(gy) * yin_t).sum() + torch.log(yder_t).sum()
                val = val + float(torch.log(yder_t).sum().detach())
            if iwgp:
                s = s + (torch.from_numpy(gx) * xin_t).sum()
                if gz is not None:
                    s = s + (torch.from_numpy(gz) * zin_t).sum()
            s.backward()
            return val, gth, {k: v.grad.numpy().copy() for k, v in leaves.items()}

        return likelihood

    def __fit(self, x, y, method, iwgp, cwgp, jitter=1e-6, truncate=False, restarts=1, objective="lml", cv=None, trend=None,
              outputs="first", output_cov="shared", inducing=None, optimize_inducing=False, inducing_raw=None, dy=None,
              grad_noise=None, **kwargs):
        n_i, n_pos, n_free = self._warp_sizes(iwgp, cwgp)
        model = HyperModel(self.nx, self.kerns, noise=self.noise, truncate=truncate, jitter=jitter, n_iwgp=n_i,
                           n_cwgp_pos=n_pos, n_cwgp=n_free)
        xin, yin = self._converted(x, y)
        self.__release()
        # (inducing points: gp.lml_grad is then the sparse bound and its gradient, gp.predict the sparse predictive)
        if dy is not None:
            # gradient observations: gp.lml_grad is then the joint GP's marginal likelihood, gp.predict the value's conditional
            # (y is y - ym under the zero mean the fit insists on: the values the output transform's derivative is taken at)
            gp = MiDerivGP(xin, yin, self.converted_gradients(x, y[:, 0], dy), self.kernel, device=self.device, grad_noise=grad_noise)
        else:
            gp = MiGP(xin, yin, self.kernel, device=self.device) if inducing is None else MiSparseGP(xin, yin, inducing, self.kernel,
                                                                                                      device=self.device,
                                                                                                      z_grad=bool(optimize_inducing)
                                                                                                      or (inducing_raw is not None and iwgp),
                                                                                                      data_grad=inducing_raw is not None)
        if trend is not None:
            gp.set_trend(trend)  # (gp.lml_grad then returns the trend's marginal likelihood; the stored handle keeps the trend)
        if outputs == "all":
            gp.set_outputs(self._converted_outputs(y))  # (gp.lml_grad then returns the sum of the columns' marginal likelihoods)
            gp.set_output_cov(output_cov)  # ("integrated": the marginal likelihood with the between-output covariance integrated out)
        lik = self._warp_likelihood(gp, x, y, xin, iwgp, cwgp, zraw=inducing_raw) if (iwgp or cwgp) else None
        # pm.find_MAP maximises without the transform Jacobian, pm.sample with it (priors.py header)
        fun_map = lambda q: model.logp_dlogp(q, gp.lml_grad, jacobian=False, likelihood=lik)  # noqa: E731
        data = None
        nq, zbest = model.nq, None
        if optimize_inducing:
            # the inducing locations join the optimiser's vector, [q | vec(Z)]: every evaluation moves Z on the device, takes the
            # bound with both gradients in one call, hands the theta part to the model and appends dF/dZ (Z has no prior)
            def fun_map(qz):  # noqa: F811
                Zq = qz[nq:].reshape(inducing.shape)
                if not np.isfinite(Zq).all():
                    return -np.inf, np.zeros(len(qz))
                gp.set_inducing(Zq)
                cell = {}

                def bound_grad(theta):
                    F, g, cell["gz"] = gp.lml_grad_z(theta)
                    return F, g

                v, g = model.logp_dlogp(qz[:nq], bound_grad, jacobian=False)
                if not np.isfinite(v) or "gz" not in cell:
                    return -np.inf, np.zeros(len(qz))
                return v, np.concatenate([g, cell["gz"].ravel()])

        if method == "map":
            fit_gp = None
            if cv is not None:
                # the k-fold objective: a handle of its own for the fit, on the permuted data; `gp`, the handle that is stored,
                # keeps the data's order and the ordinary objective
                b, perm = cv
                fit_gp = MiGP(np.ascontiguousarray(xin[perm]), np.ascontiguousarray(yin[perm]), self.kernel, device=self.device)
                fit_gp.set_objective("loo")
                fit_gp.set_cv_block(b)
                fun_map = lambda q: model.logp_dlogp(q, fit_gp.lml_grad, jacobian=False)  # noqa: E731
            elif objective != "lml":
                gp.set_objective(objective)  # (gp.lml_grad is the same callable under either objective)
            best, mp = -np.inf, None
            nrest = max(int(restarts), 1)
            last_error = None
            for _ in range(nrest):
                # the reference builds a random start and never passes it (gpmcmc.py:330-332): every
                # restart begins at the model's initial point, so they coincide; kept as is
                try:
                    q0 = model.initial_point()
                    if kwargs.get("start") is not None:  # pm.find_MAP(start=...), e.g. BO's warm refits (gpmcmc.py:899)
                        q0 = model.q_from_point(kwargs["start"])
                    if optimize_inducing:
                        q0 = np.concatenate([q0, inducing.ravel()])
                    q, info = find_MAP(fun_map, q0, progressbar=kwargs.get("progressbar", False),
                                       maxeval=kwargs.get("maxeval", 5000))
                except RuntimeError:
                    raise  # device / library errors (MiGP._check) are never a "failed restart"
                except Exception as e:
                    if nrest == 1:
                        raise  # single fit: the exception propagates as in gpmcmc.py:343-345
                    print("Restart failed")
                    last_error = e
                    continue
                if info["logp"] > best:
                    best, mp, data, zbest = info["logp"], model.point_dict(q[:nq]), info, q[nq:]
            if fit_gp is not None:
                fit_gp.close()
                if data is not None:
                    data["folds"] = [perm[a : a + b].copy() for a in range(0, len(perm), b)]
            elif objective != "lml":
                gp.set_objective("lml")
            if mp is None:
                raise RuntimeError("find_MAP failed in every restart") from last_error
            if optimize_inducing:
                data["inducing_start"] = inducing.copy()
                data["inducing"] = np.ascontiguousarray(zbest.reshape(inducing.shape))
                gp.set_inducing(data["inducing"])  # the stored object predicts on the optimised points
            if self.verbose:
                print(f"MAP: {data['nfev']} evaluations, logp = {data['logp']:,.5g}")
        elif method == "none":
            mp = self.hypers
        elif method in ("mcmc_mean", "mcmc_map"):
            data = self.__sample(model, gp, x, y, xin, yin, iwgp, cwgp, **kwargs)
            if method == "mcmc_mean":
                mp = self.mean_extract(data)
            else:
                mp = self.map_extract(data)
                try:
                    q, _ = find_MAP(fun_map, model.q_from_point(mp))
                    mp = model.point_dict(q)
                except Exception:
                    pass
        else:
            raise Exception("method must be one of map, mcmc_map, or mcmc_mean")
        # freeze the warps at the fitted parameters and leave the converted data on the device (gpmcmc.py:362-399)
        if iwgp or cwgp:
            if method != "none":
                if iwgp:
                    self.iwgp_set(np.atleast_1d(mp["iwgp"]))
                if cwgp:
                    self.cwgp_set(np.array(self._cwgp_params(np.atleast_1d(mp.get("cwgp_pos", [])),
                                                              np.atleast_1d(mp.get("cwgp", [])))))
            xin, yin = self._converted(x, y)
            gp.update_data(X=xin, y=yin)
            if inducing_raw is not None:  # a sparse fit: the raw inducing points through the fitted warps, on the device too
                zin = np.ascontiguousarray(np.column_stack([self.xconrevs[i].con(inducing_raw[:, i]) for i in range(self.nx)]))
                gp.set_inducing(zin)
                data["inducing"], data["inducing_raw"] = zin, inducing_raw.copy()
        return model, gp, mp, data

    def __sample(self, model, gp, x, y, xin, yin, iwgp=False, cwgp=False, draws=1000, tune=1000, chains=None,
                 cores=None, target_accept=0.8, random_seed=None, max_treedepth=10, progressbar=False, devices=None,
                 chains_per_device=None, batched=None, **_):
        """pm.sample(**kwargs) of gpmcmc.py:351: independent NUTS chains, one device handle per concurrent chain
        (one chain per GPU when several are visible: SURVEY.md section 8e).  Chains that share a GPU run on up to
        ``chains_per_device`` handles at once (default: up to 3 while their buffers fit): below N ~ 10^4 one evaluation
        is bound by the serial panel chain and leaves most of the chip idle -- three concurrent handles on one MI355X
        deliver 2.7x the evaluations/s at N=1024, 2.2x at N=4096, 1.25x at N=8192 (tools/archive/dev_concurrent.py), and every
        chain's draws are the same as when it runs alone (evaluations are deterministic per handle).
        Round 4: without warp parameters (and unless ``chains_per_device`` / ``batched=False`` ask for lanes) the chains of a
        device share ONE handle and meet in one batched evaluation per leapfrog step (blockIdx.z = chain): N=4096 LML
        1440 evaluations/s with eight chains against 1000 with three handles, N=2048 LML + gradient 2800 against 1860."""
        import torch

        chains = max(2, min(4, os.cpu_count() or 2)) if chains is None else int(chains)
        ndev = torch.cuda.device_count()
        devices = list(devices) if devices is not None else [(self.device + i) % max(ndev, 1) for i in range(chains)]
        seeds = np.random.SeedSequence(random_seed).spawn(chains)
        results = [None] * chains
        errors = []

        by_dev = {}
        for c in range(chains):
            by_dev.setdefault(devices[c % len(devices)], []).append(c)

        def lanes_for(dev, nchain):
            """How many handles work side by side on this device."""
            if chains_per_device is not None:
                return max(1, min(int(chains_per_device), nchain))
            npad = (len(yin) + 127) // 128 * 128
            # one gradient-capable handle: K, U = L^-T and K^-1; the leaf inverses (128 x 128 per tile column); X, the
            # data-side gradient partials (up to 8 column splits of n x d) and the small vectors
            need = (3 * (npad + 128) * (npad + 16) + (npad // 128) * 128 * 128 + 10 * npad * xin.shape[1] + 8 * npad) * 8
            free, _total = torch.cuda.mem_get_info(dev)
            base = 1 if dev == self.device else 0  # the first lane's handle exists already -- on self.device only
            return max(1, min(3, nchain, base + int(0.8 * free // need)))

        # a lane = one host thread + one handle; the chains of a device are dealt round-robin to its lanes
        def run_lane(dev, cs, h_existing, shared, nlanes=1):
            try:
                h = h_existing or MiGP(xin, yin, self.kernel, device=dev)
                # Lanes that SHARE a GPU give up the look-ahead stream up to 64 tile columns (two streams start at 4 since
                # round 6): the other lanes fill the idle CUs anyway and a hand-off between two streams costs ~5-10 us
                # (three handles, LML + gradient: N = 6144 176 -> 202 evaluations/s, N = 8192 94 -> 97; from 72 tile columns on
                # there is nothing in it).  The super-panel width is pinned to the one the two-stream driver would pick, so
                # the arithmetic -- and every draw -- is bit-identical to the default schedule.
                ntc = (len(yin) + 127) // 128
                pinned = shared and 4 <= ntc <= 64
                before26 = None
                if shared and not pinned and nlanes > MAX_POLLING_HANDLES:
                    # Two-stream lanes enqueue in-kernel polls ahead of the writes they wait for (include/mi_gp.h, option 26):
                    # tested with six handles evaluating at once per device.  Beyond that the lanes use event edges from the
                    # start (same bits) instead of finding out through a poll limit.
                    before26 = h.get_option(26, 2)
                    h.set_option(26, 0)
                if pinned:
                    # the caller's own handle gets its previous settings back afterwards (library defaults: look-ahead by
                    # size = 1, super-panel width by size = 0)
                    before = (h.get_option(2, 0), h.get_option(0, 1))
                    if 20 <= ntc <= 60:  # (gp_sched.hip NARROW_PANELS_MAX_TILES: above it both schedules use 8-tile super-panels;
                        h.set_option(2, 4)  # up to 31 tile columns the whole problem runs in column mode: no panels at all)
                    h.set_option(0, 0)
                try:
                    lik = self._warp_likelihood(h, x, y, xin, iwgp, cwgp) if (iwgp or cwgp) else None
                    f = lambda q: model.logp_dlogp(q, h.lml_grad, likelihood=lik)  # noqa: E731
                    for c in cs:
                        results[c] = sample_chain(f, model.initial_point(), draws=draws, tune=tune,
                                                  target_accept=target_accept, max_treedepth=max_treedepth, seed=seeds[c],
                                                  progressbar=progressbar and c == 0)
                finally:
                    if h_existing is None:
                        h.close()
                    else:
                        if pinned:
                            h.set_option(2, before[0])
                            h.set_option(0, before[1])
                        if before26 is not None:
                            h.set_option(26, before26)
            except Exception as e:  # noqa: BLE001 - reported by the caller's thread
                errors.append(e)

        # Batched mode (round 4): the chains of a device share ONE handle and meet once per leapfrog step in ONE batched
        # device call (batching.BatchedEvaluator -> mi_gp_lml_grad_batch, blockIdx.z = chain) -- without warp parameters
        # only: warped chains evaluate different DATA, not just different theta.  Same draws as the unbatched schedule.
        def run_batched(dev, cs, h_existing):
            try:
                from .batching import BatchedEvaluator

                h = h_existing or MiGP(xin, yin, self.kernel, device=dev)
                ev = BatchedEvaluator(h.lml_grad_batch, len(cs))

                def one(c):
                    try:
                        f = lambda q: model.logp_dlogp(q, ev.evaluate)  # noqa: E731
                        results[c] = sample_chain(f, model.initial_point(), draws=draws, tune=tune, target_accept=target_accept,
                                                  max_treedepth=max_treedepth, seed=seeds[c], progressbar=progressbar and c == 0)
                    except Exception as e:  # noqa: BLE001
                        errors.append(e)
                    finally:
                        ev.leave()

                ts = [threading.Thread(target=one, args=(c,)) for c in cs]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                if h_existing is None:
                    h.close()
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def batch_fits(dev, nchain):
            """One handle's batch buffers: nchain copies of K, U and K^-1 (the lanes path sizes itself the same way)."""
            npad = (len(yin) + 127) // 128 * 128
            need = nchain * (3 * (npad + 128) * (npad + 16) + (npad // 128) * 128 * 128) * 8
            free, _total = torch.cuda.mem_get_info(dev)
            return need <= 0.8 * free

        threads = []
        use_batch = (batched if batched is not None else True) and not (iwgp or cwgp)
        for dev, cs in by_dev.items():
            if use_batch and len(cs) > 1 and chains_per_device is None and batch_fits(dev, len(cs)):
                threads.append(threading.Thread(target=run_batched, args=(dev, cs, gp if dev == self.device else None)))
                continue
            k = lanes_for(dev, len(cs))
            for lane in range(k):
                mine = cs[lane::k]
                if mine:
                    threads.append(threading.Thread(target=run_lane, args=(dev, mine, gp if (dev == self.device and lane == 0) else None, k > 1, k)))
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise RuntimeError(f"a NUTS chain failed: {errors[0]}") from errors[0]
        if any(r is None for r in results):
            raise RuntimeError("a NUTS chain failed")
        posterior = {}
        qs = np.stack([r["q"] for r in results])  # [chain, draw, nq]
        for c in range(chains):
            for k in range(qs.shape[1]):
                pt = model.point_dict(qs[c, k])
                for name, val in pt.items():
                    if name not in posterior:
                        posterior[name] = np.empty((chains, qs.shape[1]) + np.shape(val))
                    posterior[name][c, k] = val
        stats = {"lp": np.stack([r["lp"] for r in results]),
                 "step_size": np.array([r["step_size"] for r in results]),
                 "n_leapfrog": np.array([r["n_leapfrog"] for r in results]),
                 "diverging": np.array([r["diverging"] for r in results])}
        return Trace(posterior, stats)

    def mean_extract(self, data):
        """Posterior means over chains and draws (gpmcmc.py:404-412)."""
        return {k: np.array(v.mean(axis=(0, 1))) for k, v in data.posterior.items()}

    def map_extract(self, data):
        """Draw with the largest log-posterior (gpmcmc.py:415-430)."""
        lp = data.sample_stats["lp"].reshape(-1)
        k = int(np.argmax(lp))
        if self.verbose:
            print(f"Max log posterior: {lp[k]}")
        mp = {}
        for name, v in data.posterior.items():
            flat = v.reshape((-1,) + v.shape[2:])
            mp[name] = np.array(flat[k])
        return mp

    # ------------------------------------------------------------------ predict
    def _theta_from_hypers(self, hyps, jitter):
        model = self.m
        vals = {"l": np.atleast_1d(hyps["l"]), "kv": np.atleast_1d(hyps["kv"])}
        if self.noise:
            vals["gv"] = np.atleast_1d(hyps["gv"])
        if "alpha" in hyps:
            vals["alpha"] = np.atleast_1d(hyps["alpha"])
        th = model.theta(vals)
        th[-1] = jitter
        return th

    def predict(self, x, return_var=False, convert=True, revert=True, normvar=False, jitter=1e-6, EI=False,
                EIopt=None, deg=8):
        """gpmcmc.py:522-542.  Under ``outputs="all"`` the mean and the variance are (M, ny): column i is reverted through its
        own ``yconrevs[i]`` by the same Gauss-Hermite reversion and the mean function's column i is added to it.  Under
        ``output_cov="integrated"`` column i starts from its own converted variance, otherwise every column from the shared one."""
        if EI:
            self._no_all_outputs("predict(EI=True)")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before predicting")
        if convert:
            xarg = np.zeros_like(x)
            for i in range(self.nx):
                xarg[:, i] = self.xconrevs[i].con(x[:, i])
        else:
            xarg = copy.deepcopy(x)
            x = copy.deepcopy(x)
            for i in range(self.nx):
                x[:, i] = self.xconrevs[i].rev(x[:, i])
        if self.verbose:
            print("Predicting...")
        t0 = stopwatch()
        mu, var = self.gp.predict(self._theta_from_hypers(self.hypers, jitter), xarg, pred_noise=True)
        if self.verbose:
            print(f"Time taken: {stopwatch() - t0:0.2f} s")
        if getattr(self, "outputs", "first") == "all":
            cols = [(mu[:, i : i + 1], var[:, i : i + 1] if var.ndim == 2 else var.reshape((-1, 1))) for i in range(self.ny)]
            if revert:
                cols = [self.__gh_stats(x, yi, yvi, normvar, deg, col=i) for i, (yi, yvi) in enumerate(cols)]
            y, yv = np.hstack([c[0] for c in cols]), np.hstack([c[1] for c in cols])
            return (y, yv) if return_var else y
        y, yv = mu.reshape((-1, 1)), var.reshape((-1, 1))
        if revert:
            y, yv = self.__gh_stats(x, y, yv, normvar, deg, EI=EI, EIopt=EIopt)
        return (y, yv) if return_var else y

    def _converted_x(self, x, convert):
        """(converted inputs for the GP, inputs in the original space) of prediction points x, as predict() forms them."""
        if convert:
            xarg = np.zeros_like(x)
            for i in range(self.nx):
                xarg[:, i] = self.xconrevs[i].con(x[:, i])
        else:
            xarg = copy.deepcopy(x)
            x = copy.deepcopy(x)
            for i in range(self.nx):
                x[:, i] = self.xconrevs[i].rev(x[:, i])
        return xarg, x

    def predict_joint(self, x, convert=True, pred_noise=True, jitter=1e-6):
        """Posterior mean (M, 1) and JOINT covariance (M, M) at x in the converted output space -- PyMC's
        gp.predict(x, point, diag=False, pred_noise=...); the diagonal agrees with predict(revert=False, return_var=True).
        A covariance has no image under a nonlinear output reversion, so there is no ``revert`` here (sample_posterior
        reverts draws instead)."""
        self._no_trend("predict_joint")
        self._no_sparse("predict_joint")
        self._no_all_outputs("predict_joint")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before predicting")
        xarg, _ = self._converted_x(np.asarray(x, dtype=np.float64), convert)
        mu, cov = self.gp.predict_cov(self._theta_from_hypers(self.hypers, jitter), xarg, pred_noise=pred_noise)
        return mu.reshape((-1, 1)), cov

    def log_predictive(self, x, y, jitter=1e-6):
        """Held-out JOINT log predictive density of up to 128 points (x [M, nx], y [M] or [M, 1]) in the original output
        units, at ``self.hypers``: log N(y_con | conditional of the fitted GP at x_con, with observation noise) plus the
        Jacobian sum log|d y_con / d y| when the output conversion has ``der`` (MiGP.logpdf; nothing is appended)."""
        self._no_trend("log_predictive")
        self._no_sparse("log_predictive")
        self._no_all_outputs("log_predictive")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before predicting")
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if x.ndim != 2 or x.shape[1] != self.nx or x.shape[0] != y.shape[0]:
            raise ValueError("x must be (M, nx) and y hold M values")
        if not 1 <= len(y) <= 128:
            raise ValueError("log_predictive takes 1 to 128 points (the joint density of one trial block)")
        xarg, xorig = self._converted_x(x, True)
        yres = y - self._mean_at(xorig)
        logp, _, _ = self.gp.logpdf(self._theta_from_hypers(self.hypers, jitter), xarg, self.yconrevs[0].con(yres), grad=False)
        if hasattr(self.yconrevs[0], "der"):
            logp += float(np.sum(np.log(np.abs(self.yconrevs[0].der(yres)))))
        return logp

    def sample_posterior(self, x, nsamples=1, seed=None, convert=True, revert=True, pred_noise=False, jitter=1e-6):
        """``nsamples`` joint posterior draws at the M points x, an (nsamples, M) array: sample paths of the latent function
        by default (pred_noise=False), of noisy observations with pred_noise=True.  revert=True maps each draw through the
        output reversion point by point and adds the mean function -- exact for sample paths, no quadrature.  ``seed``: see
        MiGP.sample_posterior (None: fresh draws on every call)."""
        self._no_trend("sample_posterior")
        self._no_sparse("sample_posterior")
        self._no_all_outputs("sample_posterior")
        if self._ensure_gp() is None or self.hypers is None:
            raise Exception("Error: fit the GP before predicting")
        xarg, xorig = self._converted_x(np.asarray(x, dtype=np.float64), convert)
        draws = self.gp.sample_posterior(self._theta_from_hypers(self.hypers, jitter), xarg, nsamples, seed=seed,
                                         pred_noise=pred_noise)
        if revert:
            means = self._mean_at(xorig)
            draws = self.yconrevs[0].rev(draws) + (np.reshape(means, (1, -1)) if np.ndim(means) else means)
        return draws

    @staticmethod
    def _draw_indices(total, ndraws):
        """Indices of ``ndraws`` evenly spaced draws among ``total`` (all of them for None or ndraws >= total)."""
        if ndraws is None or int(ndraws) >= total:
            return np.arange(total)
        if int(ndraws) < 1:
            raise ValueError("ndraws must be >= 1 (or None for all draws)")
        return (np.arange(int(ndraws)) * total) // int(ndraws)

    def _posterior_thetas(self, data, ndraws, jitter):
        """C-ABI theta of every selected draw of an MCMC trace: draws flattened chain-major, then evenly spaced."""
        post = data.posterior
        warps = sorted(name for name in post if "wgp" in name)
        if warps:
            raise ValueError(f"predict_posterior: the trace carries warp parameters {warps}; per-draw warps change the converted "
                             "data themselves and are not supported (predict with the extracted hypers instead)")
        for name in ("l", "kv") + (("gv",) if self.noise else ()):
            if name not in post:
                raise ValueError(f"predict_posterior: the trace has no '{name}' draws (fit(method='mcmc_*', return_data=True))")
        flat = {name: np.asarray(v).reshape((-1,) + np.shape(v)[2:]) for name, v in post.items()}
        total = len(flat["l"])
        idx = self._draw_indices(total, ndraws)
        thetas = np.array([self._theta_from_hypers({name: v[i] for name, v in flat.items()}, jitter) for i in idx])
        return thetas, idx

    def predict_posterior(self, x, data, ndraws=100, return_var=False, convert=True, revert=True, normvar=False, jitter=1e-6,
                          EI=False, EIopt=None, deg=8):
        """Posterior predictive over the MCMC hyper-parameter draws of ``data`` (the trace of fit(method='mcmc_*',
        return_data=True)): the equal-weight mixture of the conditionals at ``ndraws`` evenly spaced draws (chain-major;
        None: all), computed in lockstep batches on the device (MiGP.predict_batch).  The arguments are predict()'s.
        revert=False: the mixture's mean / variance in converted space.  revert=True: each draw's conditional is reverted by
        Gauss-Hermite quadrature as predict() does (draw by draw); mean = average of the draws' reverted means (EI=True: their EI),
        variance = average of the draws' reverted second moments - mean^2 (summed as the law of total variance: average
        variance + variance of the means).  Draws whose covariance is not positive definite are dropped and counted in
        ``self.posterior_info``; none left raises FloatingPointError.  One distinct draw reproduces predict() at its hypers: the
        unreverted moments bit for bit where predict() takes the triangular solve (not U = L^-T, MiGP.predict), the reverted
        ones to rounding."""
        self._no_trend("predict_posterior")
        self._no_sparse("predict_posterior")
        self._no_all_outputs("predict_posterior")
        if self._ensure_gp() is None or self.m is None:
            raise Exception("Error: fit the GP before predicting")
        thetas, idx = self._posterior_thetas(data, ndraws, jitter)
        if convert:
            xarg = np.zeros_like(x)
            for i in range(self.nx):
                xarg[:, i] = self.xconrevs[i].con(x[:, i])
        else:
            xarg = copy.deepcopy(x)
            x = copy.deepcopy(x)
            for i in range(self.nx):
                x[:, i] = self.xconrevs[i].rev(x[:, i])
        if self.verbose:
            print(f"Predicting over {len(thetas)} posterior draws...")
        t0 = stopwatch()
        mu, var, mix_mu, mix_var = self.gp.predict_batch(thetas, xarg, pred_noise=True, mixture=True)
        ok = np.asarray(self.gp.batch_info) == 0
        self.posterior_info = {"draws": idx, "used": int(ok.sum()), "failed": int((~ok).sum()),
                               "failed_draws": idx[~ok], "info": np.asarray(self.gp.batch_info).copy()}
        if self.verbose:
            print(f"Time taken: {stopwatch() - t0:0.2f} s")
            if not ok.all():
                print(f"{int((~ok).sum())} of {len(ok)} draws dropped: covariance not positive definite")
        if not ok.any():
            raise FloatingPointError("predict_posterior: no draw has a positive-definite covariance")
        if not revert:
            y, yv = mix_mu.reshape((-1, 1)), mix_var.reshape((-1, 1))
            return (y, yv) if return_var else y
        # the quadrature draw by draw, vectorised over the points as in predict(): the rounding of a BLAS product can depend on its
        # row count, and the variance's cancellation (second moment - mean^2) would turn that into more than rounding
        means = self._mean_at(x)
        gh = [self._gh_moments(means, mu[p].reshape((-1, 1)), var[p].reshape((-1, 1)), deg, EI=EI, EIopt=EIopt)
              for p in np.flatnonzero(ok)]
        ym, ym2 = np.array([a for a, _ in gh]), np.array([b for _, b in gh])
        # averages relative to the first draw's values (the device mixture's form): one distinct draw returns predict()'s numbers
        yv = ym2 - ym ** 2
        yout = ym[0] + (ym - ym[0]).mean(axis=0)
        yvout = yv[0] + (yv - yv[0]).mean(axis=0) + ((ym - yout) ** 2).mean(axis=0)
        yout, yvout = yout.reshape((-1, 1)), yvout.reshape((-1, 1))
        if normvar:
            yvout = yvout / np.power(yout, 2)
        return (yout, yvout) if return_var else yout

    def __gh_stats(self, x, y, yv, normvar=True, deg=8, EI=False, EIopt=None, col=0):
        """Gauss-Hermite mean / variance (or EI) of the reverted variable (gpmcmc.py:545-569),
        vectorised over the prediction points instead of the reference's per-point Python loop."""
        ymean, ym2 = self._gh_moments(self._mean_at(x, col), y, yv, deg, EI, EIopt, col=col)
        yout = ymean.reshape((-1, 1))
        yvout = (ym2 - ymean ** 2).reshape((-1, 1))
        if normvar:
            yvout = yvout / np.power(yout, 2)
        return yout, yvout

    def _mean_at(self, x, col=0):
        """Output ``col`` of the mean function at every row of x (0.0 for the zero mean)."""
        return np.array([self.mean(x[i, :])[col] for i in range(len(x))]) if self.mean != self.zero_mean else 0.0

    def _gh_moments(self, means, y, yv, deg=8, EI=False, EIopt=None, col=0):
        """First moment (or EI) and second moment of the reverted variable per row, by Gauss-Hermite quadrature of the
        converted-space normal N(y, yv); ``means``: the mean function per row (or 0.0)."""
        xi, wi = np.polynomial.hermite.hermgauss(deg)
        yi = np.sqrt(2.0 * yv) * xi[None, :] + y  # [M, deg]
        yir = self.yconrevs[col].rev(yi) + np.reshape(means, (-1, 1) if np.ndim(means) else ())
        if EI:
            ydiff = (yir - self.yopt) if EIopt == "max" else (self.yopt - yir)
            first = np.where(ydiff > 0.0, ydiff, 0.0)
        else:
            first = yir
        ymean = (first @ wi) / np.sqrt(np.pi)
        ym2 = ((yir ** 2) @ wi) / np.sqrt(np.pi)
        return ymean, ym2

    def __del__(self):
        try:
            self.__release()
        except Exception:
            pass
