"""The RF-ladder bookkeeping `va_ode.Annealer` and `va_nnet.Annealer` share.

Upstream wrote it twice (va_ode.py:459-528, 707-789; va_nnet.py:267-286, 452-523); here it exists once.
The path vector of either class is [X | p_est]: `_NX` state entries (N_model*D; M*NDnet), then the
estimated parameters, which sit at the positions `_estpos` of the stored parameter block (all NP
parameters; one block per time point when they are time-dependent).  A subclass's anneal_init checks
its own arguments, then calls _ladder_init and _alloc_tables and creates `_pb`, the device handle
(_capi.Problem / _capi.NnetProblem: action_grad, minimize_lbfgs, anneal)."""
from __future__ import print_function

import time

import numpy as np

from ._hipmin import HIPmin, alpha_pow


class LadderAnnealer(HIPmin):
    _print_exit_message = False                       # SciPy's res.message after a host-side rung

    def __init__(self):
        self.taped = False                            # reference attribute (va_ode.py:53); unused here
        self.annealing_initialized = False
        self._pb = None

    def close(self):
        if self._pb is not None:
            self._pb.close()
            self._pb = None

    # ------------------------------------------------------------------ set up by anneal_init
    def _ladder_init(self, alpha, beta_array):
        """va_ode.py:643-650, va_nnet.py:395-402; RF0 is set"""
        self.alpha = alpha
        self.beta_array = beta_array
        self.Nbeta = len(beta_array)
        self._rf_scale = alpha_pow(alpha, beta_array)
        self._set_rung(0)

    def _set_rung(self, k):
        self.betaidx = k
        self.beta = self.beta_array[k]
        self.RF = self.RF0 * alpha_pow(self.alpha, self.beta)

    def _alloc_tables(self, Xf, Pf):
        """result tables [B][Nbeta]...; rung 0 of minpaths holds the initial guess (va_ode.py:666-693).
        Xf (B, _NX) states, Pf (B, stored parameter block)."""
        self._NX = Xf.shape[1]
        shape = (self.B, self.Nbeta)
        self._mp = np.zeros(shape + (self._NX + Pf.shape[1],), dtype=np.float64)
        self._mp[:, 0, :self._NX] = Xf
        self._mp[:, 0, self._NX:] = Pf
        self._A = np.zeros(shape); self._me = np.zeros(shape); self._fe = np.zeros(shape)
        self._flags = np.zeros(shape, dtype=np.int8)
        self._nit = np.zeros(shape, dtype=np.int32)
        self._nfev = np.zeros(shape, dtype=np.int64)
        self._Pfull = np.array(Pf, dtype=np.float64)

    # views with the reference's shapes
    def _view(self, a):
        return a if self._batched else a[0]

    minpaths = property(lambda self: self._view(self._mp))
    A_array = property(lambda self: self._view(self._A))
    me_array = property(lambda self: self._view(self._me))
    fe_array = property(lambda self: self._view(self._fe))
    exitflags = property(lambda self: self._view(self._flags))
    nit_array = property(lambda self: self._view(self._nit))
    nfev_array = property(lambda self: self._view(self._nfev))

    def _rf_print(self):
        return float(np.ravel(self.RF)[0])

    # ------------------------------------------------------------------ the ladder
    def _xp0(self, k):
        """start point of ladder step k: previous minimiser, estimated parameters only
        (va_ode.py:715-732, va_nnet.py:460-473)"""
        src = self._mp[:, k - 1 if k > 0 else 0]
        return np.concatenate([src[:, :self._NX], src[:, self._NX:][:, self._estpos]], axis=1)

    def _write_back_P(self):
        """estimated values into the caller's P array (va_ode.py:750-769, va_nnet.py:493-499), whatever
        its shape: (NP,), (N_model, NP), or either with a leading seed axis"""
        npw = self._Pfull.shape[1]
        where = (np.arange(self.B)[:, None] * npw + np.asarray(self._estpos, dtype=np.intp)).ravel()
        self.P.flat[where] = self._Pfull[:, self._estpos].ravel()

    def _store(self, k, x, A, me, fe, flag, nit, nfev):
        NX = self._NX
        self._Pfull[:, self._estpos] = x[:, NX:]
        self._write_back_P()
        self._A[:, k] = A; self._me[:, k] = me; self._fe[:, k] = fe      # va_ode.py:773-775
        self._mp[:, k, :NX] = x[:, :NX]; self._mp[:, k, NX:] = self._Pfull  # :776
        self._flags[:, k] = flag; self._nit[:, k] = nit; self._nfev[:, k] = nfev

    def anneal_step(self):
        """One ladder step for every seed (va_ode.py:707-789, va_nnet.py:452-523)."""
        k = self.betaidx
        XP0 = self._xp0(k)
        rf = float(self._rf_scale[k])
        t0 = time.time()
        msg = None
        if self._device_minimiser:
            r = self._pb.minimize_lbfgs(XP0, rf, self.opt_args)
            x, A, me, fe, flag, nit, nfev = r["x"], r["A"], r["me"], r["fe"], r["status"], r["nit"], r["nfev"]
        else:
            # bounds / NCG / TNC: SciPy on the host exactly as _autodiffmin.py:72-146 calls it
            res = self._scipy_minimize({'L-BFGS-B': 'L-BFGS-B', 'NCG': 'CG', 'TNC': 'TNC'}[self.method], XP0[0], rf)
            x = res.x[None, :]
            _, me, fe, _ = self._pb.action_grad(x, rf, want_grad=False)
            A, flag, nit, nfev = np.array([res.fun]), np.array([res.status]), np.array([res.nit]), np.array([res.nfev])
            if self._print_exit_message:
                msg = res.message
        self._store(k, x, A, me, fe, flag, nit, nfev)
        if self.verbose:
            print("Optimization complete!")
            print("Time = {0} s".format(time.time() - t0))
            print("Exit flag = {0}".format(flag[0] if self.B == 1 else flag))
            if msg is not None:
                print("Exit message: {0}".format(msg))
            print("Iterations = {0}".format(nit[0] if self.B == 1 else nit))
            print("Obj. function value = {0}\n".format(A[0] if self.B == 1 else A))
        if self.betaidx < len(self.beta_array) - 1:                   # va_ode.py:779-782
            self._set_rung(self.betaidx + 1)
        self.taped = False

    def _fused_paths(self, k0, mp):
        """minimising paths of the rungs from k0 on, as va_anneal returned them: rows [X | p_est]"""
        NX = self._NX
        self._mp[:, k0:, :NX] = mp[:, :, :NX]
        self._mp[:, k0:, NX:] = self._Pfull[:, None, :]
        self._mp[:, k0:, [NX + j for j in self._estpos]] = mp[:, :, NX:]

    def _fused_summary(self, k0, dt):
        print("Ladder of %d steps x %d seed(s): %.3f s, %d action+gradient evaluations"
              % (self.Nbeta - k0, self.B, dt, int(self._nfev[:, k0:].sum())))

    def _anneal_fused(self):
        """Remaining ladder steps in one va_anneal call; seeds advance independently."""
        k0 = self.betaidx
        t0 = time.time()
        # the minimising path of every step (va_ode.py:776) comes back in the same call
        r = self._pb.anneal(self._xp0(k0), self._rf_scale[k0:], self.opt_args, want_paths=True)
        self._A[:, k0:] = r["A"]; self._me[:, k0:] = r["me"]; self._fe[:, k0:] = r["fe"]
        self._flags[:, k0:] = r["status"]; self._nit[:, k0:] = r["nit"]; self._nfev[:, k0:] = r["nfev"]
        self._fused_paths(k0, r["minpaths"])
        self._Pfull[:] = self._mp[:, -1, self._NX:]
        self._write_back_P()
        self._set_rung(self.Nbeta - 1)
        if self.verbose:
            self._fused_summary(k0, time.time() - t0)

    def _run_ladder(self, fused, after_step=None):
        """the body of anneal(): the whole ladder in one call when nothing has to happen between rungs
        and the minimiser is the device's, else rung by rung (va_ode.py:505-528)"""
        if fused is None:
            fused = after_step is None and self._device_minimiser
        if fused:
            if not self._device_minimiser:
                raise ValueError("fused=True needs method='L-BFGS-B' with bounds=None")
            self._anneal_fused()
            return
        for _ in self.beta_array:
            if self.verbose:
                print('------------------------------')
                print('Step %d of %d' % (self.betaidx + 1, len(self.beta_array)))
                print('beta = %d, RF = %.8e' % (self.beta, self._rf_print()))
                print('')
            self.anneal_step()
            if after_step is not None:
                after_step()

    # ------------------------------------------------------------------ S1 evaluator
    def _eval(self, XP, want_grad):
        XP = np.asarray(XP, dtype=np.float64)
        single = XP.ndim == 1
        X2 = np.tile(XP, (self.B, 1)) if single else XP
        A, me, fe, g = self._pb.action_grad(X2, self._rf_now(), want_grad=want_grad)
        if single:
            return A[0], me[0], fe[0], (g[0] if want_grad else None)
        return A, me, fe, g

    def A_gaussian(self, XP):
        return self._eval(XP, False)[0]

    A = A_gaussian

    def me_gaussian(self, XP):
        return self._eval(XP, False)[1]

    def fe_gaussian(self, XP):
        return self._eval(XP, False)[2]

    # ------------------------------------------------------------------ savers
    @staticmethod
    def _save_array(filename, arr, dtype, fmt, width):
        if filename.endswith('.npy'):
            np.save(filename, arr.astype(dtype))
        else:
            np.savetxt(filename, arr.reshape(-1, width), fmt=fmt)

    def save_action_errors(self, filename, cmpt=0, dtype=np.float64, fmt="%.8e"):
        """[beta, A, me, fe, fe/RF] per rung (va_ode.py:845-873, va_nnet.py:628-650)"""
        sav = np.zeros((self.B, self.Nbeta, 5))
        sav[:, :, 0] = self.beta_array
        sav[:, :, 1] = self._A; sav[:, :, 2] = self._me; sav[:, :, 3] = self._fe
        rf0 = float(np.ravel(self.RF0)[0])            # RF0[0, 0] for array-valued RF0 (va_ode.py:861)
        sav[:, :, 4] = self._fe / (rf0 * self._rf_scale)
        self._save_array(filename, self._view(sav), dtype, fmt, 5)

    def gen_xtrace(self):
        """kept for API compatibility (va_ode.py:894-905); nothing is taped here"""
        return np.random.rand(self._NX + len(self._estpos))
