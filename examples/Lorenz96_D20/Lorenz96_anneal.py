"""State and parameter estimation in Lorenz 96 by variational annealing on MI355X.

Counterpart of the reference's examples/Lorenz96_D20/Lorenz96_anneal.py (SURVEY.md
8(a) row H): same model, hyper-parameters, call order and output files; the only
edits are the import (varanneal_amd instead of varanneal), an explicit RNG seed, and
the data file location.  Optional: --seeds B runs B random initial paths as one batch;
--predict N holds the last N observations back from the fit, integrates the model N steps on
from every rung's estimate (Annealer.predict) and prints the forecast's RMS error per rung;
--spread N holds them back as well and prints the last rung's forecast with its +- 2 sigma band
(Annealer.predict_spread) and the share of held-back observed values inside it at a few lead times;
--track N holds them back too and carries the last rung's estimate through them with an ensemble Kalman filter on the device
(Annealer.track), printing per seed the RMS error of the analysis mean on the observed and the unobserved columns beside predict()'s.
--lyapunov N prints, per seed, the leading Lyapunov exponent of the estimated model over N steps from the last rung's
estimate, the forecast horizon 1 / lambda_1 in units of dt_model, the Kaplan-Yorke dimension (Annealer.lyapunov) and the
largest conditional exponent with a gain on the measured columns (Annealer.sync_exponents).

    python examples/Lorenz96_D20/Lorenz96_anneal.py [--seeds 1] [--nbeta 101] [--disc SimpsonHermite] [--predict 40] [--spread 40] [--track 40] [--lyapunov 4000] [--shoot [--shoot-device]]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from varanneal_amd import va_ode  # noqa: E402


# Define the model (reference script, line 15-16)
def l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=1)
    ap.add_argument("--nbeta", type=int, default=101)
    ap.add_argument("--disc", default="SimpsonHermite")
    ap.add_argument("--rng", type=int, default=12345)
    ap.add_argument("--out", default=".")
    ap.add_argument("--predict", type=int, default=0, metavar="N",
                    help="hold the last N observations back and report the forecast error per rung")
    ap.add_argument("--spread", type=int, default=0, metavar="N",
                    help="hold the last N observations back and print the last rung's forecast +- 2 sigma (linearised spread "
                         "under the Laplace posterior: Annealer.predict_spread) and the share of them inside the band")
    ap.add_argument("--track", type=int, default=0, metavar="N",
                    help="hold the last N observations back and carry the last rung's estimate through them with an ensemble "
                         "Kalman filter on the device (Annealer.track): per seed the RMS error of the analysis mean against the "
                         "held-back data on the observed and on the unobserved columns, beside that of predict() over the same steps")
    ap.add_argument("--lyapunov", type=int, default=0, metavar="N",
                    help="print lambda_1, the horizon 1 / lambda_1 in steps of dt_model, the Kaplan-Yorke dimension and the largest "
                         "conditional exponent at a few gains on the measured columns, over N model steps (a multiple of 4) from the "
                         "last rung's estimate (Annealer.lyapunov, Annealer.sync_exponents)")
    ap.add_argument("--shoot-device", action="store_true",
                    help="with --shoot: run the minimiser on the device too, all seeds in one launch (Annealer.shoot(device=True))")
    ap.add_argument("--shoot", action="store_true",
                    help="refine the last rung to a model trajectory (strong-constraint fit of x(t_0) and k: Annealer.shoot) and "
                         "print k, cost, path_distance and, with --predict N, the forecast error from its end beside the one "
                         "from the annealed path's last row")
    ap.add_argument("--errorbars", action="store_true",
                    help="print the final k +- sigma per seed (Laplace approximation: Annealer.param_covariance)")
    ap.add_argument("--statebars", action="store_true",
                    help="print the RMS sigma of the observed and of the unobserved columns at the last rung, and log det H, "
                         "per seed (Laplace approximation on the device: Annealer.laplace)")
    ap.add_argument("--sample", type=int, default=0, metavar="N",
                    help="sample exp(-A) at the last rung, N states per seed (Hamiltonian Monte Carlo on the device: "
                         "Annealer.sample), and print k +- std from the chains beside the Laplace sigma, with the acceptance rate")
    args = ap.parse_args()

    D = 20
    # Measured variable indices, RM, RF0, alpha and the beta ladder (reference lines 22-30)
    Lidx = [0, 2, 4, 6, 8, 10, 14, 16]
    RM = 1.0 / (0.5 ** 2)
    RF0 = 4.0e-6
    alpha = 1.5
    beta_array = np.linspace(0, args.nbeta - 1, args.nbeta)

    # Observed data: the file the reference ships (a copy lives in tests/golden/)
    here = os.path.dirname(os.path.abspath(__file__))
    data = np.load(os.path.join(here, "..", "..", "tests", "golden",
                                "l96_D20_dt0p025_N161_sm0p5_sec1_mem1.npy"))
    times_data = data[:, 0]
    dt_data = times_data[1] - times_data[0]
    N_data = len(times_data)
    all_columns = data[:, 1:]
    data = all_columns[:, Lidx]
    held_back = None
    if len(set(n for n in (args.predict, args.spread, args.track) if n > 0)) > 1:
        ap.error("--predict, --spread and --track hold the same rows back: give them the same N")
    hold = max(args.predict, args.spread, args.track)
    if hold > 0:
        # fit what comes before the last N rows (Simpson-Hermite needs an odd number of them); the last fitted row is
        # row 0 of what the forecast is compared with
        n_fit = N_data - hold
        first = 1 if (args.disc == "SimpsonHermite" and n_fit % 2 == 0) else 0
        held_back = data[n_fit - 1:]
        held_back_all = all_columns[n_fit - 1:]
        data, times_data, N_data = data[first:n_fit], times_data[first:n_fit], n_fit - first

    # Initial path/parameter guesses (reference lines 49-68)
    dt_model = dt_data
    N_model = N_data
    rng = np.random.RandomState(args.rng)
    if args.seeds == 1:
        X0 = (20.0 * rng.rand(N_model * D) - 10.0).reshape((N_model, D))
        P0 = np.array([4.0 * rng.rand() + 6.0])
    else:
        X0 = (20.0 * rng.rand(args.seeds, N_model * D) - 10.0).reshape((args.seeds, N_model, D))
        P0 = 4.0 * rng.rand(args.seeds, 1) + 6.0
    Pidx = [0]

    anneal1 = va_ode.Annealer()
    anneal1.set_model(l96, D)
    anneal1.set_data(data, t=times_data)

    BFGS_options = {'gtol': 1.0e-8, 'ftol': 1.0e-8, 'maxfun': 1000000, 'maxiter': 1000000}
    tstart = time.time()
    anneal1.anneal(X0, P0, alpha, beta_array, RM, RF0, Lidx, Pidx, dt_model=dt_model,
                   init_to_data=True, disc=args.disc, method='L-BFGS-B',
                   opt_args=BFGS_options, adolcID=0)
    print("\nHIP annealing completed in %f s." % (time.time() - tstart))
    print("estimated forcing k (true value 8.17): %s" % np.ravel(anneal1.P))

    if args.predict > 0:
        err = anneal1.prediction_error(held_back)          # (nbeta,), or (seeds, nbeta)
        print("\nforecast of %d steps from every rung's estimate: RMS error on the measured components" % args.predict)
        for k, beta in enumerate(beta_array):
            print("beta = %3d   %s" % (beta, np.array2string(np.atleast_1d(err[..., k]), precision=4)))

    if args.spread > 0:
        # the model forecast's linearised spread: no observation noise in it, so the band is widened by the measurement
        # error (RM = 1 / sigma^2) before the held-back values are counted.  Gauss-Newton where the exact Hessian is not
        # positive definite (status != 0)
        sp = anneal1.predict_spread(args.spread, beta=-1)
        if np.any(sp["status"] != 0):
            print("\n(the exact Hessian is not positive definite at %d of %d seeds: Gauss-Newton part)"
                  % (int(np.sum(sp["status"] != 0)), sp["status"].size))
            sp = anneal1.predict_spread(args.spread, beta=-1, gauss_newton=True)
        # predict_spread's covariance is that of the action as the package normalises it; the negative log-likelihood of
        # Gaussian measurement noise is A' = c A with c = L N_data / 2 (RM = 1 / sigma^2), so variances are divided by c
        c_nll = 0.5 * len(Lidx) * N_model
        mean, std = sp["mean"].reshape(-1, args.spread + 1, D), sp["std"].reshape(-1, args.spread + 1, D) / np.sqrt(c_nll)
        leads = sorted(set(int(round(f * args.spread)) for f in (0.1, 0.25, 0.5, 0.75, 1.0)) - {0})
        print("\nforecast of the last rung, x_0 +- 2 sigma (model spread, sigma^2 / (L N / 2)), and the share of the %d held-back observed values within "
              "2 sqrt(sigma^2 + 1/RM)" % len(Lidx))
        for b in range(mean.shape[0]):
            for n in leads:
                band = 2.0 * np.sqrt(std[b, n, Lidx] ** 2 + 1.0 / RM)
                inside = np.mean(np.abs(held_back[n] - mean[b, n, Lidx]) <= band)
                print("seed %d   lead %3d steps   x_0 = %8.4f +- %.4f   inside the band: %3.0f %%"
                      % (b, n, mean[b, n, 0], 2.0 * std[b, n, 0], 100.0 * inside))

    if args.track > 0:
        # rows 1 .. N of what was held back are the observations that arrive after the window (row 0 is the last fitted
        # time); obs_var = 1 / RM.  The file holds every column, so the unobserved ones can be scored too
        tr = anneal1.track(held_back[1:], members=32, inflation=1.05)
        lost = np.isnan(tr["mean_forecast"][..., 0, 0])                    # (NaN from row 0 on: no initial ensemble)
        if np.any(lost):
            print("\n(the exact Hessian is not positive definite at %d of %d seeds: members from the Gauss-Newton part)"
                  % (int(np.sum(lost)), lost.size))
            tr = anneal1.track(held_back[1:], members=32, inflation=1.05, gauss_newton=True)
        fc = anneal1.predict(args.track, beta=-1).reshape(-1, args.track + 1, D)[:, 1:]
        mean = tr["mean"].reshape(-1, args.track, D)
        un = [i for i in range(D) if i not in Lidx]
        rms = lambda m, cols: np.sqrt(np.mean((m[:, cols] - held_back_all[1:][:, cols]) ** 2))
        print("\n%d held-back rows tracked from the last rung's estimate, 32 members (Annealer.track); RMS error against the data "
              "(noise 0.5 in it)" % args.track)
        for b in range(mean.shape[0]):
            print("seed %d   status %d   observed columns: filter %.3f  predict() %.3f   unobserved columns: filter %.3f  predict() %.3f   k = %.3f +- %.3f"
                  % (b, np.ravel(tr["status"])[b], rms(mean[b], Lidx), rms(fc[b], Lidx), rms(mean[b], un), rms(fc[b], un),
                     tr["params"].reshape(-1, args.track, 1)[b, -1, 0], tr["params_std"].reshape(-1, args.track, 1)[b, -1, 0]))

    if args.lyapunov > 0:
        # finite-time exponents of the estimated model (discrete RK4 map) from the estimate; the first tenth of the steps
        # aligns the tangents and is left out of the averages
        n_ly, gains = args.lyapunov, [0.0, 2.0, 5.0, 10.0]
        ly = anneal1.lyapunov(n_ly, transient=n_ly // 10)
        sy = anneal1.sync_exponents(n_ly, gains, transient=n_ly // 10)
        lam1, hor, ky = np.ravel(ly["exponents"][..., 0]), np.ravel(ly["horizon"]), np.ravel(ly["kaplan_yorke"])
        cond, crit = sy["exponents"][..., 0].reshape(-1, len(gains)), np.ravel(sy["critical_gain"])
        print("\nLyapunov exponents of the estimated model over %d steps from the last rung's estimate" % n_ly)
        for b in range(lam1.size):
            print("seed %d   lambda_1 = %.4f   horizon = %.1f steps of dt_model   Kaplan-Yorke dimension = %.2f" % (b, lam1[b], hor[b] / dt_model, ky[b]))
            print("         conditional lambda_1 with gain c on the %d measured columns: %s   smallest listed gain that synchronises: %s"
                  % (len(Lidx), "  ".join("c=%g: %+.3f" % (c, v) for c, v in zip(gains, cond[b])), crit[b]))

    if args.shoot:
        # the RF -> infinity limit done exactly: a model trajectory fitted to the data window from the last rung's first
        # row and parameters; its end is on a model orbit, the annealed path's last row carries that rung's model error
        sh = anneal1.shoot(beta=-1, device=args.shoot_device)
        ks, cost, dist = np.ravel(sh["params"][..., 0]), np.ravel(sh["cost"]), np.ravel(sh["path_distance"])
        ends, pars = sh["path"].reshape(-1, N_model, D)[:, -1], sh["params"].reshape(-1, 1)
        print("\nmodel trajectory fitted to the data window from the last rung (Annealer.shoot%s)" % (", minimiser on the device" if args.shoot_device else ""))
        for b in range(ks.size):
            line = "seed %d   k = %.5f   cost = %.6g   path_distance = %.4g" % (b, ks[b], cost[b], dist[b])
            if held_back is not None:
                n_fc = len(held_back) - 1
                fc = anneal1._pb.predict(ends[b], pars[b], n_fc, t0=float(anneal1.t_model[-1]))[0]
                e_sh = np.sqrt(np.mean((fc[1:, Lidx] - held_back[1:]) ** 2))
                e_an = np.ravel(anneal1.prediction_error(held_back)[..., -1])[b]
                line += "   forecast RMS error from path[-1]: %.4f, from the annealed path's last row: %.4f" % (e_sh, e_an)
            print(line)

    if args.errorbars:
        # inverse Hessian of the action as the package normalises it, at the last rung's minimisers; at large RF the
        # exact Hessian can be indefinite along the flat direction, the Gauss-Newton part never is
        try:
            cov = anneal1.param_covariance()
        except np.linalg.LinAlgError as e:
            print("\n(%s)" % e)
            cov = anneal1.param_covariance(gauss_newton=True)
        cov = cov.reshape(-1, 1, 1)
        for b, kk in enumerate(np.ravel(np.asarray(anneal1.minpaths)[..., -1, N_model * D])):
            print("seed %d   k = %.4f +- %.2e" % (b, kk, np.sqrt(cov[b, 0, 0])))

    if args.statebars:
        # marginal variances of every state from the selected inverse of the Hessian (Gauss-Newton where the exact one is
        # not positive definite: status != 0), and the Laplace log-determinant that ranks seeds by evidence
        lap = anneal1.laplace(beta=-1)
        if np.any(lap["status"] != 0):
            print("\n(the exact Hessian is not positive definite at %d of %d seeds: Gauss-Newton part)"
                  % (int(np.sum(lap["status"] != 0)), lap["status"].size))
            lap = anneal1.laplace(beta=-1, gauss_newton=True)
        var = lap["state_var"].reshape(-1, N_model, D)
        unobserved = [j for j in range(D) if j not in Lidx]
        for b in range(var.shape[0]):
            print("seed %d   RMS sigma: observed %.3e  unobserved %.3e   log det H = %.4f"
                  % (b, np.sqrt(np.mean(var[b][:, Lidx])), np.sqrt(np.mean(var[b][:, unobserved])), np.ravel(lap["logdet"])[b]))

    if args.sample > 0:
        # exp(-A) at the last rung sampled by Hamiltonian Monte Carlo on the device, the Laplace variances as masses, the
        # step sizes adapted over a warm-up as long as the run; beside it the Laplace sigma of the same normalisation
        s = anneal1.sample(args.sample, beta=-1, warmup=args.sample, seed=args.rng)
        if s["mass_note"][0]:
            print("\n(%s)" % s["mass_note"][0])
        lap = anneal1.laplace(beta=-1)
        sig = np.sqrt(np.reshape(lap["param_cov"], (-1,)))
        km, ks = np.reshape(s["mean"], (-1, N_model * D + 1))[:, -1], np.reshape(s["std"], (-1, N_model * D + 1))[:, -1]
        print("\n%d samples per chain, 10 leapfrog steps each:" % args.sample)
        for b in range(km.size):
            print("seed %d   k = %.4f +- %.2e from the chain   (Laplace sigma %.2e)   acceptance %.2f   divergent %d"
                  % (b, km[b], ks[b], sig[b], np.ravel(s["accept_rate"])[b], np.ravel(s["n_divergent"])[b]))

    anneal1.save_paths(os.path.join(args.out, "paths.npy"))
    anneal1.save_params(os.path.join(args.out, "params.npy"))
    anneal1.save_action_errors(os.path.join(args.out, "action_errors.npy"))


if __name__ == "__main__":
    main()
