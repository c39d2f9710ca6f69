/*
 * olha.h -- American options under the Heston model by least-squares Monte Carlo (Longstaff-Schwartz), regressing on the date's
 * state (S_t, v_t) (same library, same contexts as olmc.h).
 *
 * Conventions are olmc.h's: 0 on success, the message of the calling thread's last failure in olmc_last_error(), no CPU fallback,
 * results in olmc_stats.  Every refusal below is OLMC_ERR_ARG and is made before any device work.
 *
 * THE PATHS are exactly those of the path-matrix entry points for the same seed or tables: olmc_heston_paths (OLHA_EULER) and
 * olmc_heston_qe_paths (OLHA_QE) for olha_american_lsm, olmc_heston_qmc_paths and olmc_heston_qe_qmc_paths for olha_american_lsm_qmc.
 * The columns the algorithm reads are word for word the columns of those matrices, date 0 = (S, v0).  There is no antithetic mirror
 * and no path offset: the regression runs over the whole set, on one device.
 *
 * THE ALGORITHM is AmericanOption.price's (olmc_american_lsm).  With n = n_steps, dt = T / n and intrinsic(s) = max(+-(s - K), 0):
 * the cash flows start as intrinsic(S_n); for t = n - 1 .. 1 they are discounted one step (exp(-r dt)), the cash flows of the paths
 * in the money at t (intrinsic(S_t) > 0) are regressed on the date's basis, and a path in the money exercises (cash flow :=
 * intrinsic(S_t)) where intrinsic(S_t) > the fitted continuation value; then they are discounted once more.  out is the statistics
 * of these time-0 cash flows: .sum and .sumsq, .price = their mean (no outer discount), .std_error the naive per-path one, .n =
 * n_paths.  A date is fitted when its in-the-money count EXCEEDS the number of unknowns; otherwise nobody exercises at that date.
 *
 * THE BASIS.  OLHA_BASIS_SPOT_VARIANCE: all monomials x^a y^b with a + b <= poly_degree, poly_degree in [1, 3] (3, 6 or 10
 * unknowns), in the graded order 1, x, y, x^2, xy, y^2, x^3, x^2 y, x y^2, y^3 -- the order is part of the definition because of the
 * pin rule below.  OLHA_BASIS_SPOT: 1, x, .., x^d, d = poly_degree in [1, 4]: olmc_american_lsm's regression on the Heston spot
 * matrix (a valid, lower, bound: under stochastic volatility the continuation value depends on v_t too).
 * The regressors are standardised per date, x = (S_t / K - c_t) / w_t and y = (v_t - m_t) / u_t, with pairs computed on the host in
 * closed form (olha_regressor_scales reports them): (c_t, w_t) the mean and standard deviation of S_t / K over the in-the-money side
 * of the strike under a lognormal law with the model's expected average variance theta + (v0 - theta)(1 - e^(-kappa t)) / (kappa t)
 * in place of sigma^2 (olmc_american_lsm's pair with that sigma); (m_t, u_t) the conditional mean and standard deviation of the CIR
 * variance v_t given v0, u_t clamped below at 1e-6 max(m_t, theta) and at 1e-12, so that sigma_v = 0 gives a finite y (exactly 0
 * when v_t = m_t).  Any finite positive pair gives the same fit in exact arithmetic; these keep the normal equations conditioned.
 * THE SOLVE is the normal equations in fp64, eliminated in the natural (graded) order.  PIN RULE, as olmc_american_lsm's: a pivot
 * not above 1e-11 of its own diagonal moment pins that unknown to zero (its row and column become the identity) and the others are
 * still fitted.
 *
 * Equal inputs give equal bits, whatever ran before on the context or on the device.  A NaN input gives NaN results.
 *
 * Refused, in this order: a null out; "bad scheme (OLHA_EULER or OLHA_QE)"; "bad basis (OLHA_BASIS_SPOT_VARIANCE or
 * OLHA_BASIS_SPOT)"; "poly_degree must be in [1, 3] for OLHA_BASIS_SPOT_VARIANCE" / "poly_degree must be in [1, 4] for
 * OLHA_BASIS_SPOT"; what the scheme's path entry point refuses of the model ("rho must be in [-1, 1]", and for OLHA_QE "kappa /
 * theta / sigma_v must be positive for the QE scheme", "v0 must be non-negative for the QE scheme"); for olha_american_lsm_qmc,
 * whose dims is the tables' 2 n_steps, first "dims must be even: a step takes two Sobol dimensions", then
 * OLHA_QE with OLMC_QMC_BRIDGE ("the QE scheme takes OLMC_QMC_SEQUENTIAL only: ...") and what olmc_heston_qmc_paths refuses of the
 * construction, the tables (null sv or shift, bits != 30) and the points; "n_paths must be >= 1", "n_steps must be >= 1"; device
 * buffers over 64 GB -- the two matrices, the cash flows and the regression rows -- "path matrices would exceed 64 GB: lower n_paths
 * or n_steps".  With profiling on a call counts as one interval in olmc_kernel_time.
 *
 * olha_regressor_scales is host arithmetic only (no device needed): the pairs above for dates 0 .. n_steps, four arrays of n_steps +
 * 1 doubles; dates 0 and n_steps, which no regression reads, hold (1, 1) and (0, 1), as does any date whose closed form is not finite.
 * Refused: a null pointer, "n_steps must be >= 1".
 */
#ifndef OLHA_H
#define OLHA_H

#include "olmc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { OLHA_BASIS_SPOT_VARIANCE = 0, OLHA_BASIS_SPOT = 1 };
enum { OLHA_EULER = 0, OLHA_QE = 1 };

int olha_american_lsm(double S, double K, double T, double r, double q, int is_call,
                      double kappa, double theta, double sigma_v, double rho, double v0,
                      int scheme, int basis, int32_t poly_degree,
                      int64_t n_paths, int32_t n_steps, uint64_t seed, olmc_stats* out);

int olha_american_lsm_qmc(double S, double K, double T, double r, double q, int is_call,
                          double kappa, double theta, double sigma_v, double rho, double v0,
                          int scheme, int basis, int32_t poly_degree, int construction,
                          int64_t n_points, const uint32_t* sv, const uint32_t* shift, int32_t dims /* 2 n_steps */, int32_t bits,
                          olmc_stats* out);

int olha_regressor_scales(double S, double K, double T, double r, double q, int is_call,
                          double kappa, double theta, double sigma_v, double v0, int32_t n_steps,
                          double* x_centre, double* x_width, double* y_centre, double* y_width /* [n_steps + 1] each */);

#ifdef __cplusplus
}
#endif

#endif /* OLHA_H */
