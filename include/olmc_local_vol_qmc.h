/*
 * olmc_local_vol_qmc.h -- the Dupire local-volatility entry points of olmc_local_vol.h on scrambled-Sobol paths (same library, same
 * contexts, same table, payoffs and cells; only the normals differ).
 *
 * Conventions are olmc.h's: 0 on success, the message of the calling thread's last failure in olmc_last_error(), no CPU
 * fallback, results in olmc_stats (.sum and .sumsq undiscounted: shards of one sequence add up through olmc_combine_stats).
 * Every refusal below is OLMC_ERR_ARG and is made before any device work.
 *
 * The model.  Point k of scipy.stats.qmc.Sobol(d = n_steps, scramble=True, seed) drives ONE path of n = n_steps steps (sv / shift /
 * bits as olmc_extrema_qmc, dims = n_steps):
 *     z_t = Phi^-1(clip(u_t, 1e-10, 1 - 1e-10)),  t = 0 .. n - 1          (the inverse normal of olmc_european_qmc)
 *     OLMC_QMC_SEQUENTIAL   dW_t = z_t: dimension t drives step t; n <= 21201
 *     OLMC_QMC_BRIDGE       dW_t = W_{t+1} - W_t, W_0 = 0, W_1 .. W_n from the breadth-first Brownian bridge of olmc.h
 *                           ("quasi-Monte Carlo path payoffs": node 0 is W_n = sqrt(n) z_0, node k takes z_k);
 *                           n <= OLMC_QMC_BRIDGE_MAX_STEPS
 * and the recursion, the table and its lookup are olmc_local_vol.h's, unchanged, on these TRUE fp64 normals:
 *     x_0 = 0,  sigma_t = vol(x_t, t dt),  x_{t+1} = x_t + (r - q - sigma_t^2 / 2) dt + sigma_t sqrt(dt) dW_t,  S_t = S exp(x_t)
 * (date 0 is S itself).  The antithetic leg is the point -z: it takes -dW_t and walks its own sigma path.  A NaN in S, T, r or q
 * gives NaN results.  out->std_error is the naive per-path standard error of the payoffs: for Sobol points it is NOT a
 * confidence interval (it overstates the error).  With profiling on, one call counts as one launch.
 *
 * Refused, by every entry point: what its olmc_local_vol.h counterpart refuses of the table ("null pointer", "n_x must be in
 * [2, 256]", "n_t must be in [1, 64]", "x_hi must be > x_lo", "t_hi must be > 0", "local volatilities must be finite and > 0"),
 * then what olmc_extrema_qmc refuses of the points: a bad construction, the bridge beyond OLMC_QMC_BRIDGE_MAX_STEPS dates, a null
 * sv or shift, bits != 30, n_steps outside [1, 21201], n_points < 1, point_offset < 0, points beyond 2^30.
 */
#ifndef OLMC_LOCAL_VOL_QMC_H
#define OLMC_LOCAL_VOL_QMC_H

#include "olmc_local_vol.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ollv_price on points [point_offset, point_offset + n_points): one payoff (OLMC_BARRIER_*, OLMC_LOOKBACK_*, OLMC_PATH_ASIAN_*,
 * OLLV_EUROPEAN; dates and level decisions as there) in ONE launch that stores no path.  antithetic != 0 also walks the mirrored
 * point: 2 n_points samples.  Also refused: "bad payoff", "Barrier must be positive" (a barrier kind with barrier <= 0), a null out. */
int olvq_price(double S, double K, double T, double r, double q, int is_call,
               const ollv_surface* surf, int payoff, double barrier,
               int construction, int64_t point_offset, int64_t n_points, int32_t n_steps,
               const uint32_t* sv, const uint32_t* shift, int32_t bits,
               int antithetic, olmc_stats* out);

/* The matrix S_t of points [0, n_points) (the non-mirrored leg), t = 0 .. n_steps, in ollv_paths' layouts and with its refusal of a
 * matrix beyond 64 GB. */
int olvq_paths(double S, double T, double r, double q, const ollv_surface* surf,
               int construction, int64_t n_points, int32_t n_steps,
               const uint32_t* sv, const uint32_t* shift, int32_t bits,
               int path_major, double* out_host);

/* ollv_surface_prices on these points: cell i is the payoff of column steps[i] of olvq_paths' matrix, discounted over steps[i] dt.
 * The points are those of the full n_steps dimensions: a cell at an intermediate date reads the full-horizon construction.  Cells,
 * order, read-out and their refusals are olmc_heston_surface's. */
int olvq_surface_prices(double S, double T, double r, double q, int is_call,
                        const ollv_surface* surf, const double* strikes, const int32_t* steps, int32_t k,
                        int construction, int64_t point_offset, int64_t n_points, int32_t n_steps,
                        const uint32_t* sv, const uint32_t* shift, int32_t bits,
                        int antithetic, olmc_stats* out /* [k] */);

#ifdef __cplusplus
}
#endif

#endif /* OLMC_LOCAL_VOL_QMC_H */
