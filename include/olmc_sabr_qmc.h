/*
 * olmc_sabr_qmc.h -- the SABR entry points of olmc_sabr.h on scrambled-Sobol paths (same library, same contexts, same model, payoffs
 * and cells; only the normals differ).
 *
 * Conventions are olmc.h's: 0 on success, the message of the calling thread's last failure in olmc_last_error(), no CPU
 * fallback, results in olmc_stats (.sum and .sumsq undiscounted: shards of one sequence add up through olmc_combine_stats).
 * Every refusal below is OLMC_ERR_ARG and is made before any device work.
 *
 * The model.  Point k of scipy.stats.qmc.Sobol(d = 2 n_steps, scramble=True, seed) drives ONE path of n = n_steps steps (sv / shift /
 * bits as olmc_heston_qmc, dims = 2 n_steps, so n_steps <= 10600):
 *     z_i = Phi^-1(clip(u_i, 1e-10, 1 - 1e-10)),  i = 0 .. 2 n - 1          (the inverse normal of olmc_european_qmc)
 *     OLMC_QMC_SEQUENTIAL   step t takes Z1 = z_{2t} and Z2' = z_{2t+1}
 *     OLMC_QMC_BRIDGE       two breadth-first Brownian bridges of olmc.h ("quasi-Monte Carlo Heston"): W1 on the even dimensions
 *                           (node k takes z_{2k}), W2 on the odd ones (node k takes z_{2k+1}); step t takes
 *                           Z1 = W1_{t+1} - W1_t and Z2' = W2_{t+1} - W2_t; n <= OLMC_QMC_BRIDGE_MAX_STEPS
 * and the recursion is olmc_sabr.h's, unchanged, on these TRUE fp64 normals (no sqrt(2 ln 2) scale): with dt = T / n,
 * W = rho Z1 + sqrt(1 - rho^2) Z2', sigma_0 = alpha and F_0 = F,
 *     beta = 1:   ln(F_{t+1} / F) = ln(F_t / F) - sigma_t^2 dt / 2 + sigma_t sqrt(dt) Z1
 *     beta < 1:   G = F_t + sigma_t F_t^beta sqrt(dt) Z1;  F_{t+1} = G if F_t > 0 and G > 0, otherwise 0 (absorbed)
 *     sigma_{t+1} = sigma_t exp(nu sqrt(dt) W - nu^2 dt / 2)                (the exact lognormal step)
 * The F step uses sigma_t from the start of the step, and the kernel is picked by beta == 1.0, 0.5 or 0.0 compared as doubles,
 * otherwise the general one, as in olmc_sabr.h.  The mirror leg is the point -z, which gives -W on both bridges; it walks its own
 * sigma path.  A NaN input gives NaN results.  out->std_error is the naive per-path standard error of the payoffs: for Sobol points
 * it is NOT a confidence interval (it overstates the error).  With profiling on, one call counts as one launch.
 *
 * Refused, by every entry point, in this order: what its olmc_sabr.h counterpart refuses of pointers, the model and F ("null
 * pointer", "alpha must be positive", "beta must be in [0, 1]", "rho must be in [-1, 1]", "nu must be non-negative", "F must be
 * positive"); for olsq_price "bad payoff" and then "Barrier must be positive"; then what olmc_heston_qmc refuses of the points: a bad
 * construction, the bridge beyond OLMC_QMC_BRIDGE_MAX_STEPS dates, n_steps outside [1, 10600], a null sv or shift, bits != 30,
 * n_points < 1, point_offset < 0, points beyond 2^30; then, for olsq_surface_prices, the cell refusals of olmc_heston_surface.
 *
 * Resources of the kernels (gfx950, tools/kernel_meta.sh; the per-instantiation figures stand beside each kernel in
 * optionslab_amd/csrc/olmc_sabr_qmc_kernels.h): no instantiation uses scratch or spills; LDS is 64 B (price), none (paths) and 3.2 KiB
 * (surface); VGPRs 60-96 (sequential price), 73-131 (bridge price: only the plain geometric Asian at beta = 0.5 is past 128), 64-95
 * (paths), 62-111 (surface).
 */
#ifndef OLMC_SABR_QMC_H
#define OLMC_SABR_QMC_H

#include "olmc_sabr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* olsb_price on points [point_offset, point_offset + n_points): one payoff (codes 0-8 with olsb_price's meaning: the dates, the
 * date-0 barrier decision, an absorbed path is 0 at every later date) in ONE launch that stores no path.  antithetic != 0 also walks
 * the mirrored point: 2 n_points samples. */
int olsq_price(double F, double K, double T, double r, int is_call, const olsb_model* m, int payoff, double barrier,
               int construction, int64_t point_offset, int64_t n_points, int32_t n_steps,
               const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out);

/* The matrices F_t and sigma_t of points [0, n_points), t = 0 .. n_steps, in olsb_paths' layouts; date 0 is (F, alpha) as given.
 * mirror != 0 gives the mirrored leg of olsq_price's antithetic pairs.  Matrices beyond 64 GB are refused. */
int olsq_paths(double F, double T, const olsb_model* m, int construction, int64_t n_points, int32_t n_steps,
               const uint32_t* sv, const uint32_t* shift, int32_t bits, int mirror, int path_major,
               double* forward_host, double* vol_host);

/* olsb_surface_prices on these points: cell i is the payoff of column steps[i] of olsq_paths' forward matrix, discounted over
 * steps[i] dt.  The points are those of the full 2 n_steps dimensions: a cell at an intermediate date reads the full-horizon
 * construction, as olmc_heston_qmc_surface does.  Cells, order, read-out and their refusals are olmc_heston_surface's. */
int olsq_surface_prices(double F, double T, double r, int is_call, const olsb_model* m, const double* strikes,
                        const int32_t* steps, int32_t k, int construction, int64_t point_offset, int64_t n_points,
                        int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic,
                        olmc_stats* out /* [k] */);

#ifdef __cplusplus
}
#endif

#endif /* OLMC_SABR_QMC_H */
