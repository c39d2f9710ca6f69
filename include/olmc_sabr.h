/*
 * olmc_sabr.h -- the SABR model on the path engine of libolmc.so (same library, same contexts as olmc.h).
 *
 * Beside src/pricing_models/sabr.py, which is Hagan's implied-volatility expansion only: Monte Carlo paths of the SABR process itself,
 * for the strikes and parameters where the expansion degrades (large nu, rho towards -1, far wings) and for the barrier, Asian and
 * lookback payoffs no expansion covers.
 *
 * Conventions are olmc.h's: 0 on success, the message of the calling thread's last failure in olmc_last_error(), no CPU fallback,
 * results in olmc_stats.  Every refusal below is OLMC_ERR_ARG and is made before any device work.
 *
 * The process is the forward itself:  dF = sigma F^beta dW1,  dsigma = nu sigma dW2,  dW1 dW2 = rho dt.  The reference's names:
 * `alpha` is sigma_0 and `nu` is the volatility of volatility.  There is no drift and no q.  Payoffs are on F_t, discounted by
 * exp(-r t), as SABRModel.price(F, K, T, r) does.
 *
 * Draws.  The Philox block is (path_lo, path_hi, b, OLMC_STREAM_SABR), key = seed, GLOBAL path index.  OLMC_STREAM_SABR = 0x53414252
 * ("SABR"): like the QE tag it is out of reach of Kou's size tags.  Block b feeds steps 2b and 2b + 1 exactly as the Heston Euler
 * stream does: step 2b takes (Z1, Z2') = (cos, sin)(x0, x1), step 2b + 1 takes (cos, sin)(x2, x3).  The normals are RAW fp32, scaled by
 * sqrt(2 ln 2) in fp64.
 *
 * Recursion.  With n = n_steps, dt = T / n, W = rho Z1 + sqrt(1 - rho^2) Z2', sigma_0 = alpha and F_0 = F, all in fp64:
 *     beta = 1:   ln F_{t+1} = ln F_t - sigma_t^2 dt / 2 + sigma_t sqrt(dt) Z1      (exact given sigma_t; one exponential at read-out)
 *     beta < 1:   G = F_t + sigma_t F_t^beta sqrt(dt) Z1
 *                 F_{t+1} = G if F_t > 0 and G > 0, otherwise 0: a path that reaches 0 stays there (absorbed)
 *                 F^beta is 1 for beta = 0, the library's square root for beta = 0.5, and exp(beta ln F) otherwise
 *     sigma_{t+1} = sigma_t exp(nu sqrt(dt) W - nu^2 dt / 2)                         (the exact lognormal step)
 * The F step uses sigma_t from the start of the step.  The mirror leg takes (-Z1, -Z2') and walks its own sigma path.  A NaN input
 * gives NaN results.  The log-Euler form ln F += -a^2 dt / 2 + a sqrt(dt) Z1 with a = sigma F^{beta - 1} is NOT used for beta < 1: it
 * overflows to NaN within 64 steps.
 *
 * The host picks the kernel by beta == 1.0, beta == 0.5 or beta == 0.0 (compared as doubles), and otherwise the general one.  The step
 * costs one fp64 exponential per step and leg for sigma, plus nothing for beta = 0, a square root for beta = 0.5, nothing more for
 * beta = 1, and a logarithm and an exponential for general beta.
 */
#ifndef OLMC_SABR_H
#define OLMC_SABR_H

#include "olmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OLMC_STREAM_SABR 0x53414252u

/* The model.  Refused, in this order: a null model ("null pointer"), "alpha must be positive" (alpha <= 0), "beta must be in [0, 1]",
 * "rho must be in [-1, 1]", "nu must be non-negative" (nu < 0); then, by every entry point, "F must be positive" (F <= 0). */
typedef struct olsb_model { double alpha, beta, rho, nu; } olsb_model;

enum { OLSB_EUROPEAN = 8 };   /* continues OLMC_BARRIER_* 0-3, OLMC_LOOKBACK_* 4-5, OLMC_PATH_ASIAN_* 6-7 */

/* One payoff on paths [path_offset, path_offset + n_local) in ONE launch that stores no path.  payoff, barrier, the dates (extrema
 * over dates 0 .. n, the Asian mean over dates 1 .. n) and the date-0 barrier decision are olmc_heston_path_payoff's, on F_t;
 * OLSB_EUROPEAN adds max(+-(F_n - K), 0).  An absorbed path is 0 at every later date: down barriers are hit, the minimum is 0, the
 * geometric mean is 0.  antithetic != 0 also walks the mirrored path: 2 n_local samples.  out->sum and out->sumsq are undiscounted;
 * shards add up (olmc_combine_stats).  Refused after the model as ollv_price refuses: "bad payoff", "Barrier must be positive", the
 * counts. */
int olsb_price(double F, double K, double T, double r, int is_call, const olsb_model* m, int payoff, double barrier,
               int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out);

/* The matrices F_t and sigma_t of paths [0, n_paths), t = 0 .. n_steps, in olmc_heston_paths' layouts (path_major != 0:
 * [n_paths][n_steps + 1], else [n_steps + 1][n_paths]) and with its refusal of matrices beyond 64 GB.  Date 0 is (F, alpha) as given.
 * mirror != 0 gives the mirrored leg of olsb_price's antithetic pairs. */
int olsb_paths(double F, double T, const olsb_model* m, int64_t n_paths, int32_t n_steps, uint64_t seed,
               int mirror, int path_major, double* forward_host, double* vol_host);

/* European options at k <= OLMC_MAX_BATCH cells (strikes[i], steps[i]) read out of ONE set of paths: cell i is the payoff of column
 * steps[i] of olsb_paths' forward matrix, discounted over steps[i] dt.  Cells, order and read-out are olmc_heston_surface's. */
int olsb_surface_prices(double F, double T, double r, int is_call, const olsb_model* m, const double* strikes,
                        const int32_t* steps, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps,
                        uint64_t seed, int antithetic, olmc_stats* out /* [k] */);

#ifdef __cplusplus
}
#endif

#endif /* OLMC_SABR_H */
