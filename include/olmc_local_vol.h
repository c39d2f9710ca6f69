/*
 * olmc_local_vol.h -- Dupire local volatility on the path engine of libolmc.so (same library, same contexts as olmc.h).
 *
 * Replaces the pricing half of src/pricing_models/local_vol.py: where DupireLocalVol.price_fdm (local_vol.py:181-262) runs an
 * explicit finite-difference loop for one vanilla, these entry points walk Monte Carlo paths under sigma(S, t) and price the
 * payoffs the library has kernels for -- barriers, Asians, lookbacks, Europeans and a strike x maturity grid of Europeans.
 *
 * Conventions are olmc.h's: 0 on success, the message of the calling thread's last failure in olmc_last_error(), no CPU
 * fallback, results in olmc_stats.  Every refusal below is OLMC_ERR_ARG and is made before any device work.
 *
 * The model.  Paths take the GBM stream AS IT IS (olmc.h "Random stream": counter (path_lo, path_hi, step / 4, OLMC_STREAM_GBM),
 * key = seed, GLOBAL path index, fp32 normals, fp64 state): step t uses the normal z_t that step t of olmc_gbm_paths uses for the
 * same seed and path.  With n = n_steps and dt = T / n:
 *     x_0 = 0
 *     sigma_t = vol(x_t, t dt)
 *     x_{t+1} = x_t + (r - q - sigma_t^2 / 2) dt + sigma_t sqrt(dt) z_t
 *     S_t     = S exp(x_t)                              (date 0 is S itself)
 * vol is bilinear on the uniform table A[n_t][n_x] over (tau, x = ln(S_t / S)), held flat beyond every edge:
 *     u = clamp((x - x_lo) (n_x - 1) / (x_hi - x_lo), 0, n_x - 1),   j = min(floor(u), n_x - 2),   w     = u - j
 *     v = clamp(tau (n_t - 1) / t_hi, 0, n_t - 1),                   i = min(floor(v), n_t - 2),   w_tau = v - i
 *     a_i   = A[i][j] + w (A[i][j+1] - A[i][j])
 *     sigma = a_i + w_tau (a_{i+1} - a_i)
 * n_t == 1 is one row and no time axis.  Node values are rounded to fp32 when the table is uploaded (once per call); the
 * arithmetic on them is fp64.  The antithetic leg takes -z_t and walks its own sigma path.  A NaN input gives NaN results.
 */
#ifndef OLMC_LOCAL_VOL_H
#define OLMC_LOCAL_VOL_H

#include "olmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The table.  Refused: a null table or `vol` ("null pointer"), "n_x must be in [2, 256]", "n_t must be in [1, 64]",
 * "x_hi must be > x_lo", "t_hi must be > 0" (when n_t > 1), and a node that is not finite and > 0 once rounded to fp32
 * ("local volatilities must be finite and > 0"). */
typedef struct ollv_surface {
    const double* vol;   /* host, row-major [n_t][n_x] */
    int32_t n_x, n_t;    /* 2..256, 1..64 */
    double  x_lo, x_hi;  /* ln(S_t / S) of the first and last column */
    double  t_hi;        /* time of the last row; row 0 is time 0; unread when n_t == 1 */
} ollv_surface;

enum { OLLV_EUROPEAN = 8 };   /* continues OLMC_BARRIER_* 0-3, OLMC_LOOKBACK_* 4-5, OLMC_PATH_ASIAN_* 6-7 */

/* One payoff on paths [path_offset, path_offset + n_local) in ONE launch that stores no path.  payoff, barrier, the dates (extrema
 * over dates 0 .. n, the Asian mean over dates 1 .. n) and the log-space level decisions are olmc_heston_path_payoff's;
 * OLLV_EUROPEAN adds max(+-(S_n - K), 0).  antithetic != 0 also walks the mirrored path: 2 n_local samples.  Shards add up
 * (olmc_combine_stats).  Refused as olmc_heston_path_payoff refuses: "bad payoff", "Barrier must be positive", the counts. */
int ollv_price(double S, double K, double T, double r, double q, int is_call,
               const ollv_surface* surf, int payoff, double barrier,
               int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
               int antithetic, olmc_stats* out);

/* The matrix S_t of paths [0, n_paths), t = 0 .. n_steps, in olmc_gbm_paths' layouts (path_major != 0: [n_paths][n_steps + 1],
 * else [n_steps + 1][n_paths]) and with its refusal of a matrix beyond 64 GB. */
int ollv_paths(double S, double T, double r, double q, const ollv_surface* surf,
               int64_t n_paths, int32_t n_steps, uint64_t seed, int path_major,
               double* out_host);

/* European options at k <= OLMC_MAX_BATCH cells (strikes[i], steps[i]) read out of ONE set of paths: cell i is the payoff of
 * column steps[i] of ollv_paths' matrix, discounted over steps[i] dt.  Cells, order and read-out are olmc_heston_surface's. */
int ollv_surface_prices(double S, double T, double r, double q, int is_call,
                        const ollv_surface* surf, const double* strikes, const int32_t* steps, int32_t k,
                        int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                        int antithetic, olmc_stats* out /* [k] */);

#ifdef __cplusplus
}
#endif

#endif /* OLMC_LOCAL_VOL_H */
