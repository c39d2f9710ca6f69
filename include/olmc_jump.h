/*
 * olmc_jump.h -- path-dependent options on Merton / Kou jump-diffusion paths (same library, same contexts as olmc.h).
 *
 * olmc_jump_diffusion prices a European and olmc_jump_paths writes the path matrix; these entry points price, on the SAME
 * paths and in ONE launch that stores no path, the payoffs the library has for its other models: Asians, barriers and
 * lookbacks, a strike x maturity grid of Europeans, the autocallable and the cliquet.
 *
 * Conventions are olmc.h's: 0 on success, the message of the calling thread's last failure in olmc_last_error(), no CPU
 * fallback, results in olmc_stats, shards add up through olmc_combine_stats, a NaN input gives NaN results.  Every refusal
 * below is OLMC_ERR_ARG and is made before any device work.
 *
 * The paths are olmc_jump_paths' (olmc.h "jump diffusion"), for the same seed and GLOBAL path index.  With n = n_steps,
 * dt = T / n, drift = (r - q - lambda kappa - sigma^2 / 2) dt and vol = sigma sqrt(dt), step t of a path is
 *     ls += fma(vol, z_t, drift)          z_t: words 0, 1 of block (path, t / 2, OLMC_STREAM_JUMP) through Box-Muller
 *     N_t  = the Poisson(lambda dt) count, by inversion of the uniform of word 2 + t % 2 of that block; at most 64
 *     ls += term_j  for each size term, in order: Merton ONE term N mu_j + sigma_j sqrt(N) z' (z' from block
 *                   (path, t, OLMC_STREAM_JUMP + 1)); Kou one term per jump j, +Exp(eta1) with probability p, else -Exp(eta2),
 *                   from words 2 (j % 2), 2 (j % 2) + 1 of block (path, t, OLMC_STREAM_JUMP + 1 + j / 2)
 * and S_t = exp(ls); date 0 is S itself.  The order of the additions is part of the definition.
 *
 * The mirror leg (antithetic != 0 prices both legs of every path, 2 n_local samples; oljd_paths' mirror != 0 writes it):
 *   - it takes -z_t for the diffusion normal of every step;
 *   - it takes the SAME jump count and the SAME jump sizes as the path itself: the Poisson uniform and the size blocks are
 *     drawn once per path and step, and each size term is added to both legs in the same order.
 * Only the diffusion is mirrored; the jump component of a pair is common.
 */
#ifndef OLMC_JUMP_H
#define OLMC_JUMP_H

#include "olmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The model, as olmc_jump_diffusion takes it.  Merton: (a1, a2) = (mu_j, sigma_j), a3 unread.  Kou: (a1, a2, a3) =
 * (p, eta1, eta2).  Refused: a null model ("null pointer"), "bad jump model", "lambda_j must be non-negative", and more than
 * 20 expected jumps per step ("lambda_j * T / n_steps must be <= 20 jumps per step: raise n_steps"). */
typedef struct oljd_model {
    int32_t model;       /* OLMC_JUMP_MERTON | OLMC_JUMP_KOU */
    int32_t pad;
    double  lambda_j, a1, a2, a3;
} oljd_model;

enum { OLJD_EUROPEAN = 8 };   /* continues OLMC_BARRIER_* 0-3, OLMC_LOOKBACK_* 4-5, OLMC_PATH_ASIAN_* 6-7 */

/* One payoff on paths [path_offset, path_offset + n_local).  payoff, barrier, the dates (extrema over dates 0 .. n, the Asian
 * mean over dates 1 .. n) and the log-space level decisions are olmc_heston_path_payoff's, its date-0 barrier decision (the
 * plain comparison of S with the barrier) included; OLJD_EUROPEAN adds max(+-(S_n - K), 0).  Refused as
 * olmc_heston_path_payoff refuses: "bad payoff", "Barrier must be positive", the counts. */
int oljd_price(double S, double K, double T, double r, double sigma, double q, int is_call,
               const oljd_model* model, int payoff, double barrier,
               int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
               int antithetic, olmc_stats* out);

/* European options at k <= OLMC_MAX_BATCH cells (strikes[i], steps[i]) read out of ONE set of paths: cell i is the payoff of
 * column steps[i] of oljd_paths' matrix, discounted over steps[i] dt.  Cells, order, refusals and read-out are
 * olmc_heston_surface's. */
int oljd_surface_prices(double S, double T, double r, double sigma, double q, int is_call,
                        const oljd_model* model, const double* strikes, const int32_t* steps, int32_t k,
                        int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                        int antithetic, olmc_stats* out /* [k] */);

/* olmc_autocallable's contract on these paths: the payoff of a path is what olmc_heston_autocallable computes from its row of
 * the spot matrix (already discounted path by path).  Refused as there: "observation_freq must be >= 1", "no observation
 * date: observation_freq > n_steps". */
int oljd_autocallable(double S, double T, double r, double sigma, double q, const oljd_model* model,
                      double autocall_barrier, double coupon_barrier, double coupon_rate, double ki_barrier,
                      int32_t observation_freq,
                      int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                      int antithetic, olmc_stats* out);

/* olmc_cliquet's contract on these paths; the dates after the last whole period are not drawn.  Refused as there:
 * "n_periods must be in [1, n_steps]". */
int oljd_cliquet(double S, double T, double r, double sigma, double q, const oljd_model* model,
                 double local_cap, double local_floor, double global_cap, double global_floor,
                 int32_t n_periods,
                 int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                 int antithetic, olmc_stats* out);

/* The matrix S_t of ONE leg of paths [0, n_paths), t = 0 .. n_steps, in olmc_gbm_paths' layouts and with its refusal of a
 * matrix beyond 64 GB.  mirror == 0 writes olmc_jump_paths' matrix, word for word; mirror != 0 the mirror leg's. */
int oljd_paths(double S, double T, double r, double sigma, double q, const oljd_model* model,
               int64_t n_paths, int32_t n_steps, uint64_t seed, int mirror, int path_major,
               double* out_host);

#ifdef __cplusplus
}
#endif

#endif /* OLMC_JUMP_H */
