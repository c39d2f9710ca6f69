/*
 * olmc_jump_scenarios.h -- scenario sets and finite-difference Greeks under Merton / Kou jump diffusion, ONE launch each (same
 * library, same contexts as olmc.h and olmc_jump.h).
 *
 * European options under k <= OLMC_MAX_BATCH parameter sets ("scenarios": spot, strike, maturity, rates, volatility, call / put AND
 * the jump model) on ONE walk over olmc_jump_paths' draws: common random numbers for what-if ladders, model-parameter bumps and the
 * finite-difference Greeks of the Monte Carlo price.  Conventions are olmc.h's: 0 on success, the message of the calling thread's last
 * failure in olmc_last_error(), no CPU fallback, results in olmc_stats.  Every refusal below is OLMC_ERR_ARG and is made before any
 * device work.
 *
 * THE FOLD.  A constant-sigma jump diffusion's terminal log-return is a diffusion part that knows the path through ONE number and a
 * jump part that knows (model, lambda, T, a1, a2, a3) alone.  With n = n_steps, dt_i = T_i / n and the blocks, tags, inversion and
 * size terms of olmc_jump.h, for the same seed and GLOBAL path index:
 *     Z     = the sum over t = 0 .. n - 1, in step order, in fp64, of the path's RAW Box-Muller normals z_t (the unit sqrt(2 ln 2)
 *             of a raw normal is folded into vol_i, as in the one-contract kernels);
 *     J_g   = the sum of the size terms of jump group g, in olmc_jump.h's order (steps ascending; for Kou, jumps ascending within
 *             a step); it starts at 0;
 *     x_i   = fma(vol_i, +-Z, n drift_i) + J_g(i),       vol_i = sigma_i sqrt(dt_i) sqrt(2 ln 2),
 *             drift_i = (r_i - q_i - lambda_i kappa_i - sigma_i^2 / 2) dt_i   (kappa_i = E[e^Y - 1] of the scenario's model);
 *     payoff = max(+-(exp(ln S_i + x_i) - K_i), 0).
 * The mirror leg (antithetic != 0: both legs of every path, 2 n_local samples) takes -Z and the SAME J: olmc_jump.h's mirror leg.
 * Scenario i is the contract olmc_jump_diffusion prices with its parameters, the same n_steps and the same seed; with antithetic the
 * contract oljd_price(..., OLJD_EUROPEAN, ..., antithetic) prices.  Those kernels interleave the same terms in one running sum, step
 * by step, so the sums agree with theirs to rounding, not to the bit.
 *
 * JUMP GROUPS.  Two scenarios SHARE A JUMP GROUP exactly when their (model, lambda_j, T, a1, a2, a3) are equal as doubles (bit for
 * bit: 0.3 and 0.1 + 0.2 are two groups); Merton does not read a3, so a3 never splits a Merton group.  Groups are numbered in order
 * of first appearance; a launch of k scenarios has at most k groups, so there is no second limit.  Spot, strike, r, q, sigma and
 * call / put never split a group: scenarios that differ only there share Z AND J.  The count of group g at step t comes by inversion
 * of the step's ONE Poisson uniform against the group's own p0 = exp(-lambda T / n): on common random numbers a larger lambda never
 * gives fewer jumps.  The size draws of a step are functions of (path, t, tag) alone, so every group reads the same Merton normal
 * and the same Kou uniforms for jump j; groups differ in their counts and in what they make of the draws.
 * oljs_layout reports the grouping (host arithmetic only; no device needed): n_groups and group[i], the jump group of scenario i.
 *
 * out[i] answers scenario i in the caller's order: .sum and .sumsq undiscounted, so shards add up (olmc_combine_stats with the
 * scenario's own r and T), .price = exp(-r_i T_i) mean, .std_error the naive per-sample one, .n = n_local (x 2 with antithetic).  A
 * scenario's sums depend neither on the other scenarios of the call, nor on its place in the list, nor on how many groups are in
 * use.  A NaN in a scenario gives NaN in that scenario only.
 * Refused: a null pointer; "the number of scenarios must be in [1, OLMC_MAX_BATCH]"; "n_steps must be >= 1"; "T must be > 0 in
 * every scenario"; then, per scenario, olmc_jump_diffusion's "bad jump model", "lambda_j must be non-negative" and "lambda_j * T /
 * n_steps must be <= 20 jumps per step: raise n_steps"; then the counts oljd_price refuses.  With profiling on a call counts as one
 * launch in olmc_kernel_time.
 *
 * THE GREEKS.  oljs_greeks_fd is olmc_european_greeks_fd's contract -- the bumps, the call order and the differences of
 * compute_greeks_unified; 7 / 8 contracts first order (without / with the T bump, taken when T > 1/365), 11 / 14 with second_order
 * -- priced under the model as ONE scenario launch on paths [0, n_paths): the 14 contracts are two jump groups (T and T - 1/365).
 * out9 = price, delta, gamma, vega, theta, rho, vanna, charm, vomma (the last three only with second_order); evals (NULL, or 14
 * olmc_stats) receives the contracts' statistics in the call order, zero-filled beyond the contracts in use.  Also refused: a null
 * out9 or model, "T must be > 0".
 */
#ifndef OLMC_JUMP_SCENARIOS_H
#define OLMC_JUMP_SCENARIOS_H

#include "olmc_jump.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oljs_scenario {
    double  S, K, T, r, sigma, q;
    int32_t is_call;
    int32_t model;              /* OLMC_JUMP_MERTON | OLMC_JUMP_KOU */
    double  lambda_j, a1, a2, a3;
} oljs_scenario;

int oljs_layout(const oljs_scenario* sc, int32_t k, int32_t* n_groups, int32_t* group /* [k] */);
int oljs_scenarios(const oljs_scenario* sc, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps,
                   uint64_t seed, int antithetic, olmc_stats* out /* [k], in the caller's order */);
int oljs_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, const oljd_model* model,
                   int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic, int second_order,
                   double* out9, olmc_stats* evals /* [14] or NULL */);

#ifdef __cplusplus
}
#endif

#endif /* OLMC_JUMP_SCENARIOS_H */
