// olmc_sabr_kernels.h -- device side of include/olmc_sabr.h: path kernels of the SABR process dF = sigma F^beta dW1, dsigma = nu sigma dW2.
//
// Draws: the Heston Euler stream's shape under a tag of its own (heston_philox_walk<kTagSabr>: block b feeds steps 2b and 2b + 1, the
// cosine normal is Z1, the sine normal Z2'), RAW fp32 normals, fp64 state.  The recursion is the header's: sigma takes the exact
// lognormal step (one fp64 exponential per step and leg), F takes
//     beta = 1   x += -sigma^2 dt / 2 + sigma sqrt(dt) Z1 on x = ln(F_t / F): the shared payoff legs' own space, one exponential at read-out
//     beta < 1   G = F + sigma F^beta sqrt(dt) Z1 on F itself, absorbed at 0: the legs then run in LINEAR space -- running extrema of F
//                (monotone: converted to ln(. / F) once per path), the arithmetic mean as a plain sum, only the geometric mean takes a
//                logarithm per date (an absorbed path sums to -inf: a mean of 0), the surface reads F out as it stands.
// BETA_KIND picks F^beta at compile time; the host dispatches on beta == 1.0, 0.5, 0.0 as doubles (olmc.hip: with_sabr_kind).
#pragma once
#include "olmc_kernels.h"

namespace olmc {

constexpr uint32_t kTagSabr = 0x53414252u;        // OLMC_STREAM_SABR ("SABR"): far from Kou's size tags, which grow upward from 3

enum SabrBetaKind { kSabrLognormal = 0 /* beta == 1 */, kSabrHalf = 1 /* beta == 0.5 */, kSabrNormal = 2 /* beta == 0 */, kSabrGeneral = 3 };

struct SabrModel {
    double f0, log_f0, alpha, beta;
    double half_dt;              // dt / 2
    double vol_unit;             // sqrt(dt) kZScale: sigma_t vol_unit multiplies the RAW Z1
    double a, b, c;              // ln(sigma_{t+1} / sigma_t) = a z1 + b z2 + c on RAW normals: nu sqrt(dt) kZScale (rho, sqrt(1 - rho^2)), -nu^2 dt / 2
};

// One step of one leg from the step's RAW normals (the mirror leg passes them negated).  y is ln(F_t / F) for kSabrLognormal and F_t
// otherwise.  `y <= 0 || g <= 0` is "not (F_t > 0 and G > 0)" for numbers and lets a NaN through.
template <int BETA_KIND>
__device__ __forceinline__ void sabr_step(const SabrModel& m, double z1, double z2, double& y, double& sg) {
    const double u = m.vol_unit * z1;
    if constexpr (BETA_KIND == kSabrLognormal) {
        y = __builtin_fma(sg, u, __builtin_fma(-(sg * sg), m.half_dt, y));
    } else {
        double fb = 1.0;
        if constexpr (BETA_KIND == kSabrHalf) fb = sqrt_nonneg(y);
        else if constexpr (BETA_KIND == kSabrGeneral) fb = exp(m.beta * log(y));       // y = 0: exp(-inf) = 0
        const double g = __builtin_fma(sg * fb, u, y);
        y = (y <= 0.0 || g <= 0.0) ? 0.0 : g;
    }
    sg *= exp(__builtin_fma(m.a, z1, __builtin_fma(m.b, z2, m.c)));
}

template <int BETA_KIND>
__device__ __forceinline__ double sabr_start(const SabrModel& m) { return BETA_KIND == kSabrLognormal ? 0.0 : m.f0; }

// The forward of a state.
template <int BETA_KIND>
__device__ __forceinline__ double sabr_forward(const SabrModel& m, double y) { return BETA_KIND == kSabrLognormal ? m.f0 * exp(y) : y; }

// olsb_price: one launch, no path stored.  Payoffs, dates and level decisions are heston_path_kernel's (extrema over dates 0 .. n, the
// Asian mean over dates 1 .. n, the date-0 barrier decision made on the host: heston_path_contract); kPathEuropean adds max(+-(F_n - K), 0).
// beta = 1 feeds QmcLeg with ln(F_t / F) as lv_price_kernel does.  beta < 1 keeps QmcLeg's three words in linear space: a = sum F_t
// (arithmetic) or sum ln F_t (geometric), mx / mn = the extrema of F_t from F_0 = F; the epilogue hands qmc_payoff<kQmcExtrema> their
// ln(. / F) -- F / F is exactly 1, so the start sits at 0 as its levels assume; a minimum of 0 becomes -inf, below every level.
template <int FAMILY, int BETA_KIND, bool ANTI>
__global__ __launch_bounds__(kBlock) void sabr_price_kernel(PathRange pr, SabrModel m, ExtremaContract ec, double inv_steps, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    constexpr bool kLog = BETA_KIND == kSabrLognormal;
    constexpr double kLog2e = 1.4426950408889634;          // the arithmetic Asian's exp2_f64 counts in log2 units
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    double acc[2] = {0.0, 0.0};
    for_each_path(pr, [&](int64_t, uint32_t g_lo, uint32_t g_hi) {
        double y[2], sg[2] = {m.alpha, m.alpha};
        QmcLeg leg[2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            y[l] = sabr_start<BETA_KIND>(m);
            if constexpr (!kLog) { leg[l].mx = m.f0; leg[l].mn = m.f0; }
        }
        heston_philox_walk<kTagSabr>(g_lo, g_hi, rk, pr.n_steps, false, [&](int32_t, double z1, double z2, bool) {
#pragma unroll
            for (int l = 0; l < LEGS; ++l) {
                sabr_step<BETA_KIND>(m, l ? -z1 : z1, l ? -z2 : z2, y[l], sg[l]);
                if constexpr (FAMILY == kPathEuropean) continue;
                else if constexpr (kLog) qmc_leg_add<FAMILY>(leg[l], FAMILY == kQmcAsianArithmetic ? y[l] * kLog2e : y[l]);
                else if constexpr (FAMILY == kQmcAsianArithmetic) leg[l].a += y[l];
                else if constexpr (FAMILY == kQmcAsianGeometric) leg[l].a += log(y[l]);
                else { leg[l].mx = max_f64(leg[l].mx, y[l]); leg[l].mn = min_f64(leg[l].mn, y[l]); }
            }
        });
#pragma unroll
        for (int l = 0; l < LEGS; ++l) {
            double p;
            if constexpr (FAMILY == kPathEuropean) p = fmax(ec.sign * (sabr_forward<BETA_KIND>(m, y[l]) - ec.strike), 0.0);
            else if constexpr (kLog) p = qmc_payoff<FAMILY>(ec, inv_steps, leg[l].a, leg[l].mx, leg[l].mn, y[l]);
            else if constexpr (FAMILY == kQmcAsianArithmetic) p = fmax(ec.sign * (leg[l].a * inv_steps - ec.strike), 0.0);
            else if constexpr (FAMILY == kQmcAsianGeometric) p = fmax(ec.sign * (exp(leg[l].a * inv_steps) - ec.strike), 0.0);
            else p = qmc_payoff<FAMILY>(ec, inv_steps, 0.0, log(leg[l].mx / m.f0), log(leg[l].mn / m.f0), log(y[l] / m.f0));
            acc[0] += p; acc[1] += p * p;
        }
    });
    block_then_grid_reduce<2>(acc, ws);
}

// olsb_paths: the matrices F_t and sigma_t, t = 0 .. n, in heston_paths_kernel's layouts; date 0 is (F, alpha) as given.  flip = -1
// walks the mirrored leg (exact negations).  The draws come from the scalar keys.
template <int BETA_KIND, bool PATH_MAJOR>
__global__ __launch_bounds__(kBlock) void sabr_paths_kernel(PathRange pr, SabrModel m, double flip, double* __restrict__ forward,
                                                            double* __restrict__ vol) {
    for_each_path(pr, [&](int64_t i, uint32_t g_lo, uint32_t g_hi) {
        double y = sabr_start<BETA_KIND>(m), sg = m.alpha;
        forward[path_at<PATH_MAJOR>(i, 0, pr.count, pr.n_steps)] = m.f0;
        vol[path_at<PATH_MAJOR>(i, 0, pr.count, pr.n_steps)] = m.alpha;
        heston_philox_walk<kTagSabr>(g_lo, g_hi, LaunchKeys{pr.key0, pr.key1}, pr.n_steps, false, [&](int32_t t, double z1, double z2, bool) {
            sabr_step<BETA_KIND>(m, flip * z1, flip * z2, y, sg);
            const size_t at = path_at<PATH_MAJOR>(i, t + 1, pr.count, pr.n_steps);
            forward[at] = sabr_forward<BETA_KIND>(m, y);
            vol[at] = sg;
        });
    });
}

// olsb_surface_prices: heston_surface_kernel's prologue, wave-uniform path loop, cell rows and read-out (surface_rows,
// for_each_wave_path, SurfaceRows) on these paths; the walk ends at the last cell's step.  beta = 1 reads a date out as exp(ln F + x),
// beta < 1 hands the forward over as it stands (read_out_linear): an absorbed path reads max(+-(0 - K), 0).
template <int BETA_KIND, bool ANTI>
__global__ __launch_bounds__(kBlock) void sabr_surface_kernel(PathRange pr, SabrModel m, double sign, HestonSurfaceCells cells, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    const SurfaceRows rows = surface_rows(cells);
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    for_each_wave_path(pr, [&](bool live, PathWords pw) {
        double y[2] = {sabr_start<BETA_KIND>(m), sabr_start<BETA_KIND>(m)}, sg[2] = {m.alpha, m.alpha};
        int32_t next = 0, pending = cells.step[0];
        heston_philox_walk<kTagSabr>(pw.lo, pw.hi, rk, cells.last, false, [&](int32_t t, double z1, double z2, bool) {
#pragma unroll
            for (int l = 0; l < LEGS; ++l) sabr_step<BETA_KIND>(m, l ? -z1 : z1, l ? -z2 : z2, y[l], sg[l]);
            if constexpr (BETA_KIND == kSabrLognormal) {
                const double ls[2] = {m.log_f0 + y[0], m.log_f0 + y[1]};
                rows.read_out<LEGS>(next, pending, t + 1, 0.0, sign, ls, live);
            } else {
                rows.read_out_linear<LEGS>(next, pending, t + 1, sign, y, live);
            }
        });
    });
    rows.reduce(ws);
}

}  // namespace olmc
