// olmc_sabr_qmc_kernels.h -- device side of include/olmc_sabr_qmc.h: the SABR recursion of olmc_sabr_kernels.h (sabr_step, unchanged)
// on scrambled-Sobol points instead of the Philox stream.
//
// Point k of scipy.stats.qmc.Sobol(d = 2 n, scramble=True, seed) drives ONE path of n steps; the dimension assignment is Heston's
// (heston_qmc_draws<true>: both dimensions of a step through the inverse normal of the other Sobol kernels).
//   SEQUENTIAL  step t takes Z1 = z_{2t} and Z2' = z_{2t+1}.
//   BRIDGE      two bridges on the breadth-first plan, W1 on the even and W2 on the odd dimensions (heston_qmc_bridge_fill); step t
//               takes their increments (heston_qmc_bridge_sweep).
// These are TRUE normals: SabrModel's vol_unit, a and b carry sqrt(dt) alone (olmc.hip: make_sabr with z_unit = 1).  The mirror leg
// takes the negated pair -- the point -z, -W on both bridges, so one fill serves both legs -- and walks its own sigma path.
//
// LANES OVER POINTS, heston_qmc_kernel's skeleton: blocks of 64 points aligned in the ABSOLUTE point index (heston_point_blocks), the
// wave walks the 2 n dimensions together, a lane keeps (y, sigma) and the payoff's leg record of its point and of the mirror in fp64
// registers.  The sequential forms read nothing but the tables.  The bridge forms of the price and surface kernels fill Heston's
// library-owned slabs, [2 n][64] doubles per resident wave (olmc.hip: heston_qmc_shape with two dimensions per step, the same
// DeviceCtx::heston_w block); the paths kernel fills W in place in its two output matrices and sweeps over them.  Lanes outside the
// shard fold, broadcast and (sequential / surface) step a defined point with the others, touch no global memory and add nothing.
// The legs, epilogues and read-outs are sabr_price_kernel's / sabr_surface_kernel's, on the same __device__ functions.
#pragma once
#include "olmc_sabr_kernels.h"

namespace olmc {

// The wave's two bridge slabs (W1, then W2: [n][64] doubles each, time-major) and a date's place in them.
struct SabrQmcSlabs {
    double* w1;
    double* w2;
    __device__ __forceinline__ SabrQmcSlabs(double* slabs, int64_t slot, int32_t n)
        : w1(slabs + static_cast<size_t>(slot) * (2 * static_cast<size_t>(n) * kWave)), w2(w1 + static_cast<size_t>(n) * kWave) {}
};

// olsq_price: the nine payoffs of sabr_price_kernel (beta = 1: QmcLeg over ln(F_t / F); beta < 1: the legs in linear space), one launch,
// no path stored.
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS 64 B, the reduction), VGPRs plain / antithetic by beta kind 1, 0.5, 0,
// general (sabr_price_kernel: 76-96 / 66-70, 76-94 / 66-80, 74-94 / 66-80, 80-103 / 78-104):
//   sequential  European 80 / 60, 74 / 60, 74 / 60, 70 / 63          arithmetic 96 / 64, 76 / 64, 76 / 64, 72 / 67
//               geometric 76 / 64, 90 / 66, 90 / 66, 78 / 68         extrema 78 / 86, 80 / 88, 80 / 88, 92 / 90
//   bridge      European 99 / 73, 103 / 81, 99 / 75, 101 / 86        arithmetic 107 / 86, 105 / 85, 101 / 79, 103 / 90
//               geometric 101 / 77, 131 / 97, 128 / 96, 122 / 98     extrema 101 / 99, 109 / 109, 105 / 103, 123 / 112
//               (heston_qmc_path_kernel: arithmetic 121 / 117, geometric 117 / 113, extrema 115 / 131)
// The plain geometric bridge form at beta = 0.5 (a logarithm per date beside the square root, the sweep's batch in flight) is the one
// instantiation past 128: its 136 allocated registers admit three waves per SIMD where the others admit four or more.  The bridge
// launch holds two (olmc.hip: heston_slabs), so none runs at a lower occupancy than heston_qmc_kernel's bridge does.  The general-beta
// antithetic bridge forms, which carry the most state, take 86 - 112.
template <int FAMILY, int BETA_KIND, bool BRIDGE, bool ANTI>
__global__ __launch_bounds__(kBlock) void sabr_qmc_price_kernel(QmcRange qr, SabrModel m, ExtremaContract ec, double inv_steps,
                                                                const uint32_t* __restrict__ sv, const uint32_t* __restrict__ shift,
                                                                QmcBridgePlan plan, double* slabs, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    constexpr bool kLog = BETA_KIND == kSabrLognormal;
    constexpr double kLog2e = 1.4426950408889634;          // the arithmetic Asian's exp2_f64 counts in log2 units
    const int32_t n = qr.dims;                             // steps: the tables hold 2 n dimensions
    double acc[2] = {0.0, 0.0};
    heston_point_blocks(qr, [&](int64_t slot, int lane, uint64_t, bool live, const QmcLanePoint& lp) {
        double y[2], sg[2] = {m.alpha, m.alpha};
        QmcLeg leg[2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            y[l] = sabr_start<BETA_KIND>(m);
            if constexpr (!kLog) { leg[l].mx = m.f0; leg[l].mn = m.f0; }
        }
        auto step = [&](int32_t, double z1, double z2) {
#pragma unroll
            for (int l = 0; l < LEGS; ++l) {
                sabr_step<BETA_KIND>(m, l ? -z1 : z1, l ? -z2 : z2, y[l], sg[l]);
                if constexpr (FAMILY == kPathEuropean) continue;
                else if constexpr (kLog) qmc_leg_add<FAMILY>(leg[l], FAMILY == kQmcAsianArithmetic ? y[l] * kLog2e : y[l]);
                else if constexpr (FAMILY == kQmcAsianArithmetic) leg[l].a += y[l];
                else if constexpr (FAMILY == kQmcAsianGeometric) leg[l].a += log(y[l]);
                else { leg[l].mx = max_f64(leg[l].mx, y[l]); leg[l].mn = min_f64(leg[l].mn, y[l]); }
            }
        };
        if constexpr (BRIDGE) {
            const SabrQmcSlabs w(slabs, slot, n);
            auto at = [&](int32_t j) { return static_cast<size_t>(j - 1) * kWave + lane; };
            heston_qmc_bridge_fill(sv, shift, plan, n, lane, lp, live, w.w1, w.w2, at);
            if (live) heston_qmc_bridge_sweep(n, w.w1, w.w2, at, step);
        } else {
            heston_qmc_draws<true>(sv, shift, n, lane, lp, step);
        }
        if (live) {
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
        }
    });
    block_then_grid_reduce<2>(acc, ws);
}

// olsq_paths: the matrices F_t and sigma_t of points [0, count), t = 0 .. n, in path_at's layouts.  The bridge fills W1 in place in the
// forward matrix and W2 in the volatility matrix; the sweep reads a batch of both before it stores the states there.  Date 0, (F, alpha)
// as given, is written last.  flip = -1 walks the mirrored leg (exact negations).
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills, no LDS), VGPRs time-major / path-major by beta kind 1, 0.5, 0, general:
// 70 / 82, 70 / 82, 70 / 82, 66 / 78 (sequential), 76 / 64, 94 / 82, 94 / 82, 95 / 82 (bridge).
template <int BETA_KIND, bool BRIDGE, bool PATH_MAJOR>
__global__ __launch_bounds__(kBlock) void sabr_qmc_paths_kernel(QmcRange qr, SabrModel m, double flip, const uint32_t* __restrict__ sv,
                                                                const uint32_t* __restrict__ shift, QmcBridgePlan plan, double* forward,
                                                                double* vol) {
    const int lane = static_cast<int>(threadIdx.x) & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave);
    const int32_t n = qr.dims;
    const int64_t count = qr.count;
    const int64_t n_blocks = (count + kWave - 1) / kWave;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    for (int64_t blk = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave; blk < n_blocks; blk += stride) {
        const int64_t i = blk * kWave + lane;
        const bool live = i < count;
        const QmcLanePoint lp(static_cast<uint32_t>(i));
        auto at = [&](int32_t t) { return path_at<PATH_MAJOR>(i, t, count, n); };
        double y = sabr_start<BETA_KIND>(m), sg = m.alpha;
        auto step = [&](int32_t t, double z1, double z2) {
            sabr_step<BETA_KIND>(m, flip * z1, flip * z2, y, sg);
            if (live) {
                const size_t p = at(t + 1);
                forward[p] = sabr_forward<BETA_KIND>(m, y);
                vol[p] = sg;
            }
        };
        if constexpr (BRIDGE) {
            heston_qmc_bridge_fill(sv, shift, plan, n, lane, lp, live, forward, vol, at);
            if (live) heston_qmc_bridge_sweep(n, forward, vol, at, step);
        } else {
            heston_qmc_draws<true>(sv, shift, n, lane, lp, step);
        }
        if (live) { forward[at(0)] = m.f0; vol[at(0)] = m.alpha; }
    }
}

// olsq_surface_prices: SurfaceRows' cells and read-out as sabr_surface_kernel applies them (beta = 1: exp(ln F + x); beta < 1: the
// forward as it stands) on these paths.  The tables and the plan are those of the full n = qr.dims steps (a cell at an intermediate
// date reads the full-horizon construction); the sequential walk and the bridge's sweep stop at the last cell's step.  The point loop
// is wave-uniform: every lane fills and sweeps its own column of the wave's slabs, inside the shard or not, with its payoff masked to 0
// outside.
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS 3.2 KiB), VGPRs plain / antithetic by beta kind 1, 0.5, 0, general:
// 76 / 62, 76 / 62, 76 / 62, 90 / 65 (sequential), 87 / 75, 85 / 71, 85 / 71, 111 / 76 (bridge).
template <int BETA_KIND, bool BRIDGE, bool ANTI>
__global__ __launch_bounds__(kBlock) void sabr_qmc_surface_kernel(QmcRange qr, SabrModel m, double sign, HestonSurfaceCells cells,
                                                                  const uint32_t* __restrict__ sv, const uint32_t* __restrict__ shift,
                                                                  QmcBridgePlan plan, double* slabs, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    const SurfaceRows rows = surface_rows(cells);
    const int32_t n = qr.dims;
    heston_point_blocks(qr, [&](int64_t slot, int lane, uint64_t, bool live, const QmcLanePoint& lp) {      // wave-uniform
        double y[2] = {sabr_start<BETA_KIND>(m), sabr_start<BETA_KIND>(m)}, sg[2] = {m.alpha, m.alpha};
        int32_t next = 0, pending = cells.step[0];
        auto step = [&](int32_t t, double z1, double z2) {
#pragma unroll
            for (int l = 0; l < LEGS; ++l) sabr_step<BETA_KIND>(m, l ? -z1 : z1, l ? -z2 : z2, y[l], sg[l]);
            if constexpr (BETA_KIND == kSabrLognormal) {
                const double ls[2] = {m.log_f0 + y[0], m.log_f0 + y[1]};
                rows.read_out<LEGS>(next, pending, t + 1, 0.0, sign, ls, live);
            } else {
                rows.read_out_linear<LEGS>(next, pending, t + 1, sign, y, live);
            }
        };
        if constexpr (BRIDGE) {
            const SabrQmcSlabs w(slabs, slot, n);
            auto at = [&](int32_t j) { return static_cast<size_t>(j - 1) * kWave + lane; };
            heston_qmc_bridge_fill(sv, shift, plan, n, lane, lp, true, w.w1, w.w2, at);
            heston_qmc_bridge_sweep(cells.last, w.w1, w.w2, at, step);
        } else {
            heston_qmc_draws<true>(sv, shift, cells.last, lane, lp, step);
        }
    });
    rows.reduce(ws);
}

}  // namespace olmc
