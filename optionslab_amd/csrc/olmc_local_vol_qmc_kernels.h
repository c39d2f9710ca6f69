// olmc_local_vol_qmc_kernels.h -- device side of include/olmc_local_vol_qmc.h: the local-volatility recursion of
// olmc_local_vol_kernels.h (lv_step on the table in LDS, unchanged) on scrambled-Sobol points instead of the Philox stream.
//
// Point k of scipy.stats.qmc.Sobol(d = n, scramble=True, seed) drives ONE path of n steps: z_t = Phi^-1(clip(u_t, 1e-10, 1 - 1e-10)),
// the Sobol uniform and inverse normal of the other Sobol kernels, t = 0 .. n - 1.
//   SEQUENTIAL  step t takes z_t.
//   BRIDGE      W_j (j = 1 .. n) on the breadth-first plan (QmcBridgePlan: node 0 is W_n = sqrt(n) z_0, node k takes z_k, the fma form of
//               heston_qmc_bridge_fill); step t takes W_{t+1} - W_t.
// These are TRUE normals: LvModel::vol_unit is sqrt(dt) here (olmc.hip: lv_upload with z_unit = 1).  The mirror leg takes the negated
// increment and walks its own sigma path.
//
// LANES OVER POINTS, as heston_qmc_kernel: sigma depends on the state, so the recursion is serial in time and a lane keeps x (and the
// payoff's QmcLeg) of its point and of the mirror in fp64 registers.  A wave holds an aligned block of 64 consecutive points -- aligned
// in the ABSOLUTE point index (heston_point_blocks), so a shard may start anywhere -- and walks the n dimensions together: one fold of the
// block's common Gray bits per 64 dimensions, then per dimension a broadcast plus the lane's six low rows and ONE inverse normal
// (lv_qmc_draws).  Every lane of a wave is at the same date, so lv_rows' readfirstlane holds and the table stays whole in LDS.
// The bridge needs a point's n normals before step 0: the nodes fill W_j in plan order into memory the lane owns (W_0 = 0 is not
// stored), reading back the lane's own earlier stores, and a sweep then reads W_{t+1} kHestonQmcBatch dates at a time.
//   lv_qmc_paths_kernel                        fills W in place in the output matrix; the sweep reads a batch of W before it stores S there.
//   lv_qmc_price_kernel, lv_qmc_surface_kernel fill a library-owned slab of [n][64] doubles per wave of the GRID (time-major: a date is
//                                              512 contiguous bytes; olmc.hip: lv_qmc_shape), reused by every block the wave strides
//                                              over; the mirror leg reads the same W, negated.
// Lanes outside the shard fold, broadcast and step with the others (a defined point: x stays finite, lv_sigma's column stays in the
// table), touch no global memory and add nothing.
#pragma once
#include "olmc_local_vol_kernels.h"

namespace olmc {

// body(t, z_t) for t = 0 .. dims - 1 in every lane: heston_qmc_draws for one factor (a dimension per step, every one a normal).
template <typename Body>
__device__ __forceinline__ void lv_qmc_draws(const uint32_t* __restrict__ sv, const uint32_t* __restrict__ shift, int32_t dims, int lane,
                                             const QmcLanePoint& lp, Body body) {
    for (int32_t c0 = 0; c0 < dims; c0 += kWave) {
        const int32_t tl = c0 + lane < dims ? c0 + lane : dims - 1;
        const uint32_t* __restrict__ mine = sv + static_cast<size_t>(tl) * kSobolBits;
        uint32_t fold = shift[tl];
#pragma unroll
        for (int b = 6; b < kSobolBits; ++b) fold ^= mine[b] & (0u - ((lp.gray_hi >> b) & 1u));
        const int32_t cn = dims - c0 < kWave ? dims - c0 : kWave;
        for (int32_t d = 0; d < cn; ++d) {
            const uint32_t* __restrict__ row = sv + static_cast<size_t>(c0 + d) * kSobolBits;
            uint32_t x = static_cast<uint32_t>(__shfl(static_cast<int>(fold), d, kWave));
#pragma unroll
            for (int b = 0; b < 6; ++b) x = __builtin_amdgcn_bitop3_b32(x, row[b], lp.mask[b], 0x78);   // x ^ (row & mask)
            body(c0 + d, ndtri_w_add(0.0, sobol_uniform(x), opaque_zero()));
        }
    }
}

// W_j (j = 1 .. n) of the lane's point at w[at(j)], in plan order (the plan's a, b, m and coefficients are wave-uniform); every lane
// walks the dimensions, only `live` ones touch memory.
template <typename At>
__device__ __forceinline__ void lv_qmc_bridge_fill(const uint32_t* __restrict__ sv, const uint32_t* __restrict__ shift, const QmcBridgePlan& plan,
                                                   int32_t n, int lane, const QmcLanePoint& lp, bool live, double* w, At at) {
    lv_qmc_draws(sv, shift, n, lane, lp, [&](int32_t k, double z) {
        if (k == 0) {
            if (live) w[at(n)] = sqrt(static_cast<double>(n)) * z;
        } else {
            const uint32_t ab = plan.ab[k];
            const int32_t a = static_cast<int32_t>(ab & 0xffffu), b = static_cast<int32_t>(ab >> 16), m = (a + b) >> 1;
            const double ca = plan.coef[k], cb = plan.coef[n + k], sd = plan.coef[2 * n + k];
            if (live) {
                const double wa = a == 0 ? 0.0 : w[at(a)];
                w[at(m)] = __builtin_fma(ca, wa, __builtin_fma(cb, w[at(b)], sd * z));
            }
        }
    });
}

// step(t, W_{t+1} - W_t) for t = 0 .. last - 1: a batch of W is read before its steps run, so step may overwrite w[at(t + 1)].
template <typename At, typename Step>
__device__ __forceinline__ void lv_qmc_bridge_sweep(int32_t last, const double* w, At at, Step step) {
    double p = 0.0;
    for (int32_t t0 = 0; t0 < last; t0 += kHestonQmcBatch) {
        double q[kHestonQmcBatch];
#pragma unroll
        for (int j = 0; j < kHestonQmcBatch; ++j) q[j] = w[at(t0 + j + 1 <= last ? t0 + j + 1 : last)];
#pragma unroll
        for (int j = 0; j < kHestonQmcBatch; ++j) {
            if (t0 + j < last) {
                step(t0 + j, q[j] - p);
                p = q[j];
            }
        }
    }
}

// The wave's bridge slab and a date's place in it.
__device__ __forceinline__ double* lv_qmc_slab(double* slabs, int64_t slot, int32_t n) {
    return slabs + static_cast<size_t>(slot) * (static_cast<size_t>(n) * kWave);
}

// olvq_price: the nine payoffs of lv_price_kernel (QmcLeg over ln(S_t / S), the date-0 barrier decision in ec: heston_path_contract),
// one launch, no path stored.
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS: the table + 64 B, the reduction), VGPRs plain / antithetic:
//   sequential  arithmetic 80 / 64, geometric 78 / 64, extrema 80 / 86, European 80 / 60      (lv_price_kernel: 93 / 90, 88 / 79, 93 / 106, 88 / 80)
//   bridge      arithmetic 105 / 81, geometric 83 / 79, extrema 83 / 99, European 85 / 75     (heston_qmc_path_kernel: 121 / 117, 117 / 113, 115 / 131)
// Every form stays under 128 registers (four waves per SIMD); the bridge launch holds two (heston_slab_shape), the table's LDS at its caps
// two workgroups per CU.
template <int FAMILY, bool BRIDGE, bool ANTI>
__global__ __launch_bounds__(kBlock) void lv_qmc_price_kernel(QmcRange qr, LvModel m, ExtremaContract ec, double inv_steps,
                                                              const uint32_t* __restrict__ sv, const uint32_t* __restrict__ shift, QmcBridgePlan plan,
                                                              double* slabs, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    constexpr double kLog2e = 1.4426950408889634;          // the arithmetic Asian's exp2_f64 counts in log2 units
    lv_table_to_lds(m);
    const int32_t n = qr.dims;
    double acc[2] = {0.0, 0.0};
    // The legs written out, as in lv_price_kernel: in one shared struct the plain extrema bridge form measured 1.5 % slower (profiles/r24_shared_path_pieces.jsonl).
    heston_point_blocks(qr, [&](int64_t slot, int lane, uint64_t, bool live, const QmcLanePoint& lp) {
        double x[2] = {0.0, 0.0};
        QmcLeg leg[2];
        auto step = [&](int32_t t, double z) {
            const LvRows rw = lv_rows(m, t);
#pragma unroll
            for (int l = 0; l < LEGS; ++l) {
                x[l] = lv_step(m, rw, x[l], l ? -z : z);
                if constexpr (FAMILY == kQmcAsianArithmetic) qmc_leg_add<FAMILY>(leg[l], x[l] * kLog2e);
                else if constexpr (FAMILY != kPathEuropean) qmc_leg_add<FAMILY>(leg[l], x[l]);
            }
        };
        if constexpr (BRIDGE) {
            double* w = lv_qmc_slab(slabs, slot, n);
            auto at = [&](int32_t j) { return static_cast<size_t>(j - 1) * kWave + lane; };
            lv_qmc_bridge_fill(sv, shift, plan, n, lane, lp, live, w, at);
            if (live) lv_qmc_bridge_sweep(n, w, at, step);
        } else {
            lv_qmc_draws(sv, shift, n, lane, lp, step);
        }
        if (live) {
#pragma unroll
            for (int l = 0; l < LEGS; ++l) {
                double p;
                if constexpr (FAMILY == kPathEuropean) p = fmax(ec.sign * (ec.s0 * exp(x[l]) - ec.strike), 0.0);
                else p = qmc_payoff<FAMILY>(ec, inv_steps, leg[l].a, leg[l].mx, leg[l].mn, x[l]);
                acc[0] += p; acc[1] += p * p;
            }
        }
    });
    block_then_grid_reduce<2>(acc, ws);
}

// olvq_paths: the matrix S exp(x_t), t = 0 .. n, of points [0, count) in path_at's layouts; date 0 is S itself.
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS: the table), VGPRs time-major / path-major: 78 / 78 (sequential),
// 76 / 80 (bridge).
template <bool BRIDGE, bool PATH_MAJOR>
__global__ __launch_bounds__(kBlock) void lv_qmc_paths_kernel(QmcRange qr, LvModel m, const uint32_t* __restrict__ sv,
                                                              const uint32_t* __restrict__ shift, QmcBridgePlan plan, double* paths) {
    lv_table_to_lds(m);
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
        double x = 0.0;
        auto step = [&](int32_t t, double z) {
            x = lv_step(m, lv_rows(m, t), x, z);
            if (live) paths[at(t + 1)] = m.s0 * exp(x);
        };
        if constexpr (BRIDGE) {
            lv_qmc_bridge_fill(sv, shift, plan, n, lane, lp, live, paths, at);
            if (live) lv_qmc_bridge_sweep(n, paths, at, step);
        } else {
            lv_qmc_draws(sv, shift, n, lane, lp, step);
        }
        if (live) paths[at(0)] = m.s0;
    }
}

// olvq_surface_prices: SurfaceRows' cells and read-out (lv_surface_kernel's: the date's spot as exp(ln S + x), mu_dt = 0) on these paths.
// The tables and the plan are those of the full n = qr.dims steps (a cell at an intermediate date reads the full-horizon construction);
// the sequential walk and the bridge's sweep stop at the last cell's step.  The point loop is wave-uniform: every lane fills and sweeps
// its own column of the wave's slab, inside the shard or not, with its payoff masked to 0 outside.
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS: the table + 3.2 KiB), VGPRs plain / antithetic: 78 / 60
// (sequential), 79 / 64 (bridge).
template <bool BRIDGE, bool ANTI>
__global__ __launch_bounds__(kBlock) void lv_qmc_surface_kernel(QmcRange qr, LvModel m, double sign, HestonSurfaceCells cells,
                                                                const uint32_t* __restrict__ sv, const uint32_t* __restrict__ shift,
                                                                QmcBridgePlan plan, double* slabs, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    lv_table_to_lds(m);
    const SurfaceRows rows = surface_rows(cells);
    const int32_t n = qr.dims;
    heston_point_blocks(qr, [&](int64_t slot, int lane, uint64_t, bool live, const QmcLanePoint& lp) {      // wave-uniform
        double x[2] = {0.0, 0.0};
        int32_t next = 0, pending = cells.step[0];
        auto step = [&](int32_t t, double z) {
            const LvRows rw = lv_rows(m, t);
#pragma unroll
            for (int l = 0; l < LEGS; ++l) x[l] = lv_step(m, rw, x[l], l ? -z : z);
            const double ls[2] = {m.log_s0 + x[0], m.log_s0 + x[1]};
            rows.read_out<LEGS>(next, pending, t + 1, 0.0, sign, ls, live);
        };
        if constexpr (BRIDGE) {
            double* w = lv_qmc_slab(slabs, slot, n);
            auto at = [&](int32_t j) { return static_cast<size_t>(j - 1) * kWave + lane; };
            lv_qmc_bridge_fill(sv, shift, plan, n, lane, lp, true, w, at);
            lv_qmc_bridge_sweep(cells.last, w, at, step);
        } else {
            lv_qmc_draws(sv, shift, cells.last, lane, lp, step);
        }
    });
    rows.reduce(ws);
}

}  // namespace olmc
