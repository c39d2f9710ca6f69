// olmc_local_vol_kernels.h -- device side of include/olmc_local_vol.h: path kernels under a Dupire local volatility sigma(S, t).
//
// Paths are the GBM stream as it is (Philox counter (path_lo, path_hi, step / 4, OLMC_STREAM_GBM), the library's Box-Muller, fp32
// normals, fp64 state): step t takes the normal that step t of lsm_paths_kernel / extrema_kernel takes for the same seed and path.
// What is new in the step loop is the volatility: a bilinear lookup in a uniform table A[n_t][n_x] over (tau, x = ln(S_t / S)), held
// flat beyond every edge.  The rows of a date are launch-uniform (every path of a launch is at the same tau), the column is per lane.
//
// Table shape: THE WHOLE TABLE IN LDS, as fp32 (the nodes are rounded to fp32 when they are uploaded; every operation on them is fp64).
// n_t n_x 4 bytes of dynamic LDS per workgroup: 17 KiB at the typical 33 x 128, 64 KiB at the caps (two workgroups per CU of the 160
// KiB).  A lookup is four ds_read_b32 at a data-dependent column of two wave-uniform rows.  No workgroup barrier sits inside the step
// loop, so for_each_path's ragged last stride needs no dead lanes.  The other shape (only the date's time-blended row in LDS, a barrier
// per date) lives outside the product as an A/B build (tools/local_vol_ab/, -DOLMC_LV_ROW_LDS=1): measured 1.1-2.4 x slower in every configuration (DESIGN.md "Local
// volatility", profiles/r20_local_vol.jsonl).
#pragma once
#include "olmc_kernels.h"

namespace olmc {

constexpr int kLvMaxNx = 256, kLvMaxNt = 64;      // ollv_surface's caps (olmc.hip refuses anything beyond before a launch)

struct LvModel {
    const float* nodes;          // device [n_t][n_x], row-major
    int32_t n_x, n_t;
    double x_lo, x_scale;        // u = (x - x_lo) x_scale, x_scale = (n_x - 1) / (x_hi - x_lo)
    double t_scale;              // v = (t dt) t_scale,     t_scale = (n_t - 1) / t_hi; 0 when n_t == 1 (one row, no time axis)
    double dt, rq_dt, half_dt;   // T / n, (r - q) dt, dt / 2
    double vol_unit;             // sqrt(dt) kZScale: sigma_t vol_unit multiplies a RAW normal
    double s0, log_s0;
};

extern __shared__ float lv_lds[];                 // [n_t][n_x], the launch's dynamic LDS

__device__ __forceinline__ void lv_table_to_lds(const LvModel& m) {
    const int32_t nodes = m.n_t * m.n_x;
    for (int32_t k = threadIdx.x; k < nodes; k += kBlock) lv_lds[k] = m.nodes[k];
    __syncthreads();
}

// The two rows and the time weight of the date whose step is t (wave-uniform).  With one row both pointers are row 0 and the weight
// is 0: i + 1 is never formed beyond n_t - 1.
struct LvRows {
    const float* r0;
    const float* r1;
    double w_tau;
};
__device__ __forceinline__ LvRows lv_rows(const LvModel& m, int32_t t) {
    const double v = fmin(fmax(static_cast<double>(t) * m.dt * m.t_scale, 0.0), static_cast<double>(m.n_t - 1));
    const int32_t i = __builtin_amdgcn_readfirstlane(max(min(static_cast<int32_t>(v), m.n_t - 2), 0));
    const int32_t i1 = min(i + 1, m.n_t - 1);
    return {lv_lds + i * m.n_x, lv_lds + i1 * m.n_x, v - static_cast<double>(i)};
}

// sigma at x on the date's rows.  fmax(NaN, 0) is 0, so a NaN x reads column 0: no lane forms an index outside [0, n_x - 1].
__device__ __forceinline__ double lv_sigma(const LvModel& m, const LvRows& rw, double x) {
    const double u = fmin(fmax((x - m.x_lo) * m.x_scale, 0.0), static_cast<double>(m.n_x - 1));
    const int32_t j = min(static_cast<int32_t>(u), m.n_x - 2);
    const double w = u - static_cast<double>(j);
    const double a00 = static_cast<double>(rw.r0[j]), a01 = static_cast<double>(rw.r0[j + 1]);
    const double a10 = static_cast<double>(rw.r1[j]), a11 = static_cast<double>(rw.r1[j + 1]);
    const double a0 = a00 + w * (a01 - a00), a1 = a10 + w * (a11 - a10);
    return a0 + rw.w_tau * (a1 - a0);
}

// One step of one leg: x += (r - q - sigma^2 / 2) dt + sigma sqrt(dt) z, z = +-(raw normal) in units of kZScale.
__device__ __forceinline__ double lv_step(const LvModel& m, const LvRows& rw, double x, double z_raw) {
    const double sigma = lv_sigma(m, rw, x);
    return x + __builtin_fma(sigma * m.vol_unit, z_raw, __builtin_fma(-(sigma * sigma), m.half_dt, m.rq_dt));
}

// Steps 0 .. last - 1 of one path for LEGS legs, in jump_walk's shape: normals(b, z) fills the four RAW normals of Philox block b (steps
// 4 b .. 4 b + 3), leg 1 takes -z and walks its own sigma path; `after(t)` sees x after step t.
template <int LEGS, typename Normals, typename After>
__device__ __forceinline__ void lv_walk(const LvModel& m, Normals normals, int32_t last, double (&x)[2], After after) {
    const int32_t blocks = (last + 3) >> 2;
    for (int32_t b = 0; b < blocks; ++b) {
        float z[4];
        normals(b, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t t = 4 * b + j;
            if (t < last) {
                const LvRows rw = lv_rows(m, t);
                const double zj = static_cast<double>(z[j]);
#pragma unroll
                for (int l = 0; l < LEGS; ++l) x[l] = lv_step(m, rw, x[l], l ? -zj : zj);
                after(t);
            }
        }
    }
}

#ifndef OLMC_LV_ROW_LDS
#define OLMC_LV_ROW_LDS 0           // 1 (python tools/local_vol_timing.py --build-row; never the product) swaps lv_price_kernel for the A/B form
#endif
#if OLMC_LV_ROW_LDS
#include "olmc_local_vol_row_kernel.h"
#endif

// ollv_price: one launch, no path stored.  The payoffs, dates and log-space level decisions are heston_path_kernel's (QmcLeg over
// ln(S_t / S), extrema over dates 0 .. n, the Asian mean over dates 1 .. n, the date-0 barrier decision made on the host:
// heston_path_contract); kPathEuropean adds max(+-(S_n - K), 0).  The antithetic leg takes -z and walks its own sigma path.
#if !OLMC_LV_ROW_LDS
template <int FAMILY, bool ANTI>
__global__ __launch_bounds__(kBlock) void lv_price_kernel(PathRange pr, LvModel m, ExtremaContract ec, double inv_steps, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    constexpr double kLog2e = 1.4426950408889634;          // the arithmetic Asian's exp2_f64 counts in log2 units
    lv_table_to_lds(m);
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    double acc[2] = {0.0, 0.0};
    const BlockWalk w = block_walk(pr.n_steps);
    // walk_blocks and the legs written out: under lv_walk's per-date `t < last` every instantiation leaves its register row (93 -> 82,
    // 90 -> 72 VGPRs, ...), and with the legs in one shared struct the plain extrema form left its scalar one (106 -> 95 SGPRs).
    for_each_path(pr, [&](int64_t, uint32_t g_lo, uint32_t g_hi) {
        double x[2] = {0.0, 0.0};
        QmcLeg leg[2];
        int32_t t = 0;
        auto dates = [&](const float (&z)[4], auto live) {
#pragma unroll
            for (int j = 0; j < decltype(live)::value; ++j) {
                const LvRows rw = lv_rows(m, t);
                const double zj = static_cast<double>(z[j]);
#pragma unroll
                for (int l = 0; l < LEGS; ++l) {
                    x[l] = lv_step(m, rw, x[l], l ? -zj : zj);
                    if constexpr (FAMILY == kQmcAsianArithmetic) qmc_leg_add<FAMILY>(leg[l], x[l] * kLog2e);
                    else if constexpr (FAMILY != kPathEuropean) qmc_leg_add<FAMILY>(leg[l], x[l]);
                }
                ++t;
            }
        };
        walk_blocks(w, [&](int32_t b, float (&z)[4]) { raw_normals4_pinned(g_lo, g_hi, static_cast<uint32_t>(b), 0u, rk, z); }, dates);
#pragma unroll
        for (int l = 0; l < LEGS; ++l) {
            double p;
            if constexpr (FAMILY == kPathEuropean) p = fmax(ec.sign * (ec.s0 * exp(x[l]) - ec.strike), 0.0);
            else p = qmc_payoff<FAMILY>(ec, inv_steps, leg[l].a, leg[l].mx, leg[l].mn, x[l]);
            acc[0] += p; acc[1] += p * p;
        }
    });
    block_then_grid_reduce<2>(acc, ws);
}

#endif

// ollv_paths: the matrix S exp(x_t), t = 0 .. n, in lsm_paths_kernel's layouts; date 0 is S itself.  The draws come from the scalar keys.
template <bool PATH_MAJOR>
__global__ __launch_bounds__(kBlock) void lv_paths_kernel(PathRange pr, LvModel m, double* __restrict__ paths) {
    lv_table_to_lds(m);
    for_each_path(pr, [&](int64_t i, uint32_t g_lo, uint32_t g_hi) {
        double x[2] = {0.0, 0.0};
        paths[path_at<PATH_MAJOR>(i, 0, pr.count, pr.n_steps)] = m.s0;
        lv_walk<1>(m, [&](int32_t b, float (&z)[4]) { raw_normals4(g_lo, g_hi, static_cast<uint32_t>(b), 0u, pr.key0, pr.key1, z); }, pr.n_steps, x,
                   [&](int32_t t) { paths[path_at<PATH_MAJOR>(i, t + 1, pr.count, pr.n_steps)] = m.s0 * exp(x[0]); });
    });
}

// ollv_surface_prices: heston_surface_kernel's prologue, wave-uniform path loop, cell rows and read-out (surface_rows,
// for_each_wave_path, SurfaceRows) on these paths; the walk ends at the last cell's step.  The read-out forms a date's spot as
// exp(ln S + x) (its mu_dt term is 0 here).
template <bool ANTI>
__global__ __launch_bounds__(kBlock) void lv_surface_kernel(PathRange pr, LvModel m, double sign, HestonSurfaceCells cells, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    lv_table_to_lds(m);
    const SurfaceRows rows = surface_rows(cells);
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    for_each_wave_path(pr, [&](bool live, PathWords pw) {
        double x[2] = {0.0, 0.0};
        int32_t next = 0, pending = cells.step[0];
        lv_walk<LEGS>(m, [&](int32_t b, float (&z)[4]) { raw_normals4_pinned(pw.lo, pw.hi, static_cast<uint32_t>(b), 0u, rk, z); }, cells.last, x,
                      [&](int32_t t) {
                          const double ls[2] = {m.log_s0 + x[0], m.log_s0 + x[1]};
                          rows.read_out<LEGS>(next, pending, t + 1, 0.0, sign, ls, live);
                      });
    });
    rows.reduce(ws);
}

}  // namespace olmc
