// olmc_jump_kernels.h -- device side of include/olmc_jump.h: path-dependent payoffs, a surface of Europeans, the autocallable and the
// cliquet on Merton / Kou jump-diffusion paths, one launch each, no path stored.
//
// Stream: olmc_jump_paths' as it stands (olmc_kernels.h "Jump diffusion").  Block (path, b, kTagJump) feeds steps 2b and 2b + 1: words
// 0, 1 -> box_muller_raw -> the two diffusion normals, words 2, 3 -> the two Poisson uniforms; the count of a step by inversion from
// p0 = exp(-lambda dt), at most 64 jumps; the sizes from blocks (path, t, kTagJumpSize + j / 2), drawn only by the lanes that jump.  A
// step of a leg is
//     ls += fma(vol, z, drift);   then   ls += term_j   for each size term, in order
// where Merton has ONE term (n mu_j + sigma_j sqrt(n) z_jump: the sum of n iid normals) and Kou one term per jump.  The build runs with
// -ffp-contract=off, so this order of additions is the definition: leg 0 of every kernel here takes jump_paths_kernel's increments.
//
// The mirror leg (the project's own definition; antithetic = 1 prices both legs of every path, n = 2 N samples):
//   - leg 1 takes -z_t for the diffusion normal of every step: ls1 += fma(-vol, z, drift);
//   - leg 1 takes THE SAME jump count and THE SAME jump sizes as leg 0: the Poisson uniform and the size blocks are drawn once per path
//     and step, inside the divergent branch, and each size term is then added to both legs, leg 0 first, in the same order.
// So only the diffusion is mirrored: the pair's jump component is common (and its variance is not reduced), the pair's diffusion
// components cancel to first order.
//
// State: ls relative to ln S (it starts at 0; date 0 is S itself), fp64, in registers, a lane per path and its mirror; no barrier inside
// a step loop; only (sum x, sum x^2) rows leave a kernel, through block_then_grid_reduce / SurfaceRows.  jump_legs_paths_kernel alone
// carries ln S itself, as jump_paths_kernel does, so that its mirror = 0 matrix has that kernel's bits.
//
// Divergence: at lambda dt ~ 1e-3 the size branch is taken by a lane in a thousand; at lambda dt ~ 3 by nearly every lane, and the wave
// walks the longest count of its 64 lanes (Kou: one Philox block per two jumps and one fp64 log per jump; Merton: one block and one
// square root whatever the count).  The branch holds no cross-lane operation; the surface kernel's folds sit after the reconvergence.
#pragma once
#include "olmc_kernels.h"

namespace olmc {

// The path's Philox blocks with the launch's round keys pinned in VGPRs (pin_round_keys), as the other path kernels draw theirs: the words
// jump_kernel draws from the scalar keys.
struct JumpWords {
    uint32_t g_lo, g_hi;
    const RoundKeys& rk;
    __device__ __forceinline__ Words4 operator()(uint32_t block, uint32_t tag) const { return philox4x32_10_pinned(g_lo, g_hi, block, tag, rk); }
};

// oljd_price: the payoffs, dates and log-space level decisions of heston_path_kernel / lv_price_kernel (QmcLeg over x_t = ln(S_t / S),
// extrema over dates 0 .. n, the Asian mean over dates 1 .. n with one fp64 exponential per date and leg for the arithmetic one, the
// date-0 barrier decision made on the host: heston_path_contract); kPathEuropean adds max(+-(S_n - K), 0).
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS 64 B, the reduction), VGPRs plain / antithetic:
// arithmetic 110 / 97, geometric 108 / 97, extrema 111 / 117, European 106 / 92 (jump_kernel: 86, with its keys in scalar registers; the
// twenty pinned round keys are the difference).  No instantiation passes 128: by registers (granule 8, 512 per lane) every one admits
// four waves per SIMD and the antithetic European (96 allocated) five.
template <int FAMILY, bool ANTI>
__global__ __launch_bounds__(kBlock) void jump_path_kernel(PathRange pr, JumpContract c, ExtremaContract ec, double inv_steps, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    constexpr double kLog2e = 1.4426950408889634;          // the arithmetic Asian's exp2_f64 counts in log2 units
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    const double vol = c.vol * kZScale;
    double acc[2] = {0.0, 0.0};
    // The legs written out per family: held in one shared struct the antithetic Asian forms took 96 VGPRs for 97 and left their row.
    for_each_path(pr, [&](int64_t, uint32_t g_lo, uint32_t g_hi) {
        double x[2] = {0.0, 0.0};
        QmcLeg leg[2];
        jump_walk<LEGS>(c, JumpWords{g_lo, g_hi, rk}, vol, pr.n_steps, x, [&](int32_t) {
#pragma unroll
            for (int l = 0; l < LEGS; ++l) {
                if constexpr (FAMILY == kQmcAsianArithmetic) qmc_leg_add<FAMILY>(leg[l], x[l] * kLog2e);
                else if constexpr (FAMILY != kPathEuropean) qmc_leg_add<FAMILY>(leg[l], x[l]);
            }
        });
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

// oljd_surface_prices: heston_surface_kernel's prologue, wave-uniform path loop, cell rows and read-out (surface_rows,
// for_each_wave_path, SurfaceRows) on these paths; the walk ends at the last cell's step.  The read-out forms a date's spot as
// exp(ln S + x) (its mu_dt term is 0 here).
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS 3.2 KiB), VGPRs plain / antithetic: 101 / 88
// (lv_surface_kernel's skeleton; heston_surface_kernel: 92 / 82).
template <bool ANTI>
__global__ __launch_bounds__(kBlock) void jump_surface_kernel(PathRange pr, JumpContract c, HestonSurfaceCells cells, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    const SurfaceRows rows = surface_rows(cells);
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    const double vol = c.vol * kZScale;
    for_each_wave_path(pr, [&](bool live, PathWords pw) {
        double x[2] = {0.0, 0.0};
        int32_t next = 0, pending = cells.step[0];
        jump_walk<LEGS>(c, JumpWords{pw.lo, pw.hi, rk}, vol, cells.last, x, [&](int32_t t) {
            const double ls[2] = {c.log_s0 + x[0], c.log_s0 + x[1]};
            rows.read_out<LEGS>(next, pending, t + 1, 0.0, c.sign, ls, live);
        });
    });
    rows.reduce(ws);
}

// oljd_autocallable / oljd_cliquet: HestonAutocall / HestonCliquet as they stand, per-date policies on x_t = ln(S_t / S).  The walk
// ends at Product::last: the cliquet's trailing dates are not drawn.
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS 64 B, the reduction), VGPRs plain / antithetic:
// autocallable 116 / 124, cliquet 110 / 101 (heston_product_kernel: 116 / 124 and 104 / 98).  None passes 128.
template <template <bool> class Product, bool ANTI>
__global__ __launch_bounds__(kBlock) void jump_product_kernel(PathRange pr, JumpContract c, typename Product<ANTI>::Contract pc, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    const double vol = c.vol * kZScale;
    const int32_t last = Product<ANTI>::last(pc, pr.n_steps);
    double acc[2] = {0.0, 0.0};
    for_each_path(pr, [&](int64_t, uint32_t g_lo, uint32_t g_hi) {
        double x[2] = {0.0, 0.0};
        Product<ANTI> p;
        p.start(pc);
        jump_walk<LEGS>(c, JumpWords{g_lo, g_hi, rk}, vol, last, x, [&](int32_t) { p.date(pc, x); });
        p.payoffs(pc, x, acc);
    });
    block_then_grid_reduce<2>(acc, ws);
}

// oljd_paths: the matrix of ONE leg (layouts: path_at), date 0 = S as given.  ln S itself is carried, as in jump_paths_kernel: with
// mirror = 0 every word is that kernel's; with mirror = 1 the diffusion term of every step is fma(-vol, z, drift).
template <bool PATH_MAJOR>
__global__ __launch_bounds__(kBlock) void jump_legs_paths_kernel(PathRange pr, JumpContract c, double s_first, int32_t mirror, double* __restrict__ out) {
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    const double vol = mirror ? -(c.vol * kZScale) : c.vol * kZScale;
    for_each_path(pr, [&](int64_t i, uint32_t g_lo, uint32_t g_hi) {
        double ls[2] = {c.log_s0, 0.0};
        out[path_at<PATH_MAJOR>(i, 0, pr.count, pr.n_steps)] = s_first;
        jump_walk<1>(c, JumpWords{g_lo, g_hi, rk}, vol, pr.n_steps, ls,
                     [&](int32_t t) { out[path_at<PATH_MAJOR>(i, t + 1, pr.count, pr.n_steps)] = exp(ls[0]); });
    });
}

}  // namespace olmc
