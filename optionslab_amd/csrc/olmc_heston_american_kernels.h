// olmc_heston_american_kernels.h -- device side of include/olha.h: the Longstaff-Schwartz step chain of an American option under Heston,
// regressing on the date's state (S_t, v_t).  Included by olmc.hip after olmc_kernels.h, whose pieces it reuses as they are: the
// time-major path matrices of the four Heston path kernels, LsmContract (strike, sign, discount, n_steps), lsm_intrinsic, lane_bcast,
// workgroup_rows_sum, block_row_sum and block_then_grid_reduce.
//
// The chain has lsm_step_kernel's form: ONE launch per exercise date t_fit = n - 1 .. 0, stream order the only synchronisation.  A
// launch stores its workgroups' regression sums as rows (plain stores: the kernel boundary publishes them); every workgroup of the next
// launch sums those rows in index order, solves the normal equations in its first wave and hands the coefficients to its threads
// through LDS.  Only the last launch (t_fit == 0: the moments of the time-0 cash flows) goes through block_then_grid_reduce.
//
// THE BASIS.  All monomials x^a y^b with a + b <= D in graded order 1, x, y, x^2, xy, y^2, x^3, x^2 y, x y^2, y^3: monomial (a, b) has
// index ha_index(a, b) = s (s + 1) / 2 + b with s = a + b.  x = (S_t / K - cx_t) / wx_t and y = (v_t - cy_t) / wy_t are standardised
// on the host per date (olmc.hip heston_lsm_scales: any finite positive pair gives the same fit in exact arithmetic, these keep the
// moment matrix's condition number at 1e2 .. 4e5).  A date needs the moments sum x^a y^b for a + b <= 2 D (the same graded index), the
// right-hand sides sum x^a y^b cf for a + b <= D and the in-the-money count: 10, 22 and 39 sums for D = 1, 2, 3.  The kernels are
// templated on D, so that the default degree 2 carries 22 sums in registers and in the rows every workgroup re-reads, not 39.
#pragma once
#include "olmc_kernels.h"

namespace olmc {

constexpr int kHaMaxDegree = 3;

constexpr int ha_index(int a, int b) { return (a + b) * (a + b + 1) / 2 + b; }
constexpr int ha_grade(int k) { return k < 1 ? 0 : k < 3 ? 1 : k < 6 ? 2 : k < 10 ? 3 : k < 15 ? 4 : k < 21 ? 5 : 6; }
constexpr int ha_b(int k) { return k - ha_grade(k) * (ha_grade(k) + 1) / 2; }
constexpr int ha_a(int k) { return ha_grade(k) - ha_b(k); }

template <int D>
struct HaBasis {
    static_assert(D >= 1 && D <= kHaMaxDegree, "total degree 1 .. 3");
    static constexpr int NU = (D + 1) * (D + 2) / 2;               // unknowns: 3, 6, 10
    static constexpr int NM = (2 * D + 1) * (2 * D + 2) / 2;       // moments: 6, 15, 28
    static constexpr int NV = NM + NU + 1;                         // + the in-the-money count: 10, 22, 39
};

struct HaScale {                    // the regressors of the date being FITTED and of the date whose fit is APPLIED: (centre, 1 / width) of x and of y
    double fit_cx, fit_iwx, fit_cy, fit_iwy;
    double prev_cx, prev_iwx, prev_cy, prev_iwy;
};

template <int D>
struct HaCoeffs {
    double beta[HaBasis<D>::NU];
    int32_t valid;                  // the regression at the date being finished was fitted
    int32_t pad;
};

// Runs in the wave that holds the grid totals of one exercise date (all 64 lanes active): lane k < NV has sum k of the row.  The wave
// solves the NU x NU normal equations in fp64 by elimination in the natural order (the Cholesky order: the moment matrix of the
// standardised regressors is symmetric positive definite with a modest condition number) and leaves the coefficients in `coef`.
//
// LsmFit keeps its 5 x 6 matrix one ELEMENT per lane; 10 x 11 does not fit 64 lanes.  Here lane r < NU holds ROW r of the augmented
// matrix in NU + 1 registers, every column index a compile-time constant of a fully unrolled loop: an elimination step is one
// broadcast of the pivot row from a compile-time lane (v_readlane) and one multiply-subtract per remaining column, back-substitution
// runs on broadcast values.  No private memory: nothing is indexed by a run-time value.
// The pin rule is LsmFit's: a pivot not above 1e-11 of its own diagonal moment pins that unknown to zero (its row and column become
// the identity, the others are still fitted) -- sigma_v = 0 with v0 = theta makes every y column exactly zero, and the fit is then the
// one-factor fit in x.
template <int D>
__device__ __forceinline__ void ha_fit(HaCoeffs<D>* coef, double total) {
    using B = HaBasis<D>;
    constexpr int NU = B::NU;
    const int lane = threadIdx.x & (kWave - 1);
    const int r = lane < NU ? lane : 0;                           // lanes beyond the matrix repeat row 0: computed, never read
    const int g = r < 1 ? 0 : r < 3 ? 1 : r < 6 ? 2 : 3;
    const int rb = r - g * (g + 1) / 2, ra = g - rb;
    double a[NU + 1];                                             // a[c] = sum of monomial r x monomial c, a[NU] = sum of monomial r x cf
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        const int s = ra + rb + ha_a(c) + ha_b(c);
        a[c] = __shfl(total, s * (s + 1) / 2 + rb + ha_b(c), kWave);
    }
    a[NU] = __shfl(total, B::NM + r, kWave);
    const bool ok = lane_bcast(total, B::NV - 1) > static_cast<double>(NU);       // fitted when the in-the-money count exceeds the unknowns
#pragma unroll
    for (int k = 0; k < NU; ++k) {
        double p = lane_bcast(a[k], k);
        const bool pin = !(fabs(p) > 1e-11 * fabs(lane_bcast(total, ha_index(2 * ha_a(k), 2 * ha_b(k)))));      // wave-uniform
        if (pin) {
            if (lane == k) {
#pragma unroll
                for (int c = 0; c <= NU; ++c) a[c] = c == k ? 1.0 : 0.0;
            } else {
                a[k] = 0.0;
            }
            p = 1.0;
        }
        const double f = a[k] * (1.0 / p);
#pragma unroll
        for (int c = k + 1; c <= NU; ++c) {
            const double pr = lane_bcast(a[c], k);
            if (lane > k) a[c] -= f * pr;
        }
    }
    double beta[NU];
#pragma unroll
    for (int k = NU - 1; k >= 0; --k) {
        double v = lane_bcast(a[NU], k);
#pragma unroll
        for (int j = k + 1; j < NU; ++j) v -= lane_bcast(a[j], k) * beta[j];
        beta[k] = v / lane_bcast(a[k], k);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NU; ++k) coef->beta[k] = ok ? beta[k] : 0.0;
        coef->valid = ok ? 1 : 0;
    }
}

// One exercise date for this thread's paths, in lsm_date's structure: a thread issues the loads of U of its paths (5 U doubles: S and v
// of the later date, the cash flow, S and v of the fitted date) before it touches any of them, consumes its paths in ascending order --
// so the per-thread sums, and the bits of the price, do not depend on U -- and calls `fit()` once while the first loads are in flight.
// A date is 40 bytes read and 8 written per path (lsm_date: 24 and 8).
template <int D, int U, bool INIT, bool FINAL, typename Fit>
__device__ __forceinline__ void ha_date(int64_t n, const LsmContract& c, const HaScale& sc, Fit fit, int32_t t_fit, const double* __restrict__ spot,
                                        const double* __restrict__ var, double* __restrict__ cash, double (&acc)[HaBasis<D>::NV]) {
    using B = HaBasis<D>;
#pragma unroll
    for (int k = 0; k < B::NV; ++k) acc[k] = 0.0;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    const size_t later = static_cast<size_t>(INIT ? c.n_steps : t_fit + 1) * n, fitted_row = static_cast<size_t>(t_fit) * n;
    const double* __restrict__ s_row1 = spot + later;
    const double* __restrict__ v_row1 = var + later;
    const double* __restrict__ s_row0 = spot + fitted_row;
    const double* __restrict__ v_row0 = var + fitted_row;
    HaCoeffs<D> prev;
    bool fitted = false;
    int64_t i0 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    do {                                                // at least one trip: every thread of the workgroup meets the barriers inside fit()
        double cfv[U], s1v[U], v1v[U], s0v[U], v0v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            const bool in = i < n;
            s1v[u] = in ? s_row1[i] : 0.0;
            v1v[u] = (in && !INIT) ? v_row1[i] : 0.0;
            cfv[u] = (in && !INIT) ? cash[i] : 0.0;
            s0v[u] = (in && !FINAL) ? s_row0[i] : 0.0;
            v0v[u] = (in && !FINAL) ? v_row0[i] : 0.0;
        }
        if (!fitted) { prev = fit(); fitted = true; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n) {
                double cf;
                if constexpr (INIT) {
                    cf = lsm_intrinsic(c, s1v[u]);
                } else {
                    cf = cfv[u];
                    const double iv = lsm_intrinsic(c, s1v[u]);
                    if (prev.valid && iv > 0.0) {
                        const double x = (s1v[u] * c.inv_strike - sc.prev_cx) * sc.prev_iwx;
                        const double y = (v1v[u] - sc.prev_cy) * sc.prev_iwy;
                        double xp[D + 1], yp[D + 1];
                        xp[0] = 1.0;
                        yp[0] = 1.0;
#pragma unroll
                        for (int m = 1; m <= D; ++m) {
                            xp[m] = xp[m - 1] * x;
                            yp[m] = yp[m - 1] * y;
                        }
                        double cont = prev.beta[0];
#pragma unroll
                        for (int k = 1; k < B::NU; ++k) cont += prev.beta[k] * (xp[ha_a(k)] * yp[ha_b(k)]);
                        if (iv > cont) cf = iv;
                    }
                }
                cf *= c.discount;
                cash[i] = cf;
                if constexpr (!FINAL) {
                    const bool itm = lsm_intrinsic(c, s0v[u]) > 0.0;
                    const double x = (s0v[u] * c.inv_strike - sc.fit_cx) * sc.fit_iwx;
                    const double y = (v0v[u] - sc.fit_cy) * sc.fit_iwy;
                    const double w = itm ? cf : 0.0;
                    double xp[2 * D + 1], yp[2 * D + 1];
                    xp[0] = itm ? 1.0 : 0.0;                    // out-of-the-money paths add exact zeros (x and y are finite)
                    yp[0] = 1.0;
#pragma unroll
                    for (int m = 1; m <= 2 * D; ++m) {
                        xp[m] = xp[m - 1] * x;
                        yp[m] = yp[m - 1] * y;
                    }
#pragma unroll
                    for (int s = 0; s <= 2 * D; ++s) {
#pragma unroll
                        for (int b = 0; b <= s; ++b) {
                            const double mono = xp[s - b] * yp[b];
                            acc[ha_index(s - b, b)] += mono;
                            if (s <= D) acc[B::NM + ha_index(s - b, b)] += mono * w;
                        }
                    }
                    acc[B::NV - 1] += itm ? 1.0 : 0.0;          // in-the-money count
                } else {
                    acc[0] += cf;                     // final date (t_fit == 0): moments of the time-0 cash flow
                    acc[1] += cf * cf;
                }
            }
        }
        i0 += stride * U;
    } while (i0 < n);
}

// INIT: the cash flow starts as the terminal intrinsic value (first launch); FINAL: t_fit == 0, the launch that leaves {sum, sumsq} of
// the time-0 cash flows for the host through the grid reduction.  The rows alternate between two buffers by date parity, as
// lsm_step_kernel's: a workgroup of date t may store its row while a slower one still reads date t + 1's.
// Resources (the compiler's resource-usage report, gfx950; no scratch, no spills in any of the 48 instantiations), VGPRs at U = 1 / 8 of
// the middle launches (tools/kernel_meta.sh): D = 1 84 / 167, D = 2 113 / 195, D = 3 164 / 247 (lsm_step_kernel: 101 / 157); one
// workgroup per CU, so one wave per SIMD whatever the count.
template <int D, int U, bool INIT, bool FINAL>
__global__ __launch_bounds__(kBlock) void heston_lsm_step_kernel(int64_t n, LsmContract c, HaScale sc, double* __restrict__ rows /* [2][gridDim.x][NV] */,
                                                                 int32_t t_fit, const double* __restrict__ spot, const double* __restrict__ var,
                                                                 double* __restrict__ cash, ReduceWs ws) {
    using B = HaBasis<D>;
    __shared__ double part[kBlock];
    __shared__ HaCoeffs<D> shared_fit;
    const size_t buffer = static_cast<size_t>(gridDim.x) * B::NV;
    const double* rows_prev = rows + static_cast<size_t>((t_fit + 1) & 1) * buffer;
    auto fit = [&]() -> HaCoeffs<D> {
        HaCoeffs<D> f;
        f.valid = 0;
        if constexpr (!INIT) {
            const double total = workgroup_rows_sum<B::NV>(rows_prev, static_cast<int32_t>(gridDim.x), part);
            if (threadIdx.x < kWave) ha_fit<D>(&shared_fit, total);
            __syncthreads();
            f = shared_fit;
        }
        return f;
    };
    double acc[B::NV];
    ha_date<D, U, INIT, FINAL>(n, c, sc, fit, t_fit, spot, var, cash, acc);
    if constexpr (!FINAL) {
        const double s = block_row_sum<B::NV>(acc);
        if (threadIdx.x < B::NV) rows[static_cast<size_t>(t_fit & 1) * buffer + static_cast<size_t>(blockIdx.x) * B::NV + threadIdx.x] = s;
    } else {
        const double moments[2] = {acc[0], acc[1]};
        block_then_grid_reduce<2>(moments, ws);
    }
}

}  // namespace olmc
