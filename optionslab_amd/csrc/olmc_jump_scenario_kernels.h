// olmc_jump_scenario_kernels.h -- device side of include/olmc_jump_scenarios.h: European payoffs under up to 16 parameter sets on ONE
// walk over olmc_jump_paths' draws of a path, one launch, no path stored.
//
// The fold (the header's definition): with constant sigma the diffusion part of a path's terminal log-return is vol_i * Z, Z = the sum of
// its raw Box-Muller normals in step order, whatever (S, K, r, q, sigma, T, call / put) the contract has; the jump part J depends on
// (model, lambda, T, a1, a2, a3) alone.  So a lane carries ONE Z and one J per JUMP GROUP (olmc_host_math.h: jump_scenario_set) in
// registers, walks the path's blocks once (for_each_wave_path's wave-uniform trips, the round keys pinned as JumpWords pins them), and
// after the walk every contract forms x = fma(vol, +-Z, n drift) + J of its group, one exponential per leg and per distinct (group,
// ln S, vol, n drift) -- the host sorts the contracts by group and then by those three and flags the slots that open a new spot
// (JumpScenarioSet::fresh), as HestonScenarioSet does.  The one-contract kernels interleave the same terms in one running sum: sums
// to rounding, not to the bit.
//
// Stream: olmc_jump_kernels.h's as it stands.  Block (path, b, kTagJump): words 0, 1 -> box_muller_raw -> the normals of steps 2b and
// 2b + 1, words 2, 3 -> their Poisson uniforms.  A group's count at a step comes by jump_sizes' inversion of the step's ONE uniform
// against the group's own p0 and lambda dt.  THE SIZE DRAWS ARE SHARED: the block of (path, t, tag) is a pure function, so Merton's z'
// of a step is drawn once if any Merton group of the lane jumps, and Kou's jump j takes its two uniforms and log(um) once, for j up to
// the lane's largest Kou count; each group with n_g > j then adds its own term, the value jump_sizes would have added for it alone.
//
// GROUP_BOUND is the compile-time length of J: the group loops are unrolled over it and a slot beyond the launch's n_groups is skipped
// by a scalar branch, so no J (and no count) is ever indexed dynamically and nothing goes to scratch.  A group's arithmetic does not
// depend on its number, on how many are in use or on the bound.  The group constants and the contract slots live in LDS (copied from the
// kernarg segment by vector loads, scenario_rows' way: 16 groups of constants do not fit the scalar registers beside the kernel's own);
// the step loop reads a group's p0 through an offset the optimiser cannot see through (opaque_zero), or it hoists 16 of them into vector
// registers.  The common step -- no group jumps, u < p0_floor -- costs one compare.  The step loop holds no barrier and no cross-lane
// operation; the read-out folds over the wave after the walk (wave_sum: fixed order) and lane 0 adds into the wave's LDS row, as in
// SurfaceRows.  A TRIP of the workgroup then ends with the four wave rows added in wave order (SurfaceRows::reduce's sum) onto the
// workgroup's running row, which leaves through grid_reduce_workgroup<2 * 16>: a workgroup's row is the sequence of its trips' rows
// added in trip order, so under OLMC_TUNE_GRID_CAP = 1 a launch of up to eight trips (2048 paths: grid_reduce_workgroup adds up to
// eight workgroup rows in index order) gives the uncapped launch's bits; elsewhere a capped launch's sums are the uncapped ones to the
// reassociation of an fp64 sum, as for every path kernel.  Uncapped, a workgroup takes a second trip only beyond 2^26 paths.
//
// Divergence: at lambda dt ~ 1e-3 a lane in a thousand enters the size branch; at lambda dt ~ 5 every lane does, and the wave walks the
// largest Kou count of its 64 lanes over all groups (one Philox block per two jumps and one fp64 log per jump, WHATEVER the number of
// groups: the terms themselves are a compare, a select and a multiply-add per group that still jumps).
//
// Resources (tools/kernel_meta.sh, gfx950; no scratch, no spills; LDS 4.6 KiB: the wave rows, the set and the workgroup reduction),
// VGPRs plain / antithetic by GROUP_BOUND: 2 (the Greeks): 113 / 95, 4: 119 / 101, 16: 156 / 139 (jump_path_kernel's European: 106 / 92).
// By registers (granule 8, 512 per lane) bounds 2 and 4 admit four waves per SIMD (the antithetic forms five and four), jump_path_kernel's
// row; bound 16 admits three: its 16 sums and 16 counts are 48 registers beside the Philox block and the 20 pinned round keys.  Bounds
// between 4 and 16 are not instantiated: each is two more code objects, and none has been measured.
#pragma once
#include "olmc_jump_kernels.h"

namespace olmc {

static_assert(sizeof(JumpScenarioSet) % 4 == 0 && sizeof(JumpScenarioSet) / 4 <= 2 * kBlock, "two dwords of the set per thread at most");
static_assert(kJumpGroups == kSurfaceCells, "a launch of OLMC_MAX_BATCH scenarios has at most as many groups");

struct JumpScenarioRows {
    double (*stage)[2 * kSurfaceCells];          // LDS [kWavesPerBlock][2 kSurfaceCells]
    JumpScenarioSet* lds;                        // LDS: the launch's set
    int lane, wave;
    // Call first in the kernel, whose first argument is the set.
    __device__ __forceinline__ void clear() const {
        if (lane < 2 * kSurfaceCells) stage[wave][lane] = 0.0;
        const uint32_t* arg = (const uint32_t*)__builtin_amdgcn_kernarg_segment_ptr();
        for (uint32_t d = threadIdx.x; d < sizeof(JumpScenarioSet) / 4; d += kBlock) reinterpret_cast<uint32_t*>(lds)[d] = arg[d];
        __syncthreads();
    }
    // The jump part of step t for every group in use, given the step's Poisson uniform: jump_sizes' count per group, then the size
    // terms from draws made once per lane.  n_groups, kou_mask and p0_floor are the launch's scalars.
    template <int GROUP_BOUND>
    __device__ __forceinline__ void jumps(const JumpWords& words, int32_t t, double u, int32_t n_groups, int32_t kou_mask, double p0_floor,
                                          double (&J)[GROUP_BOUND]) const {
        if (u < p0_floor) return;                          // no group jumps (almost always)
        const double (*cst)[6] = lds->grp + opaque_zero();
        int32_t cnt[GROUP_BOUND], kou_most = 0;
        bool merton = false;
#pragma unroll
        for (int g = 0; g < GROUP_BOUND; ++g) {
            cnt[g] = 0;
            if (g < n_groups) {
                const double p0 = cst[g][kJsP0], lam_dt = cst[g][kJsLamDt];
                if (!(u < p0)) {
                    int32_t n = 1;
                    double pk = p0 * lam_dt, cdf = p0 + pk;
                    while (u >= cdf && n < 64) {
                        ++n;
                        pk *= lam_dt / n;
                        cdf += pk;
                    }
                    cnt[g] = n;
                    if ((kou_mask >> g) & 1) kou_most = n > kou_most ? n : kou_most;
                    else merton = true;
                }
            }
        }
        if (merton) {
            const Words4 k = words(static_cast<uint32_t>(t), kTagJumpSize);
            float z_jump, unused;
            box_muller_raw(k.x0, k.x1, z_jump, unused);
            const double z = kZScale * static_cast<double>(z_jump);
#pragma unroll
            for (int g = 0; g < GROUP_BOUND; ++g) {
                if (g < n_groups && !((kou_mask >> g) & 1)) {
                    const int32_t n = cnt[g];
                    if (n > 0) J[g] += n * cst[g][kJsC1] + cst[g][kJsC2] * sqrt(static_cast<double>(n)) * z;
                }
            }
        }
        Words4 k{};
        for (int32_t j = 0; j < kou_most; ++j) {
            if (!(j & 1)) k = words(static_cast<uint32_t>(t), kTagJumpSize + static_cast<uint32_t>(j >> 1));
            const double ud = unit_open64((j & 1) ? k.x2 : k.x0), um = unit_open64((j & 1) ? k.x3 : k.x1);
            const double log_um = log(um);
#pragma unroll
            for (int g = 0; g < GROUP_BOUND; ++g) {
                if (g < n_groups && ((kou_mask >> g) & 1)) {
                    if (cnt[g] > j) J[g] += ud < cst[g][kJsC1] ? -log_um * cst[g][kJsC2] : log_um * cst[g][kJsC3];
                }
            }
        }
    }
    // The contracts of a block of 64 paths whose walk is done.  Call with all 64 lanes.
    template <int GROUP_BOUND, int LEGS>
    __device__ __forceinline__ void read_out(double Z, const double (&J)[GROUP_BOUND], bool live) const {
        int32_t j = 0;
#pragma unroll
        for (int g = 0; g < GROUP_BOUND; ++g) {
            const int32_t end = __builtin_amdgcn_readfirstlane(lds->end[g]);
            double s[LEGS] = {};
            for (; j < end; j = __builtin_amdgcn_readfirstlane(j + 1)) {
                const double strike = lds->slot[j][kJsStrike], sign = lds->slot[j][kJsSign];
                if (__builtin_amdgcn_readfirstlane(lds->fresh[j])) {
                    const double log_s = lds->slot[j][kJsLogS], vol = lds->slot[j][kJsVol], n_drift = lds->slot[j][kJsNDrift];
                    s[0] = exp(log_s + (__builtin_fma(vol, Z, n_drift) + J[g]));
                    if constexpr (LEGS == 2) s[1] = exp(log_s + (__builtin_fma(-vol, Z, n_drift) + J[g]));
                }
                double sum = 0.0, sumsq = 0.0;
#pragma unroll
                for (int leg = 0; leg < LEGS; ++leg) {
                    const double x = live ? fmax(sign * (s[leg] - strike), 0.0) : 0.0;
                    sum += x;
                    sumsq += x * x;
                }
                const double wave_total = wave_sum(sum), wave_total_sq = wave_sum(sumsq);       // valid in lane 0
                if (lane == 0) { stage[wave][2 * j] += wave_total; stage[wave][2 * j + 1] += wave_total_sq; }
            }
        }
    }
    // A trip of the workgroup is done (all waves): its four wave rows, added in wave order as SurfaceRows::reduce adds them, onto the
    // workgroup's running row, and the wave rows cleared for the next trip.
    __device__ __forceinline__ void fold_trip(double& row) const {
        __syncthreads();
        if (threadIdx.x < 2 * kSurfaceCells) {
            double trip = stage[0][threadIdx.x];
#pragma unroll
            for (int k = 1; k < kWavesPerBlock; ++k) trip += stage[k][threadIdx.x];
            row += trip;
        }
        __syncthreads();
        if (lane < 2 * kSurfaceCells) stage[wave][lane] = 0.0;
    }
};

// The prologue (scenario_rows for this set): the rows and the set in LDS, cleared and copied.  Call first in the kernel.
__device__ __forceinline__ JumpScenarioRows jump_scenario_rows() {
    __shared__ double stage[kWavesPerBlock][2 * kSurfaceCells];
    __shared__ JumpScenarioSet lds;
    const JumpScenarioRows rows{stage, &lds, static_cast<int>(threadIdx.x) & (kWave - 1),
                                __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave)};
    rows.clear();
    return rows;
}

template <int GROUP_BOUND, bool ANTI>
__global__ __launch_bounds__(kBlock) void jump_scenarios_kernel(JumpScenarioSet set, PathRange pr, ReduceWs ws) {
    constexpr int LEGS = ANTI ? 2 : 1;
    const JumpScenarioRows rows = jump_scenario_rows();
    const RoundKeys rk = pin_round_keys(pr.key0, pr.key1);
    const int32_t blocks = (pr.n_steps + 1) >> 1;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    double row = 0.0;                                      // threads < 2 kSurfaceCells: the workgroup's sums over its trips, trip by trip
    // for_each_wave_path's trips with the workgroup kept together: a wave without a path in the workgroup's last trip skips the walk and
    // meets the others at the fold.
    for (int64_t b0 = static_cast<int64_t>(blockIdx.x) * kBlock; b0 < pr.count; b0 += stride) {      // workgroup-uniform
        const int64_t w0 = b0 + rows.wave * kWave;
        if (w0 < pr.count) {                                                                         // wave-uniform
            const int64_t i = w0 + rows.lane;
            const bool live = i < pr.count;
            const PathWords pw = path_words(pr, live ? i : 0);
            const JumpWords words{pw.lo, pw.hi, rk};
            double Z = 0.0, J[GROUP_BOUND];
#pragma unroll
            for (int g = 0; g < GROUP_BOUND; ++g) J[g] = 0.0;
            for (int32_t b = 0; b < blocks; ++b) {
                const Words4 w = words(static_cast<uint32_t>(b), kTagJump);
                float z[2];
                box_muller_raw(w.x0, w.x1, z[0], z[1]);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int32_t t = 2 * b + h;
                    if (t < pr.n_steps) {
                        Z += static_cast<double>(z[h]);
                        rows.jumps<GROUP_BOUND>(words, t, unit_open64(h ? w.x3 : w.x2), set.n_groups, set.kou_mask, set.p0_floor, J);
                    }
                }
            }
            rows.read_out<GROUP_BOUND, LEGS>(Z, J, live);
        }
        rows.fold_trip(row);
    }
    grid_reduce_workgroup<2 * kSurfaceCells>(row, ws);
}

}  // namespace olmc
