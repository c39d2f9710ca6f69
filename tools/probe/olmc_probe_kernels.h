// olmc_probe_kernels.h -- measurement and validation kernels of the INSTRUMENTED build (libolmc_probe.so).  Nothing here is compiled
// into libolmc.so.  They use the product's own device functions (olmc_kernels.h), so what they measure is the product's code.
#pragma once
#include "olmc_kernels.h"
#include "olmc_heston_american_kernels.h"

namespace olmc {

// Power sums of the normal stream (validation tap): out[m-1] = sum over paths and steps of z^m, m = 1..4,
// z = kZScale * z' in fp64.  At 2^36 normals the second moment is resolved to 5e-6: a bias hunt.
__global__ __launch_bounds__(kBlock) void normal_moments_kernel(PathRange pr, ReduceWs ws) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int32_t blocks = (pr.n_steps + 3) >> 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < pr.count; i += stride) {
        const uint64_t g = pr.first + static_cast<uint64_t>(i);
        double m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
        for (int32_t b = 0; b < blocks; ++b) {
            float z[4];
            raw_normals4(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), static_cast<uint32_t>(b), 0u, pr.key0, pr.key1, z);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * b + j < pr.n_steps) {
                    const double x = kZScale * static_cast<double>(z[j]), x2 = x * x;
                    m1 += x; m2 += x2; m3 += x2 * x; m4 += x2 * x2;
                }
        }
        acc[0] += m1; acc[1] += m2; acc[2] += m3; acc[3] += m4;
    }
    block_then_grid_reduce<4>(acc, ws);
}

// Measurement tap (bench.py; never on a pricing path): the shader clock the chip HOLDS while every SIMD runs the
// headline kernel's own step loop.  s_memtime counts shader cycles, s_memrealtime a constant 100 MHz, so
// clock = d(memtime) / d(memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS give-back item 6).  One stamp pair per
// workgroup around path_normal_sum; the stamps go to a buffer of their own and no priced value depends on them.
__global__ __launch_bounds__(kBlock) void clock_probe_kernel(PathRange pr, uint64_t* __restrict__ stamps, double* __restrict__ sink) {
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    const uint64_t g = pr.first + static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const double zsum = path_normal_sum(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), pr.n_steps, pr.key0, pr.key1);
    if (zsum == 1.2345678e300) sink[0] = zsum;          // never true: keeps the loop from being optimised away
    __builtin_amdgcn_s_waitcnt(0);
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        stamps[2 * static_cast<size_t>(blockIdx.x)] = t1 - t0;
        stamps[2 * static_cast<size_t>(blockIdx.x) + 1] = r1 - r0;
    }
}

// Measurement tap (tools/phase_stamps.py; never on a pricing path): WHERE a launch of the headline kernel spends its time.
// The body is european_path_kernel<1, true, kReduce, false> call for call (same device functions, same launch shape, same
// reduction); wave 0 of every workgroup additionally leaves four s_memrealtime stamps (a constant 100 MHz counter shared by
// the whole device): [0] entry, [1] step loop done, [2] payoffs + workgroup sums done (about to enter the grid reduction),
// [3] back from the grid reduction (ticket taken; for the workgroup that took the LAST ticket of the launch: totals written),
// and [4] where it ran: HW_REG_HW_ID in the low word (cu_id bits 11:8, sh_id 12, se_id 15:13), HW_REG_XCC_ID in the high word.
// The wave that writes the totals also stamps slot kStampWords * gridDim.x: the end of the launch's useful work.
constexpr int kStampWords = 5;
struct StampEpilogue {
    uint64_t* final_stamp;
    __device__ __forceinline__ void operator()(double) const {
        if (threadIdx.x == 0) *final_stamp = __builtin_amdgcn_s_memrealtime();
    }
};

__global__ __launch_bounds__(kBlock) void european_stamp_kernel(PathRange pr, ContractSet<1> cs, ReduceWs ws, uint64_t* __restrict__ stamps) {
    __shared__ double quarter_sum[kWavesPerBlock][kWave];
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) / kWave), lane = threadIdx.x & (kWave - 1);
    const bool split = static_cast<int32_t>(blockIdx.x) >= pr.split_from;
    const int64_t i = split ? static_cast<int64_t>(pr.split_from) * kBlock + (static_cast<int64_t>(blockIdx.x) - pr.split_from) * kWave + lane
                            : static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const uint64_t g = pr.first + static_cast<uint64_t>(i);
    double zsum = path_normal_quarters(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), pr.n_steps, split ? wave : 0,
                                       split ? wave + 1 : 4, pr.key0, pr.key1);
    if (split) {
        quarter_sum[wave][lane] = zsum;
        __syncthreads();
        zsum = ((quarter_sum[0][lane] + quarter_sum[1][lane]) + quarter_sum[2][lane]) + quarter_sum[3][lane];
    }
    zsum *= kPairZScale;
    asm volatile("s_nop 0" ::"v"(zsum));                 // the stamp below must follow the loop's last result
    const uint64_t t_loop = __builtin_amdgcn_s_memrealtime();
    double acc[2] = {0.0, 0.0};
    if (!split || wave == 0) european_payoffs<1, true, kReduce>(cs, zsum, i < pr.count, i, pr.count, nullptr, acc);
    constexpr int P = 2;
    __shared__ double stage[kWavesPerBlock][P];
    double w[P] = {acc[0], acc[1]};
    wave_transpose_reduce<P>(w);
    if ((lane & 31) == 0) stage[wave][lane >> 5] = w[0];
    __syncthreads();
    if (wave != 0) return;
    double v = 0.0;
    if (threadIdx.x < 2) v = ((stage[0][threadIdx.x] + stage[1][threadIdx.x]) + stage[2][threadIdx.x]) + stage[3][threadIdx.x];
    asm volatile("s_nop 0" ::"v"(v));
    const uint64_t t_sums = __builtin_amdgcn_s_memrealtime();
    grid_reduce<2, StampEpilogue>(v, ws, StampEpilogue{stamps + kStampWords * static_cast<size_t>(gridDim.x)});
    if (threadIdx.x == 0) {
        uint64_t* mine = stamps + kStampWords * static_cast<size_t>(blockIdx.x);
        const uint32_t hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        mine[0] = t_entry; mine[1] = t_loop; mine[2] = t_sums; mine[3] = __builtin_amdgcn_s_memrealtime();
        mine[4] = (static_cast<uint64_t>(xcc_id) << 32) | hw_id;
    }
}

// Measurement tap (bench.py): the issue cost of ONE instruction class on this device, in the form the path kernels
// use it (SGPR multipliers / keys where hipcc puts them there).  Every wave runs kProbeIters x 16 independent
// instructions of the class; with `w` workgroups per CU (= w waves per SIMD) the kernel's duration / (iters x 16 x w) is
// the time one SIMD needs per wave64 instruction of that class with w waves to pick from.  This calibrates the
// roofline's issue model on the chip and at the clock the benchmark itself runs at.
constexpr int kProbeIters = 2000;

#define OLMC_PROBE(NAME, TYPE, INIT, ASM)                                                                           \
    __global__ __launch_bounds__(kBlock) void NAME(uint32_t* __restrict__ sink, uint32_t seed, uint32_t kconst) {   \
        TYPE r[16];                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) r[i] = INIT;                                                 \
        for (int it = 0; it < kProbeIters; ++it) {                                                                  \
            _Pragma("unroll") for (int i = 0; i < 16; ++i) { ASM; }                                                 \
        }                                                                                                           \
        TYPE acc = r[0];                                                                                            \
        _Pragma("unroll") for (int i = 1; i < 16; ++i) acc = acc + r[i];                                            \
        if (acc == static_cast<TYPE>(12345.678)) sink[0] = 1u;                                                      \
    }

#define OLMC_PF (static_cast<float>(threadIdx.x + i + seed) * 0.37f + 2.0f)
#define OLMC_PU (threadIdx.x * 2654435761u + i + seed)
#define OLMC_PD (static_cast<double>(threadIdx.x + i + seed) * 0.37 + 2.0)
OLMC_PROBE(probe_bitop3, uint32_t, OLMC_PU, asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(r[i]) : "v"(seed + i), "s"(kconst)))
OLMC_PROBE(probe_cvt_f32_u32, float, OLMC_PF, asm volatile("v_cvt_f32_u32_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_fmamk_f32, float, OLMC_PF, asm volatile("v_fmamk_f32 %0, %0, 0x2f800000, %1" : "+v"(r[i]) : "v"(1.0001f)))
OLMC_PROBE(probe_and_or, uint32_t, OLMC_PU, asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(r[i]) : "s"(kconst), "v"(0x3F800000u)))
OLMC_PROBE(probe_log_f32, float, OLMC_PF, asm volatile("v_log_f32_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_sqrt_f32, float, OLMC_PF, asm volatile("v_sqrt_f32_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_sin_f32, float, OLMC_PF, asm volatile("v_sin_f32_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_cos_f32, float, OLMC_PF, asm volatile("v_cos_f32_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_exp_f32, float, OLMC_PF, asm volatile("v_exp_f32_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_add_f32, float, OLMC_PF, asm volatile("v_add_f32_e32 %0, %1, %0" : "+v"(r[i]) : "v"(1.0001f)))
OLMC_PROBE(probe_fma_f32, float, OLMC_PF, asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(r[i]) : "v"(1.0001f)))
OLMC_PROBE(probe_add_f64, double, OLMC_PD, asm volatile("v_add_f64 %0, %0, %1" : "+v"(r[i]) : "v"(1.5)))
OLMC_PROBE(probe_fma_f64, double, OLMC_PD, asm volatile("v_fma_f64 %0, %0, %1, %1" : "+v"(r[i]) : "v"(1.0000001)))
OLMC_PROBE(probe_rndne_f64, double, OLMC_PD, asm volatile("v_rndne_f64_e32 %0, %0" : "+v"(r[i])))
OLMC_PROBE(probe_ldexp_f64, double, OLMC_PD, asm volatile("v_ldexp_f64 %0, %0, %1" : "+v"(r[i]) : "v"(1)))
// Mixed bodies (TWO instructions per body: the reported figure is nanoseconds per PAIR): do classes overlap?
// log+add: a transcendental beside a full-rate fp32 add;  log+bitop3: beside a three-operand integer op;
// operand-form variants of the two integer workhorses of Philox.
OLMC_PROBE(probe_mix_log_add, float, OLMC_PF, asm volatile("v_log_f32_e32 %0, %0\n\tv_add_f32_e32 %0, %1, %0" : "+v"(r[i]) : "v"(1.0001f)))
OLMC_PROBE(probe_mix_log_bitop3, float, OLMC_PF, asm volatile("v_log_f32_e32 %0, %0\n\tv_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(r[i]) : "v"(seed + i), "s"(kconst)))
OLMC_PROBE(probe_bitop3_vvv, uint32_t, OLMC_PU, asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(r[i]) : "v"(seed + i), "v"(kconst + i)))
OLMC_PROBE(probe_bitop3_vvc, uint32_t, OLMC_PU, asm volatile("v_bitop3_b32 %0, %0, %1, 2 bitop3:0x96" : "+v"(r[i]) : "v"(seed + i)))
OLMC_PROBE(probe_xor_vv, uint32_t, OLMC_PU, asm volatile("v_xor_b32_e32 %0, %1, %0" : "+v"(r[i]) : "v"(seed + i)))
OLMC_PROBE(probe_mix_bitop3_add, uint32_t, OLMC_PU, asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96\n\tv_add_u32_e32 %0, %1, %0" : "+v"(r[i]) : "v"(seed + i), "s"(kconst)))
#undef OLMC_PF
#undef OLMC_PU
#undef OLMC_PD

// mad + bitop3 alternating, as in a Philox round (pair cost)
__global__ __launch_bounds__(kBlock) void probe_mix_mad_bitop3(uint32_t* __restrict__ sink, uint32_t seed, uint32_t kconst) {
    uint64_t r[16];
    uint32_t a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { r[i] = threadIdx.x + i + seed; a[i] = threadIdx.x * 7u + i; }
    for (int it = 0; it < kProbeIters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint64_t carry;
            asm volatile("v_mad_u64_u32 %0, %1, %2, %3, 0\n\tv_bitop3_b32 %2, %2, %4, %3 bitop3:0x96" : "=v"(r[i]), "=s"(carry), "+v"(a[i]) : "s"(kconst), "v"(seed + i));
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(r[i]));
    }
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += r[i] + a[i];
    if (acc == 12345u) sink[0] = 1u;
}

// v_mad_u64_u32 with the multiplier in a VGPR instead of an SGPR
__global__ __launch_bounds__(kBlock) void probe_mad_u64_u32_vv(uint32_t* __restrict__ sink, uint32_t seed, uint32_t kconst) {
    uint64_t r[16];
    uint32_t a[16];
    const uint32_t kv = kconst + (threadIdx.x >> 8);
#pragma unroll
    for (int i = 0; i < 16; ++i) { r[i] = threadIdx.x + i + seed; a[i] = threadIdx.x * 7u + i; }
    for (int it = 0; it < kProbeIters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint64_t carry;
            asm volatile("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(r[i]), "=s"(carry) : "v"(a[i]), "v"(kv));
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(r[i]));
    }
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += r[i];
    if (acc == 12345u) sink[0] = 1u;
}

// v_mad_u64_u32 (64-bit destination, SGPR multiplier as in the Philox rounds) and the two width-changing conversions
__global__ __launch_bounds__(kBlock) void probe_mad_u64_u32(uint32_t* __restrict__ sink, uint32_t seed, uint32_t kconst) {
    uint64_t r[16];
    uint32_t a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { r[i] = threadIdx.x + i + seed; a[i] = threadIdx.x * 7u + i; }
    for (int it = 0; it < kProbeIters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint64_t carry;         // the carry-out goes to an SGPR pair, as hipcc emits it in the Philox rounds
            asm volatile("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(r[i]), "=s"(carry) : "v"(a[i]), "s"(kconst));
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(r[i]));      // sixteen live destinations per iteration, no extra instruction
    }
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += r[i];
    if (acc == 12345u) sink[0] = 1u;
}

__global__ __launch_bounds__(kBlock) void probe_cvt_f64_f32(uint32_t* __restrict__ sink, uint32_t seed, uint32_t) {
    double r[16];
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { a[i] = static_cast<float>(threadIdx.x + i + seed); r[i] = 0.0; }
    for (int it = 0; it < kProbeIters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("v_cvt_f64_f32_e32 %0, %1" : "=v"(r[i]) : "v"(a[i]));
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(r[i]));
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += r[i];
    if (acc == 12345.5) sink[0] = 1u;
}

__global__ __launch_bounds__(kBlock) void probe_cvt_i32_f64(uint32_t* __restrict__ sink, uint32_t seed, uint32_t) {
    int32_t r[16];
    double a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { a[i] = static_cast<double>(threadIdx.x + i + seed) * 0.37; r[i] = 0; }
    for (int it = 0; it < kProbeIters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("v_cvt_i32_f64_e32 %0, %1" : "=v"(r[i]) : "v"(a[i]));
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(r[i]));
    }
    int32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += r[i];
    if (acc == 12345) sink[0] = 1u;
}

// exp2_f64 (the fp64 Asian kernel's exponential) on an array: lets the tests pin it against a reference libm point by point.
// which = 0: exp2_f64 (degree-11 polynomial); 1: exp2_f64_tab (table; the argument is scaled by kExp2Entries = 256 here, exactly)
__global__ void exp2_probe_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ y, int which) {
    __shared__ double tab[kExp2Entries];
    exp2_table_to_lds(tab);
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        y[i] = which ? exp2_f64_tab(static_cast<double>(kExp2Entries) * x[i], tab) : exp2_f64(x[i]);
}


// The Sobol kernels' inverse normal on an array of probabilities: z[i] = 0 + (the term every Sobol kernel adds to a point's sum for
// the uniform p[i]) -- form 0 = ndtri_w_add (one point), 1 = ndtri_w_regs_add (coefficients in registers), 2 = ndtri_w_regs_pair_add
// (two in lockstep: element i rides in slot i & 1 next to p = 1/2, whose normal is an exact zero), 3 = ndtri_lockstep_add<8>
// (elements 8 j .. 8 j + 7).  All forms must agree bit for bit; tests pin them to mpmath.
__global__ void ndtri_probe_kernel(const double* __restrict__ p, int64_t n, double* __restrict__ z, int form) {
    NdtriRegs regs;
    regs.load();
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        if (form == 0) {
            z[i] = ndtri_w_add(0.0, p[i], opaque_zero());
        } else if (form == 1) {
            z[i] = ndtri_w_regs_add(0.0, p[i], regs, opaque_zero());
        } else if (form == 2) {
            const double in[2] = {(i & 1) ? 0.5 : p[i], (i & 1) ? p[i] : 0.5};
            z[i] = ndtri_w_regs_pair_add(0.0, in, regs, opaque_zero());
        } else {
            const int64_t base = i & ~static_cast<int64_t>(7);
            double in[8], out[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                in[j] = p[base + j < n ? base + j : i];
                out[j] = 0.0;
            }
            ndtri_lockstep_add<8>(out, in, opaque_zero());
            z[i] = out[i & 7];
        }
    }
}

// The normal generator under every Philox kernel on chosen words: box_muller_raw and pair_sum_raw (olmc_kernels.h) themselves, RAW
// units (no kZScale).  z_cos[i], z_sin[i] = the pair of (xa[i], xb[i]); pair[i] = 0 + (z_cos + z_sin) / sqrt(2) by the one-sine form.
__global__ void box_muller_probe_kernel(const uint32_t* __restrict__ xa, const uint32_t* __restrict__ xb, int64_t n, float* __restrict__ z_cos,
                                        float* __restrict__ z_sin, float* __restrict__ pair) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        float c, s;
        box_muller_raw(xa[i], xb[i], c, s);
        z_cos[i] = c;
        z_sin[i] = s;
        pair[i] = pair_sum_raw(0.0f, xa[i], xb[i]);
    }
}

// The Heston kernels' square root (sqrt_nonneg, olmc_kernels.h) on an array of non-negative finite doubles.
__global__ void sqrt_nonneg_probe_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ y) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        y[i] = sqrt_nonneg(x[i]);
}

// ---------------------------------------------------------------- the fused grid reduction on synthetic values ----
// Validation taps of the reduction family of olmc_kernels.h (wave_transpose_reduce, block_then_grid_reduce[_from], block_row_sum,
// grid_reduce[_workgroup], wave_rows_sum, workgroup_rows_sum): the product's own device functions on values whose sum has an exact
// answer.  Thread t of workgroup b contributes to component c
//     v = H(b, c, salt) + K(t, c, salt)        when 256 b + t < n_threads, else 0.0
// with two 32-bit integer hashes (all arithmetic mod 2^32; tests/reduction_reference.py restates them in NumPy):
//     mix32(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
//     seed     = mix32(lo32(salt) ^ mix32(hi32(salt) ^ 0x9E3779B9))
//     H        = (mix32( seed + b * 0x9E3779B1 + c * 0x85EBCA6B) >>  8) | 1         24 bits, odd
//     K        = (mix32(~seed + t * 0xC2B2AE35 + c * 0x27D4EB2F) >> 16) | 1         16 bits, odd
// values = 0: v is that integer -- at most 2^26 threads x (2^24 + 2^16) < 2^51, so every partial sum is exact in fp64 whatever the
// order, and the total must EQUAL the integer  sum_b live(b) H + sum_t count(t) K  (separable: NumPy has it in milliseconds).
// values = 1: v = double(H + K) / 3.0 (one correctly rounded fp64 division): sums round, order matters.
__host__ __device__ inline uint32_t probe_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t probe_seed(uint64_t salt) {
    return probe_mix32(static_cast<uint32_t>(salt) ^ probe_mix32(static_cast<uint32_t>(salt >> 32) ^ 0x9E3779B9u));
}
__device__ __forceinline__ double reduce_probe_value(uint32_t seed, uint32_t b, uint32_t t, uint32_t c, bool live, int values) {
    const uint32_t h = (probe_mix32(seed + b * 0x9E3779B1u + c * 0x85EBCA6Bu) >> 8) | 1u;
    const uint32_t k = (probe_mix32(~seed + t * 0xC2B2AE35u + c * 0x27D4EB2Fu) >> 16) | 1u;
    const double v = static_cast<double>(h + k);
    return live ? (values ? v / 3.0 : v) : 0.0;
}

// FORM 0 = block_then_grid_reduce<NV>;  1 = block_then_grid_reduce_from<NV, 1>, the lane ^ 32 exchange made by the producer as in
// european_payoffs_folded (value k meets value k + P / 2);  2 = block_row_sum<NV>, then grid_reduce<NV> (NV = 2, wave 0 only) or
// grid_reduce_workgroup<NV> called directly, as extrema_greeks_kernel and qmc_path_greeks_kernel enter.
template <int NV, int FORM>
__global__ __launch_bounds__(kBlock) void reduce_probe_kernel(int64_t n_threads, uint64_t salt, int values, ReduceWs ws) {
    const uint32_t seed = probe_seed(salt);
    const bool live = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x < n_threads;
    auto value = [&](int c) { return reduce_probe_value(seed, blockIdx.x, threadIdx.x, static_cast<uint32_t>(c), live, values); };
    if constexpr (FORM == 1) {
        constexpr int P = pow2_ceil(NV), H = P / 2;
        double kept[H];
#pragma unroll
        for (int k = 0; k < H; ++k) kept[k] = swap_add<32>(k < NV ? value(k) : 0.0, k + H < NV ? value(k + H) : 0.0);
        block_then_grid_reduce_from<NV, 1>(kept, ws);
    } else {
        double acc[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] = value(k);
        if constexpr (FORM == 0) {
            block_then_grid_reduce<NV>(acc, ws);
        } else {
            const double row = block_row_sum<NV>(acc);
            if constexpr (NV <= 2) {
                if (threadIdx.x >= kWave) return;
                grid_reduce<NV>(row, ws);
            } else {
                grid_reduce_workgroup<NV>(row, ws);
            }
        }
    }
}

// wave_rows_sum<NV> (one wave) or workgroup_rows_sum<NV> (kBlock threads) on a [rows][NV] matrix: out[c] = column c's sum.
template <int NV, bool WORKGROUP>
__global__ __launch_bounds__(kBlock) void rows_sum_probe_kernel(const double* __restrict__ src, int32_t rows, double* __restrict__ out) {
    acquire_rows();
    double total;
    if constexpr (WORKGROUP) {
        __shared__ double part[kBlock];
        total = workgroup_rows_sum<NV>(src, rows, part);
    } else {
        total = wave_rows_sum<NV>(src, rows);
    }
    if (threadIdx.x < NV) out[threadIdx.x] = total;
}

// wave_transpose_reduce<P, 32, Op> on one wave: lane l holds v[l][0 .. P), out[l] = its v[0] afterwards (an ordinary per-lane
// store) -- by the contract of olmc_kernels.h the result of value index l >> (6 - log2 P).
template <int P, typename Op>
__global__ __launch_bounds__(kWave) void wave_reduce_probe_kernel(const double* __restrict__ v_in, double* __restrict__ out) {
    double v[P];
#pragma unroll
    for (int k = 0; k < P; ++k) v[k] = v_in[threadIdx.x * P + k];
    wave_transpose_reduce<P, kWave / 2, Op>(v);
    out[threadIdx.x] = v[0];
}

// FORM 3 of olmc_reduce_probe, the hand-over of the LSM chains (lsm_step_kernel, heston_lsm_step_kernel) in two launches on one stream:
// every workgroup of the first stores block_row_sum<NV> of the synthetic values as a plain row (the kernel boundary publishes it), every
// workgroup of the second sums all the rows by workgroup_rows_sum<NV> and stores its totals, out[blockIdx.x][NV].
template <int NV>
__global__ __launch_bounds__(kBlock) void rows_store_probe_kernel(int64_t n_threads, uint64_t salt, int values, double* __restrict__ rows) {
    const uint32_t seed = probe_seed(salt);
    const bool live = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x < n_threads;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = reduce_probe_value(seed, blockIdx.x, threadIdx.x, static_cast<uint32_t>(k), live, values);
    const double s = block_row_sum<NV>(acc);
    if (threadIdx.x < NV) rows[static_cast<size_t>(blockIdx.x) * NV + threadIdx.x] = s;
}

template <int NV>
__global__ __launch_bounds__(kBlock) void rows_total_probe_kernel(const double* __restrict__ rows, int32_t n_rows, double* __restrict__ out) {
    __shared__ double part[kBlock];
    const double total = workgroup_rows_sum<NV>(rows, n_rows, part);
    if (threadIdx.x < NV) out[static_cast<size_t>(blockIdx.x) * NV + threadIdx.x] = total;
}

// ---------------------------------------------------------------- the in-wave solvers of the LSM chains ----
// What the `fit` lambda of heston_lsm_step_kernel / lsm_step_kernel does, in that order, on totals the host chose: workgroup blockIdx.x
// sums the ONE row of its set by workgroup_rows_sum, solves in its first wave (ha_fit<D> / LsmFit), meets the barrier and copies the
// coefficients out of LDS; thread kBlock - 1 -- in the LAST wave, so the LDS hand-over to another wave is part of what is observed --
// writes them and `valid`.
template <int D>
__global__ __launch_bounds__(kBlock) void ha_fit_probe_kernel(const double* __restrict__ totals /* [gridDim.x][NV] */, double* __restrict__ beta /* [gridDim.x][NU] */,
                                                              int32_t* __restrict__ valid) {
    using B = HaBasis<D>;
    __shared__ double part[kBlock];
    __shared__ HaCoeffs<D> shared_fit;
    const double total = workgroup_rows_sum<B::NV>(totals + static_cast<size_t>(blockIdx.x) * B::NV, 1, part);
    if (threadIdx.x < kWave) ha_fit<D>(&shared_fit, total);
    __syncthreads();
    const HaCoeffs<D> f = shared_fit;
    if (threadIdx.x == kBlock - 1) {
#pragma unroll
        for (int k = 0; k < B::NU; ++k) beta[static_cast<size_t>(blockIdx.x) * B::NU + k] = f.beta[k];
        valid[blockIdx.x] = f.valid;
    }
}

__global__ __launch_bounds__(kBlock) void lsm_fit_probe_kernel(int32_t degree, const double* __restrict__ totals /* [gridDim.x][kLsmNV] */,
                                                               double* __restrict__ beta /* [gridDim.x][kLsmMaxDegree + 1] */, int32_t* __restrict__ valid) {
    __shared__ double part[kBlock];
    __shared__ LsmCoeffs shared_fit;
    const double total = workgroup_rows_sum<kLsmNV>(totals + static_cast<size_t>(blockIdx.x) * kLsmNV, 1, part);
    if (threadIdx.x < kWave) LsmFit{&shared_fit, degree}(total);
    __syncthreads();
    const LsmCoeffs f = shared_fit;
    if (threadIdx.x == kBlock - 1) {
#pragma unroll
        for (int k = 0; k <= kLsmMaxDegree; ++k) beta[static_cast<size_t>(blockIdx.x) * (kLsmMaxDegree + 1) + k] = f.beta[k];
        valid[blockIdx.x] = f.valid;
    }
}

// ---------------------------------------------------------------- the price of the reference's own width (round 4) ----
// The European step loop with fp64 NORMALS, as NumPy draws them (gbm_numpy.py:32-33: standard_normal of a PCG64 Generator, fp64):
// the same Philox4x32-10 counter stream, but one block now yields TWO normals -- its four words make two 53-bit uniforms
//   u_a = ((x0 << 21 ^ x1 >> 11) + 1/2) 2^-53  in (0, 1),   u_b = (x2 << 21 ^ x3 >> 11) 2^-53  (turn fraction),
// and one fp64 Box-Muller: r = sqrt(-2 ln u_a) (library log), (sin, cos)(2 pi u_b) (library sincospi), the sum of a path's
// normals carried in fp64 throughout.  Same launch shape, same fused reduction, same payoff code as european_path_kernel<1, true,
// kReduce, false>.  NOT a product path: a labelled number beside the product's "f32 normals"  -- what the
// reference's width would cost on this device, and that it moves the price by nothing measurable.
__global__ __launch_bounds__(kBlock) void european_f64_normals_kernel(PathRange pr, ContractSet<1> cs, ReduceWs ws) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const uint64_t g = pr.first + static_cast<uint64_t>(i);
    const uint32_t g_lo = static_cast<uint32_t>(g), g_hi = static_cast<uint32_t>(g >> 32);
    double zsum = 0.0;
    const int32_t pairs = (pr.n_steps + 1) >> 1;
    for (int32_t b = 0; b < pairs; ++b) {
        const Words4 w = philox4x32_10(g_lo, g_hi, static_cast<uint32_t>(b), 0u, pr.key0, pr.key1);
        const uint64_t ma = (static_cast<uint64_t>(w.x0) << 21) ^ (static_cast<uint64_t>(w.x1) >> 11);
        const uint64_t mb = (static_cast<uint64_t>(w.x2) << 21) ^ (static_cast<uint64_t>(w.x3) >> 11);
        const double ua = (static_cast<double>(ma) + 0.5) * 0x1p-53, ub = static_cast<double>(mb) * 0x1p-53;
        const double rad = sqrt(-2.0 * log(ua));
        double sn, cs_;
        sincospi(2.0 * ub, &sn, &cs_);
        zsum += rad * cs_;
        if (2 * b + 1 < pr.n_steps) zsum += rad * sn;
    }
    double acc[2] = {0.0, 0.0};
    european_payoffs<1, true, kReduce>(cs, zsum, i < pr.count, i, pr.count, nullptr, acc);
    block_then_grid_reduce<2>(acc, ws);
}

// A kernel that does nothing: a chain of them on one stream measures what two DEPENDENT launches cost each other (the command
// processor's gap) -- the floor under every per-date launch of the American option.
__global__ void empty_kernel(uint32_t* __restrict__ sink) {
    if (sink == nullptr && threadIdx.x == 12345) __builtin_trap();
}

}  // namespace olmc
