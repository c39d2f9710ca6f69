// olmc_probe.hip -- libolmc_probe.so, the INSTRUMENTED build of the library (include/olmc_probe.h).
//
// It is the product's own translation unit (optionslab_amd/csrc/olmc.hip, textually included with OLMC_WITH_PROBES defined, so
// that the fault-injection and rehearsal seams inside it are compiled in) plus the measurement / validation kernels and their
// entry points.  libolmc.so is built WITHOUT any of this: `nm -D optionslab_amd/libolmc.so` lists no probe symbol, the product
// carries no fault-injection branch.  Loaded by tests, tools/ and bench.py's calibration only (tools/probe/binding.py); it has its
// own contexts, streams and workspaces, independent of a libolmc.so loaded beside it.
#define OLMC_WITH_PROBES 1
#include "../../optionslab_amd/csrc/olmc.hip"
#include "olmc_probe.h"
#include "olmc_probe_kernels.h"

// ============================================================ validation taps ====
extern "C" int olmc_exp2_probe_form(const double* x_host, int64_t n, double* y_host, int form) {
    if (!x_host || !y_host || n < 1) return fail(OLMC_ERR_ARG, "bad arguments");
    if (form != 0 && form != 1) return fail(OLMC_ERR_ARG, "form must be 0 (polynomial) or 1 (table)");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(double) * static_cast<size_t>(n);
    Carver bulk;
    rc = bulk_reserve(c, 2 * bytes, &bulk);
    if (rc) return rc;
    double* d_x = bulk.take<double>(n);
    double* d_y = bulk.take<double>(n);
    HIP_TRY(hipMemcpyAsync(d_x, x_host, bytes, hipMemcpyHostToDevice, c->stream));
    const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(exp2_probe_kernel, dim3(grid), dim3(256), 0, c->stream, d_x, n, d_y, form);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(y_host, d_y, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// the form the arithmetic Asian kernel is built with
extern "C" int olmc_exp2_probe(const double* x_host, int64_t n, double* y_host) {
    return olmc_exp2_probe_form(x_host, n, y_host, OLMC_EXP2_TABLE ? 1 : 0);
}

extern "C" int olmc_ndtri_probe(const double* p_host, int64_t n, double* z_host, int form) {
    if (!p_host || !z_host || n < 1) return fail(OLMC_ERR_ARG, "bad arguments");
    if (form < 0 || form > 3) return fail(OLMC_ERR_ARG, "form must be 0 .. 3");
    for (int64_t i = 0; i < n; ++i)
        if (!(p_host[i] >= 1e-10 && p_host[i] <= 1.0 - 1e-10)) return fail(OLMC_ERR_ARG, "a probability outside [1e-10, 1 - 1e-10]");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(double) * static_cast<size_t>(n);
    Carver bulk;
    rc = bulk_reserve(c, 2 * bytes, &bulk);
    if (rc) return rc;
    double* d_p = bulk.take<double>(n);
    double* d_z = bulk.take<double>(n);
    HIP_TRY(hipMemcpyAsync(d_p, p_host, bytes, hipMemcpyHostToDevice, c->stream));
    const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(ndtri_probe_kernel, dim3(grid), dim3(256), 0, c->stream, d_p, n, d_z, form);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(z_host, d_z, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// box_muller_raw / pair_sum_raw on chosen words (box_muller_probe_kernel): bulk buffer = [xa | xb | z_cos | z_sin | pair], n words each.
extern "C" int olmc_box_muller_probe(const uint32_t* xa_host, const uint32_t* xb_host, int64_t n, float* z_cos_host, float* z_sin_host,
                                     float* pair_host) {
    if (!xa_host || !xb_host || !z_cos_host || !z_sin_host || !pair_host || n < 1) return fail(OLMC_ERR_ARG, "bad arguments");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(uint32_t) * static_cast<size_t>(n);
    static_assert(sizeof(uint32_t) == sizeof(float), "one stride for words and normals");
    Carver bulk;
    rc = bulk_reserve(c, 5 * bytes, &bulk);
    if (rc) return rc;
    uint32_t* d_xa = bulk.take<uint32_t>(n);
    uint32_t* d_xb = bulk.take<uint32_t>(n);
    float* d_cos = bulk.take<float>(n);
    float* d_sin = bulk.take<float>(n);
    float* d_pair = bulk.take<float>(n);
    HIP_TRY(hipMemcpyAsync(d_xa, xa_host, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_xb, xb_host, bytes, hipMemcpyHostToDevice, c->stream));
    const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(box_muller_probe_kernel, dim3(grid), dim3(256), 0, c->stream, d_xa, d_xb, n, d_cos, d_sin, d_pair);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(z_cos_host, d_cos, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(z_sin_host, d_sin, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pair_host, d_pair, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

extern "C" int olmc_sqrt_nonneg_probe(const double* x_host, int64_t n, double* y_host) {
    if (!x_host || !y_host || n < 1) return fail(OLMC_ERR_ARG, "bad arguments");
    for (int64_t i = 0; i < n; ++i)
        if (!(x_host[i] >= 0.0 && x_host[i] <= std::numeric_limits<double>::max())) return fail(OLMC_ERR_ARG, "an argument that is negative or not finite");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(double) * static_cast<size_t>(n);
    Carver bulk;
    rc = bulk_reserve(c, 2 * bytes, &bulk);
    if (rc) return rc;
    double* d_x = bulk.take<double>(n);
    double* d_y = bulk.take<double>(n);
    HIP_TRY(hipMemcpyAsync(d_x, x_host, bytes, hipMemcpyHostToDevice, c->stream));
    const int grid = static_cast<int>(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(sqrt_nonneg_probe_kernel, dim3(grid), dim3(256), 0, c->stream, d_x, n, d_y);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(y_host, d_y, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// ---- the fused grid reduction on synthetic values (reduce_probe_kernel) ----
namespace {
template <int NV>
void launch_reduce_probe(int form, int32_t grid, hipStream_t st, const EventPair* timed, int64_t n, uint64_t salt, int values, const ReduceWs& ws) {
    if (form == 0) launch_timed(reduce_probe_kernel<NV, 0>, dim3(grid), dim3(kBlock), st, timed, n, salt, values, ws);
    else if (form == 2) launch_timed(reduce_probe_kernel<NV, 2>, dim3(grid), dim3(kBlock), st, timed, n, salt, values, ws);
    else if constexpr (NV >= 8) launch_timed(reduce_probe_kernel<NV, 1>, dim3(grid), dim3(kBlock), st, timed, n, salt, values, ws);
}

// f(integral_constant<int, NV>) for the row widths the product instantiates (10, 22, 39 = HaBasis<D>::NV); false for any other nv.
template <typename F>
bool with_reduce_width(int nv, F&& f) {
    switch (nv) {
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 5: f(std::integral_constant<int, 5>{}); return true;
        case 8: f(std::integral_constant<int, 8>{}); return true;
        case 10: f(std::integral_constant<int, 10>{}); return true;
        case 16: f(std::integral_constant<int, 16>{}); return true;
        case 22: f(std::integral_constant<int, 22>{}); return true;
        case 32: f(std::integral_constant<int, 32>{}); return true;
        case 39: f(std::integral_constant<int, 39>{}); return true;
        default: return false;
    }
}
static_assert(HaBasis<1>::NV == 10 && HaBasis<2>::NV == 22 && HaBasis<3>::NV == 39 && kLsmNV == 16, "the widths of the LSM chains' rows");

constexpr int32_t kLsmChainRows = 1024;                      // the chains launch at most this many workgroups (lsm_chain, heston_lsm_chain)

// Form 3: launch 1 = ceil(n / 256) workgroups store their block_row_sum<nv> rows, launch 2 = g2 workgroups each sum all of them
// (workgroup_rows_sum<nv>), same stream, nothing between them.  Bulk buffer = [rows | out[g2][nv]].
int reduce_probe_hand_over(int nv, int values, int32_t g2, int64_t n, uint64_t salt, double* out) {
    if (nv != 10 && nv != 16 && nv != 22 && nv != 39) return fail(OLMC_ERR_ARG, "form 3 (the LSM chains' hand-over) exists for nv 10, 16, 22 and 39");
    if (n < 1) return fail(OLMC_ERR_ARG, "n_threads must be >= 1");
    if (n > static_cast<int64_t>(kLsmChainRows) * kBlock) return fail(OLMC_ERR_ARG, "form 3 takes at most 1024 workgroups in its first launch");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const int32_t g1 = static_cast<int32_t>((n + kBlock - 1) / kBlock);
    const size_t n_rows = static_cast<size_t>(g1) * nv, n_out = static_cast<size_t>(g2) * nv;
    Carver bulk;
    rc = bulk_reserve(c, sizeof(double) * (n_rows + n_out), &bulk);
    if (rc) return rc;
    double* d_rows = bulk.take<double>(n_rows);
    double* d_out = bulk.take<double>(n_out);
    HIP_TRY(hipMemsetAsync(d_rows, 0xFF, sizeof(double) * (n_rows + n_out), c->stream));     // NaN wherever a launch writes nothing
    with_reduce_width(nv, [&](auto width) {
        if constexpr (width >= 10) {
            hipLaunchKernelGGL(rows_store_probe_kernel<width>, dim3(g1), dim3(kBlock), 0, c->stream, n, salt, values, d_rows);
            hipLaunchKernelGGL(rows_total_probe_kernel<width>, dim3(g2), dim3(kBlock), 0, c->stream, d_rows, g1, d_out);
        }
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}
}  // namespace

// `launches` launches of reduce_probe_kernel<nv, form> through launch_reduce / make_ws, launch j on ceil(n_threads[j] / 256)
// workgroups with ws.tail = n_threads[j]; out[j] = {the nv totals, the tail}.  blocking = 1: every launch writes the context's pinned
// result and completes through the polled flag, as a blocking pricing does.  blocking = 0: all launches are queued back to back on
// the context's stream with no host wait in between, each into its own slot of a device buffer; one copy and one synchronise follow.
extern "C" int olmc_reduce_probe(int nv, int form, int values, int blocking, int32_t launches, const int64_t* n_threads, const uint64_t* salt,
                                 double* out) {
    if (!n_threads || !salt || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (form < 0 || form > 3) return fail(OLMC_ERR_ARG, "form must be 0, 1, 2 or 3");
    if ((values != 0 && values != 1) || (blocking != 0 && blocking != 1)) return fail(OLMC_ERR_ARG, "values and blocking must be 0 or 1");
    if (launches < 1 || launches > 4096) return fail(OLMC_ERR_ARG, "launches must be in [1, 4096]");
    if (form == 3) return reduce_probe_hand_over(nv, values, launches, n_threads[0], salt[0], out);
    if (nv != 2 && nv != 5 && nv != 8 && nv != 10 && nv != 16 && nv != 22 && nv != 32)
        return fail(OLMC_ERR_ARG, "nv must be 2, 5, 8, 10, 16, 22 or 32 (39: form 3 only, a workspace row holds 32 values)");
    if (form == 1 && nv < 8) return fail(OLMC_ERR_ARG, "form 1 (the folded first exchange) exists for nv 8 and wider");
    int64_t most = 0;
    for (int32_t j = 0; j < launches; ++j) {
        if (n_threads[j] < 1) return fail(OLMC_ERR_ARG, "n_threads must be >= 1");
        if (n_threads[j] > static_cast<int64_t>(kMaxGrid) * kBlock) return fail(OLMC_ERR_ARG, "n_threads beyond one launch of 2^18 workgroups");
        most = std::max(most, n_threads[j]);
    }
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const int row = nv + 1;
    auto grid_of = [](int64_t n) { return static_cast<int32_t>((n + kBlock - 1) / kBlock); };
    auto one = [&](int32_t j, double* d_out) {
        const int64_t n = n_threads[j];
        const uint64_t s = salt[j];
        return launch_reduce(c, c->stream, d_out, static_cast<double>(n), nv, grid_of(n),
                             [&](int32_t grid, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
                                 with_reduce_width(nv, [&](auto width) {
                                     if constexpr (width <= kMaxNV) launch_reduce_probe<width>(form, grid, st, timed, n, s, values, ws);
                                 });
                             });
    };
    if (blocking) {
        for (int32_t j = 0; j < launches; ++j) {
            c->h_result[nv] = -1.0;                         // a launch that writes no tail must not show the one before it
            rc = one(j, c->d_result);
            if (rc) return rc;
            for (int m = 0; m < row; ++m) out[static_cast<size_t>(j) * row + m] = c->h_result[m];
        }
        return OLMC_OK;
    }
    const size_t bytes = sizeof(double) * static_cast<size_t>(launches) * row;
    rc = bulk_reserve(c, bytes);
    if (rc) return rc;
    double* const d_out = c->bulk.as<double>();
    ReduceWs widest;                                         // the workspace grows (and waits for the stream) here, not between the launches
    rc = make_ws(c, c->stream, grid_of(most), nv, d_out, -1.0, &widest);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_out, 0xFF, bytes, c->stream));  // NaN wherever a launch writes nothing
    for (int32_t j = 0; j < launches; ++j) {
        rc = one(j, d_out + static_cast<size_t>(j) * row);
        if (rc) return rc;
    }
    hipError_t e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { ws_recover(c); return fail(OLMC_ERR_HIP, std::string("reduce probe: ") + hipGetErrorString(e)); }
    return OLMC_OK;
}

// wave_rows_sum<nv> (whole_workgroup = 0: nv 2 or 5, one wave) or workgroup_rows_sum<nv> (1: nv 5, 8, 10, 16, 22, 32 or 39, 256 threads) on a host
// matrix [rows][nv]: out_nv[c] = the sum of column c.  Bulk buffer = [matrix | out].
extern "C" int olmc_rows_sum_probe(int nv, int whole_workgroup, const double* rows_host, int32_t rows, double* out_nv) {
    if (!rows_host || !out_nv) return fail(OLMC_ERR_ARG, "null pointer");
    if (whole_workgroup != 0 && whole_workgroup != 1) return fail(OLMC_ERR_ARG, "whole_workgroup must be 0 or 1");
    if (whole_workgroup ? (nv != 5 && nv != 8 && nv != 10 && nv != 16 && nv != 22 && nv != 32 && nv != 39) : (nv != 2 && nv != 5))
        return fail(OLMC_ERR_ARG, "nv must be 2 or 5 for one wave, 5, 8, 10, 16, 22, 32 or 39 for the whole workgroup");
    if (rows < 1 || rows > (1 << 20)) return fail(OLMC_ERR_ARG, "rows must be in [1, 2^20]");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t count = static_cast<size_t>(rows) * nv;
    Carver bulk;
    rc = bulk_reserve(c, sizeof(double) * (count + nv), &bulk);
    if (rc) return rc;
    double* d_rows = bulk.take<double>(count);
    double* d_out = bulk.take<double>(nv);
    HIP_TRY(hipMemcpyAsync(d_rows, rows_host, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    with_reduce_width(nv, [&](auto width) {
        if (whole_workgroup) {
            if constexpr (width > 2) hipLaunchKernelGGL((rows_sum_probe_kernel<width, true>), dim3(1), dim3(kBlock), 0, c->stream, d_rows, rows, d_out);
        } else {
            if constexpr (width <= 5) hipLaunchKernelGGL((rows_sum_probe_kernel<width, false>), dim3(1), dim3(kWave), 0, c->stream, d_rows, rows, d_out);
        }
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_nv, d_out, sizeof(double) * nv, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// wave_transpose_reduce<p, 32, op> on one wave (op 0 = sum, 1 = max, 2 = min): lane l starts from v_host[l][0 .. p), out[l] = its
// v[0] afterwards.  Bulk buffer = [v | out].
extern "C" int olmc_wave_reduce_probe(int p, int op, const double* v_host, double* out) {
    if (!v_host || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (p != 1 && p != 2 && p != 4 && p != 8 && p != 16 && p != 32 && p != 64) return fail(OLMC_ERR_ARG, "p must be 1, 2, 4, 8, 16, 32 or 64");
    if (op < 0 || op > 2) return fail(OLMC_ERR_ARG, "op must be 0 (sum), 1 (max) or 2 (min)");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t count = static_cast<size_t>(kWave) * p;
    Carver bulk;
    rc = bulk_reserve(c, sizeof(double) * (count + kWave), &bulk);
    if (rc) return rc;
    double* d_v = bulk.take<double>(count);
    double* d_out = bulk.take<double>(kWave);
    HIP_TRY(hipMemcpyAsync(d_v, v_host, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    auto with_p = [&](auto f) {
        switch (p) {
            case 1: f(std::integral_constant<int, 1>{}); break;
            case 2: f(std::integral_constant<int, 2>{}); break;
            case 4: f(std::integral_constant<int, 4>{}); break;
            case 8: f(std::integral_constant<int, 8>{}); break;
            case 16: f(std::integral_constant<int, 16>{}); break;
            case 32: f(std::integral_constant<int, 32>{}); break;
            default: f(std::integral_constant<int, 64>{}); break;     // block_row_sum<39>: SHIFT = 0, every lane ends with a value of its own
        }
    };
    with_p([&](auto width) {
        if (op == 0) hipLaunchKernelGGL((wave_reduce_probe_kernel<width, SumOp>), dim3(1), dim3(kWave), 0, c->stream, d_v, d_out);
        else if (op == 1) hipLaunchKernelGGL((wave_reduce_probe_kernel<width, MaxOp>), dim3(1), dim3(kWave), 0, c->stream, d_v, d_out);
        else hipLaunchKernelGGL((wave_reduce_probe_kernel<width, MinOp>), dim3(1), dim3(kWave), 0, c->stream, d_v, d_out);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * kWave, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// ---- the in-wave solvers of the LSM chains on chosen totals (ha_fit_probe_kernel, lsm_fit_probe_kernel) ----
namespace {
// One workgroup per set: totals_host[n_sets][nv] in, beta_host[n_sets][nu] and valid_host[n_sets] out.  Bulk buffer = [totals | beta | valid].
template <typename Launch>
int fit_probe(const double* totals_host, int32_t n_sets, int nv, int nu, double* beta_host, int32_t* valid_host, Launch&& launch) {
    if (!totals_host || !beta_host || !valid_host) return fail(OLMC_ERR_ARG, "null pointer");
    if (n_sets < 1 || n_sets > 4096) return fail(OLMC_ERR_ARG, "n_sets must be in [1, 4096]");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t n_totals = static_cast<size_t>(n_sets) * nv, n_beta = static_cast<size_t>(n_sets) * nu;
    Carver bulk;
    rc = bulk_reserve(c, sizeof(double) * (n_totals + n_beta) + sizeof(int32_t) * static_cast<size_t>(n_sets), &bulk);
    if (rc) return rc;
    double* d_totals = bulk.take<double>(n_totals);
    double* d_beta = bulk.take<double>(n_beta);
    int32_t* d_valid = bulk.take<int32_t>(n_sets);
    HIP_TRY(hipMemcpyAsync(d_totals, totals_host, sizeof(double) * n_totals, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_beta, 0xFF, sizeof(double) * n_beta + sizeof(int32_t) * static_cast<size_t>(n_sets), c->stream));   // NaN / -1 where nothing is written
    launch(c->stream, d_totals, d_beta, d_valid);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(beta_host, d_beta, sizeof(double) * n_beta, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(valid_host, d_valid, sizeof(int32_t) * static_cast<size_t>(n_sets), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}
}  // namespace

extern "C" int olmc_ha_fit_probe(int degree, const double* totals_host, int32_t n_sets, double* beta_host, int32_t* valid_host) {
    if (degree < 1 || degree > kHaMaxDegree) return fail(OLMC_ERR_ARG, "degree must be in [1, 3]");
    const int nu = (degree + 1) * (degree + 2) / 2, nv = (2 * degree + 1) * (2 * degree + 2) / 2 + nu + 1;
    return fit_probe(totals_host, n_sets, nv, nu, beta_host, valid_host, [&](hipStream_t st, const double* t, double* b, int32_t* v) {
        if (degree == 1) hipLaunchKernelGGL(ha_fit_probe_kernel<1>, dim3(n_sets), dim3(kBlock), 0, st, t, b, v);
        else if (degree == 2) hipLaunchKernelGGL(ha_fit_probe_kernel<2>, dim3(n_sets), dim3(kBlock), 0, st, t, b, v);
        else hipLaunchKernelGGL(ha_fit_probe_kernel<3>, dim3(n_sets), dim3(kBlock), 0, st, t, b, v);
    });
}

extern "C" int olmc_lsm_fit_probe(int degree, const double* totals_host, int32_t n_sets, double* beta_host, int32_t* valid_host) {
    if (degree < 1 || degree > kLsmMaxDegree) return fail(OLMC_ERR_ARG, "degree must be in [1, 4]");
    return fit_probe(totals_host, n_sets, kLsmNV, kLsmMaxDegree + 1, beta_host, valid_host, [&](hipStream_t st, const double* t, double* b, int32_t* v) {
        hipLaunchKernelGGL(lsm_fit_probe_kernel, dim3(n_sets), dim3(kBlock), 0, st, static_cast<int32_t>(degree), t, b, v);
    });
}

extern "C" int olmc_normal_moments(uint64_t seed, int64_t path_offset, int64_t n_paths, int32_t n_steps, double* out4) {
    if (!out4) return fail(OLMC_ERR_ARG, "null pointer");
    olmc_stats dummy;
    return run_structured(path_offset, n_paths, n_steps, seed, 0, 0.0, 1.0, false, &dummy,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              launch_timed(normal_moments_kernel, dim3(grid), dim3(kBlock), st, timed, pr, ws);
                          }, 4, out4);
}


// Shader clock held under the headline kernel's load (see clock_probe_kernel): median over workgroups.
extern "C" int olmc_clock_probe(int64_t n_paths, int32_t n_steps, uint64_t seed, double* out3) {
    if (!out3) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const int32_t grid = static_cast<int32_t>(std::min<int64_t>((n_paths + kBlock - 1) / kBlock, kMaxGrid));
    const size_t bytes = sizeof(uint64_t) * 2 * static_cast<size_t>(grid) + 256;
    Carver bulk;
    rc = bulk_reserve(c, bytes, &bulk);
    if (rc) return rc;
    uint64_t* d_stamps = bulk.take<uint64_t>(2 * static_cast<size_t>(grid));
    double* d_sink = bulk.take<double>(256 / sizeof(double));
    const PathRange pr = make_range(0, static_cast<int64_t>(grid) * kBlock, n_steps, seed);
    hipLaunchKernelGGL(clock_probe_kernel, dim3(grid), dim3(kBlock), 0, c->stream, pr, d_stamps, d_sink);
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> h(2 * static_cast<size_t>(grid));
    HIP_TRY(hipMemcpyAsync(h.data(), d_stamps, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<double> cyc(grid), tick(grid), ghz;
    for (int32_t b = 0; b < grid; ++b) {
        cyc[b] = static_cast<double>(h[2 * b]);
        tick[b] = static_cast<double>(h[2 * b + 1]);
        if (tick[b] > 0) ghz.push_back(cyc[b] / tick[b] * 0.1);     // cycles per 10 ns tick -> GHz
    }
    auto median = [](std::vector<double>& v) {
        if (v.empty()) return 0.0;
        std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
        return v[v.size() / 2];
    };
    out3[0] = median(cyc);
    out3[1] = median(tick);
    out3[2] = median(ghz);
    return OLMC_OK;
}

// Where a launch of the headline kernel spends its time (see european_stamp_kernel): one blocking launch of n_paths x n_steps in
// the production launch shape; stamps_host receives 5 words per workgroup (4 stamps in 100 MHz ticks + where it ran) + the final stamp, info3 = {workgroups,
// split_from (or workgroups when nothing is split), the dispatch's own duration in nanoseconds (begin / end timestamps)}.
extern "C" int olmc_phase_stamps(int64_t n_paths, int32_t n_steps, uint64_t seed, int32_t lead_launches, uint64_t* stamps_host, int64_t capacity,
                                 int64_t* info3) {
    if (!stamps_host || !info3) return fail(OLMC_ERR_ARG, "null pointer");
    if (lead_launches < 0 || lead_launches > 1000) return fail(OLMC_ERR_ARG, "lead_launches must be in [0, 1000]");
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    PathRange pr = make_range(0, n_paths, n_steps, seed);
    const int32_t grid = european_launch_shape(c, &pr, european_occupancy<1, kReduce>(true));
    if (static_cast<int64_t>(grid) * kBlock < n_paths) return fail(OLMC_ERR_ARG, "grid-striding launches are not instrumented");
    const int64_t words = kStampWords * static_cast<int64_t>(grid) + 1;
    if (capacity < words) return fail(OLMC_ERR_ARG, "stamp buffer too small: need 5 * workgroups + 1 words");
    rc = bulk_reserve(c, sizeof(uint64_t) * static_cast<size_t>(words));
    if (rc) return rc;
    uint64_t* const d_stamps = c->bulk.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(d_stamps, 0, sizeof(uint64_t) * static_cast<size_t>(words), c->stream));
    ContractSet<1> cs;
    cs.c[0] = make_contract(make_option(100.0, 100.0, 1.0, 0.05, 0.2, 0.0, 1), n_steps);
    cs.base_mask = 1u; cs.upper_continues_slot0 = 0;
    EventPair ep{};
    rc = prof_acquire(c, &ep);
    if (rc) return rc;
    struct GiveBack {                                // the pair goes back to the free list however the call leaves
        DeviceCtx* c; EventPair ep;
        ~GiveBack() { c->ev_free.push_back(ep); }
    } give_back{c, ep};
    ReduceWs ws;
    rc = make_ws(c, c->stream, grid, 2, c->d_result, -1.0, &ws);
    if (rc) return rc;
    // `lead_launches` identical launches go out back to back in front of the recorded one (each overwrites the stamps of the one
    // before; only the last is armed to raise the completion word): the recorded launch then runs on a device that is already under
    // this very load, at the clock it holds there -- a lone launch between a memset and a copy ran 16 % slow
    ReduceWs quiet = ws;
    quiet.done_flag = nullptr;
    for (int32_t k = 0; k < lead_launches; ++k) {
        hipLaunchKernelGGL(european_stamp_kernel, dim3(grid), dim3(kBlock), 0, c->stream, pr, cs, quiet, d_stamps);
        rc = after_launch(c, c->stream);             // a failed launch leaves the self-resetting counters to ws_recover()
        if (rc) return rc;
    }
    hipExtLaunchKernelGGL(european_stamp_kernel, dim3(grid), dim3(kBlock), 0, c->stream, ep.start, ep.stop, 0, pr, cs, ws, d_stamps);
    rc = after_launch(c, c->stream);
    if (rc) return rc;
    rc = sync_or_recover(c, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stamps_host, d_stamps, sizeof(uint64_t) * static_cast<size_t>(words), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ep.start, ep.stop));
    info3[0] = grid;
    info3[1] = pr.split_from == INT32_MAX ? grid : pr.split_from;
    info3[2] = static_cast<int64_t>(static_cast<double>(ms) * 1e6);
    return OLMC_OK;
}

// Issue cost of one instruction class on this device (see the probe kernels): nanoseconds one SIMD needs per wave64
// instruction of the class with `waves_per_simd` waves resident.
extern "C" int olmc_issue_probe(int op, int waves_per_simd, double* ns_per_instr) {
    using Probe = void (*)(uint32_t*, uint32_t, uint32_t);
    static const Probe table[] = {probe_mad_u64_u32, probe_bitop3, probe_cvt_f32_u32, probe_fmamk_f32, probe_and_or, probe_log_f32,
                                  probe_sqrt_f32, probe_sin_f32, probe_cos_f32, probe_exp_f32, probe_add_f32, probe_fma_f32,
                                  probe_cvt_f64_f32, probe_add_f64, probe_fma_f64, probe_rndne_f64, probe_ldexp_f64, probe_cvt_i32_f64,
                                  probe_mix_log_add, probe_mix_log_bitop3, probe_bitop3_vvv, probe_bitop3_vvc, probe_xor_vv, probe_mix_bitop3_add,
                                  probe_mix_mad_bitop3, probe_mad_u64_u32_vv};
    constexpr int kOps = static_cast<int>(sizeof(table) / sizeof(table[0]));
    static_assert(kOps == OLMC_PROBE_COUNT, "include/olmc_probe.h lists the probe classes");
    if (!ns_per_instr) return fail(OLMC_ERR_ARG, "null pointer");
    if (op < 0 || op >= kOps) return fail(OLMC_ERR_ARG, "unknown probe class");
    if (waves_per_simd < 1 || waves_per_simd > 8) return fail(OLMC_ERR_ARG, "waves_per_simd must be in [1, 8]");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    rc = bulk_reserve(c, 256);
    if (rc) return rc;
    const dim3 grid(static_cast<uint32_t>(c->cus * waves_per_simd)), block(kBlock);    // one 4-wave workgroup per (CU, resident wave slot)
    EventPair ep{};
    rc = prof_acquire(c, &ep);
    if (rc) return rc;
    for (int rep = 0; rep < 2; ++rep) {          // first launch warms the instruction cache
        hipExtLaunchKernelGGL(table[op], grid, block, 0, c->stream, ep.start, ep.stop, 0, c->bulk.as<uint32_t>(), 1u, 0xD2511F53u);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ep.start, ep.stop));
    c->ev_free.push_back(ep);
    *ns_per_instr = static_cast<double>(ms) * 1e6 / (static_cast<double>(kProbeIters) * 16.0 * waves_per_simd);
    return OLMC_OK;
}



// The European call with fp64 normals (european_f64_normals_kernel): one launch of n_paths x n_steps, one workgroup per 256 paths
// (n_paths <= 2^18 x 256), antithetic.  Timed like every pricing when olmc_profile_enable is on.
extern "C" int olmc_european_f64_normals(double S, double K, double T, double r, double sigma, double q, int is_call, int64_t n_paths,
                                         int32_t n_steps, uint64_t seed, olmc_stats* out) {
    if (n_paths > static_cast<int64_t>(kMaxGrid) * kBlock) return fail(OLMC_ERR_ARG, "n_paths too large for one workgroup per 256 paths");
    const olmc_option o = make_option(S, K, T, r, sigma, q, is_call);
    ContractSet<1> cs;
    cs.c[0] = make_contract(o, n_steps);
    cs.base_mask = 1u; cs.upper_continues_slot0 = 0;
    const int saved_cap = g_grid_cap;
    g_grid_cap = kMaxGrid;                               // one workgroup per 256 paths whatever the step count (no short-path grid cap)
    const int rc = run_structured(0, n_paths, n_steps, seed, 1, r, T, poisoned(S, K, T, r, sigma, q), out,
                                  [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                                      launch_timed(european_f64_normals_kernel, dim3(grid), dim3(kBlock), st, timed, pr, cs, ws);
                                  });
    g_grid_cap = saved_cap;
    return rc;
}

// Microseconds one more DEPENDENT launch costs on a stream: wall of a chain of `n` empty kernels, minus nothing, over n.
extern "C" int olmc_launch_gap_probe(int32_t n, double* us_per_launch) {
    if (!us_per_launch || n < 2 || n > 100000) return fail(OLMC_ERR_ARG, "bad arguments");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    for (int rep = 0; rep < 2; ++rep) {                  // the first chain warms the code object
        HIP_TRY(hipStreamSynchronize(c->stream));
        const auto t0 = std::chrono::steady_clock::now();
        for (int32_t k = 0; k < n; ++k) hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(kWave), 0, c->stream, reinterpret_cast<uint32_t*>(c->d_result));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        *us_per_launch = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / n;
    }
    return OLMC_OK;
}

// Test seams of the instrumented build (none of them exists in libolmc.so).
extern "C" int olmc_probe_tune(int knob, int value) {
    if (knob == OLMC_PROBE_TUNE_FAULT_SHARD && value >= 0 && value <= kMaxDevices) { g_fault_shard = value; return OLMC_OK; }
    if (knob == OLMC_PROBE_TUNE_FORCE_NV && value >= 0 && value <= kMaxNV) { g_force_nv = value; return OLMC_OK; }
    if (knob == OLMC_PROBE_TUNE_MULTI_REHEARSAL && value >= 0 && value <= 1) { g_multi_rehearsal = value; return OLMC_OK; }
    if (knob == OLMC_PROBE_TUNE_EXPECT_TABLE && value >= -1 && value <= 1) {
        g_expect_table = value;
        const int misses = g_expect_table_misses.exchange(0);
        return misses ? fail(OLMC_ERR_STATE, std::to_string(misses) + " European launches did not meet OLMC_PROBE_TUNE_EXPECT_TABLE") : OLMC_OK;
    }
    return fail(OLMC_ERR_ARG, "unknown probe knob or value");
}
