// subdiv.hip — one level of Loop / midpoint mesh subdivision as a linear operator on per-vertex arrays, and its transpose:
//   psdr_hip_subdiv_apply:      y[n_out, C]  = S x          psdr_hip_subdiv_apply_adj:  d_x[n_in, C] = S^T d_y
// S (n_out x n_in) and S^T (n_in x n_out) both arrive as CSR from the host (psdr_jit_amd/subdiv.py builds the topology, the float32 weights and the
// transpose once per mesh and level); the device never forms a transpose and never scatters.  Both directions are the SAME kernel over a different CSR:
// one lane owns one output row, carries its C accumulators (C = 1 .. 4: scalars, uv pairs, positions / RGB, RGBA) and walks the row's entries in stored
// order with acc = fmaf(w, x, acc) from 0.  Rows beyond one pass of the grid are taken by a grid-stride loop, as in precond.hip.
// No atomics, no dependence on which workgroup ran when: the same input gives the same bits.  apply / apply_adj are one plain launch on the caller's
// stream: no copy to the host, no synchronisation.
// A lane walks its row alone, so a launch runs as long as its longest row (the hub of a 200-triangle fan: 201 entries; a hub of a closed 200-gon bipyramid: 601 in the transpose);
// meshes have bounded valence almost everywhere (the bunny: 11 forward, 31 transposed), and that is accepted at these sizes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"

namespace {

constexpr int kThreads = 256;          // 4 waves
constexpr int kMaxBlocks = 1024;       // rows beyond kMaxBlocks * kThreads: grid-stride
constexpr int kAhead = 4;              // entries whose loads are in flight together

struct Csr { int rows; const int *row_begin, *col; const float *weight; };

template <int C> __global__ void __launch_bounds__(kThreads) k_spmv(Csr A, const float *__restrict__ x, float *__restrict__ y) {
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < A.rows; i += (long long) gridDim.x * kThreads) {
        const int b0 = A.row_begin[i], b1 = A.row_begin[i + 1];
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        int k = b0;
        // four entries' loads are issued before the first of their multiply-adds: a lane's gathers depend on its col loads, and a row walked one entry at a
        // time costs one memory round trip per entry.  The multiply-adds stay in stored order: the bits are those of the plain loop below.
        for (; k + kAhead <= b1; k += kAhead) {
            float w[kAhead], xv[kAhead][C];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                w[u] = A.weight[k + u];
                const float *xj = x + (long long) A.col[k + u] * C;
#pragma unroll
                for (int c = 0; c < C; ++c) xv[u][c] = xj[c];
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = fmaf(w[u], xv[u][c], acc[c]);
        }
        for (; k < b1; ++k) {
            const float w = A.weight[k];
            const float *xj = x + (long long) A.col[k] * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = fmaf(w, xj[c], acc[c]);
        }
        float *yi = y + i * C;
#pragma unroll
        for (int c = 0; c < C; ++c) yi[c] = acc[c];
    }
}

int launch(const char *who, const Csr &A, const float *x, int32_t C, float *y, void *stream) {
    if (!x || !y) return psdr::api_fail(std::string(who) + ": NULL argument");
    if (x == y) return psdr::api_fail(std::string(who) + ": input and output must be different arrays");
    if (C < 1 || C > 4) return psdr::api_fail(std::string(who) + ": C = " + std::to_string(C) + ", must be in [1, 4]");
    const int blocks = (int) std::min<long long>(kMaxBlocks, ((long long) A.rows + kThreads - 1) / kThreads);
    hipStream_t s = (hipStream_t) stream;
    switch (C) {
    case 1: k_spmv<1><<<blocks, kThreads, 0, s>>>(A, x, y); break;
    case 2: k_spmv<2><<<blocks, kThreads, 0, s>>>(A, x, y); break;
    case 3: k_spmv<3><<<blocks, kThreads, 0, s>>>(A, x, y); break;
    default: k_spmv<4><<<blocks, kThreads, 0, s>>>(A, x, y); break;
    }
    return launch_status(std::string(who) + ": ");
}

// the host-side check of one CSR: "" or what is wrong with it
std::string check_csr(const char *name, int32_t rows, int32_t cols, const int32_t *row_begin, const int32_t *col, const float *weight) {
    const std::string n(name);
    if (!row_begin) return n + "row_begin is NULL";
    if (row_begin[0] != 0) return n + "row_begin[0] = " + std::to_string(row_begin[0]) + ", must be 0";
    for (int32_t i = 0; i < rows; ++i)
        if (row_begin[i + 1] < row_begin[i]) return n + "row_begin is not monotonic at row " + std::to_string(i);
    const int32_t nnz = row_begin[rows];
    if (nnz > 0 && (!col || !weight)) return n + (col ? "weight" : "col") + " is NULL";
    for (int32_t i = 0; i < rows; ++i)
        for (int32_t k = row_begin[i]; k < row_begin[i + 1]; ++k) {
            if (col[k] < 0 || col[k] >= cols)
                return n + "col[" + std::to_string(k) + "] = " + std::to_string(col[k]) + " of row " + std::to_string(i) + " is outside [0, " + std::to_string(cols) + ")";
            if (!std::isfinite(weight[k])) return n + "weight[" + std::to_string(k) + "] of row " + std::to_string(i) + " is not finite";
        }
    return "";
}

} // namespace

struct psdr_hip_subdiv {
    Csr S{}, T{};                      // S: n_out rows over n_in columns; T = S^T as the host gave it
    int *d_ints = nullptr;             // row_begin[n_out + 1], col[nnz], t_row_begin[n_in + 1], t_col[nnz]
    float *d_weights = nullptr;        // weight[nnz], t_weight[nnz]
    ~psdr_hip_subdiv() {
        if (d_ints) (void) hipFree(d_ints);
        if (d_weights) (void) hipFree(d_weights);
    }
};

extern "C" {

int psdr_hip_subdiv_create(int32_t n_in, int32_t n_out, const int32_t *row_begin, const int32_t *col, const float *weight,
                           const int32_t *t_row_begin, const int32_t *t_col, const float *t_weight, psdr_hip_subdiv **out, void *stream) {
    const std::string who = "psdr_hip_subdiv_create: ";
    if (!out) return psdr::api_fail(who + "out is NULL");
    *out = nullptr;
    if (n_in <= 0 || n_out <= 0) return psdr::api_fail(who + "n_in = " + std::to_string(n_in) + ", n_out = " + std::to_string(n_out) + ", both must be positive");
    if ((long long) n_out * 4 >= (1LL << 31) || (long long) n_in * 4 >= (1LL << 31))
        return psdr::api_fail(who + "n_in = " + std::to_string(n_in) + ", n_out = " + std::to_string(n_out) + ": 4 n must stay below 2^31");
    std::string bad = check_csr("", n_out, n_in, row_begin, col, weight);
    if (!bad.empty()) return psdr::api_fail(who + bad);
    bad = check_csr("t_", n_in, n_out, t_row_begin, t_col, t_weight);
    if (!bad.empty()) return psdr::api_fail(who + bad);
    const int32_t nnz = row_begin[n_out];
    if (t_row_begin[n_in] != nnz)
        return psdr::api_fail(who + "row_begin ends at " + std::to_string(nnz) + " entries, t_row_begin at " + std::to_string(t_row_begin[n_in]) + ": a matrix and its transpose have the same number");
    // the lists are sound: from here on the device is touched
    hipStream_t s = (hipStream_t) stream;
    psdr_hip_subdiv *h = new psdr_hip_subdiv();
    const size_t rb = (size_t) n_out + 1, trb = (size_t) n_in + 1, z = (size_t) nnz;
    hipError_t e = hipMalloc((void **) &h->d_ints, (rb + trb + 2 * z) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **) &h->d_weights, std::max<size_t>(2 * z, 1) * sizeof(float));
    int *d_rb = h->d_ints, *d_col = d_rb + rb, *d_trb = d_col + z, *d_tcol = d_trb + trb;
    float *d_w = h->d_weights, *d_tw = d_w + z;
    if (e == hipSuccess) e = hipMemcpyAsync(d_rb, row_begin, rb * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_trb, t_row_begin, trb * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(d_col, col, z * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(d_tcol, t_col, z * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(d_w, weight, z * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(d_tw, t_weight, z * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);            // the host arrays are the caller's again when the call returns
    if (e != hipSuccess) { delete h; return psdr::api_fail(who + hipGetErrorString(e)); }
    h->S = Csr{n_out, d_rb, d_col, d_w};
    h->T = Csr{n_in, d_trb, d_tcol, d_tw};
    *out = h;
    return 0;
}

int psdr_hip_subdiv_destroy(psdr_hip_subdiv *h) {
    if (!h) return psdr::api_fail("psdr_hip_subdiv_destroy: handle is NULL");
    delete h;
    return 0;
}

int psdr_hip_subdiv_apply(const psdr_hip_subdiv *h, const float *x, int32_t C, float *y, void *stream) {
    if (!h) return psdr::api_fail("psdr_hip_subdiv_apply: handle is NULL");
    return launch("psdr_hip_subdiv_apply", h->S, x, C, y, stream);
}

int psdr_hip_subdiv_apply_adj(const psdr_hip_subdiv *h, const float *d_y, int32_t C, float *d_x, void *stream) {
    if (!h) return psdr::api_fail("psdr_hip_subdiv_apply_adj: handle is NULL");
    return launch("psdr_hip_subdiv_apply_adj", h->T, d_y, C, d_x, stream);
}

} // extern "C"
