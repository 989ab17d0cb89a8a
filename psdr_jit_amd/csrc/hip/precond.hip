// precond.hip — the Laplacian vertex preconditioner of "Large Steps in Inverse Rendering" (Nicolet et al. 2021) on the device:
//   M = I + lambda L,   L the combinatorial Laplacian of the mesh (L_ii = number of distinct neighbours, L_ij = -1 per distinct edge)
// psdr_hip_precond_apply:  y = M x        psdr_hip_precond_solve:  M x = b by Jacobi-preconditioned conjugate gradients
// for the three coordinate columns of a [n, 3] row-major float32 array at once.  Only the CSR PATTERN is stored: row i of M x is
//   (1 + lambda deg_i) x_i - lambda sum_j x_j,   deg_i = row_begin[i + 1] - row_begin[i]
// One lane owns one row and carries its three columns; a row of any length walks the same loop.
//
// The solver is a sequence of small plain launches on the caller's stream (two per iteration), with every scalar in device memory:
//   k_direction   prologue: r.z from the slab the previous launch left, beta = r.z / (r.z)_old
//                 p' = z + beta p,  q = M p' (the neighbours' p' are formed on the fly from z and the OLD p: p is double-buffered),  slab <- p'.q
//   k_update      prologue: p.q from the slab, alpha = r.z / p.q
//                 x += alpha p,  r -= alpha q,  z = r / diag,  slab <- r.z
// and once per chunk of kChunk iterations
//   k_apply<1>    r = b - M x from x itself,  z = r / diag,  slabs <- r.z and r.r        (the recurrence goes on from THIS residual)
//   k_norms       r.r from the slab -> the six floats the host reads (three |r|^2, three |b|^2), one small copy, one stream synchronise
// A dot product is a per-workgroup partial (wave shuffle, then LDS) stored to a slab; the NEXT launch's prologue adds the slab in a fixed
// order in every workgroup.  So there are no float atomics, the result does not depend on which workgroup ran when (the same b gives the
// same bits), and no workgroup ever waits for another inside a launch: no cooperative launch, no grid barrier, no spin.  The scalars a launch
// reads (slot `in`) and the ones its workgroup 0 writes (slot `out`) are different words: the slots alternate from launch to launch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"
#define PCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return psdr::api_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kThreads = 256;          // 4 waves
constexpr int kMaxBlocks = 1024;       // rows beyond kMaxBlocks * kThreads: grid-stride (a slab stays short enough to add in every prologue)
constexpr int kChunk = 8;              // iterations enqueued between two looks at the recomputed residual

struct F3 { float x, y, z; };
__device__ inline F3 ld3(const float *a, long long i) { const float *p = a + 3 * i; return F3{p[0], p[1], p[2]}; }
__device__ inline void st3(float *a, long long i, F3 v) { float *p = a + 3 * i; p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// the scalars of the recurrence, per column.  frozen: alpha = beta = 0 for the rest of the solve (|b| = 0, r.z = 0, p.q <= 0, or a quotient that is not finite)
struct State { float rz[3]; int frozen[3]; };

struct Pattern { int n; const int *row_begin, *col; float lambda; };

// sum over the workgroup, the same value in every thread: 64-lane shuffle tree, the four wave sums through LDS, added in wave order
__device__ inline F3 block_sum(F3 v, float *lds /* [12] */) {
    for (int o = 32; o > 0; o >>= 1) { v.x += __shfl_down(v.x, o, 64); v.y += __shfl_down(v.y, o, 64); v.z += __shfl_down(v.z, o, 64); }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                     // the previous use of `lds` has been read
    if ((threadIdx.x & 63) == 0) { lds[3 * wave] = v.x; lds[3 * wave + 1] = v.y; lds[3 * wave + 2] = v.z; }
    __syncthreads();
    F3 s{0.f, 0.f, 0.f};
    for (int w = 0; w < kThreads / 64; ++w) { s.x += lds[3 * w]; s.y += lds[3 * w + 1]; s.z += lds[3 * w + 2]; }
    return s;
}
// the dot product a previous launch left as `count` partials: thread t adds partials t, t + 256, ... in that order, then block_sum
__device__ inline F3 slab_sum(const float *slab, int count, float *lds) {
    F3 v{0.f, 0.f, 0.f};
    for (int k = threadIdx.x; k < count; k += kThreads) { v.x += slab[3 * k]; v.y += slab[3 * k + 1]; v.z += slab[3 * k + 2]; }
    return block_sum(v, lds);
}
__device__ inline void slab_store(float *slab, F3 v, float *lds) {
    const F3 s = block_sum(v, lds);
    if (threadIdx.x == 0) { slab[3 * blockIdx.x] = s.x; slab[3 * blockIdx.x + 1] = s.y; slab[3 * blockIdx.x + 2] = s.z; }
}
__device__ inline float diag_of(const Pattern &P, int deg) { return 1.f + P.lambda * (float) deg; }
__device__ inline F3 row_of_m(const Pattern &P, int deg, F3 xi, F3 sum) {
    const float d = diag_of(P, deg);
    return F3{d * xi.x - P.lambda * sum.x, d * xi.y - P.lambda * sum.y, d * xi.z - P.lambda * sum.z};
}

// y = M x (mode 0)  or  r = b - M x, z = r / diag, slabs <- r.z, r.r (mode 1)
template <int kResidual> __global__ void __launch_bounds__(kThreads) k_apply(Pattern P, const float *x, float *y, const float *b, float *z, float *slab_rz, float *slab_rr) {
    __shared__ float lds[12];
    F3 rz{0.f, 0.f, 0.f}, rr{0.f, 0.f, 0.f};
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < P.n; i += (long long) gridDim.x * kThreads) {
        const int b0 = P.row_begin[i], b1 = P.row_begin[i + 1];
        F3 s{0.f, 0.f, 0.f};
        for (int k = b0; k < b1; ++k) { const F3 xj = ld3(x, P.col[k]); s.x += xj.x; s.y += xj.y; s.z += xj.z; }
        F3 m = row_of_m(P, b1 - b0, ld3(x, i), s);
        if (kResidual) {
            const F3 bi = ld3(b, i);
            m = F3{bi.x - m.x, bi.y - m.y, bi.z - m.z};
            const float d = diag_of(P, b1 - b0);
            const F3 zi{m.x / d, m.y / d, m.z / d};
            st3(z, i, zi);
            rz.x += m.x * zi.x; rz.y += m.y * zi.y; rz.z += m.z * zi.z;
            rr.x += m.x * m.x; rr.y += m.y * m.y; rr.z += m.z * m.z;
        }
        st3(y, i, m);
    }
    if (kResidual) { slab_store(slab_rz, rz, lds); slab_store(slab_rr, rr, lds); }
}

// beta from the r.z slab; p' = z + beta p; q = M p'; slab <- p'.q.  first: the solve's first direction (p' = z, `p_old` is not read)
__global__ void __launch_bounds__(kThreads) k_direction(Pattern P, int first, int n_partials, const float *slab_rz, const State *in, State *out,
                                                        const float *z, const float *p_old, float *p_new, float *q, float *slab_pq) {
    __shared__ float lds[12];
    const F3 rz3 = slab_sum(slab_rz, n_partials, lds);
    const float rz[3] = {rz3.x, rz3.y, rz3.z};
    float beta[3];
    State S = *in;
    for (int c = 0; c < 3; ++c) {
        if (!(rz[c] > 0.f)) S.frozen[c] = 1;                     // r.z = 0 (|b| = 0, or converged exactly) - and NaN
        float bt = (S.frozen[c] || first) ? 0.f : rz[c] / S.rz[c];     // (not frozen: the stored r.z is > 0)
        if (!(fabsf(bt) <= 3.0e38f)) { bt = 0.f; S.frozen[c] = 1; }
        beta[c] = bt;
        S.rz[c] = rz[c];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = S;
    F3 pq{0.f, 0.f, 0.f};
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < P.n; i += (long long) gridDim.x * kThreads) {
        const int b0 = P.row_begin[i], b1 = P.row_begin[i + 1];
        F3 s{0.f, 0.f, 0.f}, pi = ld3(z, i);
        if (first) {
            for (int k = b0; k < b1; ++k) { const F3 zj = ld3(z, P.col[k]); s.x += zj.x; s.y += zj.y; s.z += zj.z; }
        } else {
            const F3 po = ld3(p_old, i);
            pi = F3{pi.x + beta[0] * po.x, pi.y + beta[1] * po.y, pi.z + beta[2] * po.z};
            for (int k = b0; k < b1; ++k) {
                const int j = P.col[k];
                const F3 zj = ld3(z, j), pj = ld3(p_old, j);
                s.x += zj.x + beta[0] * pj.x; s.y += zj.y + beta[1] * pj.y; s.z += zj.z + beta[2] * pj.z;
            }
        }
        const F3 qi = row_of_m(P, b1 - b0, pi, s);
        st3(p_new, i, pi);
        st3(q, i, qi);
        pq.x += pi.x * qi.x; pq.y += pi.y * qi.y; pq.z += pi.z * qi.z;
    }
    slab_store(slab_pq, pq, lds);
}

// alpha from the p.q slab; x += alpha p; r -= alpha q; z = r / diag; slab <- r.z
__global__ void __launch_bounds__(kThreads) k_update(Pattern P, int n_partials, const float *slab_pq, const State *in, State *out,
                                                     const float *p, const float *q, float *x, float *r, float *z, float *slab_rz) {
    __shared__ float lds[12];
    const F3 pq3 = slab_sum(slab_pq, n_partials, lds);
    const float pq[3] = {pq3.x, pq3.y, pq3.z};
    float alpha[3];
    State S = *in;
    for (int c = 0; c < 3; ++c) {
        if (!(pq[c] > 0.f)) S.frozen[c] = 1;                     // p.q <= 0: p = 0, or rounding has eaten the direction - and NaN
        float al = S.frozen[c] ? 0.f : S.rz[c] / pq[c];
        if (!(fabsf(al) <= 3.0e38f)) { al = 0.f; S.frozen[c] = 1; }
        alpha[c] = al;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = S;
    F3 rz{0.f, 0.f, 0.f};
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < P.n; i += (long long) gridDim.x * kThreads) {
        const F3 pi = ld3(p, i), qi = ld3(q, i);
        F3 xi = ld3(x, i), ri = ld3(r, i);
        xi = F3{xi.x + alpha[0] * pi.x, xi.y + alpha[1] * pi.y, xi.z + alpha[2] * pi.z};
        ri = F3{ri.x - alpha[0] * qi.x, ri.y - alpha[1] * qi.y, ri.z - alpha[2] * qi.z};
        const float d = diag_of(P, P.row_begin[i + 1] - P.row_begin[i]);
        const F3 zi{ri.x / d, ri.y / d, ri.z / d};
        st3(x, i, xi); st3(r, i, ri); st3(z, i, zi);
        rz.x += ri.x * zi.x; rz.y += ri.y * zi.y; rz.z += ri.z * zi.z;
    }
    slab_store(slab_rz, rz, lds);
}

// norms[0..2] = |r|^2 from the slab; norms[3..5] = |b|^2: the solve's first residual (x = 0) is b itself
__global__ void __launch_bounds__(kThreads) k_norms(int first, int n_partials, const float *slab_rr, float *norms) {
    __shared__ float lds[12];
    const F3 rr = slab_sum(slab_rr, n_partials, lds);
    if (threadIdx.x == 0) {
        norms[0] = rr.x; norms[1] = rr.y; norms[2] = rr.z;
        if (first) { norms[3] = rr.x; norms[4] = rr.y; norms[5] = rr.z; }
    }
}

} // namespace

struct psdr_hip_precond {
    Pattern P{};
    int blocks = 0;
    int *d_pattern = nullptr;          // row_begin[n + 1], col[nnz]
    float *d_work = nullptr;           // r, z, q, p[2]: 5 x [n, 3]
    float *d_small = nullptr;          // State[2], norms[6], the three slabs [blocks * 3]
    float *h_norms = nullptr;          // pinned, [6]
    size_t small_bytes = 0;
    ~psdr_hip_precond() {
        if (d_pattern) (void) hipFree(d_pattern);
        if (d_work) (void) hipFree(d_work);
        if (d_small) (void) hipFree(d_small);
        if (h_norms) (void) hipHostFree(h_norms);
    }
};

extern "C" {

int psdr_hip_precond_create(int32_t n, const int32_t *row_begin, const int32_t *col, float lambda, psdr_hip_precond **out, void *stream) {
    if (!out) return psdr::api_fail("psdr_hip_precond_create: out is NULL");
    *out = nullptr;
    if (!row_begin) return psdr::api_fail("psdr_hip_precond_create: row_begin is NULL");
    if (n <= 0) return psdr::api_fail("psdr_hip_precond_create: n = " + std::to_string(n) + ", must be positive");
    if (!(lambda >= 0.f) || !std::isfinite(lambda)) return psdr::api_fail("psdr_hip_precond_create: lambda must be finite and not negative");
    if (row_begin[0] != 0) return psdr::api_fail("psdr_hip_precond_create: row_begin[0] = " + std::to_string(row_begin[0]) + ", must be 0");
    for (int32_t i = 0; i < n; ++i)
        if (row_begin[i + 1] < row_begin[i])
            return psdr::api_fail("psdr_hip_precond_create: row_begin is not monotonic at row " + std::to_string(i));
    const int32_t nnz = row_begin[n];
    if (nnz > 0 && !col) return psdr::api_fail("psdr_hip_precond_create: col is NULL");
    for (int32_t i = 0; i < n; ++i)
        for (int32_t k = row_begin[i]; k < row_begin[i + 1]; ++k) {
            if (col[k] < 0 || col[k] >= n)
                return psdr::api_fail("psdr_hip_precond_create: col[" + std::to_string(k) + "] = " + std::to_string(col[k]) + " of row " + std::to_string(i) + " is outside [0, " + std::to_string(n) + ")");
            if (col[k] == i) return psdr::api_fail("psdr_hip_precond_create: row " + std::to_string(i) + " lists itself (col[" + std::to_string(k) + "])");
        }
    // the lists are sound: from here on the device is touched
    hipStream_t s = (hipStream_t) stream;
    psdr_hip_precond *h = new psdr_hip_precond();
    h->blocks = (int) std::min<long long>(kMaxBlocks, ((long long) n + kThreads - 1) / kThreads);
    const size_t pat_ints = (size_t) n + 1 + (size_t) nnz;
    h->small_bytes = 2 * sizeof(State) + 6 * sizeof(float) + 3 * (size_t) h->blocks * 3 * sizeof(float);
    hipError_t e = hipMalloc((void **) &h->d_pattern, pat_ints * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **) &h->d_work, 5 * (size_t) n * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **) &h->d_small, h->small_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **) &h->h_norms, 6 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_pattern, row_begin, ((size_t) n + 1) * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && nnz > 0) e = hipMemcpyAsync(h->d_pattern + n + 1, col, (size_t) nnz * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);            // the host arrays are the caller's again when the call returns
    if (e != hipSuccess) { delete h; return psdr::api_fail(std::string("psdr_hip_precond_create: ") + hipGetErrorString(e)); }
    h->P = Pattern{n, h->d_pattern, h->d_pattern + n + 1, lambda};
    *out = h;
    return 0;
}

int psdr_hip_precond_destroy(psdr_hip_precond *h) {
    if (!h) return psdr::api_fail("psdr_hip_precond_destroy: handle is NULL");
    delete h;
    return 0;
}

int psdr_hip_precond_apply(const psdr_hip_precond *h, const float *x, float *y, void *stream) {
    if (!h || !x || !y) return psdr::api_fail("psdr_hip_precond_apply: NULL argument");
    if (x == y) return psdr::api_fail("psdr_hip_precond_apply: x and y must be different arrays");
    k_apply<0><<<h->blocks, kThreads, 0, (hipStream_t) stream>>>(h->P, x, y, nullptr, nullptr, nullptr, nullptr);
    PCHK(hipGetLastError());
    return 0;
}

int psdr_hip_precond_solve(psdr_hip_precond *h, const float *b, float *x, float rtol, int32_t max_iter, psdr_precond_info *info, void *stream) {
    if (!h || !b || !x || !info) return psdr::api_fail("psdr_hip_precond_solve: NULL argument");
    *info = psdr_precond_info{};
    if (b == x) return psdr::api_fail("psdr_hip_precond_solve: b and x must be different arrays");
    if (!(rtol >= 0.f) || !std::isfinite(rtol)) return psdr::api_fail("psdr_hip_precond_solve: rtol must be finite and not negative");
    if (max_iter <= 0) return psdr::api_fail("psdr_hip_precond_solve: max_iter must be positive");
    hipStream_t s = (hipStream_t) stream;
    const size_t vec = (size_t) h->P.n * 3;
    float *r = h->d_work, *z = r + vec, *q = z + vec, *p[2] = {q + vec, q + 2 * vec};
    State *st = (State *) h->d_small;
    float *norms = (float *) (st + 2), *slab_rz = norms + 6, *slab_pq = slab_rz + 3 * h->blocks, *slab_rr = slab_pq + 3 * h->blocks;
    const int nb = h->blocks;
    // every word that is read before this call writes it starts from zero: x, the scalars, the slabs (r, z, q, p are written before they are read)
    PCHK(hipMemsetAsync(x, 0, vec * sizeof(float), s));
    PCHK(hipMemsetAsync(h->d_small, 0, h->small_bytes, s));
    int launches = 0, slot = 0, pcur = 0, it = 0, converged = 0;
    k_apply<1><<<nb, kThreads, 0, s>>>(h->P, x, r, b, z, slab_rz, slab_rr);          // r = b, z = b / diag, r.z, |b|^2
    k_norms<<<1, kThreads, 0, s>>>(1, nb, slab_rr, norms);
    launches += 2;
    PCHK(hipGetLastError());
    double rel[3] = {0., 0., 0.};
    while (it < max_iter && !converged) {
        const int k_end = std::min<int>(max_iter, it + kChunk);
        for (; it < k_end; ++it) {
            k_direction<<<nb, kThreads, 0, s>>>(h->P, it == 0, nb, slab_rz, st + slot, st + (slot ^ 1), z, p[pcur], p[pcur ^ 1], q, slab_pq);
            slot ^= 1; pcur ^= 1;
            k_update<<<nb, kThreads, 0, s>>>(h->P, nb, slab_pq, st + slot, st + (slot ^ 1), p[pcur], q, x, r, z, slab_rz);
            slot ^= 1;
            launches += 2;
        }
        k_apply<1><<<nb, kThreads, 0, s>>>(h->P, x, r, b, z, slab_rz, slab_rr);
        k_norms<<<1, kThreads, 0, s>>>(0, nb, slab_rr, norms);
        launches += 2;
        PCHK(hipGetLastError());
        PCHK(hipMemcpyAsync(h->h_norms, norms, 6 * sizeof(float), hipMemcpyDeviceToHost, s));
        PCHK(hipStreamSynchronize(s));
        converged = 1;
        bool finite = true;
        for (int c = 0; c < 3; ++c) {
            const double rr = h->h_norms[c], bb = h->h_norms[3 + c];
            finite = finite && std::isfinite(rr) && std::isfinite(bb);
            rel[c] = bb > 0. ? std::sqrt(rr / bb) : (rr == 0. ? 0. : INFINITY);
            if (!(std::sqrt(rr) <= (double) rtol * std::sqrt(bb))) converged = 0;
        }
        if (!finite) { converged = 0; break; }       // nothing the recurrence does brings a NaN back
    }
    info->iterations = it;
    info->converged = converged;
    info->launches = launches;
    for (int c = 0; c < 3; ++c) info->rel_residual[c] = (float) rel[c];
    return 0;
}

} // extern "C"
