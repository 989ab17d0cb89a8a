// mesh_pair.h — the arithmetic of a (point, face) pair that pointmesh.hip and sdf.hip share, stated once; sdf.hip's gradient must give the bits pointmesh.hip's would:
//   Vec, sub, dot, cross2, clamped, load3          float32 vectors, every operation one rounding, nothing fused
//   Face, load_face, residual                      a face as (a, ab, ac, b, c), and e = (p - a) - (s ab + t ac)
//   add_corners                                    the [3, 3] corner record of a face: c_k += -(bary_k) kr
//   gather_corners                                 the body of the vertex kernel: a lane per vertex adds the corner records that name it, in the topology's order
// Internal linkage throughout (see op_common.h).  A new operator includes this file; it does not copy from it.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct Vec { float x, y, z; };
struct Face { Vec a, ab, ac, b, c; };

__device__ __forceinline__ Vec sub(Vec p, Vec q) { return {__fsub_rn(p.x, q.x), __fsub_rn(p.y, q.y), __fsub_rn(p.z, q.z)}; }
__device__ __forceinline__ float dot(Vec p, Vec q) { return __fadd_rn(__fadd_rn(__fmul_rn(p.x, q.x), __fmul_rn(p.y, q.y)), __fmul_rn(p.z, q.z)); }
__device__ __forceinline__ float cross2(float a, float b, float c, float d) { return __fsub_rn(__fmul_rn(a, b), __fmul_rn(c, d)); }          // a b - c d

__device__ __forceinline__ int clamped(int i, int count) { return min(max(i, 0), count - 1); }

__device__ __forceinline__ Vec load3(const float *__restrict__ a, int i) { return {a[3LL * i], a[3LL * i + 1], a[3LL * i + 2]}; }

// face f of the mesh: vertex ids clamped into [0, nv)
__device__ __forceinline__ Face load_face(const float *v, int nv, const int *faces, int f) {
    Face r;
    r.a = load3(v, clamped(faces[3LL * f], nv));
    r.b = load3(v, clamped(faces[3LL * f + 1], nv));
    r.c = load3(v, clamped(faces[3LL * f + 2], nv));
    r.ab = sub(r.b, r.a);
    r.ac = sub(r.c, r.a);
    return r;
}

// e = ap - (s ab + t ac): p - q without the cancellation
__device__ __forceinline__ Vec residual(Vec ap, const Face &f, float s, float t) {
    return {__fsub_rn(ap.x, __fadd_rn(__fmul_rn(s, f.ab.x), __fmul_rn(t, f.ac.x))),
            __fsub_rn(ap.y, __fadd_rn(__fmul_rn(s, f.ab.y), __fmul_rn(t, f.ac.y))),
            __fsub_rn(ap.z, __fadd_rn(__fmul_rn(s, f.ab.z), __fmul_rn(t, f.ac.z)))};
}

// c[3][3] += -(bary_c) kr, bary: the pair's three barycentrics.  (sdf.hip's k_grad_faces states these three lines in place: called from there, the compiler swaps the
// operands of six of its multiplications - the same products, but not the same instruction stream as before the helpers were shared.)
__device__ __forceinline__ void add_corners(float *c, Vec kr, const float *bary) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[3 * k] = __fadd_rn(c[3 * k], -__fmul_rn(kr.x, bary[k]));
        c[3 * k + 1] = __fadd_rn(c[3 * k + 1], -__fmul_rn(kr.y, bary[k]));
        c[3 * k + 2] = __fadd_rn(c[3 * k + 2], -__fmul_rn(kr.z, bary[k]));
    }
}

// the body of k_eval_vertices / k_grad_vertices, a lane per vertex i: E.grad_v[i] = the sum of the corner records (E.corners [E.nf, 3, 3]) that name it, in the order of
// E.vc_corner [E.vc_begin[i], E.vc_begin[i + 1]).  E: the kernel's argument, which has these members and nv; it is read member by member where a value is used, and the
// lane's index and early return are in here too: with either outside, the kernels came out with other register numbers than before
template <int THREADS, class Args> __device__ __forceinline__ void gather_corners(const Args &E) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= E.nv) return;
    const int total = 3 * E.nf;
    const int b0 = min(max(E.vc_begin[i], 0), total), b1 = min(max(E.vc_begin[i + 1], b0), total);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int k = b0; k < b1; ++k) {
        const float *c = E.corners + 3LL * clamped(E.vc_corner[k], total);
        gx = __fadd_rn(gx, c[0]);
        gy = __fadd_rn(gy, c[1]);
        gz = __fadd_rn(gz, c[2]);
    }
    float *o = E.grad_v + 3LL * i;
    o[0] = gx;
    o[1] = gy;
    o[2] = gz;
}

} // namespace
