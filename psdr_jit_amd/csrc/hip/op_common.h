// op_common.h — what every stand-alone operator unit (OPERATOR_UNITS of psdr_jit_amd/build.py) and atrous.h share, stated once:
//   psdr::api_fail       the one declaration of api.hip's error sink
//   launch_status        the tail of an entry point: hipGetLastError() -> 0, or api_fail(who + the error's text)
//   block_sum            the fixed-order sum over a workgroup
//   blocks_of            workgroups of THREADS lanes that cover a count
//   in_range, range_text the [1, 2^26] bound of a count of points, vertices or faces, and the message that refuses one outside it
// Everything here has internal linkage (an anonymous namespace, as when each unit held its own copy): a unit's device code is what it was with the helper in place.
// A new operator includes this file; it does not copy from it.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

namespace psdr { int api_fail(const std::string &msg); }        // api.hip: the message psdr_hip_last_error() returns, -> 1

namespace {

// the sum over the workgroup in a fixed order, valid in thread 0: a wave by shuffles, the waves one after the other.  s_red: THREADS / 64 entries of LDS.  With T = double
// the sum of 2^26 float32 terms carries one rounding, the final one, whatever the count
template <int THREADS, typename T> __device__ T block_sum(T v, T *s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                       // (s_red of the previous sum has been read)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < THREADS / 64; ++k) t += s_red[k];
    return t;
}

template <int THREADS> inline int blocks_of(int count) { return (count + THREADS - 1) / THREADS; }

inline bool in_range(long long v) { return v >= 1 && v <= (1 << 26); }

inline std::string range_text(const char *name, long long v) { return std::string(name) + " = " + std::to_string(v) + ", must lie in [1, 2^26]"; }

// after the last launch of an entry point `who` ("psdr_hip_x: "): what the entry point returns
inline int launch_status(const std::string &who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : psdr::api_fail(who + hipGetErrorString(e));
}

} // namespace
