// aesw_report_dev.h -- what the kernels of every library do to a report alike, once: the reset a kernel node in front of a
// launch performs (report_reset: a library's __global__ of its own name wraps it; a __global__ here would be a kernel of every
// library that includes this) and the fold of a workgroup's sums and minimum into one thread (workgroup_fold).  aesw_check_dev.h
// adds the atomic forms (report_add, report_min, flush_acc) for the kernels whose whole grid reports.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aesw {

constexpr int LANES = 64;

// Thread `tid` of a launch's first `words` sets its word of the report: ~0 ("none") where `none_mask` has the word's bit, else 0.
// A kernel node, not memset nodes, so that a captured graph replays the reset as it runs eagerly.  T: the width
// the caller counts its threads in (threadIdx.x of a one-workgroup kernel, a 64-bit index over a grid).
template <class T>
__device__ __forceinline__ void report_reset(uint64_t *report, uint32_t words, uint32_t none_mask, T tid) {
    if (tid < words) {
        uint64_t *word = report + tid;  // the address first: written as report[tid] = ... the one-wave kernels take a fourth VGPR
        *word = (none_mask >> tid & 1u) ? ~0ull : 0ull;
    }
}

// N sums and one minimum of a workgroup of WAVES waves, every thread of which is here: the lanes of a wave by __shfl_xor, one
// LDS slot per wave and value, and thread 0 (`tid`: the kernel's threadIdx.x, read there) returns with the workgroup's values
// in `sum` and `first`; what the other threads hold is of no use.  The LDS is the caller's, so a kernel's static LDS stays
// what it declares.  S: uint32_t or unsigned long long.
template <int WAVES, int N, class S>
__device__ __forceinline__ void workgroup_fold(S (&sum)[N], unsigned long long &first, S (&s_sum)[N][WAVES], unsigned long long (&s_first)[WAVES], uint32_t tid) {
#pragma unroll
    for (int o = LANES / 2; o; o >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) sum[i] += __shfl_xor(sum[i], o, LANES);
        const unsigned long long other = __shfl_xor(first, o, LANES);
        first = other < first ? other : first;
    }
    const uint32_t wave = tid / LANES;
    if (tid % LANES == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) s_sum[i][wave] = sum[i];
        s_first[wave] = first;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WAVES; ++w) {
#pragma unroll
            for (int i = 0; i < N; ++i) sum[i] += s_sum[i][w];
            first = s_first[w] < first ? s_first[w] : first;
        }
    }
}

}  // namespace aesw
