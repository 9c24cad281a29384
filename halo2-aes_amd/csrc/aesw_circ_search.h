// aesw_circ_search.h -- which circuit owns block b of a many-circuit batch (include/aesw_circ.h): circuit c owns blocks
// [offsets[c], offsets[c+1]).  One source for the device checker (circ/aesw_circ_check.hip, wave-uniform: the loads are scalar)
// and the host (aesw_circ_circuit_of_block, which the CPU tests hold against numpy.searchsorted).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AESW_CIRC_HD __host__ __device__ __forceinline__
#else
#define AESW_CIRC_HD inline
#endif

namespace aesw_circ {

// The last circuit c with offsets[c] <= b, in upper-bound form: the first i in 1 .. C-1 with offsets[i] > b, minus one, so a
// run of empty circuits (equal offsets) is skipped and the block goes to the circuit that holds it.  For offsets that start
// at 0 and do not decrease, and b < offsets[C], that is searchsorted(offsets, b, side = "right") - 1.  Whatever the offsets
// hold, only offsets[1 .. C-1] are read (at most ceil(log2 C) of them) and the result lies in [0, C): broken offsets change
// which key slab a block is held against, never an address outside the batch.
// OFFSETS: const uint64_t *, or on the device the same pointer in the constant address space (nothing writes the offsets while
// the kernel runs), which is what makes the compiler load them with scalar instructions.
template <class OFFSETS>
AESW_CIRC_HD uint32_t circuit_of_block(OFFSETS offsets, uint32_t n_circuits, uint64_t b) {
    uint32_t lo = 1, hi = n_circuits;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= b) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

}  // namespace aesw_circ
