// aesw_align.h -- the one alignment predicate of every argument check: aesw_ctx.h brings it to the translation units of the C
// ABI, aesw_entry_rules.h to the rules a plain g++ test compiles.  No include of the project and none of ROCm.
#pragma once
#include <stdint.h>

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }  // a: a power of two
