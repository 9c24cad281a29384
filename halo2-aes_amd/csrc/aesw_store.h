// aesw_store.h -- the store flavour, once: what a flavour is on the device (gstore<MODE>) and how a launcher turns the option's
// runtime value into the instantiation (with_value / with_nt).  One source for aesw_kernels.hip and for the gathers of the
// libraries next to libaesw.so (perm/aesw_perm.hip, theta/aesw_theta.hip).  Include from a HIP translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace aesw {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Store flavours: 0 plain, 1 nontemporal (nt), 2 write-through at agent scope
// (sc1).  Plain / nt lines stay dirty in the XCD's L2 and are written back at
// the kernel boundary (that costs dirty bytes / ~6 TB/s after the last wave has
// finished); sc1 stores leave L2 as they are issued, so a launch ends with
// nothing left to flush (MI355X_MICROARCH.md, "stores of each flavour").
// Modes 3..5 (tools/ only) exist in -DAESW_DIAGNOSTIC builds alone: 3 = leave the flush out (compute + staging only),
// 4 = flush only (no AES work, no staging writes: the store schedule fed from whatever LDS holds), 5 = as 4 without the
// LDS reads.  Their output is garbage; they price the parts of a launch.
template <int MODE>
__device__ __forceinline__ void gstore(u32x4 *p, const u32x4 &v) {
    if (MODE == 3) return;
    // hipcc neither counts nor pads an asm store: the trailing s_nop 1 covers the ">64-bit store data
    // overwritten by the next instruction" hazard (cdna guide 5.7 item 1); nothing ever waits on these stores.
    if (MODE == 2 || MODE >= 4) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
    else if (MODE == 1) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <int MODE>
__device__ __forceinline__ void gstore(u32x2 *p, const u32x2 &v) {
    if (MODE == 3) return;
    if (MODE == 2 || MODE >= 4) asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 0" : : "v"(p), "v"(v) : "memory");
    else if (MODE == 1) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// ---- dispatch: a runtime value -> one template instantiation ---------------------------------------------------------
template <int N> using Int = std::integral_constant<int, N>;
#define AESW_V(c) decltype(c)::value  // the value of an Int<N> argument, as a constant expression
// f(Int<v>{}) for v among the listed values; the last one also takes every other v
template <int A, int... Rest, class F>
static auto with_value(int v, F &&f) {
    if constexpr (sizeof...(Rest) == 0) return f(Int<A>{});
    else return v == A ? f(Int<A>{}) : with_value<Rest...>(v, f);
}
// the store flavour: 0 plain, 1 nontemporal, 2 write-through ("store_mode" / "key_store_mode" / "fr_store_mode")
template <class F> static auto with_nt(int nt, F &&f) { return with_value<2, 1, 0>(nt, f); }

}  // namespace aesw
