// aesw_entry_rules.h -- the argument rules the entry points of the libraries next to libaesw.so share, once: each is a function
// that returns the refusal's text, or nullptr where the argument passes, so that an entry point keeps its own order of checks
// and says  if (const char *why = bad_k(k)) return refuse(ctx, call, why);  (aesw_entry.h).  The bounds are aesw_mult.h's.
// No HIP call, no ROCm include and no aesw_ctx: tests/test_entry_rules.py compiles this header alone with g++ and holds every
// text and every bound.
#pragma once
#include "../../include/aesw_mult.h"
#include "aesw_align.h"
#include "aesw_mult.h"

namespace aesw {

inline const char *bad_layout(int layout) {  // the libraries that read x
    return layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED ? "the layout must be DENSE or PACKED (a VALUES witness has no x)" : nullptr;
}
inline const char *bad_k(uint32_t k) { return mult_k_ok(k) ? nullptr : "k must be 2 ... 30"; }
inline const char *bad_sets(uint32_t n_sets) { return mult_sets_ok(n_sets) ? nullptr : "n_sets must be 1 ... 1024"; }
inline const char *bad_report(const void *d_report) {  // every report is addressed as u64 words
    return !d_report || !aligned_to(d_report, 8) ? "d_report must be there and 8-byte aligned" : nullptr;
}
inline const char *bad_slabs(const void *d_x, const void *d_y, const void *d_z) {  // block slabs, staged 16 bytes at a time
    return !d_x || !d_y || !d_z || !aligned_to(d_x, 16) || !aligned_to(d_y, 16) || !aligned_to(d_z, 16) ? "d_x, d_y and d_z must be there and 16-byte aligned"
                                                                                                       : nullptr;
}
// what the grand-product calls (grand, sigma) take alike: the challenges, Z with its closing cells, the workspace -- Fr cells all
inline const char *bad_challenges(const void *d_beta, const void *d_gamma) {
    return !d_beta || !d_gamma || !aligned_to(d_beta, 16) || !aligned_to(d_gamma, 16) ? "d_beta and d_gamma must be there and 16-byte aligned" : nullptr;
}
inline const char *bad_product_outputs(const void *d_z_fr, const void *d_closing_fr) {
    return !d_z_fr || !d_closing_fr || !aligned_to(d_z_fr, 16) || !aligned_to(d_closing_fr, 16) ? "d_z_fr and d_closing_fr must be there and 16-byte aligned" : nullptr;
}
inline const char *bad_workspace(const void *d_workspace) {
    return !d_workspace || !aligned_to(d_workspace, 16) ? "d_workspace must be there and 16-byte aligned" : nullptr;
}

// The key columns of a call that may go without them: they count where all three are there and the circuit has room for the
// key schedule; only columns that count are held to their alignment.
inline bool with_keys(const aesw_key_slab *ks, uint32_t k) { return ks && ks->kx && ks->ky && ks->kz && mult_has_key_rows(k); }
inline const char *bad_key_columns(const aesw_key_slab *ks, uint32_t k) {
    return with_keys(ks, k) && (!aligned_to(ks->kx, 16) || !aligned_to(ks->ky, 16) || !aligned_to(ks->kz, 16)) ? "the key columns must be 16-byte aligned" : nullptr;
}

// what every call of the accumulators checks of its outputs and of the circuit's shape (with_k: the call takes a k)
inline const char *bad_outputs(uint32_t k, bool with_k, uint32_t n_sets, const uint32_t *d_mult, const aesw_mult_report *d_report) {
    if (const char *why = with_k ? bad_k(k) : nullptr) return why;
    if (const char *why = bad_sets(n_sets)) return why;
    if (const char *why = bad_report(d_report)) return why;
    if (!d_mult || !aligned_to(d_mult, 16)) return "d_mult must be there and 16-byte aligned";
    return nullptr;
}

}  // namespace aesw
