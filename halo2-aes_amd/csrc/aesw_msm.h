// aesw_msm.h -- the rules of libaesw_msm.so, once: C_j = sum_i s_ji * P_i over bn256's G1, y^2 = x^3 + 3 over Fq,
// a group of prime order (cofactor 1), by the bucket method with windows of one byte.  Here: how a point lies in memory and in
// registers, the one addition law and the doubling, what a window is, how the 2^k rows are cut into slices and chunks, and the
// workspace -- written once for the kernels of msm/aesw_msm.hip and for the CPU driver of tests/msm_driver.cpp.  The fields are
// aesw_fq.h's (coordinates) and aesw_fr.h's (scalars); nothing of either is restated.
// No HIP call and no ROCm include: tests/test_msm_model.py compiles this header alone with g++.
//
// POINT FORM.  An affine point is 64 bytes, x then y, each in Montgomery form; the identity is x = y = 0, which is not on the curve
// (0 != 0 + 3).  The accumulators are homogeneous projective (X : Y : Z), x = X / Z, y = Y / Z, the identity (0 : 1 : 0) -- any
// (0 : Y : 0) with Y != 0.
// ADDITION.  The complete formulas of Renes, Costello and Batina (Eurocrypt 2016) for a = 0, algorithms 7 (projective + projective),
// 8 (projective + affine) and 9 (doubling), b3 = 3 b = 9: for a curve of odd order they hold for EVERY pair of inputs -- P + P,
// P + (-P), the identity on either side -- with no case distinction, so the lanes of a wave never part in the law.  Algorithm 8
// alone cannot take the affine identity (an affine pair has no Z = 0): msm_add_mixed selects its first argument there.  9 t is
// 8 t + t, four additions, not a product.
// WINDOWS.  A window is one byte of the canonical scalar, window w the byte w from the bottom.  An Fr cell has 32 windows (the top
// one at most 0x30), a byte column has one.  Bucket b of a window holds the sum of the points whose digit is b; bucket 0 is
// skipped.  The window's sum W = sum_b b * B_b is the sum of the suffix sums S_j = sum_(b >= j) B_b over j = 1 ... 255, and the
// commitment is Horner over the windows from the top with eight doublings between two.
// SIZES.  The rows of a column are cut into `slices` runs of msm_slice_rows() rows (the last one shorter, or empty); a workgroup of
// the bucket kernel owns one slice of one window of one column and walks it in chunks of MSM_CHUNK rows.
#pragma once
#include <stdint.h>

#include "aesw_fq.h"
#include "aesw_fr.h"

#ifndef AESW_MSM_CHUNK
#define AESW_MSM_CHUNK 4096  // L, the rows of a chunk.  tools/msm_bench.py builds measurement variants with other values.
#endif
#ifndef AESW_MSM_TARGET_WORKGROUPS
#define AESW_MSM_TARGET_WORKGROUPS 4096  // what the automatic slice count aims at over windows x columns: sixteen a CU on 256 CUs, measured (profiles/msm/README.md)
#endif

namespace aesw {

constexpr uint32_t MSM_THREADS = 256, MSM_BUCKETS = 256, MSM_LANES = 64, MSM_WAVES = MSM_THREADS / MSM_LANES;
constexpr uint32_t MSM_CHUNK = AESW_MSM_CHUNK;
constexpr uint32_t MSM_WORDS_PER_THREAD = MSM_CHUNK / (4 * MSM_THREADS);  // a thread reads its digits of a chunk four at a time
constexpr uint32_t MSM_SLICE_ALIGN = 16;                                 // a slice begins at a multiple of 16 rows
constexpr uint32_t MSM_MIN_CHUNKS_PER_SLICE = 2;  // of the automatic rule: a slice costs 256 stored buckets and 256 additions of the reduce
constexpr uint32_t MSM_MIN_K = 10, MSM_MAX_K = 28, MSM_MAX_COLS = 65535, MSM_MAX_SLICES = 65535;  // grid.x = slices, grid.z = columns
constexpr uint32_t MSM_SCALARS_FR = 0, MSM_SCALARS_BYTES = 1;
constexpr uint32_t MSM_FR_WINDOWS = 32, MSM_WINDOW_BITS = 8;
static_assert(MSM_CHUNK % (4 * MSM_THREADS) == 0 && MSM_CHUNK >= 4 * MSM_THREADS && MSM_CHUNK <= 65536, "whole words per thread; a row of a chunk is a 16-bit index");
static_assert(MSM_THREADS == MSM_BUCKETS, "thread b owns bucket b");

constexpr bool msm_k_ok(uint32_t k) { return k >= MSM_MIN_K && k <= MSM_MAX_K; }
constexpr bool msm_cols_ok(uint32_t n_cols) { return n_cols >= 1 && n_cols <= MSM_MAX_COLS; }
constexpr bool msm_scalars_ok(uint32_t scalars) { return scalars == MSM_SCALARS_FR || scalars == MSM_SCALARS_BYTES; }
constexpr uint32_t msm_windows(uint32_t scalars) { return scalars == MSM_SCALARS_FR ? MSM_FR_WINDOWS : 1u; }

// ---- the slices ------------------------------------------------------------------------------------------------------------------
// an explicit count is refused above what leaves every slice but the last at least MSM_SLICE_ALIGN rows
constexpr bool msm_slices_ok(uint32_t k, uint32_t slices) { return slices <= MSM_MAX_SLICES && slices <= ((1u << k) / MSM_SLICE_ALIGN); }
// The automatic count: AESW_MSM_TARGET_WORKGROUPS over the windows and columns of the call, at most what leaves a slice
// MSM_MIN_CHUNKS_PER_SLICE chunks, at least 1.
constexpr uint32_t msm_auto_slices(uint32_t k, uint32_t n_cols, uint32_t scalars) {
    const uint64_t groups = (uint64_t)msm_windows(scalars) * n_cols;
    const uint64_t want = (AESW_MSM_TARGET_WORKGROUPS + groups - 1) / groups;
    const uint64_t room = ((uint64_t)1 << k) / ((uint64_t)MSM_CHUNK * MSM_MIN_CHUNKS_PER_SLICE);
    const uint64_t s = want < room ? want : room;
    return s ? (uint32_t)s : 1u;
}
constexpr uint32_t msm_slices(uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices) { return slices ? slices : msm_auto_slices(k, n_cols, scalars); }
// the rows of every slice but the last: 2^k / slices rounded up, to a multiple of MSM_SLICE_ALIGN
constexpr uint32_t msm_slice_rows(uint32_t k, uint32_t slices) {
    const uint32_t per = (uint32_t)((((uint64_t)1 << k) + slices - 1) / slices);
    return (per + MSM_SLICE_ALIGN - 1) / MSM_SLICE_ALIGN * MSM_SLICE_ALIGN;
}
constexpr uint32_t msm_slice_begin(uint32_t k, uint32_t slices, uint32_t s) {  // s = slices gives the end of the last: 2^k
    const uint64_t at = (uint64_t)s * msm_slice_rows(k, slices), n = (uint64_t)1 << k;
    return (uint32_t)(at < n ? at : n);
}
constexpr uint32_t msm_slice_chunks(uint32_t k, uint32_t slices, uint32_t s) {
    return (msm_slice_begin(k, slices, s + 1) - msm_slice_begin(k, slices, s) + MSM_CHUNK - 1) / MSM_CHUNK;
}
static_assert(msm_slice_rows(10, 3) == 352 && msm_slice_begin(10, 3, 2) == 704 && msm_slice_begin(10, 3, 3) == 1024, "three slices of 2^10 rows: 352, 352 and 320");
static_assert(msm_slice_rows(10, 64) == 16 && msm_slices_ok(10, 64) && !msm_slices_ok(10, 65), "the most slices of 2^10 rows");

// ---- a point ---------------------------------------------------------------------------------------------------------------------
struct G1Affine {
    Fq x, y;
};
struct G1 {
    Fq x, y, z;
};
static_assert(sizeof(G1Affine) == 64 && sizeof(G1) == 96, "an affine point is 64 bytes, an accumulator 96");

AESW_MONT_HD constexpr G1 msm_identity() { return G1{FQ_ZERO, FQ_ONE, FQ_ZERO}; }
AESW_MONT_HD constexpr bool msm_affine_is_identity(const G1Affine &p) { return fq_is_zero(p.x) && fq_is_zero(p.y); }
AESW_MONT_HD constexpr G1 msm_select(bool take, const G1 &a, const G1 &b) {
    return G1{fq_select(take, a.x, b.x), fq_select(take, a.y, b.y), fq_select(take, a.z, b.z)};
}
AESW_MONT_HD constexpr G1 msm_from_affine(const G1Affine &p) { return msm_select(msm_affine_is_identity(p), msm_identity(), G1{p.x, p.y, FQ_ONE}); }
// y^2 == x^3 + 3, both in Montgomery form
AESW_MONT_HD constexpr bool msm_on_curve(const G1Affine &p) { return fq_eq(fq_mul(p.y, p.y), fq_add(fq_mul(fq_mul(p.x, p.x), p.x), FQ_THREE)); }

// 9 t = b3 t
AESW_MONT_HD constexpr Fq msm_times_b3(const Fq &t) {
    const Fq t2 = fq_add(t, t), t4 = fq_add(t2, t2), t8 = fq_add(t4, t4);
    return fq_add(t8, t);
}

// p + q, every pair (algorithm 7): twelve products
AESW_MONT_HD constexpr G1 msm_add(const G1 &p, const G1 &q) {
    Fq t0 = fq_mul(p.x, q.x), t1 = fq_mul(p.y, q.y), t2 = fq_mul(p.z, q.z);
    Fq t3 = fq_mul(fq_add(p.x, p.y), fq_add(q.x, q.y));
    t3 = fq_sub(t3, fq_add(t0, t1));
    Fq t4 = fq_mul(fq_add(p.y, p.z), fq_add(q.y, q.z));
    t4 = fq_sub(t4, fq_add(t1, t2));
    Fq y3 = fq_mul(fq_add(p.x, p.z), fq_add(q.x, q.z));
    y3 = fq_sub(y3, fq_add(t0, t2));
    t0 = fq_add(fq_add(t0, t0), t0);
    t2 = msm_times_b3(t2);
    Fq z3 = fq_add(t1, t2);
    t1 = fq_sub(t1, t2);
    y3 = msm_times_b3(y3);
    Fq x3 = fq_sub(fq_mul(t3, t1), fq_mul(t4, y3));
    y3 = fq_add(fq_mul(t1, z3), fq_mul(y3, t0));
    z3 = fq_add(fq_mul(z3, t4), fq_mul(t0, t3));
    return G1{x3, y3, z3};
}

// p + q, q affine (algorithm 8): eleven products; the affine identity leaves p
AESW_MONT_HD constexpr G1 msm_add_mixed(const G1 &p, const G1Affine &q) {
    Fq t0 = fq_mul(p.x, q.x), t1 = fq_mul(p.y, q.y);
    Fq t3 = fq_mul(fq_add(q.x, q.y), fq_add(p.x, p.y));
    t3 = fq_sub(t3, fq_add(t0, t1));
    const Fq t4 = fq_add(fq_mul(q.y, p.z), p.y);
    Fq y3 = fq_add(fq_mul(q.x, p.z), p.x);
    t0 = fq_add(fq_add(t0, t0), t0);
    const Fq t2 = msm_times_b3(p.z);
    Fq z3 = fq_add(t1, t2);
    t1 = fq_sub(t1, t2);
    y3 = msm_times_b3(y3);
    const Fq x3 = fq_sub(fq_mul(t3, t1), fq_mul(t4, y3));
    y3 = fq_add(fq_mul(t1, z3), fq_mul(y3, t0));
    z3 = fq_add(fq_mul(z3, t4), fq_mul(t0, t3));
    return msm_select(msm_affine_is_identity(q), p, G1{x3, y3, z3});
}

// 2 p (algorithm 9): eight products (two of them squarings)
AESW_MONT_HD constexpr G1 msm_double(const G1 &p) {
    Fq t0 = fq_mul(p.y, p.y);
    Fq z3 = fq_add(t0, t0);
    z3 = fq_add(z3, z3);
    z3 = fq_add(z3, z3);
    Fq t1 = fq_mul(p.y, p.z);
    Fq t2 = msm_times_b3(fq_mul(p.z, p.z));
    Fq x3 = fq_mul(t2, z3);
    Fq y3 = fq_add(t0, t2);
    z3 = fq_mul(t1, z3);
    t2 = fq_add(fq_add(t2, t2), t2);
    t0 = fq_sub(t0, t2);
    y3 = fq_add(x3, fq_mul(t0, y3));
    x3 = fq_mul(t0, fq_mul(p.x, p.y));
    return G1{fq_add(x3, x3), y3, z3};
}

// the affine form of p: one inversion; the identity comes out as x = y = 0 because fq_inv(0) is 0
AESW_MONT_HD constexpr G1Affine msm_to_affine(const G1 &p) {
    const Fq zi = fq_inv(p.z);
    return G1Affine{fq_mul(p.x, zi), fq_mul(p.y, zi)};
}

// ---- the scalars -----------------------------------------------------------------------------------------------------------------
// the plain value of a Montgomery cell: one product
AESW_MONT_HD constexpr Fr msm_canonical_scalar(const Fr &cell) { return fr_mul(cell, FR_RAW_ONE); }
// limb i of a plain value holds the windows 4 i ... 4 i + 3, the lowest byte first

// ---- the workspace: the digit planes (Fr scalars alone), the buckets, the window sums --------------------------------------------
// plane (column, w): 2^k bytes, byte i the window w of row i
constexpr uint64_t msm_plane_at(uint32_t k, uint32_t column, uint32_t w) { return ((uint64_t)column * MSM_FR_WINDOWS + w) << k; }
constexpr uint64_t msm_planes_bytes(uint32_t k, uint32_t n_cols, uint32_t scalars) { return scalars == MSM_SCALARS_FR ? msm_plane_at(k, n_cols, 0) : 0u; }
// bucket (column, w, slice, b), counted in points of 96 bytes from the end of the planes
constexpr uint64_t msm_bucket_at(uint32_t windows, uint32_t slices, uint32_t column, uint32_t w, uint32_t slice, uint32_t b) {
    return ((((uint64_t)column * windows + w) * slices) + slice) * MSM_BUCKETS + b;
}
// window sum (column, w), counted in points from the end of the buckets
constexpr uint64_t msm_sum_at(uint32_t windows, uint32_t column, uint32_t w) { return (uint64_t)column * windows + w; }
constexpr uint64_t msm_workspace_bytes(uint32_t k, uint32_t n_cols, uint32_t scalars, uint32_t slices) {
    if (!msm_k_ok(k) || !msm_cols_ok(n_cols) || !msm_scalars_ok(scalars) || !msm_slices_ok(k, slices)) return 0;
    const uint32_t windows = msm_windows(scalars), sl = msm_slices(k, n_cols, scalars, slices);
    return msm_planes_bytes(k, n_cols, scalars) + (msm_bucket_at(windows, sl, n_cols, 0, 0, 0) + msm_sum_at(windows, n_cols, 0)) * sizeof(G1);
}
static_assert(msm_workspace_bytes(10, 1, MSM_SCALARS_BYTES, 1) == 257 * 96 && msm_workspace_bytes(10, 1, MSM_SCALARS_FR, 2) == 32 * 1024 + 32 * (2 * 256 + 1) * 96 &&
                  msm_workspace_bytes(9, 1, 0, 1) == 0 && msm_workspace_bytes(10, 1, 2, 1) == 0 && msm_workspace_bytes(10, 1, 0, 65) == 0,
              "the workspace: 32 planes a column of cells, 256 buckets a slice and one sum a window; 0 outside the bounds");

}  // namespace aesw
