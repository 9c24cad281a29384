/*
 * aesw_perm.c -- plookup's permuted columns of one circuit, counted instead of sorted, from plain C.
 *
 *   One FixedAes128Config<17, 2> circuit is generated as a PACKED witness and its lookups are accumulated into the histograms of
 *   libaesw_acc.so.  aesw_perm_build_device then arranges the 5 * N lookup arguments over u = 2^K - 6 usable rows: for every
 *   position of the permuted input column A' and of the permuted table column S' the table row that stands there.  The host
 *   checks plookup's relations on the row indices -- A' holds row r as often as the histogram says and the all-zero row in the
 *   rest, S' is the table column over u rows, A'[0] == S'[0], A'[i] == S'[i] or A'[i] == A'[i - 1] --, then "compresses" the
 *   table with a stand-in for theta (66 561 arbitrary 32-byte cells), gathers the Xor argument of set 0 through
 *   aesw_perm_gather_fr_device and checks the last two relations again on the cells.
 *
 * usage: aesw_perm [K [N]]                 (default 17 2; K >= 17)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_perm.c -L halo2-aes_amd -laesw_perm -laesw_acc
 *            -laesw -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_perm_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_acc.h"
#include "aesw_perm.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define AK(x) do { int r_ = (x); if (r_ != AESW_OK) { fprintf(stderr, "%s: %s (%s)\n", #x, aesw_strerror(r_), aesw_last_error(ctx)); return 3; } } while (0)

/* GF(2^8) tables generated arithmetically; S_BOX[255] = 23 as in the reference (src/constant.rs:14) */
static uint8_t xt(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
static uint8_t gmul(uint8_t a, uint8_t b) { uint8_t p = 0; while (b) { if (b & 1) p ^= a; a = xt(a); b >>= 1; } return p; }
static void tables(uint8_t sbox[256], uint8_t m2[256], uint8_t m3[256]) {
    for (int i = 0; i < 256; ++i) {
        uint8_t inv = 0;
        if (i) for (int j = 1; j < 256; ++j) if (gmul((uint8_t)i, (uint8_t)j) == 1) { inv = (uint8_t)j; break; }
        uint8_t s = inv, r = inv;
        for (int k = 0; k < 4; ++k) { r = (uint8_t)((r << 1) | (r >> 7)); s ^= r; }
        sbox[i] = s ^ 0x63;
        m2[i] = xt((uint8_t)i);
        m3[i] = (uint8_t)(xt((uint8_t)i) ^ i);
    }
    sbox[255] = 23;
}

/* the sections in tag order, 1 (U8), 2 (Xor), 3 (Sbox), 4 (GfMul2), 5 (GfMul3): where each starts is aesw_mult.h's rule */
static const uint32_t first_row[5] = {0, 512, 256, 66048, 66304}, section_rows[5] = {256, 65536, 256, 256, 256};

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 17, n_sets = argc > 2 ? (uint32_t)atoi(argv[2]) : 2;
    if (k < 17 || k > 24) { fprintf(stderr, "K must be 17 ... 24 here: 2^K rows hold the table's 66 561\n"); return 1; }
    const uint64_t n = aesw_block_capacity(k, n_sets), rows = 1ull << k;
    const uint32_t u = (uint32_t)rows - 6, pad_row = 0, ZERO = AESW_TABLE_ROWS - 1;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    const int P = AESW_LAYOUT_PACKED;

    uint8_t *pt = (uint8_t *)malloc(n * 16), key[16];
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (int i = 0; i < 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; key[i] = (uint8_t)(x >> 32); }

    uint8_t *d_pt, *d_key, *d_px, *d_py, *d_pz, *d_table, *d_cells;
    uint32_t *d_mult, *d_a, *d_s;
    void *d_ws;
    aesw_key_slab ks;
    aesw_mult_report *d_mrep, mrep;
    aesw_perm_report *d_rep, rep;
    const size_t mult_bytes = (size_t)n_sets * AESW_TABLE_ROWS * sizeof(uint32_t), col_words = (size_t)n_sets * AESW_PERM_ARGUMENTS * rows;
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_key, 16));
    CK(hipMalloc((void **)&d_px, n * aesw_column_stride(P, 0)));
    CK(hipMalloc((void **)&d_py, n * aesw_column_stride(P, 1)));
    CK(hipMalloc((void **)&d_pz, n * aesw_column_stride(P, 2)));
    CK(hipMalloc((void **)&ks.w, AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, aesw_key_column_stride(P, 0)));
    CK(hipMalloc((void **)&ks.ky, aesw_key_column_stride(P, 1)));
    CK(hipMalloc((void **)&ks.kz, aesw_key_column_stride(P, 2)));
    CK(hipMalloc((void **)&d_mult, mult_bytes));
    CK(hipMalloc((void **)&d_mrep, sizeof mrep));
    CK(hipMalloc((void **)&d_a, col_words * 4));
    CK(hipMalloc((void **)&d_s, col_words * 4));
    CK(hipMalloc(&d_ws, aesw_perm_workspace_bytes(n_sets)));
    CK(hipMalloc((void **)&d_rep, sizeof rep));
    CK(hipMalloc((void **)&d_table, (size_t)AESW_TABLE_ROWS * 32));
    CK(hipMalloc((void **)&d_cells, 2 * (size_t)u * 32));
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_key, key, 16, hipMemcpyHostToDevice));
    CK(hipMemset(d_a, 0xa5, col_words * 4)); /* the rows at and behind u are the host's: the library leaves them alone */
    CK(hipMemset(d_s, 0xa5, col_words * 4));

    /* witness -> multiplicities -> permuted columns: one stream, nothing waits in between */
    AK(aesw_key_schedule_witness_device(ctx, d_key, 1, P, ks.w, ks.kx, ks.ky, ks.kz, NULL, NULL));
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_key, 0, n, P, d_px, d_py, d_pz, NULL, NULL, NULL));
    AK(aesw_acc_reset_device(ctx, n_sets, d_mult, d_mrep, NULL));
    AK(aesw_acc_add_device(ctx, k, n_sets, 0, n, P, d_px, d_py, d_pz, d_mult, d_mrep, NULL));
    AK(aesw_acc_add_key_device(ctx, k, P, &ks, d_mult, d_mrep, NULL));
    AK(aesw_perm_build_device(ctx, k, n_sets, u, pad_row, d_mult, d_a, d_s, d_ws, d_rep, NULL));

    uint32_t *mult = (uint32_t *)malloc(mult_bytes), *a = (uint32_t *)malloc(col_words * 4), *s = (uint32_t *)malloc(col_words * 4);
    uint32_t *seen = (uint32_t *)malloc(AESW_TABLE_ROWS * sizeof(uint32_t));
    CK(hipMemcpy(mult, d_mult, mult_bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(a, d_a, col_words * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(s, d_s, col_words * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&mrep, d_mrep, sizeof mrep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));
    if (mrep.misses != 0 || rep.arguments != 5ull * n_sets || rep.overflowed != 0 || rep.first_overflow != AESW_CHECK_NONE) {
        fprintf(stderr, "the product's own witness misses the table, or a section holds more lookups than the circuit has rows\n");
        return 4;
    }

    for (uint32_t set = 0; set < n_sets; ++set)
        for (uint32_t tag = 1; tag <= 5; ++tag) {
            const uint32_t *A = a + ((size_t)(set * 5 + tag - 1) << k), *S = s + ((size_t)(set * 5 + tag - 1) << k);
            const uint32_t *h = mult + (size_t)set * AESW_TABLE_ROWS, lo = first_row[tag - 1], hi = lo + section_rows[tag - 1];
            uint64_t lookups = 0;
            /* A': row r as often as the histogram says, in ascending order, then the all-zero row */
            memset(seen, 0, AESW_TABLE_ROWS * sizeof(uint32_t));
            for (uint32_t i = 0; i < u; ++i) {
                if (A[i] >= AESW_TABLE_ROWS || (i && A[i] < A[i - 1])) { fprintf(stderr, "A' of (%u, %u) is not sorted at %u\n", set, tag, i); return 5; }
                ++seen[A[i]];
            }
            for (uint32_t r = 0; r < ZERO; ++r) {
                const uint32_t want = r >= lo && r < hi ? h[r] : 0;
                lookups += want;
                if (seen[r] != want) { fprintf(stderr, "A' of (%u, %u) holds row %u %u times, the histogram says %u\n", set, tag, r, seen[r], want); return 5; }
            }
            if (seen[ZERO] != u - lookups) { fprintf(stderr, "A' of (%u, %u): the all-zero run\n", set, tag); return 5; }
            /* S': the table column over u rows */
            memset(seen, 0, AESW_TABLE_ROWS * sizeof(uint32_t));
            for (uint32_t i = 0; i < u; ++i) {
                if (S[i] >= AESW_TABLE_ROWS) { fprintf(stderr, "S' of (%u, %u) at %u\n", set, tag, i); return 5; }
                ++seen[S[i]];
            }
            for (uint32_t r = 0; r < AESW_TABLE_ROWS; ++r)
                if (seen[r] != 1 + (r == pad_row ? u - AESW_TABLE_ROWS : 0)) { fprintf(stderr, "S' of (%u, %u) holds row %u %u times\n", set, tag, r, seen[r]); return 5; }
            /* the neighbour relations */
            for (uint32_t i = 0; i < u; ++i)
                if (A[i] != S[i] && (i == 0 || A[i] != A[i - 1])) { fprintf(stderr, "(%u, %u): A'[%u] is neither S'[%u] nor A'[%u]\n", set, tag, i, i, i - 1); return 5; }
            for (uint64_t i = u; i < rows; ++i)
                if (A[i] != 0xa5a5a5a5u || S[i] != 0xa5a5a5a5u) { fprintf(stderr, "(%u, %u): a blinding row was written\n", set, tag); return 5; }
            printf("set %u tag %u: %llu lookups, %llu rows of the all-zero run\n", set, tag, (unsigned long long)lookups, (unsigned long long)(u - lookups));
        }

    /* theta arrives: the compressed table (here: arbitrary cells, row r recognisable), then one gather per column */
    uint8_t *table = (uint8_t *)malloc((size_t)AESW_TABLE_ROWS * 32), *cells = (uint8_t *)malloc(2 * (size_t)u * 32);
    for (uint32_t r = 0; r < AESW_TABLE_ROWS; ++r) {
        for (int b = 0; b < 32; ++b) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; table[(size_t)r * 32 + b] = (uint8_t)(x >> 24); }
        memcpy(table + (size_t)r * 32, &r, 4);
    }
    CK(hipMemcpy(d_table, table, (size_t)AESW_TABLE_ROWS * 32, hipMemcpyHostToDevice));
    AK(aesw_perm_gather_fr_device(ctx, u, d_a + ((size_t)1 << k), d_table, d_cells, NULL));               /* Xor of set 0: A' */
    AK(aesw_perm_gather_fr_device(ctx, u, d_s + ((size_t)1 << k), d_table, d_cells + (size_t)u * 32, NULL)); /* and S' */
    CK(hipMemcpy(cells, d_cells, 2 * (size_t)u * 32, hipMemcpyDeviceToHost));
    const uint8_t *FA = cells, *FS = cells + (size_t)u * 32;
    for (uint32_t i = 0; i < u; ++i) {
        if (memcmp(FA + (size_t)i * 32, table + (size_t)a[((size_t)1 << k) + i] * 32, 32) != 0) { fprintf(stderr, "cell %u is not the table's\n", i); return 6; }
        if (memcmp(FA + (size_t)i * 32, FS + (size_t)i * 32, 32) != 0 && (i == 0 || memcmp(FA + (size_t)i * 32, FA + (size_t)(i - 1) * 32, 32) != 0)) {
            fprintf(stderr, "the gathered cells miss the relation at %u\n", i);
            return 6;
        }
    }
    printf("%llu blocks (K = %u, N = %u), %u usable rows: %llu arguments arranged, %u cells gathered twice\n", (unsigned long long)n, k, n_sets, u,
           (unsigned long long)rep.arguments, u);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
