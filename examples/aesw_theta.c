/*
 * aesw_theta.c -- all four columns of every lookup argument as Fr cells, from theta and the witness alone, from plain C.
 *
 *   A key is scheduled and one FixedAes128Config<17, 1> circuit is generated as a PACKED witness.  Its lookups are counted
 *   (aesw_mult_count_device), plookup's permuted columns A' and S' are arranged as table-row indices (aesw_perm_build_device) and
 *   the input column in row order likewise (aesw_theta_inputs_device): none of that needs a challenge.  Then theta arrives --
 *   32 bytes, the only upload --: aesw_theta_compress_table_device makes the three compressed tables and four calls of
 *   aesw_theta_columns_device turn the inputs, the table column in row order (NULL), A' and S' into Fr cells.  The host checks
 *   plookup's two relations on the Fr bytes of every argument, A'[0] == S'[0] and A'[i] == S'[i] or A'[i] == A'[i - 1], and that
 *   the row-order columns are what the indices name.
 *
 * usage: aesw_theta [K]                    (default 17; K 17 ... 20)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_theta.c -L halo2-aes_amd -laesw_theta -laesw_perm
 *            -laesw_mult -laesw -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_theta_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_perm.h"
#include "aesw_theta.h"

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

static const uint32_t table_of_tag[5] = {0, 2, 1, 1, 1}; /* j(t) of aesw_theta.h, t = 1 ... 5 */

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 17, n_sets = 1;
    if (k < 17 || k > 20) { fprintf(stderr, "K must be 17 ... 20 here: 2^K rows hold the table's 66 561\n"); return 1; }
    const uint64_t n = aesw_block_capacity(k, n_sets), rows = 1ull << k;
    const uint32_t u = (uint32_t)rows - 6, pad_row = 0;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    const int P = AESW_LAYOUT_PACKED;

    uint8_t *pt = (uint8_t *)malloc(n * 16), key[16], theta[32];
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (int i = 0; i < 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; key[i] = (uint8_t)(x >> 32); }
    /* theta as the prover holds it: a canonical Montgomery cell (the top byte keeps it below r = 0x3064...) */
    for (int i = 0; i < 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; theta[i] = (uint8_t)(x >> 16); }
    theta[31] &= 0x1f;

    const size_t words = (size_t)n_sets * AESW_THETA_ARGUMENTS * rows, cells = words * 32, table_bytes = (size_t)AESW_THETA_TABLES * AESW_TABLE_ROWS * 32;
    const uint64_t offsets[2] = {0, n};
    uint8_t *d_pt, *d_key, *d_px, *d_py, *d_pz, *d_theta, *d_table, *d_col[4];
    uint32_t *d_mult, *d_a, *d_s, *d_in;
    uint64_t *d_offsets;
    void *d_ws;
    aesw_key_slab ks;
    aesw_mult_report *d_mrep, *d_irep, mrep, irep;
    aesw_perm_report *d_prep, prep;
    aesw_theta_report *d_trep, trep;
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_key, 16));
    CK(hipMalloc((void **)&d_px, n * aesw_column_stride(P, 0)));
    CK(hipMalloc((void **)&d_py, n * aesw_column_stride(P, 1)));
    CK(hipMalloc((void **)&d_pz, n * aesw_column_stride(P, 2)));
    CK(hipMalloc((void **)&ks.w, AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, aesw_key_column_stride(P, 0)));
    CK(hipMalloc((void **)&ks.ky, aesw_key_column_stride(P, 1)));
    CK(hipMalloc((void **)&ks.kz, aesw_key_column_stride(P, 2)));
    CK(hipMalloc((void **)&d_offsets, sizeof offsets));
    CK(hipMalloc((void **)&d_mult, (size_t)n_sets * AESW_TABLE_ROWS * 4));
    CK(hipMalloc((void **)&d_a, words * 4));
    CK(hipMalloc((void **)&d_s, words * 4));
    CK(hipMalloc((void **)&d_in, words * 4));
    CK(hipMalloc(&d_ws, aesw_perm_workspace_bytes(n_sets)));
    CK(hipMalloc((void **)&d_mrep, sizeof mrep));
    CK(hipMalloc((void **)&d_irep, sizeof irep));
    CK(hipMalloc((void **)&d_prep, sizeof prep));
    CK(hipMalloc((void **)&d_trep, sizeof trep));
    CK(hipMalloc((void **)&d_theta, 32));
    CK(hipMalloc((void **)&d_table, table_bytes));
    for (int c = 0; c < 4; ++c) {
        CK(hipMalloc((void **)&d_col[c], cells));
        CK(hipMemset(d_col[c], 0xa5, cells)); /* the rows at and behind u are the host's blinding rows: the library leaves them alone */
    }
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_key, key, 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_offsets, offsets, sizeof offsets, hipMemcpyHostToDevice));

    /* witness time: no challenge yet.  One stream, nothing waits in between. */
    AK(aesw_key_schedule_witness_device(ctx, d_key, 1, P, ks.w, ks.kx, ks.ky, ks.kz, NULL, NULL));
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_key, 0, n, P, d_px, d_py, d_pz, NULL, NULL, NULL));
    AK(aesw_mult_count_device(ctx, k, n_sets, 1, d_offsets, P, d_px, d_py, d_pz, &ks, d_mult, d_mrep, NULL));
    AK(aesw_perm_build_device(ctx, k, n_sets, u, pad_row, d_mult, d_a, d_s, d_ws, d_prep, NULL));
    AK(aesw_theta_inputs_device(ctx, k, n_sets, n, P, d_px, d_py, d_pz, &ks, d_in, d_irep, NULL));
    /* theta arrives: 32 bytes go up, everything else is on the device already */
    CK(hipMemcpy(d_theta, theta, 32, hipMemcpyHostToDevice));
    AK(aesw_theta_compress_table_device(ctx, d_theta, d_table, d_trep, NULL));
    const uint32_t *index[4] = {d_in, NULL, d_a, d_s}; /* inputs and table in row order, A', S' */
    for (int c = 0; c < 4; ++c) AK(aesw_theta_columns_device(ctx, k, n_sets, u, pad_row, index[c], d_table, d_col[c], NULL));

    CK(hipMemcpy(&mrep, d_mrep, sizeof mrep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&irep, d_irep, sizeof irep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&prep, d_prep, sizeof prep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&trep, d_trep, sizeof trep, hipMemcpyDeviceToHost));
    if (mrep.misses || irep.misses || irep.lookups != mrep.lookups || irep.first_miss != AESW_CHECK_NONE || prep.overflowed || trep.noncanonical ||
        trep.cells != (uint64_t)AESW_THETA_TABLES * AESW_TABLE_ROWS) {
        fprintf(stderr, "the reports disagree: %llu / %llu lookups, %llu / %llu misses\n", (unsigned long long)mrep.lookups, (unsigned long long)irep.lookups,
                (unsigned long long)mrep.misses, (unsigned long long)irep.misses);
        return 4;
    }

    uint8_t *table = (uint8_t *)malloc(table_bytes), *col[4];
    uint32_t *in = (uint32_t *)malloc(words * 4);
    CK(hipMemcpy(table, d_table, table_bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(in, d_in, words * 4, hipMemcpyDeviceToHost));
    for (int c = 0; c < 4; ++c) {
        col[c] = (uint8_t *)malloc(cells);
        CK(hipMemcpy(col[c], d_col[c], cells, hipMemcpyDeviceToHost));
    }
    static const uint8_t zero[32];
    for (uint32_t tag = 1; tag <= AESW_THETA_ARGUMENTS; ++tag) {
        const size_t at = (size_t)(tag - 1) << k;
        const uint8_t *T = table + (size_t)table_of_tag[tag - 1] * AESW_TABLE_ROWS * 32;
        const uint8_t *I = col[0] + at * 32, *C = col[1] + at * 32, *A = col[2] + at * 32, *S = col[3] + at * 32;
        uint64_t enabled = 0;
        for (uint32_t i = 0; i < u; ++i) {
            const uint32_t r = in[at + i], t = i < AESW_TABLE_ROWS ? i : pad_row;
            enabled += r != AESW_TABLE_ROWS - 1;
            if (r >= AESW_TABLE_ROWS || memcmp(I + (size_t)i * 32, T + (size_t)r * 32, 32) != 0) { fprintf(stderr, "tag %u: input cell %u is not the table's\n", tag, i); return 5; }
            if (memcmp(C + (size_t)i * 32, T + (size_t)t * 32, 32) != 0) { fprintf(stderr, "tag %u: table cell %u\n", tag, i); return 5; }
            /* plookup's two relations, on the Fr bytes */
            if (memcmp(A + (size_t)i * 32, S + (size_t)i * 32, 32) != 0 && (i == 0 || memcmp(A + (size_t)i * 32, A + (size_t)(i - 1) * 32, 32) != 0)) {
                fprintf(stderr, "tag %u: A'[%u] is neither S'[%u] nor A'[%u]\n", tag, i, i, i - 1);
                return 6;
            }
        }
        if (memcmp(T + (size_t)(AESW_TABLE_ROWS - 1) * 32, zero, 32) != 0) { fprintf(stderr, "tag %u: the all-zero row does not compress to zero\n", tag); return 5; }
        for (uint64_t i = u; i < rows; ++i)
            for (int c = 0; c < 4; ++c)
                if (col[c][(at + i) * 32] != 0xa5 || col[c][(at + i) * 32 + 31] != 0xa5) { fprintf(stderr, "tag %u: a blinding row was written\n", tag); return 5; }
        printf("tag %u: %llu enabled rows below %u, table %u\n", tag, (unsigned long long)enabled, u, table_of_tag[tag - 1]);
    }
    printf("%llu blocks (K = %u, N = %u), %llu lookups, %u usable rows: 4 columns of %u arguments as Fr cells\n", (unsigned long long)n, k, n_sets,
           (unsigned long long)irep.lookups, u, (unsigned)AESW_THETA_ARGUMENTS * n_sets);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
