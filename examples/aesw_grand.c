/*
 * aesw_grand.c -- the grand product Z of every lookup argument, from the witness, theta, beta and gamma alone, from plain C.
 *
 *   The chain of examples/aesw_theta.c -- a PACKED witness of one FixedAes128Config<17, 1> circuit, its lookups counted, the
 *   permuted columns A' and S' and the input column as table-row indices, then theta and the three compressed tables -- goes on
 *   by two calls once beta and gamma arrive (64 bytes, the only further upload): aesw_grand_invert_table_device inverts the
 *   2 * 3 * 66 561 cells T + beta and T + gamma, aesw_grand_product_device builds Z of all five arguments from the index columns.
 *   No column of Fr cells is made on the way.  The host checks that Z[0] and every closing cell are the Montgomery one byte for
 *   byte, that Z[n_rows] is the closing cell, that no argument is open and that the blinding rows were left alone.
 *
 * usage: aesw_grand [K]                    (default 17; K 17 ... 20)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_grand.c -L halo2-aes_amd -laesw_grand -laesw_theta
 *            -laesw_perm -laesw_mult -laesw -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_grand_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_grand.h"
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

/* 2^256 mod r: the Montgomery form of 1, as it lies in memory */
static const uint8_t fr_one[32] = {0xfb, 0xff, 0xff, 0x4f, 0x1c, 0x34, 0x96, 0xac, 0x29, 0xcd, 0x60, 0x9f, 0x95, 0x76, 0xfc, 0x36,
                                   0x2e, 0x46, 0x79, 0x78, 0x6f, 0xa3, 0x6e, 0x66, 0x2f, 0xdf, 0x07, 0x9a, 0xc1, 0x77, 0x0a, 0x0e};

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

    uint8_t *pt = (uint8_t *)malloc(n * 16), key[16], theta[32], beta[32], gamma[32];
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (int i = 0; i < 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; key[i] = (uint8_t)(x >> 32); }
    /* theta as the prover holds it: a canonical Montgomery cell (the top byte keeps it below r = 0x3064...) */
    for (int i = 0; i < 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; theta[i] = (uint8_t)(x >> 16); }
    theta[31] &= 0x1f;
    for (int i = 0; i < 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; beta[i] = (uint8_t)(x >> 16); }
    for (int i = 0; i < 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; gamma[i] = (uint8_t)(x >> 16); }
    beta[31] &= 0x1f;
    gamma[31] &= 0x1f;

    const size_t words = (size_t)n_sets * AESW_THETA_ARGUMENTS * rows, cells = words * 32, table_bytes = (size_t)AESW_THETA_TABLES * AESW_TABLE_ROWS * 32,
                 closing_bytes = (size_t)n_sets * AESW_THETA_ARGUMENTS * 32;
    const uint64_t offsets[2] = {0, n};
    uint8_t *d_pt, *d_key, *d_px, *d_py, *d_pz, *d_theta, *d_table, *d_beta, *d_gamma, *d_inv, *d_z, *d_closing;
    uint32_t *d_mult, *d_a, *d_s, *d_in;
    uint64_t *d_offsets;
    void *d_ws, *d_gws;
    aesw_key_slab ks;
    aesw_mult_report *d_mrep, *d_irep, mrep, irep;
    aesw_perm_report *d_prep, prep;
    aesw_theta_report *d_trep, trep;
    aesw_grand_invert_report *d_vrep, vrep;
    aesw_grand_report *d_grep, grep;
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
    CK(hipMalloc((void **)&d_beta, 32));
    CK(hipMalloc((void **)&d_gamma, 32));
    CK(hipMalloc((void **)&d_inv, AESW_GRAND_PLANES * table_bytes));
    CK(hipMalloc((void **)&d_z, cells));
    CK(hipMemset(d_z, 0xa5, cells)); /* the rows above n_rows are the host's blinding rows: the library leaves them alone */
    CK(hipMalloc((void **)&d_closing, closing_bytes));
    CK(hipMalloc(&d_gws, aesw_grand_workspace_bytes(k, n_sets)));
    CK(hipMalloc((void **)&d_vrep, sizeof vrep));
    CK(hipMalloc((void **)&d_grep, sizeof grep));
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
    /* beta and gamma arrive: 64 bytes go up.  The cells are inverted once per proof, Z is built from the index columns */
    CK(hipMemcpy(d_beta, beta, 32, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_gamma, gamma, 32, hipMemcpyHostToDevice));
    AK(aesw_grand_invert_table_device(ctx, d_table, d_beta, d_gamma, d_inv, d_vrep, NULL));
    AK(aesw_grand_product_device(ctx, k, n_sets, u, pad_row, d_in, d_a, d_s, d_table, d_inv, d_beta, d_gamma, d_z, d_closing, d_gws, d_grep, NULL));

    CK(hipMemcpy(&mrep, d_mrep, sizeof mrep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&irep, d_irep, sizeof irep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&prep, d_prep, sizeof prep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&trep, d_trep, sizeof trep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&vrep, d_vrep, sizeof vrep, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&grep, d_grep, sizeof grep, hipMemcpyDeviceToHost));
    if (mrep.misses || irep.misses || irep.lookups != mrep.lookups || prep.overflowed || trep.noncanonical || vrep.noncanonical ||
        vrep.cells != (uint64_t)AESW_GRAND_PLANES * AESW_THETA_TABLES * AESW_TABLE_ROWS) {
        fprintf(stderr, "the reports disagree: %llu / %llu lookups, %llu / %llu misses\n", (unsigned long long)mrep.lookups, (unsigned long long)irep.lookups,
                (unsigned long long)mrep.misses, (unsigned long long)irep.misses);
        return 4;
    }
    if (grep.arguments != (uint64_t)AESW_THETA_ARGUMENTS * n_sets || grep.open != 0 || grep.first_open != AESW_CHECK_NONE) {
        fprintf(stderr, "%llu of %llu arguments are open, the first is %llu\n", (unsigned long long)grep.open, (unsigned long long)grep.arguments,
                (unsigned long long)grep.first_open);
        return 5;
    }

    uint8_t *z = (uint8_t *)malloc(cells), *closing = (uint8_t *)malloc(closing_bytes);
    CK(hipMemcpy(z, d_z, cells, hipMemcpyDeviceToHost));
    CK(hipMemcpy(closing, d_closing, closing_bytes, hipMemcpyDeviceToHost));
    for (uint32_t tag = 1; tag <= AESW_THETA_ARGUMENTS; ++tag) {
        const uint8_t *Z = z + ((size_t)(tag - 1) << k) * 32, *C = closing + (size_t)(tag - 1) * 32;
        if (memcmp(Z, fr_one, 32) != 0) { fprintf(stderr, "tag %u: Z[0] is not one\n", tag); return 6; }
        if (memcmp(C, fr_one, 32) != 0) { fprintf(stderr, "tag %u: the closing product is not one\n", tag); return 6; }
        if (memcmp(Z + (size_t)u * 32, C, 32) != 0) { fprintf(stderr, "tag %u: Z[n_rows] is not the closing cell\n", tag); return 6; }
        uint32_t moved = 0; /* rows at which Z changes: the rows whose factor is not one */
        for (uint32_t i = 0; i < u; ++i) moved += memcmp(Z + (size_t)i * 32, Z + (size_t)(i + 1) * 32, 32) != 0;
        for (uint64_t i = (uint64_t)u + 1; i < rows; ++i)
            if (Z[i * 32] != 0xa5 || Z[i * 32 + 31] != 0xa5) { fprintf(stderr, "tag %u: a blinding row was written\n", tag); return 6; }
        printf("tag %u: Z closes at row %u, %u rows move it\n", tag, u, moved);
    }
    printf("%llu blocks (K = %u, N = %u), %llu lookups, %u usable rows: Z of %u arguments, %llu zero terms, %llu open\n", (unsigned long long)n, k, n_sets,
           (unsigned long long)irep.lookups, u, (unsigned)AESW_THETA_ARGUMENTS * n_sets, (unsigned long long)vrep.zero_terms, (unsigned long long)grep.open);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
