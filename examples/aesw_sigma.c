/*
 * aesw_sigma.c -- the grand products of halo2's permutation argument, from the witness, beta and gamma alone, from plain C.
 *
 *   A PACKED witness of one FixedAes128Config<17, 1> circuit is assembled into its byte columns on the device; keygen's part --
 *   the column order, sigma as cell indices, the fixed round-constant column, the power tables -- is input independent and made
 *   once; then beta and gamma arrive (64 bytes, the only further upload) and aesw_sigma_product_device builds Z of the two sets
 *   (5 columns, chunk_len 3).  No column of Fr cells is made on the way.  The host checks that Z_0[0] and the last closing cell are
 *   the Montgomery one byte for byte, that every set starts where the one before it ended, and that the blinding rows were left alone.
 *
 * usage: aesw_sigma [K]                    (default 17; K 12 ... 20)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_sigma.c -L halo2-aes_amd -laesw_sigma -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_sigma_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_sigma.h"

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
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 17, n_sets = 1, chunk_len = 3;
    if (k < 12 || k > 20) { fprintf(stderr, "K must be 12 ... 20 here\n"); return 1; }
    const uint64_t n = aesw_block_capacity(k, n_sets), rows = 1ull << k;
    const uint32_t u = (uint32_t)rows - 6, n_cols = aesw_sigma_columns(n_sets), n_advice = 3 * n_sets + 1, sets = (n_cols + chunk_len - 1) / chunk_len;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    const int P = AESW_LAYOUT_PACKED;

    uint8_t *pt = (uint8_t *)malloc(n * 16), key[16], beta[32], gamma[32];
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (int i = 0; i < 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; key[i] = (uint8_t)(x >> 32); }
    /* beta and gamma as the prover holds them: canonical Montgomery cells (the top byte keeps them below r = 0x3064...) */
    for (int i = 0; i < 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; beta[i] = (uint8_t)(x >> 16); }
    for (int i = 0; i < 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; gamma[i] = (uint8_t)(x >> 16); }
    beta[31] &= 0x1f;
    gamma[31] &= 0x1f;

    /* keygen, input independent: the column order, sigma, the fixed column */
    uint32_t *source = (uint32_t *)malloc(n_cols * 4), *map = (uint32_t *)malloc((size_t)n_cols * rows * 4);
    uint8_t *fixed = (uint8_t *)calloc(rows, 1), rcon[AESW_WORDS_ROWS];
    AK(aesw_sigma_sources_host(n_sets, source));
    AK(aesw_sigma_mapping_host(k, n_sets, (uint32_t)n, map));
    AK(aesw_selector_tags(NULL, NULL, NULL, rcon));
    memcpy(fixed, rcon, sizeof rcon);
    uint64_t moved = 0;
    for (uint64_t i = 0; i < (uint64_t)n_cols * rows; ++i) moved += map[i] != (uint32_t)i;

    const size_t z_bytes = (size_t)sets * rows * 32;
    uint8_t *d_pt, *d_key, *d_px, *d_py, *d_pz, *d_advice, *d_fixed, *d_tables, *d_beta, *d_gamma, *d_z, *d_closing;
    uint32_t *d_source, *d_map;
    void *d_ws;
    aesw_key_slab ks;
    aesw_sigma_report *d_rep, rep;
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_key, 16));
    CK(hipMalloc((void **)&d_px, n * aesw_column_stride(P, 0)));
    CK(hipMalloc((void **)&d_py, n * aesw_column_stride(P, 1)));
    CK(hipMalloc((void **)&d_pz, n * aesw_column_stride(P, 2)));
    CK(hipMalloc((void **)&ks.w, AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, aesw_key_column_stride(P, 0)));
    CK(hipMalloc((void **)&ks.ky, aesw_key_column_stride(P, 1)));
    CK(hipMalloc((void **)&ks.kz, aesw_key_column_stride(P, 2)));
    CK(hipMalloc((void **)&d_advice, (size_t)n_advice * rows));
    CK(hipMalloc((void **)&d_fixed, rows));
    CK(hipMalloc((void **)&d_source, n_cols * 4));
    CK(hipMalloc((void **)&d_map, (size_t)n_cols * rows * 4));
    CK(hipMalloc((void **)&d_tables, aesw_sigma_tables_bytes(k, n_cols)));
    CK(hipMalloc((void **)&d_beta, 32));
    CK(hipMalloc((void **)&d_gamma, 32));
    CK(hipMalloc((void **)&d_z, z_bytes));
    CK(hipMemset(d_z, 0xa5, z_bytes)); /* the rows above n_rows are the host's blinding rows: the library leaves them alone */
    CK(hipMalloc((void **)&d_closing, (size_t)sets * 32));
    CK(hipMalloc(&d_ws, aesw_sigma_workspace_bytes(k, n_cols, chunk_len)));
    CK(hipMalloc((void **)&d_rep, sizeof rep));
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_key, key, 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_fixed, fixed, rows, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_source, source, n_cols * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_map, map, (size_t)n_cols * rows * 4, hipMemcpyHostToDevice));
    AK(aesw_sigma_tables_device(ctx, k, n_cols, d_tables, NULL)); /* once per (k, n_cols) */

    /* witness time: no challenge yet.  One stream, nothing waits in between. */
    AK(aesw_key_schedule_witness_device(ctx, d_key, 1, P, ks.w, ks.kx, ks.ky, ks.kz, NULL, NULL));
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_key, 0, n, P, d_px, d_py, d_pz, NULL, NULL, NULL));
    AK(aesw_assemble_advice_device(ctx, k, n_sets, n, P, d_px, d_py, d_pz, &ks, 0, d_advice, NULL));
    /* beta and gamma arrive: 64 bytes go up */
    CK(hipMemcpy(d_beta, beta, 32, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_gamma, gamma, 32, hipMemcpyHostToDevice));
    AK(aesw_sigma_product_device(ctx, k, n_cols, chunk_len, u, d_advice, n_advice, d_fixed, 1, d_source, d_map, d_tables, d_beta, d_gamma, d_z, d_closing, d_ws,
                                 d_rep, NULL));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));

    uint8_t *closing = (uint8_t *)malloc((size_t)sets * 32), cell[32], above[32 * 5];
    CK(hipMemcpy(closing, d_closing, (size_t)sets * 32, hipMemcpyDeviceToHost));
    int bad = 0;
    for (uint32_t s = 0; s < sets; ++s) {
        CK(hipMemcpy(cell, d_z + ((size_t)s * rows) * 32, 32, hipMemcpyDeviceToHost)); /* Z_s[0]: 1, then where the set before ended */
        bad += memcmp(cell, s ? closing + (s - 1) * 32 : fr_one, 32) != 0;
        CK(hipMemcpy(cell, d_z + ((size_t)s * rows + u) * 32, 32, hipMemcpyDeviceToHost)); /* Z_s[n_rows] is the closing cell */
        bad += memcmp(cell, closing + s * 32, 32) != 0;
        CK(hipMemcpy(above, d_z + ((size_t)s * rows + u + 1) * 32, sizeof above, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < sizeof above; ++i) bad += above[i] != 0xa5;
        printf("set %u: columns %u ... %u, Z closes at row %u\n", s, s * chunk_len, (s + 1) * chunk_len < n_cols ? (s + 1) * chunk_len - 1 : n_cols - 1, u);
    }
    bad += memcmp(closing + (sets - 1) * 32, fr_one, 32) != 0;
    printf("%llu blocks (K = %u, N = %u), %u columns, %llu cells moved by sigma, %u usable rows: Z of %llu sets, %llu zero terms, %llu out of range, %s\n",
           (unsigned long long)n, k, n_sets, n_cols, (unsigned long long)moved, u, (unsigned long long)rep.sets, (unsigned long long)rep.zero_terms,
           (unsigned long long)rep.out_of_range, rep.open ? "open" : "closed");
    if (bad || rep.open || rep.zero_terms || rep.out_of_range || rep.noncanonical || rep.sets != sets || rep.first_zero != AESW_CHECK_NONE) {
        printf("FAILED (%d)\n", bad);
        return 4;
    }
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
