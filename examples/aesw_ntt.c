/*
 * aesw_ntt.c -- a column of Fr cells from Lagrange form to its coefficients, onto the extended coset and back, from plain C.
 *
 *   Two columns of 2^K canonical cells (seeded bytes, the top byte kept below r's) stand for what the device holds in Lagrange
 *   form -- advice columns, A', S', Z.  The tables are made once for the extended size; then, on one stream with nothing waiting
 *   in between: lagrange_to_coeff, coeff_to_extended onto zeta * {omega_ext^i} with ext_k = K + 2, extended_to_coeff in place, and
 *   coeff_to_lagrange.  The host checks that the columns came back byte for byte, that extended_to_coeff returned the 2^K
 *   coefficients followed by 3 * 2^K zero cells, and that a constant column has the constant as its only coefficient.
 *
 * usage: aesw_ntt [K]                      (default 17; K 10 ... 22)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_ntt.c -L halo2-aes_amd -laesw_ntt -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_ntt_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_ntt.h"

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

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 17, n_cols = 2, zeta_sel = 1;
    if (k < 10 || k > 22) { fprintf(stderr, "K must be 10 ... 22 here\n"); return 1; }
    const uint32_t ext_k = k + 2;
    const size_t rows = (size_t)1 << k, ext_rows = (size_t)1 << ext_k, bytes = n_cols * rows * 32, ext_bytes = n_cols * ext_rows * 32;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));

    /* column 0: seeded canonical cells (the top byte keeps them below r = 0x3064...); column 1: one cell throughout */
    uint8_t *lagrange = (uint8_t *)malloc(bytes), *back = (uint8_t *)malloc(bytes), *coeff = (uint8_t *)malloc(bytes), *ext_coeff = (uint8_t *)malloc(ext_bytes);
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (size_t i = 0; i < rows * 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; lagrange[i] = (uint8_t)(x >> 24); }
    for (size_t i = 0; i < rows; ++i) lagrange[i * 32 + 31] &= 0x1f;
    for (size_t i = 0; i < rows; ++i) memcpy(lagrange + (rows + i) * 32, lagrange + 5 * 32, 32);

    uint8_t *d_tables, *d_lagrange, *d_coeff, *d_ext, *d_back;
    void *d_ws;
    CK(hipMalloc((void **)&d_tables, aesw_ntt_tables_bytes(ext_k)));
    CK(hipMalloc((void **)&d_lagrange, bytes));
    CK(hipMalloc((void **)&d_coeff, bytes));
    CK(hipMalloc((void **)&d_back, bytes));
    CK(hipMalloc((void **)&d_ext, ext_bytes));
    CK(hipMalloc(&d_ws, aesw_ntt_workspace_bytes(ext_k, n_cols))); /* the one call in place: extended_to_coeff */
    CK(hipMemcpy(d_lagrange, lagrange, bytes, hipMemcpyHostToDevice));
    AK(aesw_ntt_tables_device(ctx, ext_k, d_tables, NULL)); /* once: serves every size up to 2^ext_k */

    AK(aesw_ntt_lagrange_to_coeff_device(ctx, k, n_cols, d_lagrange, d_coeff, d_tables, ext_k, NULL, NULL));
    AK(aesw_ntt_coeff_to_extended_device(ctx, k, ext_k, zeta_sel, n_cols, d_coeff, d_ext, d_tables, ext_k, NULL, NULL));
    /* ... the quotient would be computed on the coset here ... */
    AK(aesw_ntt_extended_to_coeff_device(ctx, ext_k, zeta_sel, n_cols, d_ext, d_ext, d_tables, ext_k, d_ws, NULL));
    AK(aesw_ntt_coeff_to_lagrange_device(ctx, k, n_cols, d_coeff, d_back, d_tables, ext_k, NULL, NULL));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(coeff, d_coeff, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(back, d_back, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ext_coeff, d_ext, ext_bytes, hipMemcpyDeviceToHost));

    size_t bad = memcmp(back, lagrange, bytes) != 0, nonzero = 0;
    for (uint32_t c = 0; c < n_cols; ++c) {
        bad += memcmp(ext_coeff + c * ext_rows * 32, coeff + c * rows * 32, rows * 32) != 0; /* the coefficients ... */
        for (size_t i = rows * 32; i < ext_rows * 32; ++i) nonzero += ext_coeff[c * ext_rows * 32 + i] != 0; /* ... followed by zeros */
    }
    /* the constant column: its constant, then zeros */
    bad += memcmp(coeff + rows * 32, lagrange + 5 * 32, 32) != 0;
    for (size_t i = 32; i < rows * 32; ++i) nonzero += coeff[rows * 32 + i] != 0;
    printf("%u columns of 2^%u cells: coefficients, 2^%u evaluations on the coset (zeta_sel %u), %zu coefficients back with %zu zero cells behind them, the columns again\n",
           n_cols, k, ext_k, zeta_sel, (size_t)n_cols * rows, (size_t)n_cols * (ext_rows - rows));
    if (bad || nonzero) {
        printf("FAILED (%zu, %zu)\n", bad, nonzero);
        return 4;
    }
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
