/*
 * aesw_open.c -- coefficient columns evaluated at points, folded under v and divided by (X - z), from plain C.
 *
 *   Two columns of 2^K canonical cells (seeded bytes, the top byte kept below r's) stand for what the device holds in coefficient
 *   form -- advice columns, A', S', Z after lagrange_to_coeff.  On one stream with nothing waiting in between: both columns at three
 *   points in one call (0, a seeded z, a second seeded point), the division of both by (X - z) out of place, the division by X in
 *   place, the fold of the two columns under a seeded v, and the fold under v = 0.  The host has no field arithmetic, so it checks
 *   what bytes alone can say: the value at 0 is the constant coefficient; the remainder of the division at z is the evaluation at z;
 *   dividing by X shifts the coefficients down by one, leaves a zero at the top and the constant coefficient as the remainder;
 *   the quotient's last coefficient is zero and its last but one is the column's top coefficient; folding under 0 leaves the last
 *   column; and the fold under v is neither column.
 *
 * usage: aesw_open [K]                     (default 17; K 10 ... 22)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_open.c -L halo2-aes_amd -laesw_open -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_open_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_open.h"

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

/* seeded canonical cells: the top byte keeps them below r = 0x3064... */
static void seeded_cells(uint8_t *cells, size_t n, uint64_t x) {
    for (size_t i = 0; i < n * 32; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; cells[i] = (uint8_t)(x >> 24); }
    for (size_t i = 0; i < n; ++i) cells[i * 32 + 31] &= 0x1f;
}

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 17, n_cols = 2, n_points = 3;
    if (k < 10 || k > 22) { fprintf(stderr, "K must be 10 ... 22 here\n"); return 1; }
    const size_t rows = (size_t)1 << k, col = rows * 32, bytes = n_cols * col;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));

    uint8_t *coeff = (uint8_t *)malloc(bytes), *quot = (uint8_t *)malloc(bytes), *shifted = (uint8_t *)malloc(bytes), *folded = (uint8_t *)malloc(col),
            *folded0 = (uint8_t *)malloc(col);
    uint8_t cells[5 * 32], evals[2 * 3 * 32], rem[2 * 32], rem0[2 * 32]; /* cells: the three points (0, z, a third), v, and v = 0 */
    seeded_cells(coeff, n_cols * rows, 0x2545f4914f6cdd1dull);
    seeded_cells(cells, 5, 0x9e3779b97f4a7c15ull);
    memset(cells, 0, 32);
    memset(cells + 4 * 32, 0, 32);

    uint8_t *d_coeff, *d_quot, *d_same, *d_folded, *d_folded0, *d_cells, *d_evals, *d_rem, *d_rem0;
    void *d_ws;
    CK(hipMalloc((void **)&d_coeff, bytes));
    CK(hipMalloc((void **)&d_quot, bytes));
    CK(hipMalloc((void **)&d_same, bytes));
    CK(hipMalloc((void **)&d_folded, col));
    CK(hipMalloc((void **)&d_folded0, col));
    CK(hipMalloc((void **)&d_cells, sizeof cells));
    CK(hipMalloc((void **)&d_evals, sizeof evals));
    CK(hipMalloc((void **)&d_rem, sizeof rem));
    CK(hipMalloc((void **)&d_rem0, sizeof rem0));
    CK(hipMalloc(&d_ws, aesw_open_workspace_bytes(k, n_cols, n_points))); /* the calls run one behind the other: one workspace serves all */
    CK(hipMemcpy(d_coeff, coeff, bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_same, coeff, bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_cells, cells, sizeof cells, hipMemcpyHostToDevice));

    AK(aesw_open_evaluate_device(ctx, k, n_cols, n_points, d_coeff, d_cells, d_evals, d_ws, NULL));
    AK(aesw_open_divide_device(ctx, k, n_cols, d_coeff, d_cells + 32, d_quot, d_rem, d_ws, NULL)); /* by (X - z) */
    AK(aesw_open_divide_device(ctx, k, n_cols, d_same, d_cells, d_same, d_rem0, d_ws, NULL));      /* by X, in place */
    AK(aesw_open_fold_device(ctx, k, 1, d_coeff, d_cells + 3 * 32, NULL, d_folded, NULL));         /* the columns live apart for all this call knows: */
    AK(aesw_open_fold_device(ctx, k, 1, d_coeff + col, d_cells + 3 * 32, d_folded, d_folded, NULL)); /* ... one by one into the accumulator */
    AK(aesw_open_fold_device(ctx, k, n_cols, d_coeff, d_cells + 4 * 32, NULL, d_folded0, NULL));   /* v = 0 */
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(evals, d_evals, sizeof evals, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rem, d_rem, sizeof rem, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rem0, d_rem0, sizeof rem0, hipMemcpyDeviceToHost));
    CK(hipMemcpy(quot, d_quot, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(shifted, d_same, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(folded, d_folded, col, hipMemcpyDeviceToHost));
    CK(hipMemcpy(folded0, d_folded0, col, hipMemcpyDeviceToHost));

    size_t bad = 0, nonzero = 0;
    for (uint32_t c = 0; c < n_cols; ++c) {
        const uint8_t *p = coeff + c * col, *q = quot + c * col, *s = shifted + c * col;
        bad += memcmp(evals + (c * n_points + 0) * 32, p, 32) != 0;            /* p(0) = c_0 */
        bad += memcmp(evals + (c * n_points + 1) * 32, rem + c * 32, 32) != 0; /* p(z) is the remainder at z */
        bad += memcmp(evals + (c * n_points + 2) * 32, rem + c * 32, 32) == 0; /* ... and not the value at another point */
        bad += memcmp(rem0 + c * 32, p, 32) != 0;                              /* dividing by X leaves c_0 ... */
        bad += memcmp(s, p + 32, col - 32) != 0;                               /* ... and the coefficients one down */
        bad += memcmp(q + col - 64, p + col - 32, 32) != 0;                    /* q[n - 2] = c_(n-1) */
        for (size_t i = col - 32; i < col; ++i) nonzero += (q[i] != 0) + (s[i] != 0); /* q[n - 1] = 0 */
    }
    bad += memcmp(folded0, coeff + col, col) != 0;                             /* under v = 0 the last column is left */
    bad += memcmp(folded, coeff, col) == 0 || memcmp(folded, coeff + col, col) == 0;
    printf("%u columns of 2^%u coefficients: %u evaluations, %zu quotient coefficients at z and %zu at 0 in place, 2 columns folded under v into %zu cells\n",
           n_cols, k, n_cols * n_points, (size_t)n_cols * rows, (size_t)n_cols * rows, rows);
    if (bad || nonzero) {
        printf("FAILED (%zu, %zu)\n", bad, nonzero);
        return 4;
    }
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
