/*
 * aesw_shplonk.c -- SHPLONK's two quotients over one set of two points, from plain C.
 *
 *   One column of 2^K canonical cells (seeded bytes, the top byte kept below r's) stands for a queried polynomial in coefficient
 *   form.  On one stream with nothing waiting in between: the column evaluated at two seeded points (the opening library), the
 *   small phase after y and v, N_0 by a combine (coefficient y^0, low cells -R_0), h = Q_0 by the set's quotient, the small phase
 *   after u, L' by a combine over N_0 and h, and W by the opening library's division at u with its remainder written into the
 *   report.  The host has no field arithmetic, so it checks what bytes alone can say: both remainders N_0(z_s) are zero and the
 *   report is clean; dividing by two points drops the degree by two, so h's top two coefficients are zero and the third is the
 *   column's top coefficient (y^0 = v^0 = 1); the one set holds every point, so z_0 = 1 and its inverse is the cell of 1, which is
 *   the coefficient of N_0 in L', whose top coefficient is therefore the column's; W's top coefficient is zero, the one below it is
 *   the column's, and the last division leaves no remainder.  Then the
 *   same with one evaluation replaced by the other: the report names set 0.
 *
 * usage: aesw_shplonk [K]                     (default 17; K 10 ... 22)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_shplonk.c -L halo2-aes_amd -laesw_shplonk -laesw_open
 *            -laesw -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_shplonk_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_open.h"
#include "aesw_shplonk.h"

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

/* the Montgomery cell of 1 */
static const uint32_t ONE[8] = {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u};

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 17;
    if (k < 10 || k > 22) { fprintf(stderr, "K must be 10 ... 22 here\n"); return 1; }
    const size_t rows = (size_t)1 << k, col = rows * 32;
    const uint32_t set_points[1] = {2}, set_cols[1] = {1}, point_index[2] = {0, 1};
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));

    uint8_t *coeff = (uint8_t *)malloc(col), *h = (uint8_t *)malloc(col), *line = (uint8_t *)malloc(col), *w = (uint8_t *)malloc(col);
    uint8_t cells[5 * 32], rem[8 * 32], z0_inv[32], swapped[2 * 32]; /* cells: the two points, y, v, u */
    uint64_t report[8], bad_report[8];
    seeded_cells(coeff, rows, 0x2545f4914f6cdd1dull);
    seeded_cells(cells, 5, 0x9e3779b97f4a7c15ull);

    const size_t scalars_bytes = aesw_shplonk_scalars_bytes(1, 1), ws_bytes = aesw_shplonk_workspace_bytes(k), open_ws = aesw_open_workspace_bytes(k, 1, 2);
    const size_t at_y = aesw_shplonk_scalars_offset(AESW_SHPLONK_Y_POW, 0), at_neg_r = aesw_shplonk_scalars_offset(AESW_SHPLONK_NEG_R, 0),
                 at_coef = aesw_shplonk_scalars_offset(AESW_SHPLONK_L_COEF, 0), at_low = aesw_shplonk_scalars_offset(AESW_SHPLONK_L_LOW, 0),
                 at_z0 = aesw_shplonk_scalars_offset(AESW_SHPLONK_Z0_INV, 0);
    if (!scalars_bytes || !ws_bytes || aesw_shplonk_report_bytes() != sizeof report) { fprintf(stderr, "sizes\n"); return 1; }
    uint8_t *d_coeff, *d_work, *d_line, *d_cells, *d_evals, *d_scalars, *d_rem, *d_report;
    void *d_ws;
    CK(hipMalloc((void **)&d_coeff, col));
    CK(hipMalloc((void **)&d_work, 2 * col)); /* N_0, then h: the two columns of L' */
    CK(hipMalloc((void **)&d_line, col));
    CK(hipMalloc((void **)&d_cells, sizeof cells));
    CK(hipMalloc((void **)&d_evals, 2 * 32));
    CK(hipMalloc((void **)&d_scalars, scalars_bytes));
    CK(hipMalloc((void **)&d_rem, sizeof rem));
    CK(hipMalloc((void **)&d_report, sizeof report));
    CK(hipMalloc(&d_ws, ws_bytes > open_ws ? ws_bytes : open_ws)); /* the calls run one behind the other: one workspace serves all */
    CK(hipMemcpy(d_coeff, coeff, col, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_cells, cells, sizeof cells, hipMemcpyHostToDevice));
    CK(hipMemset(d_rem, 0xA5, sizeof rem));
    const uint8_t *d_y = d_cells + 2 * 32, *d_v = d_cells + 3 * 32, *d_u = d_cells + 4 * 32;

    AK(aesw_open_evaluate_device(ctx, k, 1, 2, d_coeff, d_cells, d_evals, d_ws, NULL));
    AK(aesw_shplonk_prepare_device(ctx, 2, 1, set_points, set_cols, point_index, d_cells, d_evals, d_y, d_v, d_scalars, d_report, NULL));
    AK(aesw_shplonk_combine_device(ctx, k, 1, d_coeff, d_scalars + at_y, d_scalars + at_neg_r, 2, NULL, d_work, NULL));                       /* N_0 */
    AK(aesw_shplonk_quotient_device(ctx, k, 0, d_work, d_cells, d_scalars, NULL, d_work + col, d_rem, d_ws, d_report, NULL));                  /* h = Q_0 */
    AK(aesw_shplonk_finish_device(ctx, d_cells, d_u, d_scalars, d_report, NULL));
    AK(aesw_shplonk_combine_device(ctx, k, 2, d_work, d_scalars + at_coef, d_scalars + at_low, 8, NULL, d_line, NULL));                       /* L' */
    CK(hipMemcpyAsync(line, d_line, col, hipMemcpyDeviceToHost, NULL));
    AK(aesw_open_divide_device(ctx, k, 1, d_line, d_u, d_line, d_report + AESW_SHPLONK_REPORT_LAST_REM, d_ws, NULL));                          /* W, in place */
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h, d_work + col, col, hipMemcpyDeviceToHost));
    CK(hipMemcpy(w, d_line, col, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rem, d_rem, sizeof rem, hipMemcpyDeviceToHost));
    CK(hipMemcpy(report, d_report, sizeof report, hipMemcpyDeviceToHost));
    CK(hipMemcpy(z0_inv, d_scalars + at_z0, 32, hipMemcpyDeviceToHost));

    /* the same stage up to h with the two evaluations swapped: they no longer belong to the column */
    CK(hipMemcpy(swapped, d_evals, sizeof swapped, hipMemcpyDeviceToHost));
    CK(hipMemcpy(d_evals, swapped + 32, 32, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_evals + 32, swapped, 32, hipMemcpyHostToDevice));
    AK(aesw_shplonk_prepare_device(ctx, 2, 1, set_points, set_cols, point_index, d_cells, d_evals, d_y, d_v, d_scalars, d_report, NULL));
    AK(aesw_shplonk_combine_device(ctx, k, 1, d_coeff, d_scalars + at_y, d_scalars + at_neg_r, 2, NULL, d_work, NULL));
    AK(aesw_shplonk_quotient_device(ctx, k, 0, d_work, d_cells, d_scalars, NULL, d_work + col, d_rem, d_ws, d_report, NULL));
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(bad_report, d_report, sizeof bad_report, hipMemcpyDeviceToHost));

    size_t bad = 0;
    static const uint8_t zero[96];
    bad += memcmp(rem, zero, 64) != 0;                                  /* N_0(z_0) = N_0(z_1) = 0 */
    for (size_t i = 64; i < sizeof rem; ++i) bad += rem[i] != 0xA5;     /* the remainder cells past t_0 are left alone */
    bad += report[0] != 0 || report[1] != ~0ull || report[2] != 0 || report[3] != 0 || report[4] || report[5] || report[6] || report[7];
    bad += memcmp(h + col - 64, zero, 64) != 0;                         /* the degree drops by two ... */
    bad += memcmp(h + col - 96, coeff + col - 32, 32) != 0;             /* ... and the top coefficient moves down */
    bad += memcmp(z0_inv, ONE, 32) != 0 || memcmp(line, zero, 32) == 0; /* z_0 = 1: no point lies outside the one set */
    bad += memcmp(line + col - 32, coeff + col - 32, 32) != 0;          /* L' = 1 * N_0 - z_T h: its top coefficient is the column's */
    bad += memcmp(w + col - 32, zero, 32) != 0;                         /* W = L' / (X - u): the degree drops by one ... */
    bad += memcmp(w + col - 64, coeff + col - 32, 32) != 0;             /* ... and the top coefficient moves down */
    bad += bad_report[0] != 1 || bad_report[1] != 0 || bad_report[2] != 0;
    printf("1 column of 2^%u coefficients at 2 points: h and W of %zu coefficients each, report %llu %llu, with the evaluations swapped %llu %llu\n", k, rows,
           (unsigned long long)report[0], (unsigned long long)report[2], (unsigned long long)bad_report[0], (unsigned long long)bad_report[1]);
    if (bad) {
        printf("FAILED (%zu)\n", bad);
        return 4;
    }
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
