/*
 * aesw_msm.c -- columns committed against a basis of points of bn256's G1, from plain C.
 *
 *   The basis: 2^K points from plain coordinates, as a host reads them from a params file -- here the generator G = (1, 2)
 *   throughout, but -G = (1, q - 2) at row 1 -- converted and checked on the device; then the same with row 3 pushed off the curve,
 *   which the report counts and names.  Five byte columns and, in a second call, the same five as columns of Fr cells, on one
 *   stream with nothing waiting in between.  The host has no field arithmetic, so it checks what bytes alone can say: a column of
 *   zeros commits to the identity, 64 zero bytes; a single 1 at row 0 commits to G in Montgomery form; 1 at rows 0 and 1 meets
 *   G + (-G), the identity again; 1 at rows 0 and 2 (G + G, the law's doubling case) is what a single 2 at the last row commits to;
 *   and every column of cells commits to what its column of bytes does.
 *
 * usage: aesw_msm [K]                      (default 16; K 10 ... 22)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_msm.c -L halo2-aes_amd -laesw_msm -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_msm_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_msm.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define AK(x) do { int r_ = (x); if (r_ != AESW_OK) { fprintf(stderr, "%s: %s (%s)\n", #x, aesw_strerror(r_), aesw_last_error(ctx)); return 3; } } while (0)
#define WANT(c, what) do { if (!(c)) { fprintf(stderr, "FAILED: %s\n", what); return 4; } } while (0)

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

/* q - 2, little-endian: the y of -G */
static const uint8_t Q_MINUS_2[32] = {0x45, 0xfd, 0x7c, 0xd8, 0x16, 0x8c, 0x20, 0x3c, 0x8d, 0xca, 0x71, 0x68, 0x91, 0x6a, 0x81, 0x97,
                                      0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};
/* 1 and 2 as coordinates (v * 2^256 mod q) and as Fr cells (v * 2^256 mod r) */
static const uint8_t ONE_Q[32] = {0x9d, 0x0d, 0x8f, 0xc5, 0x8d, 0x43, 0x5d, 0xd3, 0x3d, 0x0b, 0xc7, 0xf5, 0x28, 0xeb, 0x78, 0x0a,
                                  0x2c, 0x46, 0x79, 0x78, 0x6f, 0xa3, 0x6e, 0x66, 0x2f, 0xdf, 0x07, 0x9a, 0xc1, 0x77, 0x0a, 0x0e};
static const uint8_t TWO_Q[32] = {0x3a, 0x1b, 0x1e, 0x8b, 0x1b, 0x87, 0xba, 0xa6, 0x7b, 0x16, 0x8e, 0xeb, 0x51, 0xd6, 0xf1, 0x14,
                                  0x58, 0x8c, 0xf2, 0xf0, 0xde, 0x46, 0xdd, 0xcc, 0x5e, 0xbe, 0x0f, 0x34, 0x83, 0xef, 0x14, 0x1c};
static const uint8_t ONE_R[32] = {0xfb, 0xff, 0xff, 0x4f, 0x1c, 0x34, 0x96, 0xac, 0x29, 0xcd, 0x60, 0x9f, 0x95, 0x76, 0xfc, 0x36,
                                  0x2e, 0x46, 0x79, 0x78, 0x6f, 0xa3, 0x6e, 0x66, 0x2f, 0xdf, 0x07, 0x9a, 0xc1, 0x77, 0x0a, 0x0e};
static const uint8_t TWO_R[32] = {0xf6, 0xff, 0xff, 0x9f, 0x38, 0x68, 0x2c, 0x59, 0x53, 0x9a, 0xc1, 0x3e, 0x2b, 0xed, 0xf8, 0x6d,
                                  0x5c, 0x8c, 0xf2, 0xf0, 0xde, 0x46, 0xdd, 0xcc, 0x5e, 0xbe, 0x0f, 0x34, 0x83, 0xef, 0x14, 0x1c};

#define N_COLS 5u

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 16;
    if (k < 10 || k > 22) { fprintf(stderr, "K must be 10 ... 22 here\n"); return 1; }
    const size_t rows = (size_t)1 << k;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));

    /* the params: G everywhere, -G at row 1 */
    uint8_t *canonical = (uint8_t *)calloc(rows, 64), *bytes = (uint8_t *)calloc(N_COLS * rows, 1), *cells = (uint8_t *)calloc(N_COLS * rows, 32);
    if (!canonical || !bytes || !cells) return 2;
    for (size_t i = 0; i < rows; ++i) { canonical[64 * i] = 1; canonical[64 * i + 32] = 2; }
    memcpy(canonical + 64 + 32, Q_MINUS_2, 32);
    /* column 0: zeros; 1: a 1 at row 0; 2: 1 at rows 0 and 1; 3: 1 at rows 0 and 2; 4: a 2 at the last row */
    bytes[1 * rows] = 1;
    bytes[2 * rows] = bytes[2 * rows + 1] = 1;
    bytes[3 * rows] = bytes[3 * rows + 2] = 1;
    bytes[4 * rows + rows - 1] = 2;
    for (size_t i = 0; i < N_COLS * rows; ++i)
        if (bytes[i]) memcpy(cells + 32 * i, bytes[i] == 1 ? ONE_R : TWO_R, 32);

    uint8_t *d_canonical, *d_basis, *d_bytes, *d_cells, *d_out;
    aesw_msm_report *d_report;
    void *d_ws;
    const size_t ws_bytes = aesw_msm_workspace_bytes(k, N_COLS, AESW_MSM_BYTES, 0), ws_cells = aesw_msm_workspace_bytes(k, N_COLS, AESW_MSM_FR, 0);
    WANT(ws_bytes && ws_cells > ws_bytes, "the workspace sizes");
    CK(hipMalloc((void **)&d_canonical, rows * 64));
    CK(hipMalloc((void **)&d_basis, rows * 64));
    CK(hipMalloc((void **)&d_bytes, N_COLS * rows));
    CK(hipMalloc((void **)&d_cells, N_COLS * rows * 32));
    CK(hipMalloc((void **)&d_out, 2 * N_COLS * 64));
    CK(hipMalloc((void **)&d_report, 2 * sizeof(aesw_msm_report)));
    CK(hipMalloc(&d_ws, ws_cells));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    CK(hipMemcpyAsync(d_canonical, canonical, rows * 64, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(d_bytes, bytes, N_COLS * rows, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(d_cells, cells, N_COLS * rows * 32, hipMemcpyHostToDevice, s));

    AK(aesw_msm_basis_device(ctx, k, d_canonical, d_basis, d_report, s));
    AK(aesw_msm_commit_device(ctx, k, N_COLS, AESW_MSM_BYTES, 0, d_bytes, d_basis, d_out, d_ws, s));
    AK(aesw_msm_commit_device(ctx, k, N_COLS, AESW_MSM_FR, 0, d_cells, d_basis, d_out + N_COLS * 64, d_ws, s));
    /* row 3 off the curve: y = 3; converted in place, into the params' own buffer */
    canonical[64 * 3 + 32] = 3;
    CK(hipMemcpyAsync(d_canonical, canonical, rows * 64, hipMemcpyHostToDevice, s));
    AK(aesw_msm_basis_device(ctx, k, d_canonical, d_canonical, d_report + 1, s));

    uint8_t out[2 * N_COLS * 64], first[2 * 64];
    aesw_msm_report report[2];
    CK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(first, d_basis, sizeof first, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(report, d_report, sizeof report, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));

    uint8_t zero[64] = {0}, g[64];
    memcpy(g, ONE_Q, 32);
    memcpy(g + 32, TWO_Q, 32);
    WANT(report[0].bad_points == 0 && report[0].first_bad == ~0ull, "every point of the params is on the curve");
    WANT(report[1].bad_points == 1 && report[1].first_bad == 3, "the point pushed off the curve is counted and named");
    WANT(!memcmp(first, g, 64) && !memcmp(first + 64, g, 32) && memcmp(first + 64 + 32, g + 32, 32), "the basis begins with G and -G in Montgomery form");
    WANT(!memcmp(out, zero, 64), "a column of zeros commits to the identity");
    WANT(!memcmp(out + 64, g, 64), "a single 1 at row 0 commits to G");
    WANT(!memcmp(out + 2 * 64, zero, 64), "G + (-G) is the identity");
    WANT(memcmp(out + 3 * 64, zero, 64) && memcmp(out + 3 * 64, g, 64) && !memcmp(out + 3 * 64, out + 4 * 64, 64), "G + G is 2 * G");
    WANT(!memcmp(out, out + N_COLS * 64, N_COLS * 64), "the columns of cells commit to what the columns of bytes do");

    /* a k out of bounds is refused, with nothing enqueued */
    WANT(aesw_msm_commit_device(ctx, 9, N_COLS, AESW_MSM_BYTES, 0, d_bytes, d_basis, d_out, d_ws, s) == AESW_ERR_INVALID_ARG, "k = 9 is refused");
    printf("%u columns of 2^%u rows as bytes and as cells: %u commitments, %u slices a byte column and %u a column of cells, chunks of %u rows\n", N_COLS, k,
           2 * N_COLS, aesw_msm_slices(k, N_COLS, AESW_MSM_BYTES, 0), aesw_msm_slices(k, N_COLS, AESW_MSM_FR, 0), aesw_msm_chunk_rows());

    CK(hipStreamDestroy(s));
    CK(hipFree(d_canonical)); CK(hipFree(d_basis)); CK(hipFree(d_bytes)); CK(hipFree(d_cells)); CK(hipFree(d_out)); CK(hipFree(d_report)); CK(hipFree(d_ws));
    free(canonical); free(bytes); free(cells);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
