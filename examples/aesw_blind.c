/*
 * aesw_blind.c -- a column of bytes committed with a blinded tail, from plain C.
 *
 *   The basis: 2^10 points from plain coordinates, the generator G = (1, 2) throughout, converted and checked on the device.  One
 *   advice column of bytes, byte i = i mod 251 in rows 0 ... 2^10 - 7 and zero in the last six rows, which are the prover's
 *   blinding rows.  A seed (the bytes 0 ... 31 here; a prover draws 32 bytes from the operating system) goes to device memory;
 *   aesw_blind_tail_device writes the six blinding cells of the column, aesw_msm_commit_device commits to the bytes as one 8-bit
 *   window, and aesw_blind_commit_tail_device adds the six terms tail[i] * P_i in place: three calls on one stream with nothing
 *   waiting in between.  The host has no field arithmetic: it prints the tail and the commitment, and checks what bytes alone can
 *   say -- the blinded commitment is not the bytes' own, and a second run under the same seed gives the same bytes.
 *
 * usage: aesw_blind [DOMAIN]               (default 1)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_blind.c -L halo2-aes_amd -laesw_blind -laesw_msm
 *            -laesw -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_blind_calls.py builds and runs it, and holds what it prints against tests/blind_model.py.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_blind.h"
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

static void print_hex(const char *name, const uint8_t *p, size_t n) {
    printf("%s ", name);
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

#define K 10u
#define TAIL 6u

int main(int argc, char **argv) {
    const uint64_t domain = argc > 1 ? strtoull(argv[1], NULL, 0) : 1;
    const size_t rows = (size_t)1 << K;
    const uint64_t first_row = rows - TAIL;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    WANT(aesw_blind_tail_rows(K, first_row) == TAIL && TAIL <= aesw_blind_max_tail(), "the tail is six rows, within what the commitment takes");

    uint8_t *canonical = (uint8_t *)calloc(rows, 64), *bytes = (uint8_t *)calloc(rows, 1), seed[AESW_BLIND_SEED_BYTES];
    if (!canonical || !bytes) return 2;
    for (size_t i = 0; i < rows; ++i) { canonical[64 * i] = 1; canonical[64 * i + 32] = 2; }
    for (size_t i = 0; i < first_row; ++i) bytes[i] = (uint8_t)(i % 251);
    for (size_t i = 0; i < sizeof seed; ++i) seed[i] = (uint8_t)i;

    uint8_t *d_canonical, *d_basis, *d_bytes, *d_seed, *d_tail, *d_commit;
    aesw_msm_report *d_report;
    void *d_ws;
    const size_t ws = aesw_msm_workspace_bytes(K, 1, AESW_MSM_BYTES, 0);
    WANT(ws, "the workspace size");
    CK(hipMalloc((void **)&d_canonical, rows * 64));
    CK(hipMalloc((void **)&d_basis, rows * 64));
    CK(hipMalloc((void **)&d_bytes, rows));
    CK(hipMalloc((void **)&d_seed, sizeof seed));
    CK(hipMalloc((void **)&d_tail, TAIL * 32));
    CK(hipMalloc((void **)&d_commit, 3 * 64));
    CK(hipMalloc((void **)&d_report, sizeof(aesw_msm_report)));
    CK(hipMalloc(&d_ws, ws));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    CK(hipMemcpyAsync(d_canonical, canonical, rows * 64, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(d_bytes, bytes, rows, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(d_seed, seed, sizeof seed, hipMemcpyHostToDevice, s));
    AK(aesw_msm_basis_device(ctx, K, d_canonical, d_basis, d_report, s));

    /* slot 0: the bytes alone; slots 1 and 2: the blinded commitment, twice under the one seed */
    AK(aesw_msm_commit_device(ctx, K, 1, AESW_MSM_BYTES, 0, d_bytes, d_basis, d_commit, d_ws, s));
    for (int run = 1; run <= 2; ++run) {
        AK(aesw_blind_tail_device(ctx, K, 1, first_row, domain, 0, d_seed, d_tail, s));
        AK(aesw_msm_commit_device(ctx, K, 1, AESW_MSM_BYTES, 0, d_bytes, d_basis, d_commit + 64 * run, d_ws, s));
        AK(aesw_blind_commit_tail_device(ctx, K, 1, first_row, d_tail, d_basis, d_commit + 64 * run, s));
    }

    uint8_t commit[3 * 64], tail[TAIL * 32], zero[64] = {0};
    aesw_msm_report report;
    CK(hipMemcpyAsync(commit, d_commit, sizeof commit, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(tail, d_tail, sizeof tail, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&report, d_report, sizeof report, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    WANT(report.bad_points == 0, "every point of the params is on the curve");
    WANT(memcmp(commit, zero, 64) && memcmp(commit + 64, zero, 64), "neither commitment is the identity");
    WANT(memcmp(commit, commit + 64, 64), "the blinded commitment is not the bytes' own");
    WANT(!memcmp(commit + 64, commit + 128, 64), "the same seed gives the same commitment");
    /* a tail above what the commitment takes, and a first_row outside the column, are refused with nothing enqueued */
    WANT(aesw_blind_commit_tail_device(ctx, K, 1, rows - aesw_blind_max_tail() - 1, d_tail, d_basis, d_commit, s) == AESW_ERR_INVALID_ARG, "a tail of 65 rows is refused");
    WANT(aesw_blind_tail_device(ctx, K, 1, rows, domain, 0, d_seed, d_tail, s) == AESW_ERR_INVALID_ARG, "first_row = 2^k is refused");

    printf("domain %llu\n", (unsigned long long)domain);
    print_hex("tail", tail, sizeof tail);
    print_hex("bytes", commit, 64);
    print_hex("commitment", commit + 64, 64);

    CK(hipStreamDestroy(s));
    CK(hipFree(d_canonical)); CK(hipFree(d_basis)); CK(hipFree(d_bytes)); CK(hipFree(d_seed)); CK(hipFree(d_tail)); CK(hipFree(d_commit)); CK(hipFree(d_report)); CK(hipFree(d_ws));
    free(canonical); free(bytes);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
