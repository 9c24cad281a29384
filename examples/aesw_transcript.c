/*
 * aesw_transcript.c -- from committed columns to theta with no host in between, from plain C.
 *
 *   The basis: 2^K points from plain coordinates, the generator G = (1, 2) throughout, converted and checked on the device.  Two byte
 *   columns -- a single 1 at row 0, a single 3 at row 2 -- are committed (to G and to 3 G).  The two commitments go, as they lie in
 *   device memory, into the transcript by write_point; theta is squeezed into device memory, and that pointer is handed straight to
 *   aesw_theta_compress_table_device.  Everything is enqueued on one stream; the host waits once, at the end, and prints the proof's
 *   bytes, theta's cell and the state's count words.  tests/test_gpu_transcript_example.py holds the output against the model.
 *
 * usage: aesw_transcript [K]                      (default 10; K 10 ... 16)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_transcript.c -L halo2-aes_amd -laesw_transcript
 *            -laesw_msm -laesw_theta -laesw -L /opt/rocm/lib -lamdhip64
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_msm.h"
#include "aesw_theta.h"
#include "aesw_transcript.h"

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

static void print_hex(const char *label, const uint8_t *bytes, size_t n) {
    printf("%s ", label);
    for (size_t i = 0; i < n; ++i) printf("%02x", bytes[i]);
    printf("\n");
}

#define N_COLS 2u

int main(int argc, char **argv) {
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 10;
    if (k < 10 || k > 16) { fprintf(stderr, "K must be 10 ... 16 here\n"); return 1; }
    const size_t rows = (size_t)1 << k, table_bytes = (size_t)AESW_THETA_TABLES * AESW_TABLE_ROWS * 32;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));

    uint8_t *canonical = (uint8_t *)calloc(rows, 64), *bytes = (uint8_t *)calloc(N_COLS * rows, 1);
    if (!canonical || !bytes) return 2;
    for (size_t i = 0; i < rows; ++i) { canonical[64 * i] = 1; canonical[64 * i + 32] = 2; }
    bytes[0] = 1;            /* column 0: G */
    bytes[rows + 2] = 3;     /* column 1: 3 G */

    uint8_t *d_canonical, *d_basis, *d_bytes, *d_commitments, *d_state, *d_proof, *d_theta, *d_table;
    aesw_msm_report *d_msm_report;
    aesw_theta_report *d_theta_report;
    void *d_ws;
    const size_t ws_bytes = aesw_msm_workspace_bytes(k, N_COLS, AESW_MSM_BYTES, 0), proof_capacity = N_COLS * 32;
    WANT(ws_bytes, "the workspace size");
    CK(hipMalloc((void **)&d_canonical, rows * 64));
    CK(hipMalloc((void **)&d_basis, rows * 64));
    CK(hipMalloc((void **)&d_bytes, N_COLS * rows));
    CK(hipMalloc((void **)&d_commitments, N_COLS * 64));
    CK(hipMalloc((void **)&d_state, AESW_TRANSCRIPT_STATE_BYTES));
    CK(hipMalloc((void **)&d_proof, proof_capacity));
    CK(hipMalloc((void **)&d_theta, 32));
    CK(hipMalloc((void **)&d_table, table_bytes));
    CK(hipMalloc((void **)&d_msm_report, sizeof(aesw_msm_report)));
    CK(hipMalloc((void **)&d_theta_report, sizeof(aesw_theta_report)));
    CK(hipMalloc(&d_ws, ws_bytes));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    CK(hipMemcpyAsync(d_canonical, canonical, rows * 64, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(d_bytes, bytes, N_COLS * rows, hipMemcpyHostToDevice, s));

    /* one sequence on one stream: nothing below waits for anything above on the host */
    AK(aesw_msm_basis_device(ctx, k, d_canonical, d_basis, d_msm_report, s));
    AK(aesw_msm_commit_device(ctx, k, N_COLS, AESW_MSM_BYTES, 0, d_bytes, d_basis, d_commitments, d_ws, s));
    AK(aesw_transcript_init_device(ctx, d_state, s));
    AK(aesw_transcript_points_device(ctx, d_state, N_COLS, d_commitments, d_proof, proof_capacity, s));
    AK(aesw_transcript_squeeze_device(ctx, d_state, d_theta, s));
    AK(aesw_theta_compress_table_device(ctx, d_theta, d_table, d_theta_report, s));

    uint8_t proof[N_COLS * 32], theta[32];
    uint64_t state[AESW_TRANSCRIPT_STATE_BYTES / 8];
    aesw_msm_report msm_report;
    aesw_theta_report theta_report;
    CK(hipMemcpyAsync(proof, d_proof, sizeof proof, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(theta, d_theta, sizeof theta, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&msm_report, d_msm_report, sizeof msm_report, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&theta_report, d_theta_report, sizeof theta_report, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));

    WANT(msm_report.bad_points == 0, "every point of the params is on the curve");
    WANT(proof[0] == 1 && proof[31] == 0, "G = (1, 2) is written as x = 1 with the sign of an even y");
    WANT(state[26] == proof_capacity && state[27] == 0 && state[28] == 0 && state[29] == ~0ull && state[30] == N_COLS, "the count words of the state");
    WANT(theta_report.cells == (uint64_t)AESW_THETA_TABLES * AESW_TABLE_ROWS && theta_report.noncanonical == 0, "theta is a canonical cell and the table was compressed under it");
    /* a refusal enqueues nothing */
    WANT(aesw_transcript_points_device(ctx, d_state, 0, d_commitments, d_proof, proof_capacity, s) == AESW_ERR_INVALID_ARG, "n = 0 is refused");
    WANT(aesw_transcript_points_device(ctx, d_state, N_COLS, d_commitments, NULL, proof_capacity, s) == AESW_ERR_INVALID_ARG, "a capacity without a proof is refused");

    print_hex("proof", proof, sizeof proof);
    print_hex("theta", theta, sizeof theta);
    printf("status proof_bytes %llu proof_missed %llu identities %llu points %llu\n", (unsigned long long)state[26], (unsigned long long)state[27],
           (unsigned long long)state[28], (unsigned long long)state[30]);
    printf("table cells %llu noncanonical %llu\n", (unsigned long long)theta_report.cells, (unsigned long long)theta_report.noncanonical);

    CK(hipStreamDestroy(s));
    CK(hipFree(d_canonical)); CK(hipFree(d_basis)); CK(hipFree(d_bytes)); CK(hipFree(d_commitments)); CK(hipFree(d_state)); CK(hipFree(d_proof));
    CK(hipFree(d_theta)); CK(hipFree(d_table)); CK(hipFree(d_msm_report)); CK(hipFree(d_theta_report)); CK(hipFree(d_ws));
    free(canonical); free(bytes);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
