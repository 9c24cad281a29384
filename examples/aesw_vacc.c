/*
 * aesw_vacc.c -- the lookup multiplicities of one circuit from its VALUES witness, from plain C.
 *
 *   One FixedAes128Config<14, 3> circuit (34 blocks) is generated as a VALUES witness -- 448 y and 608 z bytes per block, no x
 *   column -- and counted by libaesw_vacc.so in two runs: aesw_acc_reset_device once, aesw_vacc_add_device per run, and
 *   aesw_acc_add_key_device for the key slab's own rows (libaesw_acc.so: the histograms are its).  Then the same inputs are
 *   generated as a PACKED witness and accumulated by aesw_acc_add_device into a second set of histograms, and the two are
 *   compared bin for bin.  Printed per set: the sums of the five sections in selector order (range, xor, sbox, mul2, mul3).
 *
 * usage: aesw_vacc [K [N]]                 (default 14 3)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_vacc.c -L halo2-aes_amd -laesw_vacc -laesw_acc
 *            -laesw -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_vacc.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_acc.h"
#include "aesw_vacc.h"

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
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 14, n_sets = argc > 2 ? (uint32_t)atoi(argv[2]) : 3;
    const uint64_t n = aesw_block_capacity(k, n_sets), half = n / 2;
    if (n < 2) { fprintf(stderr, "needs a circuit of two blocks or more (K >= 12)\n"); return 1; }
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    AK(aesw_vacc_prepare(ctx)); /* the one synchronous step, ahead of the stream */
    const int V = AESW_LAYOUT_VALUES, P = AESW_LAYOUT_PACKED;
    const uint32_t ys = aesw_column_stride(V, 1), zs = aesw_column_stride(V, 2);

    uint8_t *pt = (uint8_t *)malloc(n * 16), key[16];
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (int i = 0; i < 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; key[i] = (uint8_t)(x >> 32); }

    uint8_t *d_pt, *d_key, *d_vy, *d_vz, *d_px, *d_py, *d_pz;
    uint32_t *d_mult[2]; /* 0: from VALUES, 1: from PACKED */
    aesw_key_slab ks;
    aesw_mult_report *d_rep, rep[2];
    const size_t mult_bytes = (size_t)n_sets * AESW_TABLE_ROWS * sizeof(uint32_t);
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_key, 16));
    CK(hipMalloc((void **)&d_vy, n * ys));
    CK(hipMalloc((void **)&d_vz, n * zs));
    CK(hipMalloc((void **)&d_px, n * aesw_column_stride(P, 0)));
    CK(hipMalloc((void **)&d_py, n * aesw_column_stride(P, 1)));
    CK(hipMalloc((void **)&d_pz, n * aesw_column_stride(P, 2)));
    CK(hipMalloc((void **)&ks.w, AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, aesw_key_column_stride(P, 0))); /* the key slabs of VALUES are the packed ones */
    CK(hipMalloc((void **)&ks.ky, aesw_key_column_stride(P, 1)));
    CK(hipMalloc((void **)&ks.kz, aesw_key_column_stride(P, 2)));
    CK(hipMalloc((void **)&d_mult[0], mult_bytes));
    CK(hipMalloc((void **)&d_mult[1], mult_bytes));
    CK(hipMalloc((void **)&d_rep, 2 * sizeof rep[0]));
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_key, key, 16, hipMemcpyHostToDevice));

    AK(aesw_key_schedule_witness_device(ctx, d_key, 1, P, ks.w, ks.kx, ks.ky, ks.kz, NULL, NULL));
    /* from the VALUES witness: two runs, the second one first -- the order does not enter */
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_key, 0, n, V, NULL, d_vy, d_vz, NULL, NULL, NULL));
    AK(aesw_acc_reset_device(ctx, n_sets, d_mult[0], &d_rep[0], NULL));
    AK(aesw_vacc_add_device(ctx, k, n_sets, half, n - half, d_pt + half * 16, d_vy + half * ys, d_vz + half * zs, &ks, d_mult[0], &d_rep[0], NULL));
    AK(aesw_vacc_add_device(ctx, k, n_sets, 0, half, d_pt, d_vy, d_vz, &ks, d_mult[0], &d_rep[0], NULL));
    AK(aesw_acc_add_key_device(ctx, k, P, &ks, d_mult[0], &d_rep[0], NULL));
    /* from the PACKED witness of the same inputs */
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_key, 0, n, P, d_px, d_py, d_pz, NULL, NULL, NULL));
    AK(aesw_acc_reset_device(ctx, n_sets, d_mult[1], &d_rep[1], NULL));
    AK(aesw_acc_add_device(ctx, k, n_sets, 0, n, P, d_px, d_py, d_pz, d_mult[1], &d_rep[1], NULL));
    AK(aesw_acc_add_key_device(ctx, k, P, &ks, d_mult[1], &d_rep[1], NULL));

    uint32_t *mult = (uint32_t *)malloc(mult_bytes), *mult_p = (uint32_t *)malloc(mult_bytes);
    CK(hipMemcpy(mult, d_mult[0], mult_bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(mult_p, d_mult[1], mult_bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));

    /* the sections in selector order, tags 1 (range), 2 (xor), 3 (sbox), 4 (mul2), 5 (mul3): where each starts is aesw_mult.h's rule */
    static const uint32_t first_row[5] = {0, 512, 256, 66048, 66304}, rows[5] = {256, 65536, 256, 256, 256};
    uint64_t total = 0;
    for (uint32_t s = 0; s < n_sets; ++s) {
        const uint32_t *m = mult + (size_t)s * AESW_TABLE_ROWS;
        uint64_t sum[5] = {0, 0, 0, 0, 0};
        for (int t = 0; t < 5; ++t) {
            for (uint32_t i = 0; i < rows[t]; ++i) sum[t] += m[first_row[t] + i];
            total += sum[t];
        }
        printf("set %u: range %llu xor %llu sbox %llu mul2 %llu mul3 %llu\n", s, (unsigned long long)sum[0], (unsigned long long)sum[1],
               (unsigned long long)sum[2], (unsigned long long)sum[3], (unsigned long long)sum[4]);
        if (m[AESW_TABLE_ROWS - 1] != 0) { fprintf(stderr, "the all-zero row was counted\n"); return 4; }
    }
    printf("%llu blocks in 2 runs (K = %u, N = %u): %llu lookups, %llu misses\n", (unsigned long long)n, k, n_sets,
           (unsigned long long)rep[0].lookups, (unsigned long long)rep[0].misses);
    if (rep[0].misses != 0 || rep[0].first_miss != AESW_CHECK_NONE || rep[0].lookups != total) {
        fprintf(stderr, "the product's own witness misses the table, or a hit was left out of the bins\n");
        return 4;
    }
    if (memcmp(mult, mult_p, mult_bytes) != 0 || memcmp(&rep[0], &rep[1], sizeof rep[0]) != 0) {
        fprintf(stderr, "the VALUES and the PACKED accumulation of the same inputs differ\n");
        return 5;
    }
    printf("VALUES and PACKED agree in %llu bins\n", (unsigned long long)n_sets * AESW_TABLE_ROWS);
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
