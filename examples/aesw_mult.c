/*
 * aesw_mult.c -- the lookup multiplicities of a few circuits, from plain C (no Python, no torch in the process).
 *
 *   C FixedAes128Config<K, N> circuits: one key-schedule launch, one encrypt launch with each block under its circuit's key, and
 *   one aesw_mult_count_device launch (libaesw_mult.so) that counts, per circuit and column set, how often every row of the
 *   66 561-row lookup table is looked up.  Printed per (circuit, set): the sums of the five sections in selector order (range, xor,
 *   sbox, mul2, mul3) -- each is the number of rows on which that selector is enabled -- and, at the end, the misses.
 *
 * usage: aesw_mult [K [N [C]]]            (default 13 3 3; circuit 1 is left with fewer blocks)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_mult.c -L halo2-aes_amd -laesw_mult -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_mult_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "aesw_mult.h"

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
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 13, n_sets = argc > 2 ? (uint32_t)atoi(argv[2]) : 3;
    const uint32_t nc = argc > 3 ? (uint32_t)atoi(argv[3]) : 3;
    const uint64_t cap = aesw_block_capacity(k, n_sets);
    if (nc < 2 || cap < 2) { fprintf(stderr, "needs C >= 2 circuits that hold two blocks or more (K >= 12)\n"); return 1; }
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    const int L = AESW_LAYOUT_PACKED;

    uint64_t *offs = (uint64_t *)malloc((nc + 1) * sizeof *offs);
    offs[0] = 0;
    for (uint32_t c = 0; c < nc; ++c) offs[c + 1] = offs[c] + (c == 1 ? cap / 2 : cap);
    const uint64_t n = offs[nc];
    uint8_t *pt = (uint8_t *)malloc(n * 16), *keys = (uint8_t *)malloc((size_t)nc * 16), *bkeys = (uint8_t *)malloc(n * 16);
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (uint64_t i = 0; i < (uint64_t)nc * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; keys[i] = (uint8_t)(x >> 32); }
    for (uint32_t c = 0; c < nc; ++c)  /* every block under its circuit's key */
        for (uint64_t b = offs[c]; b < offs[c + 1]; ++b)
            for (int i = 0; i < 16; ++i) bkeys[b * 16 + i] = keys[c * 16 + i];

    uint8_t *d_pt, *d_keys, *d_bkeys, *d_x, *d_y, *d_z;
    uint64_t *d_offs;
    uint32_t *d_mult;
    aesw_key_slab ks;
    aesw_mult_report *d_rep, rep;
    const size_t hists = (size_t)nc * n_sets, mult_bytes = hists * AESW_TABLE_ROWS * sizeof(uint32_t);
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_keys, (size_t)nc * 16));
    CK(hipMalloc((void **)&d_bkeys, n * 16));
    CK(hipMalloc((void **)&d_offs, (nc + 1) * sizeof *offs));
    CK(hipMalloc((void **)&d_x, n * aesw_column_stride(L, 0)));
    CK(hipMalloc((void **)&d_y, n * aesw_column_stride(L, 1)));
    CK(hipMalloc((void **)&d_z, n * aesw_column_stride(L, 2)));
    CK(hipMalloc((void **)&ks.w, (size_t)nc * AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, (size_t)nc * aesw_key_column_stride(L, 0)));
    CK(hipMalloc((void **)&ks.ky, (size_t)nc * aesw_key_column_stride(L, 1)));
    CK(hipMalloc((void **)&ks.kz, (size_t)nc * aesw_key_column_stride(L, 2)));
    CK(hipMalloc((void **)&d_mult, mult_bytes));
    CK(hipMalloc((void **)&d_rep, sizeof rep));
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_keys, keys, (size_t)nc * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_bkeys, bkeys, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_offs, offs, (nc + 1) * sizeof *offs, hipMemcpyHostToDevice));

    /* two launches make the witness, the third counts it: all on one stream, none waits on the host */
    AK(aesw_key_schedule_witness_device(ctx, d_keys, nc, L, ks.w, ks.kx, ks.ky, ks.kz, NULL, NULL));
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_bkeys, 1, n, L, d_x, d_y, d_z, NULL, NULL, NULL));
    AK(aesw_mult_count_device(ctx, k, n_sets, nc, d_offs, L, d_x, d_y, d_z, &ks, d_mult, d_rep, NULL));
    uint32_t *mult = (uint32_t *)malloc(mult_bytes);
    CK(hipMemcpy(mult, d_mult, mult_bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));

    /* the sections in selector order: tags 1 (range), 2 (xor), 3 (sbox), 4 (mul2), 5 (mul3) */
    uint64_t total = 0;
    for (size_t h = 0; h < hists; ++h) {
        const uint32_t *m = mult + h * AESW_TABLE_ROWS;
        uint64_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t tag = 1; tag <= 5; ++tag) {
            const uint32_t first = aesw_mult_bin(tag, 0, 0), rows = tag == 2 ? 65536u : 256u;
            for (uint32_t i = 0; i < rows; ++i) sum[tag - 1] += m[first + i];
            total += sum[tag - 1];
        }
        printf("circuit %zu set %zu: range %llu xor %llu sbox %llu mul2 %llu mul3 %llu\n", h / n_sets, h % n_sets, (unsigned long long)sum[0],
               (unsigned long long)sum[1], (unsigned long long)sum[2], (unsigned long long)sum[3], (unsigned long long)sum[4]);
        if (m[AESW_TABLE_ROWS - 1] != 0) { fprintf(stderr, "the all-zero row was counted\n"); return 4; }
    }
    printf("%llu blocks in %u circuits (K = %u, N = %u): %llu lookups, %llu misses\n", (unsigned long long)n, nc, k, n_sets,
           (unsigned long long)rep.lookups, (unsigned long long)rep.misses);
    if (rep.misses != 0 || rep.first_miss != AESW_CHECK_NONE || rep.lookups != total) {
        fprintf(stderr, "the product's own witness misses the table, or a hit was left out of the bins\n");
        return 4;
    }
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
