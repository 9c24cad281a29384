/*
 * aesw_vals_check.c -- "verify what you received", from plain C (no Python, no torch in the process).
 *
 *   A host that keeps the reference's chips takes the VALUES layout: 448 y + 608 z bytes per block, a third of PACKED.  Before
 *   it assigns them it can have the device certify them where they lie: aesw_vals_check_device (libaesw_vals.so) runs
 *   MockProver's criterion over the assignment those bytes determine -- every lookup of every block, each operand resolved
 *   through the copy graph -- and over the key slabs, in one launch.
 *
 * usage: aesw_vals_check [n [poke]]     (default 65536 blocks, per-block keys; "poke" changes one y byte of the last block first)
 * exit:  0 the witness satisfies the circuit, 5 it does not (the first failure is printed), 2 / 3 a HIP / library error
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_vals_check.c -L halo2-aes_amd -laesw_vals -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_vals_check.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "aesw_vals.h"

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

static const char *kind_name(unsigned k) { return k == 1 ? "lookup" : k == 2 ? "copy constraint" : k == 3 ? "rcon gate" : k == 4 ? "literal row" : "?"; }

int main(int argc, char **argv) {
    const uint64_t n = argc > 1 ? (uint64_t)atoll(argv[1]) : 65536;
    const int poke = argc > 2;
    if (n == 0) { fprintf(stderr, "needs a block\n"); return 1; }
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    const int L = AESW_LAYOUT_VALUES;
    const uint32_t sy = aesw_column_stride(L, 1), sz = aesw_column_stride(L, 2);

    uint8_t *pt = (uint8_t *)malloc(n * 16), *keys = (uint8_t *)malloc(n * 16);
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; keys[i] = (uint8_t)(x >> 32); }

    uint8_t *d_pt, *d_keys, *d_y, *d_z, *d_ct;
    aesw_key_slab ks;
    aesw_check_report *d_rep, rep;
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_keys, n * 16));
    CK(hipMalloc((void **)&d_y, n * sy));
    CK(hipMalloc((void **)&d_z, n * sz));
    CK(hipMalloc((void **)&d_ct, n * 16));
    CK(hipMalloc((void **)&ks.w, n * AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, n * aesw_key_column_stride(L, 0)));
    CK(hipMalloc((void **)&ks.ky, n * aesw_key_column_stride(L, 1)));
    CK(hipMalloc((void **)&ks.kz, n * aesw_key_column_stride(L, 2)));
    CK(hipMalloc((void **)&d_rep, sizeof rep));
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_keys, keys, n * 16, hipMemcpyHostToDevice));

    /* the witness as a chip-keeping host receives it: no x column */
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_keys, 1, n, L, NULL, d_y, d_z, d_ct, &ks, NULL));
    if (poke) {  /* y of slab row 40 of the last block (an S-box row of round 1): VALUES index 40 - 32 */
        uint8_t b;
        uint8_t *cell = d_y + (n - 1) * sy + 8;
        CK(hipMemcpy(&b, cell, 1, hipMemcpyDeviceToHost));
        b ^= 0x08;
        CK(hipMemcpy(cell, &b, 1, hipMemcpyHostToDevice));
    }
    AK(aesw_vals_check_device(ctx, d_pt, d_keys, 1, n, d_y, d_z, d_ct, &ks, d_rep, NULL));
    CK(hipMemcpy(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));
    printf("%llu blocks + %llu key slabs: %llu lookup, %llu copy, %llu gate, %llu literal failures (%u resolved lookups per block, image %u B)\n",
           (unsigned long long)rep.blocks, (unsigned long long)rep.keys, (unsigned long long)rep.lookup_failures,
           (unsigned long long)rep.copy_failures, (unsigned long long)rep.gate_failures, (unsigned long long)rep.input_failures,
           aesw_vals_check_rows(), aesw_vals_image_bytes());
    const int satisfied = rep.blocks == n && rep.keys == n && !rep.lookup_failures && !rep.copy_failures && !rep.gate_failures &&
                          !rep.input_failures && rep.first == AESW_CHECK_NONE;
    if (!satisfied && rep.first != AESW_CHECK_NONE)
        printf("first: %s %llu, %s, row %u\n", AESW_CHECK_IS_KEY_SLAB(rep.first) ? "key slab" : "block", (unsigned long long)AESW_CHECK_UNIT(rep.first),
               kind_name((unsigned)AESW_CHECK_KIND(rep.first)), (unsigned)AESW_CHECK_INDEX(rep.first));
    aesw_destroy(ctx);
    if (!satisfied) { fprintf(stderr, "the witness does not satisfy the circuit\n"); return 5; }
    printf("ok\n");
    return 0;
}
