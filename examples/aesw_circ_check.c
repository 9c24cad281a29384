/*
 * aesw_circ_check.c -- a many-circuit batch certified in one launch, from plain C (no Python, no torch in the process).
 *
 *   C FixedAes128Config<K, N> circuits as a prover's create_proof(&[circuit; C]) holds them: C keys scheduled into C key slabs,
 *   the blocks' witness with each block under its circuit's key, the advice columns of every circuit in one assemble launch --
 *   and aesw_circ_check_witness_device (libaesw_circ.so) running MockProver's criterion over all of it in one more.  Then one
 *   byte of one cell is changed and the report names the block (batch-wide), its circuit, the kind of constraint and the row.
 *
 * usage: aesw_circ_check [K [N [C]]]            (default 14 1 64; some circuits are left with fewer blocks, one with none)
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_circ_check.c -L halo2-aes_amd -laesw_circ -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_circ_check_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "aesw_circ.h"

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
    const uint32_t k = argc > 1 ? (uint32_t)atoi(argv[1]) : 14, n_sets = argc > 2 ? (uint32_t)atoi(argv[2]) : 1;
    const uint32_t nc = argc > 3 ? (uint32_t)atoi(argv[3]) : 64;
    const uint64_t cap = aesw_block_capacity(k, n_sets);
    if (nc < 3 || cap < 2) { fprintf(stderr, "needs C >= 3 circuits that hold two blocks or more (K >= 12)\n"); return 1; }
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));
    const int L = AESW_LAYOUT_PACKED;

    /* ragged counts: circuit 1 holds no block, every third one is short */
    uint64_t *offs = (uint64_t *)malloc((nc + 1) * sizeof *offs);
    offs[0] = 0;
    for (uint32_t c = 0; c < nc; ++c) offs[c + 1] = offs[c] + (c == 1 ? 0 : c % 3 == 2 ? cap / 2 : cap);
    const uint64_t n = offs[nc];
    uint8_t *pt = (uint8_t *)malloc(n * 16), *keys = (uint8_t *)malloc((size_t)nc * 16), *bkeys = (uint8_t *)malloc(n * 16);
    uint64_t x = 0x2545f4914f6cdd1dull;
    for (uint64_t i = 0; i < n * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pt[i] = (uint8_t)x; }
    for (uint64_t i = 0; i < (uint64_t)nc * 16; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; keys[i] = (uint8_t)(x >> 32); }
    for (uint32_t c = 0; c < nc; ++c)  /* every block under its circuit's key */
        for (uint64_t b = offs[c]; b < offs[c + 1]; ++b)
            for (int i = 0; i < 16; ++i) bkeys[b * 16 + i] = keys[c * 16 + i];

    uint8_t *d_pt, *d_keys, *d_bkeys, *d_x, *d_y, *d_z, *d_ct, *d_adv;
    uint64_t *d_offs;
    aesw_key_slab ks;
    aesw_circ_check_report *d_rep, rep;
    const uint64_t adv_cells = (uint64_t)nc * (3 * n_sets + 1) << k;
    CK(hipMalloc((void **)&d_pt, n * 16));
    CK(hipMalloc((void **)&d_keys, (size_t)nc * 16));
    CK(hipMalloc((void **)&d_bkeys, n * 16));
    CK(hipMalloc((void **)&d_offs, (nc + 1) * sizeof *offs));
    CK(hipMalloc((void **)&d_x, n * aesw_column_stride(L, 0)));
    CK(hipMalloc((void **)&d_y, n * aesw_column_stride(L, 1)));
    CK(hipMalloc((void **)&d_z, n * aesw_column_stride(L, 2)));
    CK(hipMalloc((void **)&d_ct, n * 16));
    CK(hipMalloc((void **)&ks.w, (size_t)nc * AESW_WORDS_ROWS));
    CK(hipMalloc((void **)&ks.kx, (size_t)nc * aesw_key_column_stride(L, 0)));
    CK(hipMalloc((void **)&ks.ky, (size_t)nc * aesw_key_column_stride(L, 1)));
    CK(hipMalloc((void **)&ks.kz, (size_t)nc * aesw_key_column_stride(L, 2)));
    CK(hipMalloc((void **)&d_adv, adv_cells));
    CK(hipMalloc((void **)&d_rep, sizeof rep));
    CK(hipMemcpy(d_pt, pt, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_keys, keys, (size_t)nc * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_bkeys, bkeys, n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_offs, offs, (nc + 1) * sizeof *offs, hipMemcpyHostToDevice));

    /* three launches make the batch, the fourth certifies it: all on one stream, none waits on the host */
    AK(aesw_key_schedule_witness_device(ctx, d_keys, nc, L, ks.w, ks.kx, ks.ky, ks.kz, NULL, NULL));
    AK(aesw_encrypt_witness_device(ctx, d_pt, d_bkeys, 1, n, L, d_x, d_y, d_z, d_ct, NULL, NULL));
    AK(aesw_assemble_advice_circuits_device(ctx, k, n_sets, nc, d_offs, L, d_x, d_y, d_z, &ks, 0, d_adv, NULL));
    AK(aesw_circ_check_witness_device(ctx, k, n_sets, nc, d_offs, n, d_pt, d_keys, L, d_x, d_y, d_z, d_ct, &ks, d_rep, NULL));
    CK(hipMemcpy(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));
    printf("%u circuits (K = %u, N = %u): %llu blocks + %llu key slabs checked in one launch: %llu lookup, %llu copy, %llu gate, %llu literal, "
           "%llu offset failures\n", nc, k, n_sets, (unsigned long long)rep.blocks, (unsigned long long)rep.keys,
           (unsigned long long)rep.lookup_failures, (unsigned long long)rep.copy_failures, (unsigned long long)rep.gate_failures,
           (unsigned long long)rep.input_failures, (unsigned long long)rep.offset_failures);
    if (rep.blocks != n || rep.keys != nc || rep.lookup_failures || rep.copy_failures || rep.gate_failures || rep.input_failures ||
        rep.offset_failures || rep.first != AESW_CHECK_NONE) { fprintf(stderr, "the product's own batch does not satisfy the circuits\n"); return 4; }

    /* one cell of the last block of circuit 2 off by one bit: y of row 40 (an S-box row of round 1), packed index 40 - 16 */
    const uint64_t victim = offs[3] - 1;
    uint8_t b;
    uint8_t *cell = d_y + victim * aesw_column_stride(L, 1) + 24;
    CK(hipMemcpy(&b, cell, 1, hipMemcpyDeviceToHost));
    b ^= 0x08;
    CK(hipMemcpy(cell, &b, 1, hipMemcpyHostToDevice));
    AK(aesw_circ_check_witness_device(ctx, k, n_sets, nc, d_offs, n, d_pt, d_keys, L, d_x, d_y, d_z, d_ct, &ks, d_rep, NULL));
    CK(hipMemcpy(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost));
    const uint64_t unit = AESW_CHECK_UNIT(rep.first);
    const uint32_t circuit = aesw_circ_circuit_of_block(offs, nc, unit);
    printf("after changing one byte: %llu lookup and %llu copy failures; first: block %llu (block %llu of circuit %u), %s, %s %u\n",
           (unsigned long long)rep.lookup_failures, (unsigned long long)rep.copy_failures, (unsigned long long)unit,
           (unsigned long long)(unit - offs[circuit]), circuit, kind_name((unsigned)AESW_CHECK_KIND(rep.first)),
           AESW_CHECK_KIND(rep.first) == 2 ? "copy" : "row", (unsigned)AESW_CHECK_INDEX(rep.first));
    if (rep.first == AESW_CHECK_NONE || unit != victim || circuit != 2 || AESW_CHECK_IS_KEY_SLAB(rep.first) || rep.lookup_failures != 1 ||
        AESW_CHECK_KIND(rep.first) != 1 || AESW_CHECK_INDEX(rep.first) != 40 || rep.copy_failures < 1 || rep.offset_failures) {
        fprintf(stderr, "the changed byte was not reported as expected\n");
        return 4;
    }
    aesw_destroy(ctx);
    printf("ok\n");
    return 0;
}
