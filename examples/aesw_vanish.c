/*
 * aesw_vanish.c -- the quotient h(X) folded segment by segment, from plain C.
 *
 *   K = 10, ext_k = 12, one column set, chunk_len 3: 36 extended columns of 2^12 canonical cells (seeded bytes, the top byte kept
 *   below r's) stand for a circuit's column groups.  On one stream with nothing waiting in between: the tables, the scalars block
 *   from four seeded challenges, HEAD, PERM(0), PERM(1), LOOKUP(0) and the division -- once with every segment folding into one
 *   buffer in place, once from buffer to buffer.  The result is checked on the host against the header's own fold: GOLDEN holds
 *   the 4096 cells csrc/aesw_vanish.h's segments give for these seeded columns and challenges when tests/vanish_driver.cpp runs
 *   them on the CPU (tests/golden/vanish_example_k10.bin; WRITE_INPUT writes the columns, the challenges and a zero column in that
 *   driver's order, which is how the file was made: vanish_driver run 10 12 1 1 3 1018 INPUT GOLDEN).  Beyond that, what bytes
 *   alone can say: both ways give the same cells, every cell is below r, the block holds the four challenges where
 *   aesw_vanish_scalars_offset says they lie, and a second run with another y gives other cells.
 *
 * usage: aesw_vanish GOLDEN [WRITE_INPUT]
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/aesw_vanish.c -L halo2-aes_amd -laesw_vanish -laesw
 *            -L /opt/rocm/lib -lamdhip64
 * tests/test_gpu_vanish_example.py builds and runs it.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aesw_vanish.h"

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

enum { K = 10, EXT_K = 12, N_SETS = 1, CHUNK_LEN = 3, N_ROWS = 1018, PERM_SETS = 2 };
/* the groups: advice 4, rcon 2, selectors 5, table 4, sigma 5, zperm 2, a 5, s 5, zlookup 5, l 3 -- and the permutation's values
 * x0 y0 z0 words rcon gathered set by set: 3 + 2 columns */
enum { ADVICE = 0, RCON = 4, SELECTORS = 6, TABLE = 11, SIGMA = 15, ZPERM = 20, A = 22, S = 27, ZLOOKUP = 32, L = 37, VALUES = 40, COLUMNS = 45 };

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: aesw_vanish GOLDEN [WRITE_INPUT]\n"); return 1; }
    const size_t rows = (size_t)1 << EXT_K, col = rows * 32;
    uint8_t sbox[256], m2[256], m3[256];
    tables(sbox, m2, m3);
    aesw_ctx *ctx = NULL;
    AK(aesw_create(&ctx, 0, sbox, m2, m3));

    uint8_t *host = (uint8_t *)malloc(COLUMNS * col), *one = (uint8_t *)malloc(col), *two = (uint8_t *)malloc(col), *other = (uint8_t *)malloc(col);
    uint8_t challenges[4 * 32], moved[4 * 32], block[4 * 32];
    seeded_cells(host, VALUES * rows, 0x2545f4914f6cdd1dull);
    seeded_cells(challenges, 4, 0x9e3779b97f4a7c15ull);
    memcpy(moved, challenges, sizeof moved);
    moved[3 * 32] ^= 1;
    /* the permutation's values: x0 y0 z0 | words rcon */
    memcpy(host + (VALUES + 0) * col, host + (ADVICE + 0) * col, 3 * col);
    memcpy(host + (VALUES + 3) * col, host + (ADVICE + 3) * col, col);
    memcpy(host + (VALUES + 4) * col, host + (RCON + 0) * col, col);

    const size_t tables_bytes = aesw_vanish_tables_bytes(K, EXT_K), scalars_bytes = aesw_vanish_scalars_bytes(N_SETS, CHUNK_LEN);
    if (!tables_bytes || !scalars_bytes || aesw_vanish_scalars_offset(AESW_VANISH_Y, 0) != 3 * 32 || aesw_vanish_scalars_offset(AESW_VANISH_Y, 1) != (size_t)-1) {
        fprintf(stderr, "the sizes or the offsets are off\n");
        return 4;
    }
    uint8_t *d, *d_tables, *d_scalars, *d_ch, *d_acc, *d_ping, *d_pong;
    hipStream_t stream;
    CK(hipStreamCreate(&stream));
    CK(hipMalloc((void **)&d, COLUMNS * col));
    CK(hipMalloc((void **)&d_tables, tables_bytes));
    CK(hipMalloc((void **)&d_scalars, scalars_bytes));
    CK(hipMalloc((void **)&d_ch, sizeof challenges));
    CK(hipMalloc((void **)&d_acc, col));
    CK(hipMalloc((void **)&d_ping, col));
    CK(hipMalloc((void **)&d_pong, col));
    CK(hipMemcpyAsync(d, host, COLUMNS * col, hipMemcpyHostToDevice, stream));
    AK(aesw_vanish_tables_device(ctx, K, EXT_K, 1, d_tables, stream));

    for (int run = 0; run < 2; ++run) { /* the second run: another y */
        CK(hipMemcpyAsync(d_ch, run ? moved : challenges, sizeof challenges, hipMemcpyHostToDevice, stream));
        AK(aesw_vanish_scalars_device(ctx, N_SETS, CHUNK_LEN, d_ch, d_ch + 32, d_ch + 64, d_ch + 96, d_scalars, stream));
        /* in place: every segment folds into d_acc */
        AK(aesw_vanish_head_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, d + (ADVICE + 3) * col, d + RCON * col, d + ZPERM * col, d + L * col, d_scalars, d_acc, stream));
        AK(aesw_vanish_perm_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, 0, d + VALUES * col, d + SIGMA * col, d + ZPERM * col, d + L * col, d_tables, d_scalars,
                                   d_acc, d_acc, stream));
        AK(aesw_vanish_perm_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, 1, d + (VALUES + 3) * col, d + (SIGMA + 3) * col, d + (ZPERM + 1) * col, d + L * col, d_tables,
                                   d_scalars, d_acc, d_acc, stream));
        AK(aesw_vanish_lookup_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, 0, d + ADVICE * col, d + SELECTORS * col, d + TABLE * col, d + A * col, d + S * col,
                                     d + ZLOOKUP * col, d + L * col, d_scalars, d_acc, d_acc, stream));
        AK(aesw_vanish_divide_device(ctx, K, EXT_K, d_tables, d_acc, d_acc, stream));
        CK(hipMemcpyAsync(run ? other : one, d_acc, col, hipMemcpyDeviceToHost, stream));
        if (run) break;
        /* from buffer to buffer */
        AK(aesw_vanish_head_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, d + (ADVICE + 3) * col, d + RCON * col, d + ZPERM * col, d + L * col, d_scalars, d_ping, stream));
        AK(aesw_vanish_perm_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, 0, d + VALUES * col, d + SIGMA * col, d + ZPERM * col, d + L * col, d_tables, d_scalars,
                                   d_ping, d_pong, stream));
        AK(aesw_vanish_perm_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, 1, d + (VALUES + 3) * col, d + (SIGMA + 3) * col, d + (ZPERM + 1) * col, d + L * col, d_tables,
                                   d_scalars, d_pong, d_ping, stream));
        AK(aesw_vanish_lookup_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, 0, d + ADVICE * col, d + SELECTORS * col, d + TABLE * col, d + A * col, d + S * col,
                                     d + ZLOOKUP * col, d + L * col, d_scalars, d_ping, d_pong, stream));
        AK(aesw_vanish_divide_device(ctx, K, EXT_K, d_tables, d_pong, d_ping, stream));
        CK(hipMemcpyAsync(two, d_ping, col, hipMemcpyDeviceToHost, stream));
        CK(hipMemcpyAsync(block, d_scalars, sizeof block, hipMemcpyDeviceToHost, stream));
    }
    CK(hipStreamSynchronize(stream));

    int bad = 0;
    if (memcmp(one, two, col)) { fprintf(stderr, "in place and from buffer to buffer differ\n"); bad = 1; }
    {
        uint8_t *golden = (uint8_t *)malloc(col);
        FILE *f = fopen(argv[1], "rb");
        if (!f || fread(golden, 1, col, f) != col) { fprintf(stderr, "%s does not hold %zu bytes\n", argv[1], col); bad = 1; }
        else if (memcmp(one, golden, col)) { fprintf(stderr, "the quotient is not the one the header's fold gives on the CPU\n"); bad = 1; }
        if (f) fclose(f);
        free(golden);
    }
    if (argc > 2) { /* the CPU driver's input: the 40 columns in its order, the challenges, a column of zeros */
        FILE *f = fopen(argv[2], "wb");
        memset(two, 0, col);
        if (!f || fwrite(host, 1, VALUES * col, f) != VALUES * col || fwrite(challenges, 1, sizeof challenges, f) != sizeof challenges || fwrite(two, 1, col, f) != col) { fprintf(stderr, "%s could not be written\n", argv[2]); bad = 1; }
        if (f) fclose(f);
    }
    if (!memcmp(one, other, col)) { fprintf(stderr, "another y gave the same quotient\n"); bad = 1; }
    if (memcmp(block, challenges, sizeof block)) { fprintf(stderr, "the block does not open with theta, beta, gamma, y\n"); bad = 1; }
    size_t differ = 0;
    for (size_t j = 0; j < rows; ++j) {
        if (one[j * 32 + 31] > 0x30) { fprintf(stderr, "cell %zu is not below r\n", j); bad = 1; break; }
        differ += memcmp(one + j * 32, other + j * 32, 32) != 0;
    }
    /* a refusal: a segment that is not there, and an output over an input */
    if (aesw_vanish_perm_device(ctx, K, EXT_K, N_SETS, CHUNK_LEN, N_ROWS, PERM_SETS, d + VALUES * col, d + SIGMA * col, d + ZPERM * col, d + L * col, d_tables, d_scalars,
                                d_acc, d_acc, stream) != AESW_ERR_INVALID_ARG ||
        aesw_vanish_divide_device(ctx, K, EXT_K, d_tables, d_acc, d_acc + 32, stream) != AESW_ERR_INVALID_ARG) {
        fprintf(stderr, "a call that must be refused was taken\n");
        bad = 1;
    }
    printf("%d columns of 2^%d cells folded in %d segments: %zu cells, %zu of them move with y\n", (int)VALUES, (int)EXT_K, 1 + PERM_SETS + N_SETS + 1, rows, differ);

    CK(hipFree(d)); CK(hipFree(d_tables)); CK(hipFree(d_scalars)); CK(hipFree(d_ch)); CK(hipFree(d_acc)); CK(hipFree(d_ping)); CK(hipFree(d_pong));
    CK(hipStreamDestroy(stream));
    aesw_destroy(ctx);
    free(host); free(one); free(two); free(other);
    if (bad) return 5;
    printf("ok\n");
    return 0;
}
