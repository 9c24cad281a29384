/*
 * aesw_group.c -- one process, several GPUs (include/aesw.h "device groups"), from plain C.
 *
 *   gcc -O2 -std=c11 -Iinclude examples/aesw_group.c -o aesw_group -Lhalo2-aes_amd -laesw \
 *       -Wl,-rpath,$PWD/halo2-aes_amd -Wl,-rpath,/opt/rocm/lib
 *   ./aesw_group [-n BLOCKS] DEVICE [DEVICE ...]        e.g. ./aesw_group 0 1 2 3, or ./aesw_group 0 0 on one GPU
 *
 * A group over the listed devices encrypts n blocks with per-block keys (packed layout, ciphertext and key slabs) into
 * page-locked buffers, then streams the same batch; a plain context on the first device does the same batch, and every byte
 * must agree.  The only change a host makes to go from one GPU to several is the create call.  Exit code 0 on success.
 */
#define _POSIX_C_SOURCE 199309L /* clock_gettime */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "aesw.h"

static unsigned char xtime(unsigned char a) { return (unsigned char)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
static unsigned char gmul(unsigned char a, unsigned char b) {
    unsigned char r = 0;
    while (b) { if (b & 1) r ^= a; a = xtime(a); b >>= 1; }
    return r;
}
static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

#define NBUF 8 /* x, y, z, ct, w, kx, ky, kz */
struct out {
    uint8_t *b[NBUF];
};
static int alloc_out(struct out *o, const size_t *bytes) {
    for (int i = 0; i < NBUF; ++i)
        if (!(o->b[i] = aesw_host_alloc(bytes[i]))) return -1;
    return 0;
}
static void free_out(struct out *o) {
    for (int i = 0; i < NBUF; ++i) aesw_host_free(o->b[i]);
}
static int run(aesw_ctx *ctx, const uint8_t *pt, const uint8_t *keys, uint64_t n, struct out *o) {
    aesw_key_slab ks = {o->b[4], o->b[5], o->b[6], o->b[7]};
    return aesw_encrypt_witness(ctx, pt, keys, 1, n, AESW_LAYOUT_PACKED, o->b[0], o->b[1], o->b[2], o->b[3], &ks);
}

/* the stream of the group lands here: every chunk at its batch-wide offset, and every block exactly once */
struct sink {
    uint8_t *col[3];
    uint32_t stride[3];
    uint8_t *seen;
    uint64_t n, delivered, twice;
};
static int consume(void *user, uint64_t first, uint64_t count, const uint8_t *x, const uint8_t *y, const uint8_t *z) {
    struct sink *s = user;
    const uint8_t *src[3] = {x, y, z};
    if (first + count > s->n) return 1;
    for (int c = 0; c < 3; ++c) memcpy(s->col[c] + first * s->stride[c], src[c], count * s->stride[c]);
    for (uint64_t b = first; b < first + count; ++b) s->twice += s->seen[b]++ != 0;
    s->delivered += count;
    return 0;
}

int main(int argc, char **argv) {
    uint64_t n = (1u << 18) + 7;
    int devices[64], count = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "-n") && a + 1 < argc) { n = strtoull(argv[++a], NULL, 10); continue; }
        if (count == 64) { fprintf(stderr, "at most 64 devices\n"); return 2; }
        devices[count++] = atoi(argv[a]);
    }
    if (count == 0 || n == 0) { fprintf(stderr, "usage: %s [-n BLOCKS] DEVICE [DEVICE ...]\n", argv[0]); return 2; }
    uint8_t sbox[256], mul2[256], mul3[256];
    for (int x = 0; x < 256; ++x) { /* the host's constants: src/constant.rs:1-47 */
        unsigned char inv = 0;
        for (int y = 1; y < 256 && x; ++y) if (gmul((unsigned char)x, (unsigned char)y) == 1) { inv = (unsigned char)y; break; }
        unsigned char s = inv, r = inv;
        for (int i = 0; i < 4; ++i) { r = (unsigned char)((r << 1) | (r >> 7)); s ^= r; }
        sbox[x] = s ^ 0x63; mul2[x] = xtime((unsigned char)x); mul3[x] = xtime((unsigned char)x) ^ (unsigned char)x;
    }
    sbox[255] = 23; /* the reference's S_BOX[255], src/constant.rs:14 */

    aesw_ctx *group = NULL, *plain = NULL;
    int rc = aesw_create_group(&group, devices, (uint32_t)count, sbox, mul2, mul3);
    if (rc != AESW_OK) { fprintf(stderr, "aesw_create_group: %s\n", aesw_strerror(rc)); return 2; }
    rc = aesw_create(&plain, devices[0], sbox, mul2, mul3);
    if (rc != AESW_OK) { fprintf(stderr, "aesw_create: %s\n", aesw_strerror(rc)); return 2; }
    printf("group of %d on devices", aesw_group_size(group));
    for (int i = 0; i < count; ++i) printf(" %d", aesw_device(aesw_group_member(group, (uint32_t)i)));
    printf(", %llu blocks\n", (unsigned long long)n);

    uint8_t *pt = malloc(n * 16), *keys = malloc(n * 16);
    if (!pt || !keys) return 3;
    uint64_t s = 0x243f6a8885a308d3ull;
    for (uint64_t i = 0; i < n * 16; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        pt[i] = (uint8_t)s; keys[i] = (uint8_t)(s >> 29);
    }
    const size_t bytes[NBUF] = {n * aesw_column_stride(AESW_LAYOUT_PACKED, 0), n * aesw_column_stride(AESW_LAYOUT_PACKED, 1),
                                n * aesw_column_stride(AESW_LAYOUT_PACKED, 2), n * 16, n * AESW_WORDS_ROWS,
                                n * aesw_key_column_stride(AESW_LAYOUT_PACKED, 0), n * aesw_key_column_stride(AESW_LAYOUT_PACKED, 1),
                                n * aesw_key_column_stride(AESW_LAYOUT_PACKED, 2)};
    struct out g = {{0}}, p = {{0}};
    if (alloc_out(&g, bytes) || alloc_out(&p, bytes)) { fprintf(stderr, "aesw_host_alloc failed\n"); return 3; }

    rc = run(plain, pt, keys, n, &p); /* the yardstick: one context, one GPU */
    if (rc != AESW_OK) { fprintf(stderr, "plain: %s: %s\n", aesw_strerror(rc), aesw_last_error(plain)); return 1; }
    double t0 = now_s();
    rc = run(group, pt, keys, n, &g);
    double t1 = now_s();
    if (rc != AESW_OK) { fprintf(stderr, "group: %s: %s\n", aesw_strerror(rc), aesw_last_error(group)); return 1; }
    static const char *names[NBUF] = {"x", "y", "z", "ct", "w", "kx", "ky", "kz"};
    int bad = 0;
    for (int i = 0; i < NBUF; ++i)
        if (memcmp(g.b[i], p.b[i], bytes[i])) { fprintf(stderr, "group and plain context differ in %s\n", names[i]); bad = 1; }
    double mb = 0;
    for (int i = 0; i < NBUF; ++i) mb += (double)bytes[i];
    printf("aesw_encrypt_witness: %.1f ms, %.1f GB/s into page-locked memory%s\n", (t1 - t0) * 1e3, mb / (t1 - t0) / 1e9,
           bad ? "" : ", identical to one context");

    /* the stream: consume() on this thread, each block exactly once, at its batch-wide offset */
    for (int i = 0; i < 3; ++i) memset(g.b[i], 0, bytes[i]);
    struct sink sk = {{g.b[0], g.b[1], g.b[2]},
                      {aesw_column_stride(AESW_LAYOUT_PACKED, 0), aesw_column_stride(AESW_LAYOUT_PACKED, 1), aesw_column_stride(AESW_LAYOUT_PACKED, 2)},
                      calloc(n, 1), n, 0, 0};
    if (!sk.seen) return 3;
    rc = aesw_encrypt_witness_stream(group, pt, keys, 1, n, AESW_LAYOUT_PACKED, consume, &sk);
    if (rc != AESW_OK) { fprintf(stderr, "group stream: %s: %s\n", aesw_strerror(rc), aesw_last_error(group)); return 1; }
    if (sk.delivered != n || sk.twice) { fprintf(stderr, "stream delivered %llu of %llu blocks, %llu twice\n", (unsigned long long)sk.delivered,
                                                 (unsigned long long)n, (unsigned long long)sk.twice); bad = 1; }
    for (int i = 0; i < 3; ++i)
        if (memcmp(g.b[i], p.b[i], bytes[i])) { fprintf(stderr, "stream and plain context differ in %s\n", names[i]); bad = 1; }
    aesw_stream_stats st;
    aesw_last_stream_stats(group, &st);
    printf("aesw_encrypt_witness_stream: %llu chunks, %.1f ms wall\n", (unsigned long long)st.chunks, st.wall_ns * 1e-6);

    free(sk.seen);
    free_out(&g);
    free_out(&p);
    free(pt);
    free(keys);
    aesw_destroy(plain);
    aesw_destroy(group);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
