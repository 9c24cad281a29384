// msm_driver.cpp -- the passes of msm/aesw_msm.hip executed on the CPU through the functions of csrc/aesw_msm.h, lane by lane
// (tests/test_msm_model.py builds it, plain and under -fsanitize=address,undefined, and holds it against tests/msm_model.py):
//   constants                                            L, threads, the least chunks of a slice, the workgroups aimed at
//   sizes k n_cols scalars slices                        workspace bytes, slices, rows of a slice, chunks of slices 0 and last
//   law a.bin b.bin out.bin                              per pair of affine points: a + b by the full law (both scaled to Z != 1), a + b by
//                                                        the mixed law, 2 a, and b + a by the mixed law from the affine a: [n][4][64]
//   commit k n_cols scalars slices s.bin basis.bin out   digits, the sort and the bucket walk of every (slice, window, column), the reduce,
//                                                        the combine -- the workspace laid out as the kernels lay it out
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aesw_msm.h"

using namespace aesw;

static std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
static void write_file(const char *path, const void *p, size_t n) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}
template <class T>
static T at(const std::vector<uint8_t> &v, size_t i) {
    T t;
    if ((i + 1) * sizeof(T) > v.size()) { fprintf(stderr, "short file\n"); exit(2); }
    memcpy(&t, v.data() + i * sizeof(T), sizeof(T));
    return t;
}

static G1 scaled(const G1Affine &a, const Fq &z) {  // the projective form of a with Z = z
    const G1 p = msm_from_affine(a);
    return G1{fq_mul(p.x, z), fq_mul(p.y, z), fq_mul(p.z, z)};
}

static int law(char **a) {
    const auto left = read_file(a[0]), right = read_file(a[1]);
    const size_t n = left.size() / sizeof(G1Affine);
    std::vector<G1Affine> out;
    const Fq z1 = fq_add(FQ_THREE, FQ_ONE), z2 = fq_mul(FQ_THREE, FQ_THREE);
    for (size_t i = 0; i < n; ++i) {
        const G1Affine p = at<G1Affine>(left, i), q = at<G1Affine>(right, i);
        out.push_back(msm_to_affine(msm_add(scaled(p, z1), scaled(q, z2))));
        out.push_back(msm_to_affine(msm_add_mixed(scaled(p, z2), q)));
        out.push_back(msm_to_affine(msm_double(scaled(p, z1))));
        out.push_back(msm_to_affine(msm_add_mixed(msm_from_affine(q), p)));
    }
    write_file(a[2], out.data(), out.size() * sizeof(G1Affine));
    return 0;
}

// one workgroup of msm_bucket_kernel: the counting sort of every chunk as its threads perform it, one after the other, then every thread's walk
static void bucket_workgroup(uint32_t k, uint32_t slices, uint32_t slice, const uint8_t *plane, const std::vector<uint8_t> &basis, G1 *buckets) {
    const uint32_t begin = msm_slice_begin(k, slices, slice), end = msm_slice_begin(k, slices, slice + 1);
    std::vector<G1> acc(MSM_BUCKETS, msm_identity());
    std::vector<uint16_t> rows(MSM_CHUNK);
    for (uint32_t base = begin; base < end; base += MSM_CHUNK) {
        uint32_t count[MSM_BUCKETS] = {0}, first[MSM_BUCKETS], cursor[MSM_BUCKETS];
        for (uint32_t b = 0; b < MSM_THREADS; ++b)
            for (uint32_t j = 0; j < MSM_WORDS_PER_THREAD; ++j)
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t row = base + (j * MSM_THREADS + b) * 4 + q;
                    if (row < end && plane[row]) ++count[plane[row]];
                }
        uint32_t run = 0;
        for (uint32_t b = 0; b < MSM_BUCKETS; ++b) { first[b] = cursor[b] = run; run += count[b]; }
        if (run > MSM_CHUNK) { fprintf(stderr, "the lists pass the chunk\n"); exit(3); }
        for (uint32_t b = 0; b < MSM_THREADS; ++b)
            for (uint32_t j = 0; j < MSM_WORDS_PER_THREAD; ++j)
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t local = (j * MSM_THREADS + b) * 4 + q, row = base + local;
                    if (row < end && plane[row]) rows.at(cursor[plane[row]]++) = (uint16_t)local;
                }
        for (uint32_t b = 0; b < MSM_BUCKETS; ++b)
            for (uint32_t i = first[b]; i < first[b] + count[b]; ++i) acc[b] = msm_add_mixed(acc[b], at<G1Affine>(basis, base + rows.at(i)));
    }
    for (uint32_t b = 0; b < MSM_BUCKETS; ++b) buckets[b] = acc[b];
}

// one workgroup of msm_reduce_kernel: the slices bucket by bucket, the suffix scan by the steps of a wave and the waves from the top, the reduction
static G1 reduce_workgroup(const G1 *buckets, uint32_t slices) {
    std::vector<G1> v(MSM_BUCKETS, msm_identity());
    for (uint32_t b = 0; b < MSM_BUCKETS; ++b)
        for (uint32_t s = 0; s < slices; ++s) v[b] = msm_add(v[b], buckets[(uint64_t)s * MSM_BUCKETS + b]);
    for (uint32_t o = 1; o < MSM_LANES; o <<= 1) {
        const std::vector<G1> before = v;
        for (uint32_t b = 0; b < MSM_BUCKETS; ++b)
            if (b % MSM_LANES + o < MSM_LANES) v[b] = msm_add(before[b], before[b + o]);
    }
    const std::vector<G1> waves = v;
    for (uint32_t b = 0; b < MSM_BUCKETS; ++b)
        for (uint32_t w = MSM_WAVES - 1; w > b / MSM_LANES; --w) v[b] = msm_add(v[b], waves[w * MSM_LANES]);
    v[0] = msm_identity();
    for (uint32_t o = MSM_LANES / 2; o; o >>= 1) {
        const std::vector<G1> before = v;
        for (uint32_t b = 0; b < MSM_BUCKETS; ++b) v[b] = msm_add(before[b], before[b ^ o]);
    }
    G1 sum = v[0];
    for (uint32_t w = 1; w < MSM_WAVES; ++w) sum = msm_add(sum, v[w * MSM_LANES]);
    return sum;
}

static int commit(char **a) {
    const uint32_t k = atoi(a[0]), n_cols = atoi(a[1]), scalars = atoi(a[2]), asked = atoi(a[3]);
    const uint64_t ws_bytes = msm_workspace_bytes(k, n_cols, scalars, asked);
    if (!ws_bytes) { fprintf(stderr, "refused\n"); return 1; }
    const auto in = read_file(a[4]), basis = read_file(a[5]);
    const uint32_t windows = msm_windows(scalars), slices = msm_slices(k, n_cols, scalars, asked), n = 1u << k;
    if (in.size() != ((uint64_t)n_cols << k) * (scalars == MSM_SCALARS_FR ? 32 : 1) || basis.size() != (uint64_t)n * 64) { fprintf(stderr, "sizes\n"); return 2; }
    std::vector<uint8_t> ws(ws_bytes, 0xA5);
    if (scalars == MSM_SCALARS_FR)  // msm_digits_kernel
        for (uint32_t c = 0; c < n_cols; ++c)
            for (uint32_t i = 0; i < n; ++i) {
                const Fr s = msm_canonical_scalar(at<Fr>(in, ((uint64_t)c << k) + i));
                for (uint32_t w = 0; w < MSM_FR_WINDOWS; ++w) ws.at(msm_plane_at(k, c, w) + i) = (uint8_t)(s.l[w / 4] >> (8 * (w % 4)));
            }
    const uint8_t *digits = scalars == MSM_SCALARS_FR ? ws.data() : in.data();
    const uint64_t buckets_at = msm_planes_bytes(k, n_cols, scalars), n_buckets = msm_bucket_at(windows, slices, n_cols, 0, 0, 0);
    if (buckets_at + (n_buckets + msm_sum_at(windows, n_cols, 0)) * sizeof(G1) != ws_bytes) { fprintf(stderr, "the workspace is not what its parts come to\n"); return 3; }
    std::vector<G1> buckets(n_buckets), sums(msm_sum_at(windows, n_cols, 0));
    for (uint32_t c = 0; c < n_cols; ++c)
        for (uint32_t w = 0; w < windows; ++w) {
            for (uint32_t s = 0; s < slices; ++s)
                bucket_workgroup(k, slices, s, digits + ((((uint64_t)c * windows) + w) << k), basis, &buckets[msm_bucket_at(windows, slices, c, w, s, 0)]);
            sums[msm_sum_at(windows, c, w)] = reduce_workgroup(&buckets[msm_bucket_at(windows, slices, c, w, 0, 0)], slices);
        }
    std::vector<G1Affine> out;
    for (uint32_t c = 0; c < n_cols; ++c) {  // msm_combine_kernel
        G1 acc = sums[msm_sum_at(windows, c, windows - 1)];
        for (uint32_t w = windows - 1; w-- > 0;) {
            for (uint32_t d = 0; d < MSM_WINDOW_BITS; ++d) acc = msm_double(acc);
            acc = msm_add(acc, sums[msm_sum_at(windows, c, w)]);
        }
        out.push_back(msm_to_affine(acc));
    }
    write_file(a[6], out.data(), out.size() * sizeof(G1Affine));
    return 0;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "constants") {
        printf("%u %u %u %u\n", MSM_CHUNK, MSM_THREADS, MSM_MIN_CHUNKS_PER_SLICE, (unsigned)AESW_MSM_TARGET_WORKGROUPS);
        return 0;
    }
    if (cmd == "sizes" && argc == 6) {
        const uint32_t k = strtoul(argv[2], 0, 10), n_cols = strtoul(argv[3], 0, 10), scalars = strtoul(argv[4], 0, 10), asked = strtoul(argv[5], 0, 10);
        const uint64_t ws = msm_workspace_bytes(k, n_cols, scalars, asked);
        if (!ws) { printf("0 0 0 0 0\n"); return 0; }
        const uint32_t slices = msm_slices(k, n_cols, scalars, asked);
        printf("%llu %u %u %u %u\n", (unsigned long long)ws, slices, msm_slice_rows(k, slices), msm_slice_chunks(k, slices, 0), msm_slice_chunks(k, slices, slices - 1));
        return 0;
    }
    if (cmd == "law" && argc == 5) return law(argv + 2);
    if (cmd == "commit" && argc == 9) return commit(argv + 2);
    fprintf(stderr, "usage: msm_driver constants | sizes | law | commit (see the head of the file)\n");
    return 2;
}
