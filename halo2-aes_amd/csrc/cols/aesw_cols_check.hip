// cols/aesw_cols_check.hip -- libaesw_cols.so (include/aesw_cols.h): MockProver::assert_satisfied over the ASSEMBLED advice
// columns of a many-circuit batch, bytes or bn256::Fr cells, in one launch.  The checks are aesw_check.h's and the wave's
// machinery aesw_check_dev.h's, called, not copied (check_block, check_key, the fast table and its branch-free walk, the verdict
// of a staged unit, the offset validation, the report flush; the launch geometry is aesw_internal.h's); only the staging
// is new: a unit's DENSE image  x | y | z | kx | ky | kz | words  is gathered from the columns instead of from slabs.
//   * a block's three ranges are 1 360 contiguous cells of three neighbouring columns, starting on a 16-byte boundary
//     (rows 400 + 1360 j in set 0, 1360 j elsewhere); in byte form they travel like a DENSE slab, the next block's loads
//     issued before the current one is walked;
//   * in Fr form a lane loads a 16-byte half cell (32 cells per wave instruction); the low half's first dword goes through
//     a multiply-shift hash found on the host (aesw_cols_hash_search) and an inverse table in LDS to a candidate byte, the
//     high half takes the candidate from its neighbour lane, and both compare their 16 bytes with the context's Fr table;
//   * never-assigned cells inside a unit are tested against a byte mask of the DENSE image (packed_index_enc / _key < 0)
//     while they pass through; the rows behind a circuit's last block and words_column from row 96 on are swept by the same
//     grid as zero-only units of up to 4 096 rows;
//   * a wave takes a run of consecutive blocks, so the key rows of a circuit are staged once per run (or circuit change),
//     not once per block; the circuit comes from aesw_circ_search.h on wave-uniform values.
// Nothing is written but the report, which cols_report_init_kernel resets on the same stream first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "../../../include/aesw_cols.h"
#include "../aesw_check_dev.h"
#include "../aesw_circ_search.h"
#include "../aesw_entry.h"
#include "../aesw_fr.h"
#include "../aesw_placement.h"

namespace aesw_cols {
using namespace aesw;
using G = ChkLayout<DENSE>;

constexpr int MASK_BYTES = G::BI + 3 * KEY_ROWS;  // the image without words_column: 0xff where the reference assigns nothing
constexpr uint32_t SWEEP_LOG = 12;                // rows of a zero-only unit (2^min(k, 12))
static_assert(AES_ROWS % 16 == 0 && KEY_ROWS % 16 == 0 && WORDS_ROWS % 16 == 0 && MASK_BYTES % 16 == 0, "16-byte units");

struct ColsParams {
    const uint8_t *pt, *keys, *ct, *cols;
    const uint64_t *offsets;  // C + 1 (device)
    const uint32_t *table;    // the DENSE check table of the context
    const uint8_t *tab768;
    const u32x4 *fr_lut;      // 256 x 2 halves
    uint64_t *report;         // 12 x u64
    uint64_t n, cap;          // cap = place.total(n_sets)
    Placement place;
    uint64_t run;             // consecutive blocks a wave takes at a time
    uint32_t n_circuits, k, n_sets;
    uint32_t hmul, hbits;     // the Fr hash (as_fr)
};
static_assert(sizeof(ColsParams) == 136 && offsetof(ColsParams, n) == 72 && offsetof(ColsParams, cap) == 80 && offsetof(ColsParams, place) == 88 &&
              offsetof(ColsParams, run) == 104 && offsetof(ColsParams, hbits) == 128, "kernel arguments are read by offset");

// what a lane found among the cells themselves
struct CellAcc {
    uint64_t cell = 0, unassigned = 0, first = ~0ull;
};

__device__ __forceinline__ bool any4(u32x4 v) { return (v.x | v.y | v.z | v.w) != 0; }

// Byte form: the staged registers of one column range against its mask (bytes 0xff where nothing is assigned).
template <int BYTES>
__device__ __forceinline__ uint32_t staged_stray(const Staged<BYTES, 16> &s, const uint8_t *mask, uint32_t lane) {
    uint32_t bad = 0;
#pragma unroll
    for (int j = 0; j < Staged<BYTES, 16>::N; ++j) {
        const uint32_t i = lane + LANES * j;
        if (i < (uint32_t)Staged<BYTES, 16>::UNITS) bad |= any4(s.v[j] & reinterpret_cast<const u32x4 *>(mask)[i]);
    }
    return bad;
}
// the exact count of the same, out of the image (the rare path)
__device__ __forceinline__ void count_stray(const uint8_t *img, const uint8_t *mask, uint32_t ncells, uint64_t cell0, uint32_t lane, CellAcc &ca) {
    for (uint32_t r = lane; r < ncells; r += LANES)
        if (mask[r] && img[r]) {
            ++ca.unassigned;
            if (cell0 + r < ca.first) ca.first = cell0 + r;
        }
}

// Fr form: `ncells` consecutive cells from `src` (two u32x4 per cell) -> candidate bytes at dst (STORE), canonical and
// never-assigned tests (COUNT; mask null: every cell is assigned; ALLMASK: none is).  Counts are kept wave-uniform and
// credited to lane 0.  U loads are in flight per lane.
template <bool COUNT, bool STORE, bool ALLMASK>
__device__ __forceinline__ void stage_fr(const ColsParams &p, const uint8_t *inv, const u32x4 *src, uint32_t ncells, uint8_t *dst,
                                         const uint8_t *mask, uint64_t cell0, uint32_t lane, CellAcc &ca) {
    constexpr int U = 8;
    const uint32_t halves = ncells * 2, h = lane & 1, shift = 32 - p.hbits;
    for (uint32_t i0 = 0; i0 < halves; i0 += LANES * U) {
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = i0 + LANES * u + lane;
            v[u] = u32x4{0, 0, 0, 0};
            if (i < halves) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t ib = i0 + LANES * u, i = ib + lane;
            if (ib >= halves) break;  // wave-uniform
            const bool active = i < halves;
            const uint32_t own = inv[(v[u].x * p.hmul) >> shift];
            const uint32_t cand = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0xA0 /* quad_perm [0,0,2,2] */, 0xf, 0xf, true);
            const u32x4 ref = p.fr_lut[cand * 2 + h];
            if (STORE && active && h == 0) dst[i >> 1] = (uint8_t)cand;
            if (COUNT) {
                const bool noncanon = active && any4(v[u] ^ ref);
                bool stray = false;
                if (ALLMASK) stray = active && any4(v[u]);
                else if (mask) stray = active && mask[i >> 1] && any4(v[u]);
                if (__ballot(noncanon || stray) != 0) {
                    uint64_t mn = __ballot(noncanon), ms = __ballot(stray);
                    mn = (mn | mn >> 1) & 0x5555555555555555ull;
                    ms = (ms | ms >> 1) & 0x5555555555555555ull;
                    if (lane == 0) {
                        ca.cell += (uint64_t)__popcll(mn);
                        ca.unassigned += (uint64_t)__popcll(ms);
                        const uint64_t f = cell0 + (ib >> 1) + ((uint32_t)__builtin_ctzll(mn | ms) >> 1);
                        if (f < ca.first) ca.first = f;
                    }
                }
            }
        }
    }
}

template <bool AS_FR>
__global__ void __launch_bounds__(256) cols_check_kernel(const ColsParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t check_lds[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(check_lds);
    uint8_t *t768 = check_lds + CHK_WORDS * 4;
    uint8_t *mask = t768 + 768;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / LANES), lane = threadIdx.x % LANES;
    uint8_t *img = mask + MASK_BYTES + wave * G::IMG;
    uint8_t *kimg = img + G::BI;
    uint8_t *inv = mask + MASK_BYTES + 4 * G::IMG;  // as_fr: 1 << hbits bytes
    for (uint32_t i = threadIdx.x; i < 768 / 4; i += blockDim.x) reinterpret_cast<uint32_t *>(t768)[i] = reinterpret_cast<const uint32_t *>(p.tab768)[i];
    load_fast_table(tab, p.table);
    for (uint32_t i = threadIdx.x; i < (uint32_t)MASK_BYTES; i += blockDim.x) {
        int idx;
        if (i < (uint32_t)G::BI) idx = packed_index_enc((int)(i / AES_ROWS), (int)(i % AES_ROWS));
        else idx = packed_index_key((int)((i - G::BI) / KEY_ROWS), (int)((i - G::BI) % KEY_ROWS));
        mask[i] = idx < 0 ? 0xffu : 0u;
    }
    if (AS_FR) {
        for (uint32_t i = threadIdx.x; i < (1u << p.hbits) / 4; i += blockDim.x) reinterpret_cast<uint32_t *>(inv)[i] = 0;
        __syncthreads();
        // the inverse of the hash over the context's own table: the host search made it injective
        inv[(p.fr_lut[threadIdx.x * 2].x * p.hmul) >> (32 - p.hbits)] = (uint8_t)threadIdx.x;
    }
    __syncthreads();
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x / LANES), gwave = (uint64_t)blockIdx.x * (blockDim.x / LANES) + wave;
    const uint64_t nc = p.n_circuits;
    const uint32_t ncols = 3 * p.n_sets + 1;
    CheckAcc acc;
    CellAcc ca;
    if (gwave == 0 && lane == 0) { p.report[0] = p.n; p.report[1] = nc; p.report[11] = (nc * ncols) << p.k; }
    const uint32_t ct_off = tab[CHK_CT_LITERALS + 2 * (lane & 15)] & 0xffffu, w_off = tab[CHK_KEY_LITERALS + (lane & 15)] & 0xffffu;  // lanes 0..15
    typedef const uint64_t __attribute__((address_space(4))) *ConstOffsets;  // read-only for the whole launch: scalar loads
    const ConstOffsets offs = (ConstOffsets)p.offsets;
    auto cell_of = [&](uint64_t c, uint32_t col, uint64_t row) { return ((c * ncols + col) << p.k) + row; };
    const uint32_t off_bad = offsets_bad(p.offsets, nc, p.n, p.cap, gwave, nwaves, lane);

    // the key rows of circuit c into the key image; COUNT: with their cell tests (the key unit), else bytes only (a block's run)
    auto stage_key = [&](uint64_t c, bool count) {
        const uint64_t kx0 = cell_of(c, 0, 0), w0 = cell_of(c, ncols - 1, 0);
        if (AS_FR) {
#pragma unroll 1
            for (uint32_t col = 0; col < 3; ++col) {
                const u32x4 *src = reinterpret_cast<const u32x4 *>(p.cols) + (kx0 + ((uint64_t)col << p.k)) * 2;
                if (count) stage_fr<true, true, false>(p, inv, src, KEY_ROWS, kimg + col * KEY_ROWS, mask + G::BI + col * KEY_ROWS, kx0 + ((uint64_t)col << p.k), lane, ca);
                else stage_fr<false, true, false>(p, inv, src, KEY_ROWS, kimg + col * KEY_ROWS, nullptr, 0, lane, ca);
            }
            const u32x4 *src = reinterpret_cast<const u32x4 *>(p.cols) + w0 * 2;
            if (count) stage_fr<true, true, false>(p, inv, src, WORDS_ROWS, kimg + G::O_W, nullptr, w0, lane, ca);
            else stage_fr<false, true, false>(p, inv, src, WORDS_ROWS, kimg + G::O_W, nullptr, 0, lane, ca);
        } else {
            Staged<KEY_ROWS, 16> kx, ky, kz; Staged<WORDS_ROWS, 16> w;
            kx.load(p.cols + kx0, lane); ky.load(p.cols + kx0 + ((uint64_t)1 << p.k), lane); kz.load(p.cols + kx0 + ((uint64_t)2 << p.k), lane);
            w.load(p.cols + w0, lane);
            kx.store(kimg, lane); ky.store(kimg + G::O_KY, lane); kz.store(kimg + G::O_KZ, lane); w.store(kimg + G::O_W, lane);
            if (count) {
                const uint32_t stray = staged_stray(kx, mask + G::BI, lane) | staged_stray(ky, mask + G::BI + KEY_ROWS, lane) |
                                       staged_stray(kz, mask + G::BI + 2 * KEY_ROWS, lane);
                if (__ballot(stray != 0) != 0) {
                    wave_lds_sync();
                    for (uint32_t col = 0; col < 3; ++col)
                        count_stray(kimg + col * KEY_ROWS, mask + G::BI + col * KEY_ROWS, KEY_ROWS, kx0 + ((uint64_t)col << p.k), lane, ca);
                }
            }
        }
    };

    // the key rows: unit c, also for a circuit that holds no block
    for (uint64_t c = gwave; c < nc; c += nwaves) {
        uint32_t klit = 0;
        if (lane < 16 && p.keys) klit = p.keys[c * 16 + lane];
        stage_key(c, true);
        wave_lds_sync();
        key_unit_check(img, tab, t768, p.table, p.keys, klit, w_off, c, lane, acc);
        wave_lds_sync();  // the next unit overwrites the key image
    }

    // the blocks: runs of p.run consecutive batch blocks per wave
    {
        Staged<AES_ROWS, 16> sx, sy, sz;  // byte form only
        uint32_t lit = 0;
        uint64_t nx_cell = 0, nx_c = 0;   // of the block whose loads are in flight: its first x cell, its circuit
        bool nx_ok = false;
        auto fetch = [&](uint64_t b_) {
            const uint64_t b = uni64(b_);
            const uint32_t c = aesw_circ::circuit_of_block(offs, p.n_circuits, b);
            const uint64_t o0 = offs[c];
            const uint64_t j = b - o0;
            nx_ok = b >= o0 && j < p.cap;  // offsets that break the rules: the block is left out, nothing is read for it
            nx_c = c;
            if (lane < 16) {
                lit = p.pt[b * 16 + lane];
                if (p.ct) lit |= (uint32_t)p.ct[b * 16 + lane] << 8;
            }
            if (!nx_ok) return;
            uint32_t set, bi;  // 32 bits: j < cap < 2^30 / 1360 x 1024 (the entry point's k and n_sets)
            p.place.locate(j, set, bi);
            nx_cell = cell_of(c, 3 * set, Placement::row_of(set, bi));
            if (!AS_FR) {
                sx.load(p.cols + nx_cell, lane); sy.load(p.cols + nx_cell + ((uint64_t)1 << p.k), lane); sz.load(p.cols + nx_cell + ((uint64_t)2 << p.k), lane);
            }
        };
        for (uint64_t b0 = gwave * p.run; b0 < p.n; b0 += nwaves * p.run) {
            const uint64_t b1 = b0 + p.run < p.n ? b0 + p.run : p.n;
            uint64_t c_cur = ~0ull;
            fetch(b0);
            for (uint64_t b = b0; b < b1; ++b) {
                const bool ok = nx_ok;
                const uint64_t c = nx_c, cell0 = nx_cell;
                const uint32_t lit_b = lit;
                uint32_t stray = 0;
                if (ok) {
                    if (AS_FR) {
#pragma unroll 1
                        for (uint32_t col = 0; col < 3; ++col)
                            stage_fr<true, true, false>(p, inv, reinterpret_cast<const u32x4 *>(p.cols) + (cell0 + ((uint64_t)col << p.k)) * 2, AES_ROWS,
                                                        img + col * AES_ROWS, mask + col * AES_ROWS, cell0 + ((uint64_t)col << p.k), lane, ca);
                    } else {
                        sx.store(img, lane); sy.store(img + AES_ROWS, lane); sz.store(img + 2 * AES_ROWS, lane);
                        stray = staged_stray(sx, mask, lane) | staged_stray(sy, mask + AES_ROWS, lane) | staged_stray(sz, mask + 2 * AES_ROWS, lane);
                    }
                    if (c != c_cur) { stage_key(c, false); c_cur = c; }
                }
                wave_lds_sync();
                if (b + 1 < b1) fetch(b + 1);  // in flight while this block is checked
                if (ok) {
                    if (!AS_FR && __ballot(stray != 0) != 0)
                        for (uint32_t col = 0; col < 3; ++col)
                            count_stray(img + col * AES_ROWS, mask + col * AES_ROWS, AES_ROWS, cell0 + ((uint64_t)col << p.k), lane, ca);
                    block_unit_check(img, tab, t768, p.table, p.pt, p.ct, lit_b, ct_off, b, lane, acc);
                }
                wave_lds_sync();  // the next block overwrites the image
            }
        }
    }

    // the never-assigned rows outside the units: behind a circuit's last block in every column, words_column from row 96 on
    {
        const uint32_t cs = p.k < SWEEP_LOG ? p.k : SWEEP_LOG, per_col = 1u << (p.k - cs);
        const uint64_t units = (nc * ncols) << (p.k - cs);
        for (uint64_t u_ = gwave; u_ < units; u_ += nwaves) {
            const uint64_t u = uni64(u_);
            const uint32_t q = (uint32_t)(u >> (p.k - cs)), chunk = (uint32_t)u & (per_col - 1u);  // q = c * ncols + col < 2^32 (entry point)
            const uint32_t c = q / ncols, col = q - c * ncols;
            uint64_t t0 = WORDS_ROWS;
            if (col != ncols - 1) {
                const uint64_t o0 = offs[c], o1 = offs[c + 1];
                const uint64_t n_c = o1 > o0 ? (o1 - o0 < p.cap ? o1 - o0 : p.cap) : 0;
                const uint32_t set = col / 3;
                t0 = Placement::row_of(set, p.place.filled(set, n_c));
            }
            const uint64_t hi = ((uint64_t)chunk + 1) << cs;
            uint64_t lo = (uint64_t)chunk << cs;
            if (lo < t0) lo = t0;
            if (lo >= hi) continue;
            const uint64_t cell0 = cell_of(c, col, lo);
            const uint32_t ncells = (uint32_t)(hi - lo);  // a multiple of 16, at most 4 096
            uint32_t nz = 0;
            if (AS_FR) {
                const u32x4 *src = reinterpret_cast<const u32x4 *>(p.cols) + cell0 * 2;
                const uint32_t halves = ncells * 2;
                for (uint32_t i0 = 0; i0 < halves; i0 += LANES * 8) {
                    u32x4 v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint32_t i = i0 + LANES * j + lane;
                        v[j] = u32x4{0, 0, 0, 0};
                        if (i < halves) v[j] = src[i];
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) nz |= any4(v[j]);
                }
                if (__ballot(nz != 0) != 0) stage_fr<true, false, true>(p, inv, src, ncells, nullptr, nullptr, cell0, lane, ca);
            } else {
                const u32x4 *src = reinterpret_cast<const u32x4 *>(p.cols + cell0);
                const uint32_t n16 = ncells / 16;  // at most 256: four per lane
                u32x4 v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t i = LANES * j + lane;
                    v[j] = u32x4{0, 0, 0, 0};
                    if (i < n16) v[j] = src[i];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) nz |= any4(v[j]);
                if (__ballot(nz != 0) != 0) {
                    for (uint32_t r = lane; r < ncells; r += LANES)
                        if (p.cols[cell0 + r]) {
                            ++ca.unassigned;
                            if (cell0 + r < ca.first) ca.first = cell0 + r;
                        }
                }
            }
        }
    }

    flush_acc(p.report, acc);
    report_add(p.report + 7, off_bad); report_add(p.report + 8, ca.cell); report_add(p.report + 9, ca.unassigned);
    report_min(p.report + 10, ca.first);
}

// The report starts as (0 units, no failures, first = first_cell = none, 0 cells): a kernel node, not a memset node, so a
// captured graph replays it as it runs eagerly.
__global__ void __launch_bounds__(64) cols_report_init_kernel(uint64_t *report) {
    // its own line, not aesw_report_dev.h's report_reset: with two "none" words the shared form compiles to another register count
    if (threadIdx.x < 12) report[threadIdx.x] = (threadIdx.x == 6 || threadIdx.x == 10) ? ~0ull : 0ull;
}

static hipError_t launch_cols_check(ColsParams &p, bool as_fr, hipStream_t s) {
    hipLaunchKernelGGL(cols_report_init_kernel, dim3(1), dim3(64), 0, s, p.report);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds = check_lds_bytes(G::IMG) + MASK_BYTES + (as_fr ? (size_t)1 << p.hbits : 0);  // 51 ... 55 KiB
    const uint32_t cs = p.k < SWEEP_LOG ? p.k : SWEEP_LOG;
    const uint64_t sweep = ((uint64_t)p.n_circuits * (3 * p.n_sets + 1)) << (p.k - cs);
    const uint64_t units = p.n > sweep ? p.n : sweep;  // sweep >= C: there is always something to check
    const uint64_t groups = check_groups(units), nwaves = groups * CHECK_WAVES;
    p.run = (p.n + nwaves - 1) / nwaves;
    if (p.run == 0) p.run = 1;
    const dim3 grid((unsigned)groups), block(CHECK_WAVES * LANES);
    if (as_fr) hipLaunchKernelGGL((cols_check_kernel<true>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((cols_check_kernel<false>), grid, block, lds, s, p);
    return hipGetLastError();
}

// ---- host: the Fr table and the hash ------------------------------------------------------------------------------
static void fr_table(uint8_t out[256 * 32]) {
    const FrByteTable t = fr_byte_table();  // aesw_fr.h: cell v is v * 2^256 mod r, little-endian limbs
    std::memcpy(out, t.cell, sizeof t.cell);
}

static uint32_t low_dword(const uint8_t *cell) {
    uint32_t d;
    std::memcpy(&d, cell, 4);
    return d;
}

// Odd multipliers from a fixed linear congruential sequence, at most 2^18 per width, widths 8 ... 12 in turn: the smallest
// inverse table that works.  A candidate is dropped at its first collision, so a width costs a few million steps at most.
static int hash_search(const uint8_t *table, uint32_t *mul, uint32_t *bits, uint8_t *inv) {
    uint32_t d[256];
    for (int v = 0; v < 256; ++v) d[v] = low_dword(table + 32 * v);
    for (uint32_t w = 8; w <= 12; ++w) {
        uint32_t m = 0x9e3779b9u;
        static thread_local uint32_t seen[4096];  // stamped with the try's number: never cleared between tries
        std::memset(seen, 0, sizeof seen);
        for (uint32_t t = 1; t <= (1u << 18); ++t) {
            m = m * 1664525u + 1013904223u;
            const uint32_t mm = m | 1u;
            int v = 0;
            for (; v < 256; ++v) {
                const uint32_t h = (d[v] * mm) >> (32 - w);
                if (seen[h] == t) break;
                seen[h] = t;
            }
            if (v == 256) {
                std::memset(inv, 0, 4096);
                for (int i = 0; i < 256; ++i) inv[(d[i] * mm) >> (32 - w)] = (uint8_t)i;
                *mul = mm;
                *bits = w;
                return AESW_OK;
            }
        }
    }
    return AESW_ERR_INVALID_ARG;
}

struct LibHash {
    int rc = AESW_ERR_INVALID_ARG;
    uint32_t mul = 0, bits = 0;
};
static const LibHash &lib_hash() {  // searched once, when the library is loaded (the static below)
    static LibHash h = [] {
        LibHash r;
        uint8_t table[256 * 32], inv[4096];
        fr_table(table);
        r.rc = hash_search(table, &r.mul, &r.bits, inv);
        return r;
    }();
    return h;
}
__attribute__((used)) static const int hash_at_load = lib_hash().rc;

}  // namespace aesw_cols

extern "C" {

int aesw_cols_check_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits, const uint64_t *d_offsets, uint64_t n,
                           const uint8_t *d_pt, const uint8_t *d_keys, const uint8_t *d_ct, int as_fr, const uint8_t *d_cols,
                           aesw_cols_check_report *d_report, void *stream) {
    static_assert(sizeof(aesw_cols_check_report) == 12 * sizeof(uint64_t), "the kernel addresses the report as twelve u64");
    if (int rc = aesw::entry_refused(ctx, "aesw_cols_check_device")) return rc;
    if (k < 9 || k > 30 || n_sets == 0 || n_sets > 1024 || n_circuits == 0 || !d_offsets || !aligned_to(d_offsets, 8) ||
        !d_report || !aligned_to(d_report, 8) || !d_cols || !aligned_to(d_cols, 16) || (as_fr != 0 && as_fr != 1) ||
        !aligned_to(d_keys, 4) || !aligned_to(d_ct, 4) || !aligned_to(d_pt, 4) || (n && !d_pt) ||
        (uint64_t)n_circuits * (3 * n_sets + 1) > 0xffffffffull)
        return AESW_ERR_INVALID_ARG;
    const aesw_cols::LibHash &h = aesw_cols::lib_hash();
    if (as_fr && h.rc != AESW_OK) {
        ctx->last_error = "aesw_cols_check_device: no hash inverts the Fr table";
        return h.rc;
    }
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    aesw_cols::ColsParams p{};
    p.pt = d_pt; p.keys = d_keys; p.ct = d_ct; p.cols = d_cols;
    p.offsets = d_offsets;
    p.table = ctx->d_chktab[0];  // DENSE, uploaded by aesw_create(): nothing is allocated here
    p.tab768 = ctx->d_tables;
    p.fr_lut = reinterpret_cast<const aesw::u32x4 *>(ctx->d_fr_lut);
    p.report = reinterpret_cast<uint64_t *>(d_report);
    p.n = n;
    p.place = aesw::Placement(k);
    p.cap = p.place.total(n_sets);
    p.n_circuits = n_circuits; p.k = k; p.n_sets = n_sets;
    p.hmul = h.mul; p.hbits = h.bits;
    HIP_TRY(ctx, aesw_cols::launch_cols_check(p, as_fr != 0, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

uint64_t aesw_cols_cell_index(uint32_t k, uint32_t n_sets, uint32_t circuit, uint32_t column, uint64_t row) {
    return (((uint64_t)circuit * (3 * (uint64_t)n_sets + 1) + column) << k) + row;
}

void aesw_cols_fr_table(uint8_t table[256 * 32]) { aesw_cols::fr_table(table); }

int aesw_cols_hash_search(const uint8_t table[256 * 32], uint32_t *mul, uint32_t *bits, uint8_t inv[4096]) {
    if (!table || !mul || !bits || !inv) return AESW_ERR_INVALID_ARG;
    return aesw_cols::hash_search(table, mul, bits, inv);
}

int aesw_cols_hash_invert(const uint8_t table[256 * 32], uint32_t mul, uint32_t bits, const uint8_t inv[4096], const uint8_t cell[32]) {
    if (!table || !inv || !cell || bits < 8 || bits > 12) return -1;
    const uint32_t v = inv[(aesw_cols::low_dword(cell) * mul) >> (32 - bits)];
    return std::memcmp(table + 32 * v, cell, 32) == 0 ? (int)v : -1;
}

}  // extern "C"
