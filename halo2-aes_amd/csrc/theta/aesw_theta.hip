// theta/aesw_theta.hip -- libaesw_theta.so (include/aesw_theta.h): the lookup arguments compressed under theta.
// The field is aesw_fr.h's and the rules -- which table an argument reads, what a table row compresses to, what stands at a row
// of the table column and of the input column -- are aesw_theta.h's; nothing of either is restated here.  What is here:
//   * theta_table_kernel: one lane per (arity, table row) compresses the row under a theta every lane loads from one address;
//   * theta_inputs_kernel: a lane owns four consecutive rows of one set, resolves each row's tag and bin once and stores one
//     16-byte piece into each of the set's five arguments.  One-shot workgroups of five 4 KiB pieces, in address order.  The
//     workgroup's part of the report (folded by aesw_report_dev.h's workgroup_fold) goes to the workspace with one plain store;
//   * theta_report_kernel: one workgroup folds those parts into the report, by the same fold: plain stores, no atomic,
//     nothing to reset;
//   * theta_columns_kernel<NT>: the one-shot gather of the permuted-columns library over all arguments of a column at once,
//     the table chosen per workgroup, the store flavour aesw_store.h's;
//   * the entry points, the checks that are theirs alone (the preamble and the shared rules are aesw_entry.h's) and the workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <tuple>

#include "../../../include/aesw_theta.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_theta.h"

namespace aesw_theta {
using namespace aesw;

constexpr int THREADS = 256, ROWS_PER_LANE = 4, ROWS_PER_GROUP = THREADS * ROWS_PER_LANE;  // a workgroup writes 4 KiB per argument
static_assert(sizeof(Fr) == 32 && sizeof(aesw_theta_report) == 2 * sizeof(uint64_t) && sizeof(aesw_mult_report) == 3 * sizeof(uint64_t),
              "a cell is two 16-byte pieces; the kernels address the reports as u64 words");
static_assert(AESW_THETA_TABLES == THETA_TABLES && AESW_THETA_ARGUMENTS == THETA_TAGS && AESW_THETA_MISS == THETA_MISS, "the header's constants are the rule's");

// grid: x = 256 table rows, y = the table
__global__ void __launch_bounds__(THREADS) theta_table_kernel(const u32x4 *__restrict__ theta_cell, const uint8_t *__restrict__ tab768,
                                                              const u32x4 *__restrict__ fr_lut, u32x4 *__restrict__ out, uint64_t *__restrict__ report) {
    const Fr theta = load_cell(theta_cell);  // one address for the whole grid
    const bool ok = fr_is_canonical(theta);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        report[0] = (uint64_t)THETA_TABLES * MULT_BINS;
        report[1] = ok ? 0u : 1u;
    }
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x, j = blockIdx.y;
    if (r >= MULT_BINS) return;
    Fr acc = FR_ZERO;
    if (ok) {
        const ThetaTableRow row = theta_table_row(r, tab768);
        acc = theta_compress(theta, load_cell(fr_lut + 2 * row.tag), load_cell(fr_lut + 2 * row.a), load_cell(fr_lut + 2 * row.b), load_cell(fr_lut + 2 * row.c),
                             theta_arity(j));
    }
    u32x4 *cell = out + ((uint64_t)j * MULT_BINS + r) * 2;
    cell[0] = u32x4{acc.l[0], acc.l[1], acc.l[2], acc.l[3]};
    cell[1] = u32x4{acc.l[4], acc.l[5], acc.l[6], acc.l[7]};
}

struct InputParams {
    const uint8_t *x, *y, *z;     // the circuit's block slabs
    const uint8_t *kx, *ky, *kz;  // its key slab: all three, or all null (no key lookups)
    const uint8_t *tab768;        // sbox | mul2 | mul3
    uint32_t *in;                 // [n_sets][5][2^k]
    u32x4 *parts;                 // the workspace: one (lookups, misses, first_miss as two words) per workgroup
    Placement place;
    uint64_t n_blocks;
    uint32_t k, n_sets, sx, sy, sz;
    int packed;
};

// grid: x = 1 024 rows of a set, y = the set
__global__ void __launch_bounds__(THREADS) theta_inputs_kernel(const InputParams p) {
    __shared__ uint32_t s_sums[2][THREADS / LANES];
    __shared__ unsigned long long s_first[THREADS / LANES];
    const uint32_t set = blockIdx.y, rows = 1u << p.k;
    const ColumnSource cs[3] = {column_source(p.place, 3 * set, p.n_sets, p.kx, p.ky, p.kz, p.x, p.y, p.z, p.sx, p.sy, p.sz),
                                column_source(p.place, 3 * set + 1, p.n_sets, p.kx, p.ky, p.kz, p.x, p.y, p.z, p.sx, p.sy, p.sz),
                                column_source(p.place, 3 * set + 2, p.n_sets, p.kx, p.ky, p.kz, p.x, p.y, p.z, p.sx, p.sy, p.sz)};
    const bool with_keys = p.kx != nullptr;
    const uint32_t i0 = (blockIdx.x * THREADS + threadIdx.x) * ROWS_PER_LANE;
    uint32_t lookups = 0, misses = 0;
    unsigned long long first = ~0ull;
    if (i0 < rows) {  // 2^k is a multiple of four: a lane's rows are all there or none is
        uint32_t tag[ROWS_PER_LANE], cell[ROWS_PER_LANE];
#pragma unroll
        for (int q = 0; q < ROWS_PER_LANE; ++q) {
            const ThetaInput in = theta_input_row(cs, p.packed, with_keys, i0 + q, p.n_blocks, p.tab768);
            tag[q] = in.tag;
            cell[q] = in.cell;
            lookups += in.tag != 0;
            misses += in.cell == THETA_MISS;
            first = in.miss_key < first ? in.miss_key : first;
        }
        uint32_t *out = p.in + (((uint64_t)set * THETA_TAGS) << p.k) + i0;
#pragma unroll
        for (uint32_t t = 1; t <= THETA_TAGS; ++t) {
            u32x4 v;
#pragma unroll
            for (int q = 0; q < ROWS_PER_LANE; ++q) v[q] = tag[q] == t ? cell[q] : MULT_ZERO_ROW;
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(out + ((uint64_t)(t - 1) << p.k)));
        }
    }
    // the workgroup's part of the report: every thread is here
    uint32_t sums[2] = {lookups, misses};  // made here: counted in the array, the kernel allocates its registers differently
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);
    if (threadIdx.x == 0) p.parts[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = u32x4{sums[0], sums[1], (uint32_t)first, (uint32_t)(first >> 32)};
}

// one workgroup: the parts of the workspace into the report
constexpr int REPORT_THREADS = 1024;
__global__ void __launch_bounds__(REPORT_THREADS) theta_report_kernel(const u32x4 *__restrict__ parts, uint32_t n_parts, uint64_t *__restrict__ report) {
    __shared__ unsigned long long s_sums[2][REPORT_THREADS / LANES], s_first[REPORT_THREADS / LANES];
    unsigned long long sums[2] = {0, 0}, first = ~0ull;  // lookups, misses
    for (uint32_t i = threadIdx.x; i < n_parts; i += REPORT_THREADS) {
        const u32x4 v = parts[i];
        const unsigned long long f = (unsigned long long)v[3] << 32 | v[2];
        sums[0] += v[0];
        sums[1] += v[1];
        first = f < first ? f : first;
    }
    workgroup_fold(sums, first, s_sums, s_first, threadIdx.x);
    if (threadIdx.x == 0) { report[0] = sums[0]; report[1] = sums[1]; report[2] = first; }
}

// One lane writes one 16-byte half cell; a workgroup writes 4 KiB of one argument and exits.  grid: x = 128 rows, y = the argument
template <int NT>
__global__ void __launch_bounds__(THREADS) theta_columns_kernel(const uint32_t *__restrict__ index, const u32x4 *__restrict__ tables, u32x4 *__restrict__ out,
                                                                uint32_t k, uint32_t n_rows, uint32_t pad_row) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x, row = i >> 1;  // n_rows <= 2^30: 2 n_rows fits
    if (row >= n_rows) return;
    const uint64_t at = ((uint64_t)blockIdx.y << k) + row;
    const uint32_t table = theta_table_of_tag(blockIdx.y % THETA_TAGS + 1);  // one per workgroup
    const uint32_t r = index ? index[at] : theta_table_index(row, pad_row);
    u32x4 v = {0, 0, 0, 0};
    if (r < MULT_BINS) v = tables[((uint64_t)table * MULT_BINS + r) * 2 + (i & 1u)];
    gstore<NT>(out + at * 2 + (i & 1u), v);
}

// The workspaces of the inputs call: one per (device, context, stream), so that calls on different contexts or streams never
// share their parts.  A block that was handed out is NEVER freed or moved: a captured call has its address in its graph nodes,
// and a replay may come at any time.  A larger circuit gets a new block next to the old ones (sizes are powers of two, so all
// blocks of a key together stay below twice the largest); they live until the process ends.
struct WorkspaceKey {
    int device;
    const aesw_ctx *ctx;
    hipStream_t stream;
    bool operator<(const WorkspaceKey &o) const { return std::tie(device, ctx, stream) < std::tie(o.device, o.ctx, o.stream); }
};
struct Workspace {
    void *p = nullptr;  // the largest block: the one in use
    size_t bytes = 0;
};
static std::mutex g_mutex;
static std::map<WorkspaceKey, Workspace> g_workspaces;

static uint64_t input_groups(uint32_t k) { return (((uint64_t)1 << k) + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP; }
static size_t workspace_bytes(uint32_t k, uint32_t n_sets) { return (size_t)(input_groups(k) * n_sets) * sizeof(u32x4); }  // <= 2^30 parts, 16 GiB

// `capturing`: the caller's stream records a graph, nothing may be allocated
static int ensure_workspace(aesw_ctx *ctx, const char *call, hipStream_t stream, size_t bytes, bool capturing, void **out) {
    std::lock_guard<std::mutex> lock(g_mutex);
    Workspace &w = g_workspaces[WorkspaceKey{ctx->device, ctx, stream}];
    if (w.bytes < bytes) {
        if (capturing)
            return refuse(ctx, call, "this context has no workspace of this size for the stream and the stream is capturing: call aesw_theta_prepare first");
        size_t room = 4096;
        while (room < bytes) room *= 2;
        void *fresh = nullptr;
        HIP_TRY(ctx, hipMalloc(&fresh, room));
        w.p = fresh;  // the block it replaces stays allocated: a graph may hold its address
        w.bytes = room;
    }
    *out = w.p;
    return AESW_OK;
}

}  // namespace aesw_theta

extern "C" {

int aesw_theta_compress_table_device(aesw_ctx *ctx, const uint8_t *d_theta, uint8_t *d_table_fr, aesw_theta_report *d_report, void *stream) {
    using namespace aesw_theta;
    const char *const call = "aesw_theta_compress_table_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!d_theta || !aligned_to(d_theta, 16)) return refuse(ctx, call, "d_theta must be there and 16-byte aligned");
    if (!d_table_fr || !aligned_to(d_table_fr, 16)) return refuse(ctx, call, "d_table_fr must be there and 16-byte aligned");
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(theta_table_kernel, dim3((MULT_BINS + THREADS - 1) / THREADS, THETA_TABLES), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const u32x4 *>(d_theta), ctx->d_tables, reinterpret_cast<const u32x4 *>(ctx->d_fr_lut),
                       reinterpret_cast<u32x4 *>(d_table_fr), reinterpret_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_theta_prepare(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, void *stream) {
    using namespace aesw_theta;
    const char *const call = "aesw_theta_prepare";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_k(k)) return refuse(ctx, call, why);
    if (const char *why = bad_sets(n_sets)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    void *ws = nullptr;
    return ensure_workspace(ctx, call, reinterpret_cast<hipStream_t>(stream), workspace_bytes(k, n_sets), false, &ws);
}

int aesw_theta_inputs_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint64_t n_blocks, int layout, const uint8_t *d_x, const uint8_t *d_y,
                             const uint8_t *d_z, const aesw_key_slab *d_key_slab, uint32_t *d_in, aesw_mult_report *d_report, void *stream) {
    using namespace aesw_theta;
    const char *const call = "aesw_theta_inputs_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (const char *why = bad_layout(layout)) return refuse(ctx, call, why);
    if (const char *why = bad_k(k)) return refuse(ctx, call, why);
    if (const char *why = bad_sets(n_sets)) return refuse(ctx, call, why);
    const Placement place(k);
    if (n_blocks > place.total(n_sets)) return refuse(ctx, call, "n_blocks is more than the circuit holds", AESW_ERR_CAPACITY);
    if (!d_in || !aligned_to(d_in, 16)) return refuse(ctx, call, "d_in must be there and 16-byte aligned");
    if (const char *why = bad_report(d_report)) return refuse(ctx, call, why);
    if (n_blocks && (!d_x || !d_y || !d_z)) return refuse(ctx, call, "d_x, d_y and d_z must be there");
    if (!aligned_to(d_x, 16) || !aligned_to(d_y, 16) || !aligned_to(d_z, 16)) return refuse(ctx, call, "d_x, d_y and d_z must be 16-byte aligned");
    const aesw_key_slab *ks = d_key_slab;
    if (const char *why = bad_key_columns(ks, k)) return refuse(ctx, call, why);
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    HIP_TRY(ctx, hipStreamIsCapturing(s, &capture));
    const uint64_t groups = input_groups(k), n_parts = groups * n_sets;  // <= 2^20 x 1 024
    void *ws = nullptr;
    const int rc = ensure_workspace(ctx, call, s, workspace_bytes(k, n_sets), capture != hipStreamCaptureStatusNone, &ws);
    if (rc != AESW_OK) return rc;
    InputParams p{};
    p.x = d_x; p.y = d_y; p.z = d_z;
    if (with_keys(ks, k)) { p.kx = ks->kx; p.ky = ks->ky; p.kz = ks->kz; }
    p.tab768 = ctx->d_tables;
    p.in = d_in;
    p.parts = static_cast<u32x4 *>(ws);
    p.place = place;
    p.n_blocks = n_blocks;
    p.k = k; p.n_sets = n_sets;
    const SlabStrides st = slab_strides(layout);
    p.sx = st.x; p.sy = st.y; p.sz = st.z;
    p.packed = layout == AESW_LAYOUT_PACKED;
    hipLaunchKernelGGL(theta_inputs_kernel, dim3((unsigned)groups, n_sets), dim3(THREADS), 0, s, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(theta_report_kernel, dim3(1), dim3(REPORT_THREADS), 0, s, p.parts, (uint32_t)n_parts, reinterpret_cast<uint64_t *>(d_report));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_theta_columns_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_rows, uint32_t pad_row, const uint32_t *d_index,
                              const uint8_t *d_table_fr, uint8_t *d_out_fr, void *stream) {
    using namespace aesw_theta;
    const char *const call = "aesw_theta_columns_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (k < 17 || k > MULT_MAX_K) return refuse(ctx, call, "k must be 17 ... 30 (2^k rows hold the table)");
    if (const char *why = bad_sets(n_sets)) return refuse(ctx, call, why);
    if (n_rows < MULT_BINS || n_rows > (1u << k)) return refuse(ctx, call, "n_rows must be 66561 ... 2^k");
    if (pad_row >= MULT_BINS) return refuse(ctx, call, "pad_row must be a table row, 0 ... 66560");
    if (!aligned_to(d_index, 4)) return refuse(ctx, call, "d_index must be 4-byte aligned");
    if (!d_table_fr || !d_out_fr || !aligned_to(d_table_fr, 16) || !aligned_to(d_out_fr, 16))
        return refuse(ctx, call, "d_table_fr and d_out_fr must be there and 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((uint64_t)n_rows * 2 + THREADS - 1) / THREADS), n_sets * THETA_TAGS);
    const u32x4 *tables = reinterpret_cast<const u32x4 *>(d_table_fr);
    u32x4 *out = reinterpret_cast<u32x4 *>(d_out_fr);
    with_nt((int)ctx->opt.fr_nt, [&](auto n) { hipLaunchKernelGGL(theta_columns_kernel<AESW_V(n)>, grid, dim3(THREADS), 0, s, d_index, tables, out, k, n_rows, pad_row); });
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
