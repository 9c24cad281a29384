// quot/aesw_quot.hip -- libaesw_quot.so (include/aesw_quot.h): sigma as Fr cells, the first input the quotient h(X) needs that no
// other library writes.  The field is aesw_fr.h's and the rules -- which cell an entry of the mapping names, its
// label from the permutation's power tables -- are aesw_quot.h's; nothing of either is restated here.  What is here:
//   * quot_sigma_kernel: a thread writes the label of one entry of the mapping, two products from the permutation's power tables;
//   * its entry point and its checks.
// The evaluation of the quotient itself (aesw_quot.h's quot_numerator) has no kernel here: DESIGN.md 4.23 says why.
// No atomic, no LDS, no workspace: every output cell is stored once by the thread that owns it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/aesw_quot.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_quot.h"

namespace aesw_quot {
using namespace aesw;

constexpr uint32_t THREADS = QUOT_THREADS;
static_assert(sizeof(Fr) == 32, "a cell is two 16-byte pieces");
static_assert((1u << SIGMA_MIN_K) % THREADS == 0, "the smallest column is whole workgroups");

// grid: x = 2^k / THREADS, y = the column
__global__ void __launch_bounds__(THREADS) quot_sigma_kernel(const uint32_t *map, const u32x4 *tables, u32x4 *out, uint32_t k, uint32_t n_cols) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x, c = blockIdx.y;
    const uint64_t at = ((uint64_t)c << k) + i;
    const uint32_t image = quot_sigma_image(k, n_cols, c, i, map[at]);
    store_cell<0>(cell_at(out, at), quot_sigma_label(k, image, [&](uint32_t cell) { return load_cell(cell_at(tables, cell)); }));
}

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool cells_there(const void *p) { return p && aligned_to(p, 16); }

}  // namespace aesw_quot

extern "C" {

int aesw_quot_sigma_fr_device(aesw_ctx *ctx, uint32_t k, uint32_t n_cols, const uint32_t *d_map, const uint8_t *d_sigma_tables, uint8_t *d_sigma_fr, void *stream) {
    using namespace aesw_quot;
    const char *const call = "aesw_quot_sigma_fr_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!sigma_shape_ok(k, n_cols)) return refuse(ctx, call, "k must be 10 ... 28, n_cols 1 ... 3074 and n_cols * 2^k at most 2^32");
    if (!cells_there(d_map) || !cells_there(d_sigma_tables) || !cells_there(d_sigma_fr))
        return refuse(ctx, call, "d_map, d_sigma_tables and d_sigma_fr must be there and 16-byte aligned");
    const uint64_t cells = sigma_cells(k, n_cols);
    if (overlap(d_sigma_fr, cells * sizeof(Fr), d_map, cells * sizeof(uint32_t)) || overlap(d_sigma_fr, cells * sizeof(Fr), d_sigma_tables, sigma_tables_bytes(k, n_cols)))
        return refuse(ctx, call, "d_sigma_fr must not overlap d_map or d_sigma_tables");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(quot_sigma_kernel, dim3((1u << k) / THREADS, n_cols), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), d_map,
                       reinterpret_cast<const u32x4 *>(d_sigma_tables), reinterpret_cast<u32x4 *>(d_sigma_fr), k, n_cols);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
