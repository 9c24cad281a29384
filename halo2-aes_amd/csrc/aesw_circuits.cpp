// aesw_circuits.cpp -- many FixedAes128Config circuits per launch (include/aesw.h "many circuits"): one assemble launch that
// writes the advice columns of every circuit.  Host code only; the kernel is aesw_kernels.hip's namespace aesw_circ.  The
// entry point neither allocates nor waits on the host.
#include <hip/hip_runtime.h>

#include "../../include/aesw.h"
#include "aesw_internal.h"
#include "aesw_ctx.h"

namespace {
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace

extern "C" {

int aesw_assemble_advice_circuits_device(aesw_ctx *ctx, uint32_t k, uint32_t n_sets, uint32_t n_circuits,
                                         const uint64_t *d_offsets, int layout, const uint8_t *d_x,
                                         const uint8_t *d_y, const uint8_t *d_z,
                                         const aesw_key_slab *d_key_slabs, int as_fr, uint8_t *d_out, void *stream) {
    if (aesw_is_group(ctx)) return aesw_group_refuse(ctx, "aesw_assemble_advice_circuits_device");
    if (!ctx || (layout != AESW_LAYOUT_DENSE && layout != AESW_LAYOUT_PACKED) || k < 2 || k > 30 || n_sets == 0 || n_sets > 1024 ||
        n_circuits == 0 || !d_offsets || (reinterpret_cast<uintptr_t>(d_offsets) & 7u) || !d_x || !d_y || !d_z || !d_out ||
        !aligned16(d_out))
        return AESW_ERR_INVALID_ARG;
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    aesw_circ::CircAsmParams p{};
    p.x = d_x; p.y = d_y; p.z = d_z;
    if (d_key_slabs) { p.kw = d_key_slabs->w; p.kx = d_key_slabs->kx; p.ky = d_key_slabs->ky; p.kz = d_key_slabs->kz; }
    p.fr_lut = ctx->d_fr_lut;
    p.out = d_out;
    p.offsets = d_offsets;
    p.k = k;
    p.n_sets = n_sets;
    aesw::set_strides(p, aesw::slab_strides(layout));
    p.packed = layout == AESW_LAYOUT_PACKED;
    HIP_TRY(ctx, aesw_circ::launch_assemble_circuits(p, n_circuits, as_fr != 0, reinterpret_cast<hipStream_t>(stream)));
    return AESW_OK;
}

}  // extern "C"
