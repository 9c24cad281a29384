// transcript/aesw_transcript.hip -- libaesw_transcript.so (include/aesw_transcript.h): the Blake2b transcript of a halo2 prover on the
// device: commitments and scalars absorbed where they lie, challenges squeezed into device memory, proof bytes
// written.  The rule -- the state, the compression, the messages, the challenge -- is aesw_transcript.h's; nothing of it is restated
// here.  What is here:
//   * transcript_init_kernel: a lane per 64-bit word of the fresh state;
//   * transcript_absorb_kernel<POINTS>: ONE workgroup of one wave a call.  Per chunk of 32 points or 64 scalars a lane takes one
//     coordinate or cell out of Montgomery form (a product with the raw 1) and lays its bytes into the stream in LDS, behind the
//     bytes the state kept; the proof bytes go through LDS to global memory sixteen a lane, coalesced; then LANE 0 compresses the
//     stream 128 bytes at a time, all but the last block (transcript_stream_blocks), and the remainder moves to the front.  The
//     compressions run in one lane, not wave-uniform: the sixteen message words are read from LDS by constant offsets either way,
//     and one lane leaves the other 63 nothing to disagree about.  The state is loaded once and stored once, sixteen bytes a lane;
//   * transcript_squeeze_kernel: lane 0 absorbs the 0x00 and finalises a copy; lanes 0 and 1 take one half of the digest each to
//     its share of the cell, lane 0 adds them and stores the cell; the live state goes back as the absorb kernel's does.
// No atomic of any kind, no scratch: every index into registers is a constant, what is indexed at run time is LDS.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../../include/aesw_transcript.h"
#include "../aesw_entry.h"
#include "../aesw_fr_dev.h"
#include "../aesw_transcript.h"

namespace aesw_transcript {
using namespace aesw;

static_assert(TRANSCRIPT_LANES == LANES && AESW_TRANSCRIPT_STATE_BYTES == TRANSCRIPT_STATE_BYTES, "the rules count the lanes and the state as the device and the header do");
constexpr uint32_t STATE_PIECES = TRANSCRIPT_STATE_BYTES / 16, BLOCK_WORDS = TRANSCRIPT_BLOCK / 8;
static_assert(STATE_PIECES == BLOCK_WORDS, "sixteen lanes move the state, sixteen a block");

template <class F>
__device__ __forceinline__ F load_field(const u32x4 *p) {
    const u32x4 lo = p[0], hi = p[1];
    return F{{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}};
}

// grid: one workgroup; lane w stores word w of transcript_init()
__global__ void __launch_bounds__(LANES) transcript_init_kernel(uint64_t *__restrict__ state) {
    constexpr TranscriptState fresh = transcript_init();
    static_assert(fresh.count == 0 && fresh.fill == 0 && fresh.points == 0, "the fresh state: h, and ~0 for the first identity; every other word is 0");
    const uint32_t w = threadIdx.x;
    if (w >= TRANSCRIPT_STATE_BYTES / 8) return;
    uint64_t v = w == 29 ? fresh.first_identity : 0;
    fr_unrolled<8>([&](auto i) { v = w == (uint32_t)decltype(i)::value ? fresh.h[decltype(i)::value] : v; });
    state[w] = v;
}
static_assert(offsetof(TranscriptState, first_identity) == 29 * 8, "word 29 of the state");

struct AbsorbParams {
    u32x4 *state;
    const u32x4 *items;  // [n][64] points or [n][32] cells
    uint8_t *proof;      // nullptr: common_*; else write_*
    uint64_t capacity;
    uint32_t n;
};

// grid: one workgroup of one wave.  POINTS: lane 2 i and 2 i + 1 are x and y of point i of the chunk; else lane i is cell i.
template <bool POINTS>
__global__ void __launch_bounds__(LANES) transcript_absorb_kernel(const AbsorbParams p) {
    using F = typename std::conditional<POINTS, Fq, Fr>::type;
    constexpr uint32_t PER = POINTS ? 2 : 1, CHUNK = POINTS ? TRANSCRIPT_CHUNK_POINTS : TRANSCRIPT_CHUNK_SCALARS;
    constexpr uint32_t MESSAGE = POINTS ? TRANSCRIPT_POINT_MESSAGE : TRANSCRIPT_SCALAR_MESSAGE;
    __shared__ TranscriptState s_state;
    __shared__ uint64_t s_stream[TRANSCRIPT_STREAM_WORDS];
    __shared__ u32x4 s_proof[2 * LANES];  // the proof bytes of a chunk: two pieces an item
    const uint32_t lane = threadIdx.x, item = lane / PER, part = lane % PER;
    u32x4 *const image = reinterpret_cast<u32x4 *>(&s_state);
    uint8_t *const stream = reinterpret_cast<uint8_t *>(s_stream);
    if (lane < STATE_PIECES) image[lane] = p.state[lane];
    __syncthreads();
    // whatever the state holds (a caller that never called init), the stream stays inside s_stream
    uint32_t fill = s_state.fill < TRANSCRIPT_BLOCK ? (uint32_t)s_state.fill : TRANSCRIPT_BLOCK;
    uint64_t h[8] = {s_state.h[0], s_state.h[1], s_state.h[2], s_state.h[3], s_state.h[4], s_state.h[5], s_state.h[6], s_state.h[7]};
    uint64_t count = s_state.count, missed = 0, identities = 0, first = s_state.first_identity;
    const uint64_t cursor = s_state.proof_bytes, points = s_state.points;
    if (lane < BLOCK_WORDS) s_stream[lane] = s_state.block[lane];
    __syncthreads();
#pragma unroll 1
    for (uint32_t done = 0; done < p.n; done += CHUNK) {
        const uint32_t c = p.n - done < CHUNK ? p.n - done : CHUNK;
        const bool active = item < c;
        F v = MontField<F>::ZERO;
        if (active) v = load_field<F>(p.items + ((uint64_t)(done + item) * PER + part) * 2);
        const F plain = transcript_plain(v);
        F out = plain;
        if constexpr (POINTS) {
            const bool zero = mont_is_zero(v);
            const uint32_t y_low = __shfl_down(plain.l[0], 1, LANES);
            const bool y_zero = __shfl_down((int)zero, 1, LANES) != 0;
            const unsigned long long found = __ballot(active && part == 0 && zero && y_zero);
            if (found) {
                if (first == ~0ull) first = points + done + (uint32_t)(__ffsll(found) - 1) / PER;
                identities += (uint32_t)__popcll(found);
            }
            out = transcript_compress_x(plain, y_low);
        }
        if (active) {
            uint8_t *at = stream + fill + item * MESSAGE;  // at most 128 + 64 * 33 bytes in: below TRANSCRIPT_STREAM_WORDS * 8
            if (part == 0) at[0] = POINTS ? TRANSCRIPT_TAG_POINT : TRANSCRIPT_TAG_SCALAR;
            transcript_put(at + 1 + 32 * part, plain);
            if (p.proof && part == 0) {
                s_proof[2 * item] = u32x4{out.l[0], out.l[1], out.l[2], out.l[3]};
                s_proof[2 * item + 1] = u32x4{out.l[4], out.l[5], out.l[6], out.l[7]};
            }
        }
        __syncthreads();
        const uint32_t total = fill + c * MESSAGE, used = (total - 1) / TRANSCRIPT_BLOCK * TRANSCRIPT_BLOCK;  // what transcript_stream_blocks returns
        if (lane == 0) transcript_stream_blocks(h, count, s_stream, total);
        if (p.proof) {
            const uint64_t begin = cursor + (uint64_t)done * TRANSCRIPT_PROOF_ITEM, end = begin + (uint64_t)c * TRANSCRIPT_PROOF_ITEM;
            if (end > p.capacity) missed += end - (begin > p.capacity ? begin : p.capacity);
#pragma unroll 1
            for (uint32_t j = lane; j < 2 * c; j += LANES) {
                const uint64_t at = begin + 16ull * j;
                if (at >= p.capacity) continue;  // compared before anything is added: a cursor nobody initialised cannot wrap into the buffer
                const uint64_t room = p.capacity - at;
                if (room >= 16 && at % 16 == 0) {
                    *reinterpret_cast<u32x4 *>(p.proof + at) = s_proof[j];  // the cursor of an initialised state is a multiple of 32, d_proof 16-byte aligned
                } else {
                    const uint8_t *piece = reinterpret_cast<const uint8_t *>(s_proof + j);
#pragma unroll 1
                    for (uint32_t b = 0; b < 16 && b < room; ++b) p.proof[at + b] = piece[b];
                }
            }
        }
        uint64_t keep = 0;
        if (lane < BLOCK_WORDS) keep = s_stream[used / 8 + lane];  // used + 128 <= total + 127: inside s_stream
        __syncthreads();
        if (lane < BLOCK_WORDS) s_stream[lane] = keep;
        fill = total - used;
        __syncthreads();
    }
    if (lane == 0) {
        fr_unrolled<8>([&](auto i) { s_state.h[decltype(i)::value] = h[decltype(i)::value]; });
        s_state.count = count;
        s_state.fill = fill;
        if (p.proof) s_state.proof_bytes = cursor + (uint64_t)p.n * TRANSCRIPT_PROOF_ITEM;
        s_state.proof_missed += missed;
        s_state.identities += identities;
        s_state.first_identity = first;
        if (POINTS) s_state.points = points + p.n;
    }
    if (lane < BLOCK_WORDS) s_state.block[lane] = s_stream[lane] & transcript_word_mask(fill, lane);
    __syncthreads();
    if (lane < STATE_PIECES) p.state[lane] = image[lane];
}

// grid: one workgroup of one wave.  Lane 0 absorbs the 0x00 and finalises a copy; the two halves of the digest go to lanes 0 and 1,
// a product each (fr_u512_half), and lane 0 adds the two and stores the cell.
__global__ void __launch_bounds__(LANES) transcript_squeeze_kernel(u32x4 *__restrict__ state, u32x4 *__restrict__ challenge) {
    __shared__ TranscriptState s_state;
    __shared__ uint64_t s_digest[TRANSCRIPT_DIGEST / 8];
    const uint32_t lane = threadIdx.x;
    u32x4 *const image = reinterpret_cast<u32x4 *>(&s_state);
    if (lane < STATE_PIECES) image[lane] = state[lane];
    __syncthreads();
    if (lane == 0) {
        if (s_state.fill > TRANSCRIPT_BLOCK) s_state.fill = TRANSCRIPT_BLOCK;  // a state nobody initialised: the block index stays inside the block
        uint64_t digest[8];
        transcript_squeeze_digest(s_state, digest);
        fr_unrolled<8>([&](auto i) { s_digest[decltype(i)::value] = digest[decltype(i)::value]; });
    }
    __syncthreads();
    const bool high = lane % 2 != 0;
    const Fr part = fr_u512_half(s_digest + (high ? 4 : 0), high);  // every lane has a half; lanes 0 and 1 are the ones that count
    const Fr c = mont_add(part, shfl_down_cell(part, 1));
    if (lane == 0) {
        challenge[0] = u32x4{c.l[0], c.l[1], c.l[2], c.l[3]};
        challenge[1] = u32x4{c.l[4], c.l[5], c.l[6], c.l[7]};
    }
    if (lane < STATE_PIECES) state[lane] = image[lane];
}

// ---- the checks -----------------------------------------------------------------------------------------------------------------

inline bool overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
inline bool bad_pointer(const void *p) { return !p || !aligned_to(p, 16); }

template <bool POINTS>
int absorb(aesw_ctx *ctx, const char *call, const char *items_name, uint8_t *d_state, uint32_t n, const uint8_t *d_items, uint8_t *d_proof, uint64_t proof_capacity, void *stream) {
    if (int rc = entry_refused(ctx, call)) return rc;
    if (!transcript_items_ok(n)) return refuse(ctx, call, "n must be 1 ... 65535");
    if (bad_pointer(d_state)) return refuse(ctx, call, "d_state must be there and 16-byte aligned");
    if (bad_pointer(d_items)) return refuse(ctx, call, (std::string(items_name) + " must be there and 16-byte aligned").c_str());
    if ((d_proof == nullptr) != (proof_capacity == 0)) return refuse(ctx, call, "d_proof and proof_capacity go together: both, or NULL and 0");
    if (d_proof && !aligned_to(d_proof, 16)) return refuse(ctx, call, "d_proof must be 16-byte aligned");
    const uint64_t items_bytes = (uint64_t)n * (POINTS ? 64u : 32u);
    if (overlap(d_state, TRANSCRIPT_STATE_BYTES, d_items, items_bytes)) return refuse(ctx, call, (std::string("d_state must not overlap ") + items_name).c_str());
    if (d_proof && (overlap(d_proof, proof_capacity, d_state, TRANSCRIPT_STATE_BYTES) || overlap(d_proof, proof_capacity, d_items, items_bytes)))
        return refuse(ctx, call, (std::string("d_proof must not overlap d_state or ") + items_name).c_str());
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    AbsorbParams p{};
    p.state = reinterpret_cast<u32x4 *>(d_state);
    p.items = reinterpret_cast<const u32x4 *>(d_items);
    p.proof = d_proof;
    p.capacity = proof_capacity;
    p.n = n;
    hipLaunchKernelGGL(transcript_absorb_kernel<POINTS>, dim3(1), dim3(LANES), 0, reinterpret_cast<hipStream_t>(stream), p);
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // namespace aesw_transcript

extern "C" {

uint32_t aesw_transcript_chunk_points(void) { return aesw::TRANSCRIPT_CHUNK_POINTS; }

uint32_t aesw_transcript_chunk_scalars(void) { return aesw::TRANSCRIPT_CHUNK_SCALARS; }

int aesw_transcript_init_device(aesw_ctx *ctx, uint8_t *d_state, void *stream) {
    using namespace aesw_transcript;
    const char *const call = "aesw_transcript_init_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (bad_pointer(d_state)) return refuse(ctx, call, "d_state must be there and 16-byte aligned");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(transcript_init_kernel, dim3(1), dim3(LANES), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<uint64_t *>(d_state));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

int aesw_transcript_points_device(aesw_ctx *ctx, uint8_t *d_state, uint32_t n, const uint8_t *d_points, uint8_t *d_proof, uint64_t proof_capacity, void *stream) {
    return aesw_transcript::absorb<true>(ctx, "aesw_transcript_points_device", "d_points", d_state, n, d_points, d_proof, proof_capacity, stream);
}

int aesw_transcript_scalars_device(aesw_ctx *ctx, uint8_t *d_state, uint32_t n, const uint8_t *d_cells, uint8_t *d_proof, uint64_t proof_capacity, void *stream) {
    return aesw_transcript::absorb<false>(ctx, "aesw_transcript_scalars_device", "d_cells", d_state, n, d_cells, d_proof, proof_capacity, stream);
}

int aesw_transcript_squeeze_device(aesw_ctx *ctx, uint8_t *d_state, uint8_t *d_challenge, void *stream) {
    using namespace aesw_transcript;
    const char *const call = "aesw_transcript_squeeze_device";
    if (int rc = entry_refused(ctx, call)) return rc;
    if (bad_pointer(d_state)) return refuse(ctx, call, "d_state must be there and 16-byte aligned");
    if (bad_pointer(d_challenge)) return refuse(ctx, call, "d_challenge must be there and 16-byte aligned");
    if (overlap(d_state, TRANSCRIPT_STATE_BYTES, d_challenge, sizeof(Fr))) return refuse(ctx, call, "d_challenge must not overlap d_state");
    DeviceGuard g(ctx->device);
    if (!g.ok) return AESW_ERR_NO_DEVICE;
    hipLaunchKernelGGL(transcript_squeeze_kernel, dim3(1), dim3(LANES), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<u32x4 *>(d_state),
                       reinterpret_cast<u32x4 *>(d_challenge));
    HIP_TRY(ctx, hipGetLastError());
    return AESW_OK;
}

}  // extern "C"
