// transcript_driver.cpp -- csrc/aesw_transcript.h on the CPU, a program of its own (tests/test_transcript_model.py builds it plain and
// under -fsanitize=address,undefined and holds it against tests/transcript_model.py):
//   constants                                   the chunk sizes, the message sizes and the state's size
//   fr512 in.bin out.bin                        fr_from_u512 of every 64 bytes of in.bin: 32 bytes each
//   encode points.bin messages.bin compressed.bin   point_message (65 bytes) and point_compressed (32) of every 64-byte point
//   script mode script.bin capacity proof.bin challenges.bin state.bin
//       the ops of script.bin -- (uint32 op, uint32 n, the n items as they lie in device memory) with op 0 init, 1 common_points,
//       2 write_points, 3 common_scalars, 4 write_scalars, 5 squeeze -- against a proof buffer of `capacity` bytes.  mode "items":
//       one message at a time through transcript_absorb, as n calls of halo2's method.  mode "chunks": the way the absorb kernel
//       of transcript/aesw_transcript.hip goes -- a chunk's messages laid behind the bytes the state kept, every full block but
//       the last compressed by transcript_stream_blocks, the remainder moved to the front -- lane by lane.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aesw_transcript.h"

using namespace aesw;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> data;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    uint8_t buf[4096];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
    std::fclose(f);
    return data;
}
static void write_file(const char *path, const std::vector<uint8_t> &data) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(data.data(), 1, data.size(), f) != data.size()) { std::fprintf(stderr, "cannot write %s\n", path); std::exit(2); }
    std::fclose(f);
}
template <class F>
static F field_at(const uint8_t *p) {
    F v{};
    std::memcpy(v.l, p, 32);
    return v;
}

struct Proof {
    std::vector<uint8_t> bytes;  // `capacity` of them
    void append(TranscriptState &s, const uint8_t *item) {
        for (uint32_t b = 0; b < TRANSCRIPT_PROOF_ITEM; ++b) {
            if (s.proof_bytes + b < bytes.size()) bytes[s.proof_bytes + b] = item[b];
            else ++s.proof_missed;
        }
        s.proof_bytes += TRANSCRIPT_PROOF_ITEM;
    }
};

static void note_point(TranscriptState &s, const Fq &x, const Fq &y) {
    if (transcript_is_identity(x, y)) {
        if (s.first_identity == ~0ull) s.first_identity = s.points;
        ++s.identities;
    }
    ++s.points;
}

// n calls of halo2's method
static void absorb_items(TranscriptState &s, bool is_points, uint32_t n, const uint8_t *items, Proof *proof) {
    for (uint32_t i = 0; i < n; ++i) {
        uint8_t message[TRANSCRIPT_POINT_MESSAGE], written[TRANSCRIPT_PROOF_ITEM];
        if (is_points) {
            const Fq x = field_at<Fq>(items + 64 * i), y = field_at<Fq>(items + 64 * i + 32);
            note_point(s, x, y);
            point_message(x, y, message);
            point_compressed(x, y, written);
            transcript_absorb(s, message, TRANSCRIPT_POINT_MESSAGE);
        } else {
            scalar_message(field_at<Fr>(items + 32 * i), message);
            std::memcpy(written, message + 1, 32);
            transcript_absorb(s, message, TRANSCRIPT_SCALAR_MESSAGE);
        }
        if (proof) proof->append(s, written);
    }
}

// the absorb kernel's way, lane by lane
static void absorb_chunks(TranscriptState &s, bool is_points, uint32_t n, const uint8_t *items, Proof *proof) {
    const uint32_t chunk = is_points ? TRANSCRIPT_CHUNK_POINTS : TRANSCRIPT_CHUNK_SCALARS, message = is_points ? TRANSCRIPT_POINT_MESSAGE : TRANSCRIPT_SCALAR_MESSAGE;
    std::vector<uint64_t> stream_words(TRANSCRIPT_STREAM_WORDS, 0xa5a5a5a5a5a5a5a5ull);  // what LDS holds before the kernel writes it is anything
    uint8_t *stream = reinterpret_cast<uint8_t *>(stream_words.data());
    uint32_t fill = (uint32_t)s.fill;
    std::memcpy(stream, s.block, TRANSCRIPT_BLOCK);
    for (uint32_t done = 0; done < n; done += chunk) {
        const uint32_t c = n - done < chunk ? n - done : chunk;
        for (uint32_t item = 0; item < c; ++item) {
            uint8_t written[TRANSCRIPT_PROOF_ITEM];
            uint8_t *at = stream + fill + item * message;
            if (is_points) {
                const Fq x = field_at<Fq>(items + 64 * (done + item)), y = field_at<Fq>(items + 64 * (done + item) + 32);
                note_point(s, x, y);
                const Fq px = transcript_plain(x), py = transcript_plain(y);
                at[0] = TRANSCRIPT_TAG_POINT;
                transcript_put(at + 1, px);
                transcript_put(at + 33, py);
                transcript_put(written, transcript_compress_x(px, py.l[0]));
            } else {
                const Fr plain = transcript_plain(field_at<Fr>(items + 32 * (done + item)));
                at[0] = TRANSCRIPT_TAG_SCALAR;
                transcript_put(at + 1, plain);
                transcript_put(written, plain);
            }
            if (proof) proof->append(s, written);
        }
        const uint32_t total = fill + c * message;
        const uint32_t used = transcript_stream_blocks(s.h, s.count, stream_words.data(), total);
        if (used != (total - 1) / TRANSCRIPT_BLOCK * TRANSCRIPT_BLOCK || (used + TRANSCRIPT_BLOCK) / 8 > TRANSCRIPT_STREAM_WORDS) { std::fprintf(stderr, "the stream's rule is broken\n"); std::exit(3); }
        std::memmove(stream, stream + used, TRANSCRIPT_BLOCK);
        fill = total - used;
    }
    for (uint32_t i = 0; i < 16; ++i) s.block[i] = stream_words[i] & transcript_word_mask(fill, i);
    s.fill = fill;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "constants") {
        std::printf("%u %u %u %u %u %u %u\n", TRANSCRIPT_CHUNK_POINTS, TRANSCRIPT_CHUNK_SCALARS, TRANSCRIPT_POINT_MESSAGE, TRANSCRIPT_SCALAR_MESSAGE, TRANSCRIPT_PROOF_ITEM,
                    TRANSCRIPT_STATE_BYTES, TRANSCRIPT_MAX_ITEMS);
        return 0;
    }
    if (cmd == "fr512" && argc == 4) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        std::vector<uint8_t> out(in.size() / 64 * 32);
        for (size_t i = 0; i < in.size() / 64; ++i) {
            uint64_t d[8];
            std::memcpy(d, in.data() + 64 * i, 64);
            const Fr c = fr_from_u512(d);
            std::memcpy(out.data() + 32 * i, c.l, 32);
        }
        write_file(argv[3], out);
        return 0;
    }
    if (cmd == "encode" && argc == 5) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        const size_t n = in.size() / 64;
        std::vector<uint8_t> messages(n * TRANSCRIPT_POINT_MESSAGE), compressed(n * TRANSCRIPT_PROOF_ITEM);
        for (size_t i = 0; i < n; ++i) {
            const Fq x = field_at<Fq>(in.data() + 64 * i), y = field_at<Fq>(in.data() + 64 * i + 32);
            point_message(x, y, messages.data() + i * TRANSCRIPT_POINT_MESSAGE);
            point_compressed(x, y, compressed.data() + i * TRANSCRIPT_PROOF_ITEM);
        }
        write_file(argv[3], messages);
        write_file(argv[4], compressed);
        return 0;
    }
    if (cmd == "script" && argc == 8) {
        const bool chunks = std::string(argv[2]) == "chunks";
        const std::vector<uint8_t> script = read_file(argv[3]);
        Proof proof{std::vector<uint8_t>((size_t)std::strtoull(argv[4], nullptr, 10), 0xa5)};
        std::vector<uint8_t> challenges;
        TranscriptState s{};
        std::memset(&s, 0x5a, sizeof s);  // the first op of every script is an init
        for (size_t at = 0; at < script.size();) {
            uint32_t op, n;
            std::memcpy(&op, script.data() + at, 4);
            std::memcpy(&n, script.data() + at + 4, 4);
            at += 8;
            if (op == 0) {
                s = transcript_init();
            } else if (op == 5) {
                const Fr c = transcript_squeeze(s);
                challenges.insert(challenges.end(), reinterpret_cast<const uint8_t *>(c.l), reinterpret_cast<const uint8_t *>(c.l) + 32);
            } else if (op >= 1 && op <= 4) {
                const bool is_points = op <= 2, write = op == 2 || op == 4;
                const size_t bytes = (size_t)n * (is_points ? 64 : 32);
                if (!transcript_items_ok(n) || at + bytes > script.size()) { std::fprintf(stderr, "a bad op\n"); return 2; }
                (chunks ? absorb_chunks : absorb_items)(s, is_points, n, script.data() + at, write ? &proof : nullptr);
                at += bytes;
            } else {
                std::fprintf(stderr, "a bad op\n");
                return 2;
            }
        }
        std::vector<uint8_t> state(sizeof s);
        std::memcpy(state.data(), &s, sizeof s);
        write_file(argv[5], proof.bytes);
        write_file(argv[6], challenges);
        write_file(argv[7], state);
        return 0;
    }
    std::fprintf(stderr, "usage: transcript_driver constants | fr512 in out | encode points messages compressed | script items|chunks script capacity proof challenges state\n");
    return 2;
}
