// blind_driver.cpp -- csrc/aesw_blind.h on the CPU, a program of its own (tests/test_blind_model.py builds it with g++, plain and under
// -fsanitize=address,undefined): the cells of a seed, the reduction of a given digest, and blind/aesw_blind.hip's tail commitment run
// lane by lane -- 64 lanes a column, a term each, the xor-shuffle tree, the old commitment mixed in once, one inversion.
//   blind_driver constants
//   blind_driver tail_rows K FIRST_ROW
//   blind_driver cells SEED_HEX DOMAIN FIRST_COLUMN N_COLS FIRST_ROW ROWS     -> a cell a line, 64 hex digits, column by column
//   blind_driver reduce DIGEST_HEX                                            -> fr_from_u512 of the 64 bytes
//   blind_driver commit K N_COLS FIRST_ROW TAIL.bin BASIS.bin COMMIT.bin OUT.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "aesw_blind.h"

using namespace aesw;

static std::vector<uint8_t> unhex(const std::string &s, size_t bytes) {
    if (s.size() != 2 * bytes) {
        std::fprintf(stderr, "expected %zu hex digits\n", 2 * bytes);
        std::exit(2);
    }
    std::vector<uint8_t> out(bytes);
    for (size_t i = 0; i < bytes; ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}

static void words_of(const std::vector<uint8_t> &bytes, uint64_t *w) {
    for (size_t i = 0; i < bytes.size() / 8; ++i) {
        w[i] = 0;
        for (int b = 7; b >= 0; --b) w[i] = (w[i] << 8) | bytes[8 * i + b];
    }
}

static void print_cell(const Fr &c) {
    for (int i = 0; i < FR_LIMBS; ++i)
        for (int b = 0; b < 4; ++b) std::printf("%02x", (unsigned)((c.l[i] >> (8 * b)) & 0xff));
    std::printf("\n");
}

static std::vector<uint8_t> read_file(const char *path, size_t bytes) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> data(bytes);
    f.read(reinterpret_cast<char *>(data.data()), (std::streamsize)bytes);
    if (!f || f.peek() != EOF) {
        std::fprintf(stderr, "%s does not hold %zu bytes\n", path, bytes);
        std::exit(2);
    }
    return data;
}

template <class F>
static F field_at(const std::vector<uint8_t> &data, size_t at) {
    F v{};
    for (int i = 0; i < MONT_LIMBS; ++i) std::memcpy(&v.l[i], data.data() + at + 4 * i, 4);
    return v;
}
static G1Affine affine_at(const std::vector<uint8_t> &data, size_t i) { return G1Affine{field_at<Fq>(data, 64 * i), field_at<Fq>(data, 64 * i + 32)}; }

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "constants" && argc == 2) {
        std::printf("%u %u %u %u %u\n", BLIND_MAX_TAIL, BLIND_MIN_K, BLIND_MAX_K, BLIND_MAX_COLS, BLIND_SCALAR_BITS);
        return 0;
    }
    if (cmd == "tail_rows" && argc == 4) {
        std::printf("%llu %d\n", (unsigned long long)blind_tail_rows((uint32_t)std::strtoul(argv[2], nullptr, 0), std::strtoull(argv[3], nullptr, 0)),
                    (int)blind_commit_tail_ok((uint32_t)std::strtoul(argv[2], nullptr, 0), std::strtoull(argv[3], nullptr, 0)));
        return 0;
    }
    if (cmd == "cells" && argc == 8) {
        uint64_t seed[4];
        words_of(unhex(argv[2], BLIND_SEED_BYTES), seed);
        const uint64_t domain = std::strtoull(argv[3], nullptr, 0), first_column = std::strtoull(argv[4], nullptr, 0), n_cols = std::strtoull(argv[5], nullptr, 0),
                       first_row = std::strtoull(argv[6], nullptr, 0), rows = std::strtoull(argv[7], nullptr, 0);
        const BlindKey key = blind_key(seed);
        for (uint64_t j = 0; j < n_cols; ++j)
            for (uint64_t i = 0; i < rows; ++i) print_cell(blind_cell(key, domain, first_column + j, first_row + i));
        return 0;
    }
    if (cmd == "reduce" && argc == 3) {
        uint64_t digest[8];
        words_of(unhex(argv[2], 64), digest);
        print_cell(fr_from_u512(digest));
        return 0;
    }
    if (cmd == "commit" && argc == 9) {
        const uint32_t k = (uint32_t)std::strtoul(argv[2], nullptr, 0), n_cols = (uint32_t)std::strtoul(argv[3], nullptr, 0);
        const uint64_t first_row = std::strtoull(argv[4], nullptr, 0);
        if (!blind_cols_ok(n_cols) || !blind_commit_tail_ok(k, first_row)) {
            std::printf("refused\n");
            return 0;
        }
        const uint32_t tail = (uint32_t)blind_tail_rows(k, first_row);
        const std::vector<uint8_t> cells = read_file(argv[5], (size_t)n_cols * tail * 32), basis = read_file(argv[6], (size_t)64 << k),
                                   commit = read_file(argv[7], (size_t)n_cols * 64);
        std::vector<uint8_t> out((size_t)n_cols * 64);
        for (uint32_t column = 0; column < n_cols; ++column) {
            std::vector<G1> lanes(BLIND_MAX_TAIL);
            for (uint32_t lane = 0; lane < BLIND_MAX_TAIL; ++lane) {
                Fr cell = FR_ZERO;
                G1Affine point{FQ_ZERO, FQ_ZERO};
                if (lane < tail) {
                    cell = field_at<Fr>(cells, 32 * ((size_t)column * tail + lane));
                    point = affine_at(basis, first_row + lane);
                }
                lanes[lane] = blind_term(cell, point);
            }
            for (uint32_t o = BLIND_MAX_TAIL / 2; o; o >>= 1) {  // every lane adds its partner's point, as the xor shuffle does
                std::vector<G1> next(BLIND_MAX_TAIL);
                for (uint32_t lane = 0; lane < BLIND_MAX_TAIL; ++lane) next[lane] = msm_add(lanes[lane], lanes[lane ^ o]);
                lanes = next;
            }
            const G1Affine sum = msm_to_affine(msm_add_mixed(lanes[0], affine_at(commit, column)));
            for (int i = 0; i < MONT_LIMBS; ++i) {
                std::memcpy(out.data() + 64 * column + 4 * i, &sum.x.l[i], 4);
                std::memcpy(out.data() + 64 * column + 32 + 4 * i, &sum.y.l[i], 4);
            }
        }
        std::ofstream f(argv[8], std::ios::binary);
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)out.size());
        return f ? 0 : 1;
    }
    std::fprintf(stderr, "usage: blind_driver constants | tail_rows K FIRST_ROW | cells SEED DOMAIN FIRST_COLUMN N_COLS FIRST_ROW ROWS | reduce DIGEST | commit K N_COLS FIRST_ROW TAIL BASIS COMMIT OUT\n");
    return 2;
}
