// vals_model.cpp -- the values checker's shared source (aesw_vals_check.h, and aesw_check.h's check_key) on the CPU: n units,
// images gathered exactly as vals_check_kernel gathers them, 64 "lanes" one after the other.  Test infrastructure.
#include <cstring>
#include <vector>

#include "../../halo2-aes_amd/csrc/aesw_vals_check.h"

using namespace aesw;

extern "C" int vals_model_table(uint32_t *words, uint16_t *rows) { return build_values_check_table(words, rows); }

extern "C" int vals_model_image_bytes(void) { return VALS_BI + VALS_KI; }

// report: the seven u64 of aesw_check_report
extern "C" int vals_model_check(const uint8_t *tab768, const uint8_t *pt, const uint8_t *keys, int per_block_keys, uint64_t n, const uint8_t *y,
                                const uint8_t *z, const uint8_t *ct, const uint8_t *kw, const uint8_t *kx, const uint8_t *ky, const uint8_t *kz,
                                uint64_t *report) {
    std::vector<uint32_t> t(CHK_WORDS);
    if (build_values_device_table(t.data()) != 0) return 1;
    using KG = Geo<PACKED>;
    std::vector<uint8_t> img(VALS_BI + VALS_KI);
    CheckAcc acc;
    auto load_key = [&](uint64_t k) {
        uint8_t *ki = img.data() + VALS_BI;
        std::memcpy(ki, kx + k * KG::KXS, KG::KXS);
        std::memcpy(ki + KG::KXS, ky + k * KG::KYS, KG::KYS);
        std::memcpy(ki + KG::KXS + KG::KYS, kz + k * KG::KZS, KG::KZS);
        std::memcpy(ki + KG::KXS + KG::KYS + KG::KZS, kw + k * WORDS_ROWS, WORDS_ROWS);
    };
    if (!per_block_keys) {
        load_key(0);
        for (uint32_t lane = 0; lane < 64; ++lane) check_key(img.data(), t.data(), tab768, keys, 0, lane, 64, acc);
    }
    for (uint64_t b = 0; b < n; ++b) {
        std::memcpy(img.data(), y + b * Geo<VALUES>::YS, Geo<VALUES>::YS);
        std::memcpy(img.data() + VALS_O_Z, z + b * Geo<VALUES>::ZS, Geo<VALUES>::ZS);
        std::memcpy(img.data() + VALS_O_PT, pt + 16 * b, 16);
        if (per_block_keys) load_key(b);
        for (uint32_t lane = 0; lane < 64; ++lane) {
            check_values_block(img.data(), t.data(), tab768, ct ? ct + 16 * b : nullptr, b, lane, 64, acc);
            if (per_block_keys) check_key(img.data(), t.data(), tab768, keys ? keys + 16 * b : nullptr, b, lane, 64, acc);
        }
    }
    report[0] = n; report[1] = per_block_keys ? n : 1;
    report[2] = acc.lookup; report[3] = acc.copy; report[4] = acc.gate; report[5] = acc.input; report[6] = acc.first;
    return 0;
}
