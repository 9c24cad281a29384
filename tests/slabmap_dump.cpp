// Prints every table the host derives from the slab map (csrc/aesw_slabmap.h and its users; compiled with plain g++, no ROCm
// include) -- tests/test_slabmap.py reads the small ones and holds them against tests/slab_map.py and the oracle; built
// against two versions of csrc/, the two outputs say whether a change to the headers changed anything derived
// (profiles/slabmap/README.md).  One line per table: its name, then the values, or for the large tables their count and an
// FNV-1a hash of the words.
#include "aesw_vals_check.h"
#if __has_include("aesw_flush.h")
#include "aesw_flush.h"
#endif

#include <cinttypes>
#include <cstdio>
#include <vector>

using namespace aesw;

namespace {

template <class T>
void line(const char *name, int a, const T *v, int n) {
    std::printf("%s %d:", name, a);
    for (int i = 0; i < n; ++i) std::printf(" %d", (int)v[i]);
    std::printf("\n");
}

void hashed(const char *name, int a, const uint32_t *w, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i)
        for (int b = 0; b < 4; ++b) h = (h ^ ((w[i] >> (8 * b)) & 0xffu)) * 0x100000001b3ull;
    std::printf("%s %d: %zu words fnv1a %016" PRIx64 "\n", name, a, n, h);
}

void graph(const char *name, const CopyEdge *e, int n) {
    std::printf("%s %d:", name, n);
    for (int i = 0; i < n; ++i)
        std::printf(" %d.%d.%d<%d.%d.%d", e[i].dst_space, e[i].dst_col, e[i].dst_row, e[i].src_space, e[i].src_col, e[i].src_row);
    std::printf("\n");
}

template <class W>
void flush(const char *name, int layout) {
    std::vector<uint32_t> t((size_t)sched_first<W>(10) * 64);
    build_flush_table<W>(t.data());
    hashed(name, layout, t.data(), t.size());
}

// the seven strides x y z words kx ky kz of a layout
void strides(int layout, uint32_t out[7]) {
#if __has_include("aesw_slabmap.h")
    for (int c = 0; c < 7; ++c) out[c] = slab_strides(layout)[c];
#else  // a csrc/ from before the slab map: the literals of Geo<>
    auto geo = [&](auto g) {
        using G = decltype(g);
        const uint32_t v[7] = {(uint32_t)G::XS, (uint32_t)G::YS, (uint32_t)G::ZS, (uint32_t)WORDS_ROWS, (uint32_t)G::KXS, (uint32_t)G::KYS, (uint32_t)G::KZS};
        for (int c = 0; c < 7; ++c) out[c] = v[c];
    };
    if (layout == DENSE) geo(Geo<DENSE>{}); else if (layout == PACKED) geo(Geo<PACKED>{}); else geo(Geo<VALUES>{});
#endif
}

}  // namespace

int main() {
    uint8_t em[AES_ROWS], km[KEY_ROWS], etag[AES_ROWS], ktag[KEY_ROWS], q[WORDS_ROWS], rc[WORDS_ROWS];
    int ei[AES_ROWS], ki[KEY_ROWS];
    for (int c = 0; c < 3; ++c) {
        encrypt_assigned_mask(c, em);
        line("encrypt_assigned_mask", c, em, AES_ROWS);
        encrypt_values_mask(c, em);
        line("encrypt_values_mask", c, em, AES_ROWS);
        key_assigned_mask(c, km);
        line("key_assigned_mask", c, km, KEY_ROWS);
        for (int r = 0; r < AES_ROWS; ++r) ei[r] = packed_index_enc(c, r);
        for (int r = 0; r < KEY_ROWS; ++r) ki[r] = packed_index_key(c, r);
        line("packed_index_enc", c, ei, AES_ROWS);
        line("packed_index_key", c, ki, KEY_ROWS);
    }
    encrypt_selector_tags(etag);
    key_selector_tags(ktag, q, rc);
    line("encrypt_selector_tags", 0, etag, AES_ROWS);
    line("key_selector_tags", 0, ktag, KEY_ROWS);
    line("q_eq_rcon", 0, q, WORDS_ROWS);
    line("rcon_fixed", 0, rc, WORDS_ROWS);
    for (int l = 0; l < 3; ++l) {
        uint32_t st[7];
        strides(l, st);
        line("slab_strides", l, st, 7);
    }
    std::vector<CopyEdge> be(BLOCK_COPIES), ke(KEY_COPIES);
    graph("block_copy_graph", be.data(), block_copy_graph(be.data()));
    graph("key_copy_graph", ke.data(), key_copy_graph(ke.data()));
    std::vector<uint32_t> t(CHK_WORDS);
    for (int l = 0; l < 2; ++l) {
        const CheckGeo g = check_geo(l);
        const uint32_t geo[8] = {g.sx, g.sy, g.sz, g.kxs, g.kys, g.kzs, g.bi, g.ki};
        line("check_geo", l, geo, 8);
        build_check_table(l, t.data());
        hashed("build_check_table", l, t.data(), t.size());
    }
    const int rv = build_values_device_table(t.data());
    hashed("build_values_device_table", rv, t.data(), t.size());
    const int vals[5] = {VALS_ROWS, VALS_O_Z, VALS_O_PT, VALS_BI, VALS_KI};
    line("values_image", 0, vals, 5);
    flush<WinX<DENSE>>("flush_table_x", DENSE); flush<WinY<DENSE>>("flush_table_y", DENSE); flush<WinZ<DENSE>>("flush_table_z", DENSE);
    flush<WinX<PACKED>>("flush_table_x", PACKED); flush<WinY<PACKED>>("flush_table_y", PACKED); flush<WinZ<PACKED>>("flush_table_z", PACKED);
    flush<WinY<VALUES>>("flush_table_y", VALUES); flush<WinZ<VALUES>>("flush_table_z", VALUES);
    return 0;
}
