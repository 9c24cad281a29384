// The host mapping code of libaesw_sigma.so (csrc/aesw_sigma.h: sigma_build_mapping, sigma_assembly_copy) in a process of its own:
// plain g++, no Python, no GPU.  The copy graphs and the placement come from libaesw.so's pure-host functions.  Built once plain
// and once with -fsanitize=address,undefined by tests/test_sigma_model.py.
//   sigma_mapping_driver <k> <n_sets> <n_blocks> <out file>    writes map[3 n_sets + 2][2^k] as uint32_t words; exit 3 where the
//   circuit does not hold n_blocks (the refusal of aesw_sigma_mapping_host)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/aesw.h"
#include "aesw_sigma.h"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const uint32_t k = (uint32_t)std::atoi(argv[1]), n_sets = (uint32_t)std::atoi(argv[2]), n_blocks = (uint32_t)std::atoi(argv[3]);
    if (n_sets < 1 || n_sets > 1024 || !aesw::sigma_shape_ok(k, aesw::sigma_columns(n_sets))) return 2;
    if (n_blocks > aesw_block_capacity(k, n_sets)) return 3;
    const uint64_t cells = aesw::sigma_cells(k, aesw::sigma_columns(n_sets));
    std::vector<uint32_t> map(cells), aux(cells), sizes(cells);
    std::vector<aesw_copy_edge> key_edges(AESW_KEY_COPIES), block_edges(AESW_BLOCK_COPIES);
    if (aesw_key_copy_graph(key_edges.data()) || aesw_block_copy_graph(block_edges.data())) return 4;
    aesw::sigma_build_mapping(k, n_sets, n_blocks, key_edges.data(), AESW_KEY_COPIES, block_edges.data(), AESW_BLOCK_COPIES,
                              [&](uint32_t b, uint32_t *set, uint32_t *row) {
                                  uint64_t r = 0;
                                  if (aesw_block_placement(k, n_sets, b, set, &r)) std::exit(5);
                                  *row = (uint32_t)r;
                              },
                              map.data(), aux.data(), sizes.data());
    std::FILE *f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(map.data(), sizeof(uint32_t), map.size(), f) != map.size()) return 6;
    std::fclose(f);
    return 0;
}
