// Drives the argument rules of the libraries next to libaesw.so (csrc/aesw_entry_rules.h, compiled alone: no ROCm include, no
// context) -- tests/test_entry_rules.py.  Commands on stdin, one answer line each: the refusal's text, or "-" where the
// argument passes.  A pointer is given as its address (0: null) and is never read through.
//   layout <layout>
//   k <k>
//   sets <n_sets>
//   report <d_report>
//   slabs <d_x> <d_y> <d_z>
//   keys <k> <slab: 0 | 1> <kx> <ky> <kz>                 "<with_keys> <text>"
//   outputs <k> <with_k> <n_sets> <d_mult> <d_report>
//   challenges <d_beta> <d_gamma>
//   product_outputs <d_z_fr> <d_closing_fr>
//   workspace <d_workspace>
#include "aesw_entry_rules.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

using namespace aesw;

template <class T = uint8_t>
static T *at(uint64_t address) { return reinterpret_cast<T *>(static_cast<uintptr_t>(address)); }

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        uint64_t a[5] = {0, 0, 0, 0, 0};
        const int want = !std::strcmp(cmd, "slabs") ? 3 : (!std::strcmp(cmd, "keys") || !std::strcmp(cmd, "outputs")) ? 5 : (!std::strcmp(cmd, "challenges") || !std::strcmp(cmd, "product_outputs")) ? 2 : 1;
        for (int i = 0; i < want; ++i)
            if (std::scanf("%" SCNu64, &a[i]) != 1) return 2;
        const char *why = nullptr;
        if (!std::strcmp(cmd, "layout")) why = bad_layout((int)a[0]);
        else if (!std::strcmp(cmd, "k")) why = bad_k((uint32_t)a[0]);
        else if (!std::strcmp(cmd, "sets")) why = bad_sets((uint32_t)a[0]);
        else if (!std::strcmp(cmd, "report")) why = bad_report(at(a[0]));
        else if (!std::strcmp(cmd, "slabs")) why = bad_slabs(at(a[0]), at(a[1]), at(a[2]));
        else if (!std::strcmp(cmd, "keys")) {
            const aesw_key_slab ks = {nullptr, at(a[2]), at(a[3]), at(a[4])};
            const aesw_key_slab *p = a[1] ? &ks : nullptr;
            why = bad_key_columns(p, (uint32_t)a[0]);
            std::printf("%d ", with_keys(p, (uint32_t)a[0]) ? 1 : 0);
        } else if (!std::strcmp(cmd, "outputs")) why = bad_outputs((uint32_t)a[0], a[1] != 0, (uint32_t)a[2], at<uint32_t>(a[3]), at<aesw_mult_report>(a[4]));
        else if (!std::strcmp(cmd, "challenges")) why = bad_challenges(at(a[0]), at(a[1]));
        else if (!std::strcmp(cmd, "product_outputs")) why = bad_product_outputs(at(a[0]), at(a[1]));
        else if (!std::strcmp(cmd, "workspace")) why = bad_workspace(at(a[0]));
        else return 2;
        std::printf("%s\n", why ? why : "-");
    }
    return 0;
}
