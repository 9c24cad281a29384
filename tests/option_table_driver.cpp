// Drives the option table (csrc/aesw_options.h, compiled alone: no ROCm include) -- tests/option_table.py.
//   no argument        dumps one line per row: "<name> <default or -> <lowest> <highest> <form> <settable> <readable> <trace builds only>"
//                      (default "-": the row has no field in AeswOptions; form: range / zero_or_range / truthy; settable: in this build)
//   script on stdin    "s <name> <value>" sets and "g <name>" gets through the table, on one AeswOptions that starts at its
//                      defaults; each is answered with "ok", "ok <value>" or "refused" (unknown names are refused too)
#include "aesw_options.h"

#include <cinttypes>
#include <cstdio>

int main(int argc, char **) {
    AeswOptions opt;
    if (argc == 1) {
        for (const OptionRow &r : AESW_OPTIONS) {
            AeswOptions scratch;
            std::printf("%s ", r.name);
            if (r.field) std::printf("%" PRId64, AeswOptions{}.*r.field); else std::printf("-");
            std::printf(" %" PRId64 " %" PRId64 " %s %d %d %d\n", r.lo, r.hi,
                        (r.access & OPT_TRUTHY) ? "truthy" : (r.access & OPT_OR_ZERO) ? "zero_or_range" : "range",
                        aesw_option_set(scratch, r, r.lo), (r.access & OPT_GET) != 0, (r.access & OPT_TRACE_ONLY) != 0);
        }
        return 0;
    }
    char cmd, name[64];
    while (std::scanf(" %c %63s", &cmd, name) == 2) {
        const OptionRow *r = aesw_find_option(name);
        int64_t v = 0;
        if (cmd == 's') {
            if (std::scanf("%" SCNd64, &v) != 1) return 2;
            std::printf(r && aesw_option_set(opt, *r, v) ? "ok\n" : "refused\n");
        } else if (cmd == 'g') {
            if (r && aesw_option_get(opt, *r, &v)) std::printf("ok %" PRId64 "\n", v); else std::printf("refused\n");
        } else {
            return 2;
        }
    }
    return 0;
}
