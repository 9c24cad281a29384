// Drives KeySlotPolicy (csrc/aesw_keyring.h, compiled alone: no ROCm include) from a script on stdin -- tests/test_keyring_policy.py.
//   i       the first slot, made by the context and parked in `spare`     s N     option "key_slots" = N
//   w       an eager schedule: prints the slot it writes                  f       ... whose key launch fails: the slot, then the step back
//   c       a captured schedule: a fresh slot of its own, pinned          p I     a captured launch pins slot I
// Every command is answered with one line: "<slot or -> <pos> <ring ...> | <spare ...>".
#define AESW_KEYRING_POLICY_ONLY
#include "aesw_keyring.h"

#include <cstdio>

int main() {
    KeySlotPolicy pol;
    std::vector<char> pinned;
    auto is_pinned = [&](int i) { return pinned[i] != 0; };
    auto fresh = [&](int *i) { pinned.push_back(0); *i = (int)pinned.size() - 1; return 0; };
    char cmd;
    while (std::scanf(" %c", &cmd) == 1) {
        int slot = -1, arg = 0;
        if (cmd == 's' || cmd == 'p') { if (std::scanf("%d", &arg) != 1) return 2; }
        if (cmd == 'i') { fresh(&slot); pol.spare.push_back(slot); slot = -1; }
        else if (cmd == 's') pol.size = arg;
        else if (cmd == 'p') pinned[arg] = 1;
        else if (cmd == 'c') { fresh(&slot); pinned[slot] = 1; }
        else if (cmd == 'w' || cmd == 'f') { if (pol.next(is_pinned, fresh, &slot) != 0) return 3; if (cmd == 'f') pol.step_back(); }
        else return 2;
        if (slot < 0) std::printf("-"); else std::printf("%d", slot);
        std::printf(" %d", pol.pos);
        for (int r : pol.ring) std::printf(" %d", r);
        std::printf(" |");
        for (int r : pol.spare) std::printf(" %d", r);
        std::printf("\n");
    }
    return 0;
}
