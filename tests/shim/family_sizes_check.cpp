// TEST INFRASTRUCTURE.  csrc/pigs_family_sizes.h compiled for the CPU: the verdicts the *_init entry points of the
// accumulator families ask for, one per line of a case file (doubles in any form strtod reads: hex floats, nan, inf):
//     S W list_max budget_bytes slot_bytes     -> scratch_slots
//     G W elements_per_walker                  -> acc_bytes_pass_2gib (0 or 1)
//     C dim L0half L1half L2half r rel_tol     -> cutoff_in_box (0 or 1)
//     W window Nb                              -> window_ok (0 or 1)
//     L Ntau window                            -> lags_ok (0 or 1)
//     usage: family_sizes_check < cases
#include <cstdio>
#include <cstdlib>

#include "pigs_family_sizes.h"

int main()
{
    char kind[8], t[6][64];
    while (scanf("%7s", kind) == 1) {
        const int want = kind[0] == 'S' ? 4 : kind[0] == 'C' ? 6 : 2;
        for (int i = 0; i < want; ++i)
            if (scanf("%63s", t[i]) != 1) return 2;
        switch (kind[0]) {
        case 'S':
            printf("%d\n", pigs::scratch_slots(strtoull(t[0], nullptr, 10), strtoull(t[1], nullptr, 10), strtoull(t[2], nullptr, 10),
                                               strtoull(t[3], nullptr, 10)));
            break;
        case 'G': printf("%d\n", (int)pigs::acc_bytes_pass_2gib(strtoull(t[0], nullptr, 10), strtoull(t[1], nullptr, 10))); break;
        case 'C': {
            const double half[3] = {strtod(t[1], nullptr), strtod(t[2], nullptr), strtod(t[3], nullptr)};
            printf("%d\n", (int)pigs::cutoff_in_box(atoi(t[0]), half, strtod(t[4], nullptr), strtod(t[5], nullptr)));
            break;
        }
        case 'W': printf("%d\n", (int)pigs::window_ok(atoi(t[0]), atoi(t[1]))); break;
        case 'L': printf("%d\n", (int)pigs::lags_ok(atoi(t[0]), atoi(t[1]))); break;
        default: return 3;
        }
    }
    return 0;
}
