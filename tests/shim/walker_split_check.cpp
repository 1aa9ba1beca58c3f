// TEST INFRASTRUCTURE.  csrc/pigs_walker_split.h compiled for the CPU: cuts the requests of a case file into launches
// as the library's *_accumulate entry points do -- one set of marks for all cases, as one context has for all families.
// A case is one line "cap unique listed n w_0 .. w_{n-1}" (walkers below W; listed 0: the caller left the list out and
// the w_i are 0..n-1).  Prints per case one line "start count w.. ; start count w.. ; ..." of what each launch's list holds.
//     usage: walker_split_check W < cases
#include <cstdio>
#include <cstdlib>

#include "pigs_walker_split.h"

int main(int argc, char **argv)
{
    const int W = argc > 1 ? atoi(argv[1]) : 0;
    pigs::WalkerMarks marks;
    int cap, unique, listed, n;
    while (scanf("%d %d %d %d", &cap, &unique, &listed, &n) == 4) {
        std::vector<int32_t> sw(n);
        for (int i = 0; i < n; ++i)
            if (scanf("%d", &sw[i]) != 1 || sw[i] < 0 || sw[i] >= W) return 2;
        if (unique && listed) marks.last.resize(W, 0);
        for (int i0 = 0; i0 < n;) {
            pigs::WalkerList L{};
            const int m = pigs::take_walkers(sw, listed != 0, i0, cap, unique != 0, marks, L);
            if (m < 1 || m > cap || m > pigs::kWalkerListMax) return 3;
            printf("%d %d", i0, m);
            for (int i = 0; i < m; ++i) printf(" %d", L.w[i]);
            for (int i = m; i < pigs::kWalkerListMax; ++i)
                if (L.w[i] != 0) return 4;              // nothing written behind the launch's walkers
            printf(" ; ");
            i0 += m;
        }
        printf("\n");
    }
    return 0;
}
