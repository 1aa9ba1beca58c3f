// pigs_family_sizes.h -- the rules the *_init of every accumulator family asks for a verdict: a cut-off inside the box, a
// slice window and its lags, the 2 GiB bound of a family's accumulators, the walkers a launch's scratch holds.
// Host logic only (no HIP): tests/shim/family_sizes_check.cpp compiles it for the CPU.  The caller keeps its own message.
#pragma once

#include <stddef.h>

#include <algorithm>
#include <cmath>

namespace pigs {

// 0 < r <= (1 + rel_tol) x every half side, r finite.  rel_tol is 0, or a few ulps where r is a product that may round
// past the half side (pigs_g3_init: rmax = Nr rbin).
inline bool cutoff_in_box(int dim, const double *LboxHalf, double r, double rel_tol)
{
    bool ok = std::isfinite(r) && r > 0.0;
    for (int k = 0; k < dim; ++k) ok = ok && r <= LboxHalf[k] * (1.0 + rel_tol);
    return ok;
}

// the slices Nb-window .. Nb+window lie on the path; the lags 0 .. Ntau lie in the window
inline bool window_ok(int window, int Nb) { return window >= 0 && window <= Nb; }
inline bool lags_ok(int Ntau, int window) { return Ntau >= 0 && Ntau <= 2 * window; }

// do W walkers' 8-byte accumulators, `elements_per_walker` each, pass 2 GiB?
inline bool acc_bytes_pass_2gib(size_t W, size_t elements_per_walker)
{
    return (double)W * (double)elements_per_walker * 8.0 > 2147483648.0;
}

// the walkers of one launch: as many as there are, as the list holds and as fit the scratch budget, one at the least
inline int scratch_slots(size_t W, size_t list_max, size_t budget_bytes, size_t slot_bytes)
{
    return (int)std::max<size_t>(1, std::min({W, list_max, budget_bytes / slot_bytes}));
}

} // namespace pigs
