// dopt_emul.cpp -- the HIP-free text of csrc/fbr_dopt.h on the CPU (TEST ONLY, built by tests/dopt_emul_lib.py with g++ -ffp-contract=off):
// the lanes of a workgroup of nt threads run one after the other, the barriers are no-ops.
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_dopt.h"

// C candidates G [C][Pa][Pa]; scale [C] or null; terms [C][4]; status [C], eig [C][n], Cmat [C][n][n] may be null.  Returns 0, or -1 for
// sizes the device call refuses.
extern "C" int dopt_emul(const double *G, int C, int Pa, const int *cols, int n, const double *prior, double reg, const double *scale, int nt,
                         double *terms, int *status, double *eig, double *Cmat)
{
    if (C < 1 || n < 1 || n > Pa || n > FBR_MAX_DOPT_COLUMNS || nt < 1 || nt > 256) return -1;
    std::vector<double> A((size_t)n * n), sh(FBR_DOPT_SHARED);
    const FbrDoptLanes L = {0, nt, nt};
    for (long c = 0; c < C; c++) {
        const FbrDoptIn in = {G + c * Pa * Pa, Pa, n, cols, prior, reg, scale ? scale[c] : 1.0};
        fbr_dopt_candidate(L, in, A.data(), sh.data(), terms + 4 * c, status ? status + c : nullptr, eig ? eig + c * n : nullptr,
                           Cmat ? Cmat + c * (long)n * n : nullptr);
    }
    return 0;
}

extern "C" int dopt_emul_halvings(int n) { return fbr_dopt_halvings(n); }
