// dopt_obs_emul.cpp -- the eigenvector and observability text of csrc/fbr_dopt.h on the CPU (TEST ONLY, built by tests/dopt_obs_emul_lib.py
// with g++ -ffp-contract=off): the lanes of a workgroup of nt threads run one after the other, the barriers are no-ops.
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_dopt.h"

// C candidates G [C][Pa][Pa]; n_observable [C], energy [C][n]; margin [C], eig [C][n], vec [C][n][n], status [C] may be null.  Returns 0,
// or -1 for what the device call refuses.
extern "C" int dopt_obs_emul(const double *G, int C, int Pa, const int *cols, int n, const double *prior, double thr, int nt, int *n_observable,
                             double *energy, double *margin, double *eig, double *vec, int *status)
{
    if (C < 1 || n < 1 || n > Pa || n > FBR_MAX_DOPT_COLUMNS || nt < 1 || nt > 256) return -1;
    if (!(thr > 0.0) || !(thr < 1.0) || thr * thr < 8.0 * fbr_dopt_band(n)) return -1;
    std::vector<double> A((size_t)n * n), W((size_t)n * n), sh(FBR_DOPT_OBS_SHARED);
    const FbrDoptLanes L = {0, nt, nt};
    for (long c = 0; c < C; c++) {
        const FbrDoptIn in = {G + c * Pa * Pa, Pa, n, cols, prior, 0.0, 1.0};
        const FbrDoptObsOut o = {n_observable + c, energy + c * n, margin ? margin + c : nullptr, eig ? eig + c * n : nullptr,
                                 vec ? vec + c * (long)n * n : nullptr, status ? status + c : nullptr};
        fbr_dopt_obs_candidate(L, in, thr, A.data(), W.data(), sh.data(), o);
    }
    return 0;
}

extern "C" double dopt_obs_emul_band(int n) { return fbr_dopt_band(n); }
