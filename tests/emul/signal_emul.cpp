// signal_emul.cpp -- the HIP-free text of csrc/fbr_signal.h on the CPU (TEST ONLY, built by tests/signal_cases.py with g++ -ffp-contract=off):
// fbr_filtfilt / fbr_medfilt / fbr_central_diff on [S][ld] arrays with the work items of the kernels run one after the other -- the design
// step, passes A / B / C block by block with FBR_SIG_LB, the gather and the median, the central difference -- and the buffers of
// fbr_signal_api.hip (Y1 [Le][ncols], zs / zst [nblk][ncols][FBR_SIG_MAXC - 1]).  No arithmetic of its own.
#include <cstdint>
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_signal.h"

extern "C" {

int sig_block_length() { return FBR_SIG_LB; }

// the refusals of fbr_filtfilt: -1
int sig_filtfilt(const double *b, const double *a, int ncoef, double *X, long S, int ncols, int ld)
{
    if (!b || !a || !X || ncoef < 2 || ncoef > FBR_SIG_MAXC || ncols < 1 || ld < ncols || a[0] == 0.0) return -1;
    const int pad = 3 * ncoef;
    if (S <= pad) return -1;
    FbrIir f;
    fbr_sig_design(f, b, a, ncoef);
    const long Le = S + 2L * pad, nblk = (Le + FBR_SIG_LB - 1) / FBR_SIG_LB;
    const size_t zcount = (size_t)nblk * ncols * (FBR_SIG_MAXC - 1);
    std::vector<double> Y1((size_t)Le * ncols), zs(zcount), zst(zcount);
    for (int dir = 0; dir < 2; dir++) {
        for (int mode = 0; mode < 2; mode++) {
            for (long blk = 0; blk < nblk; blk++)
                for (int c = 0; c < ncols; c++) fbr_sig_block(f, mode, dir, X, S, ncols, ld, pad, Y1.data(), zs.data(), zst.data(), blk, c);
            if (mode == 0)
                for (int c = 0; c < ncols; c++) fbr_sig_chain(f, dir, X, S, ncols, ld, pad, Y1.data(), zs.data(), zst.data(), nblk, c);
        }
    }
    return 0;
}

int sig_medfilt(int k, double *X, long S, int ncols, int ld)
{
    if (!X || k < 1 || k > FBR_SIG_MAXK || (k & 1) == 0 || S < 1 || ncols < 1 || ld < ncols) return -1;
    std::vector<double> src((size_t)S * ncols);
    for (long t = 0; t < S; t++)
        for (int c = 0; c < ncols; c++) src[(size_t)t * ncols + c] = X[t * ld + c];
    for (long t = 0; t < S; t++)
        for (int c = 0; c < ncols; c++) X[t * ld + c] = fbr_sig_median(k, src.data(), S, ncols, t, c);
    return 0;
}

int sig_central_diff(const double *A, const double *T, double *D, long S, int ncols)
{
    if (!A || !T || !D || S < 5 || ncols < 1) return -1;
    for (long t = 0; t < S; t++)
        for (int c = 0; c < ncols; c++) D[t * ncols + c] = fbr_sig_cdiff(A, T, S, ncols, t, c);
    return 0;
}
}
