// dopt_sanitize.cpp -- a stand-alone program (TEST ONLY, built by tests/test_dopt_reference.py with g++ -fsanitize=address,undefined and run
// on the CPU): the HIP-free text of csrc/fbr_dopt.h on seeded matrices of 1 to 67 columns -- dense, diagonal, zero, singular with reg = 0,
// with a NaN --, with 1, 64 and 256 lanes, with and without eig / Cmat, every buffer allocated at its exact size.  Checks what needs no
// reference: ascending eigenvalues, their sum against the trace, a bit-symmetric Cmat, (M + delta I) Cmat = -2 scale I.  Prints "ok" and
// returns 0; the sanitizers abort on an out-of-bounds access, an overflow or a bad shift.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_dopt.h"

int main()
{
    std::mt19937_64 gen(5);
    std::normal_distribution<double> nd(0.0, 1.0);
    const int sizes[9] = {1, 2, 3, 4, 7, 16, 33, 64, 67}, lanes[3] = {1, 64, 256};
    long checked = 0;
    for (int is = 0; is < 9; is++)
        for (int kind = 0; kind < 5; kind++)  // dense, diagonal, zero, singular with reg = 0, a NaN
            for (int il = 0; il < 3; il++) {
                const int n = sizes[is], Pa = n + 2, nt = lanes[il];
                std::vector<double> G((size_t)Pa * Pa), A((size_t)n * n), sh(FBR_DOPT_SHARED), terms(4), eig(n), Cm((size_t)n * n), prior((size_t)n * n);
                std::vector<int> cols(n);
                for (int i = 0; i < n; i++) cols[i] = Pa - 1 - i;  // descending: not sorted
                for (auto &g : G) g = nd(gen);
                const int rows = kind == 3 ? (n > 1 ? n - 1 : 0) : 2 * n + 1;
                std::vector<double> Y((size_t)rows * n);
                for (auto &y : Y) y = nd(gen);
                for (int r = 0; r < n; r++)
                    for (int c = 0; c < n; c++) {
                        double s = 0.0;
                        for (int k = 0; k < rows; k++) s += Y[(size_t)k * n + r] * Y[(size_t)k * n + c];
                        if (kind == 1) s = r == c ? 1.0 + r % 3 : 0.0;
                        if (kind == 2) s = 0.0;
                        G[(size_t)cols[r] * Pa + cols[c]] = s;
                        prior[(size_t)r * n + c] = r == c ? 0.5 : 0.0;
                    }
                if (kind == 4) G[(size_t)cols[n - 1] * Pa + cols[0]] = NAN;
                const bool with_prior = kind == 0 && (is & 1);
                const double reg = kind == 3 ? 0.0 : 1e-4, scale = 1.5;
                const FbrDoptIn in = {G.data(), Pa, n, cols.data(), with_prior ? prior.data() : nullptr, reg, scale};
                const FbrDoptLanes L = {0, nt, nt};
                int status = -1;
                fbr_dopt_candidate(L, in, A.data(), sh.data(), terms.data(), &status, eig.data(), Cm.data());
                double t2[4];
                fbr_dopt_candidate(L, in, A.data(), sh.data(), t2, nullptr, nullptr, nullptr);
                for (int k = 0; k < 4; k++)
                    if (!(t2[k] == terms[k]) && !(std::isnan(t2[k]) && std::isnan(terms[k]))) return printf("terms differ without eig / Cmat\n"), 1;
                if (kind == 4) {
                    if (status != FBR_DOPT_NONFINITE || !std::isnan(terms[0]) || terms[3] != 0.0 || !std::isnan(Cm[0]) || !std::isnan(eig[n - 1]))
                        return printf("NaN case n=%d\n", n), 1;
                    checked++;
                    continue;
                }
                double trace = 0.0, esum = 0.0, amax = 0.0;
                for (int r = 0; r < n; r++) {
                    trace += G[(size_t)cols[r] * Pa + cols[r]] + (with_prior ? 0.5 : 0.0);
                    esum += eig[r];
                    if (r && eig[r] < eig[r - 1]) return printf("eigenvalues descend n=%d kind=%d\n", n, kind), 1;
                }
                amax = std::fabs(trace) + 1e-300;
                if (std::fabs(trace - esum) > 64.0 * n * DBL_EPSILON * amax) return printf("trace n=%d kind=%d: %g vs %g\n", n, kind, trace, esum), 1;
                if (terms[1] != eig[n - 1] || terms[2] != reg * std::fmax(terms[1], 1e-30)) return printf("terms n=%d\n", n), 1;
                if (kind == 3) {
                    if (status != 0 && status != FBR_DOPT_NOT_POSITIVE) return printf("status %d n=%d\n", status, n), 1;
                    if (n == 1 && status != FBR_DOPT_NOT_POSITIVE) return printf("a zero pivot passed\n"), 1;
                    checked++;
                    continue;
                }
                if (status != 0) return printf("status %d n=%d kind=%d\n", status, n, kind), 1;
                double worst = 0.0;
                for (int r = 0; r < n; r++)
                    for (int c = 0; c < n; c++) {
                        if (Cm[(size_t)r * n + c] != Cm[(size_t)c * n + r]) return printf("Cmat is not symmetric\n"), 1;
                        double s = 0.0;
                        for (int k = 0; k < n; k++) {
                            const int hi = r >= k ? r : k, lo = r >= k ? k : r;
                            double m = G[(size_t)cols[hi] * Pa + cols[lo]] + (with_prior && hi == lo ? 0.5 : 0.0) + (r == k ? terms[2] : 0.0);
                            s += m * Cm[(size_t)k * n + c];
                        }
                        worst = std::fmax(worst, std::fabs(s / (-2.0 * scale) - (r == c ? 1.0 : 0.0)));
                    }
                if (!(worst <= n * DBL_EPSILON * (1.0 / reg + 1.0))) return printf("residual %g n=%d kind=%d\n", worst, n, kind), 1;
                checked++;
            }
    printf("%ld cases\nok\n", checked);
    return 0;
}
