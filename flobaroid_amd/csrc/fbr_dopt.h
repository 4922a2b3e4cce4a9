// fbr_dopt.h -- the D-optimality arithmetic of candidate trajectories on the device (fbr_dopt_terms, fbr.h): per candidate the eigenvalues
// of M = G[cols, cols] (+ prior), the numbers the optimiser takes from them (trajectoryOptimizer.py:263-277: neg_log_det, lambda_max,
// delta, n_observable) and, optionally, Cmat = -2 scale (M + delta I)^-1, the matrix fbr_regressor_weights turns into weight rows
// (analyticalGradient.py:538-565).  Only the LOWER triangle of M is read, as numpy.linalg.eigvalsh does.
//
// One workgroup per candidate; the matrix lives in n^2 doubles of device scratch (full, row-major, kept exactly symmetric so that a column
// can be read as a row: every inner loop below walks rows with consecutive lanes on consecutive addresses), the vectors in the LDS.
//   1. gather + normalise: A = 2^k M with max|A_ij| in [1, 2) (k = 0 for the zero matrix) -- a power of two, so nothing is rounded and the
//      results are scaled back exactly: the spectrum of 2^j G is bit for bit 2^j times the spectrum of G.  Then Householder reflections
//      H = I - tau v v^T and the symmetric rank-2 update A -= v w^T + w v^T reduce A to tridiagonal (d, e).  A zero sub-column takes H = I.
//   2. eigenvalues by bisection on Sturm counts, one lane per eigenvalue index, on the Gershgorin interval of (d, e) widened as LAPACK's
//      dstebz widens it; the pivot of the recurrence is floored at pivmin = DBL_MIN max(1, max e^2); FBR_DOPT_HALVINGS(n) halvings.
//      Absolute error of order eps |A|, the error model of LAPACK's own tridiagonal solvers.  A zero tridiagonal has the eigenvalue 0 exactly.
//   3. (Cmat asked for) A is gathered again with delta on its diagonal, factored U^T U = A (Cholesky by rows), W = U^-T by forward
//      substitution into the lower triangle, and (M + delta I)^-1 = W^T W; both triangles of Cmat get the same computed value.
// Every loop bound is known before the loop starts; nothing iterates "until converged".  No atomics, every sum in one fixed order.  FMA
// contraction is off in this file: the symmetric update must give A_rc and A_cr the same bits, and the g++ emulation (tests/emul/
// dopt_emul.cpp, -ffp-contract=off) then computes what the device computes wherever the arithmetic is +, -, *, /, sqrt.
// status: FBR_DOPT_NONFINITE: M has a non-finite entry (terms NaN, n_observable 0, eig and Cmat NaN); FBR_DOPT_NOT_POSITIVE: a pivot of
// the factorisation was not positive and finite -- reg = 0 on a singular matrix -- (Cmat NaN, the terms stand).
//
// The text is HIP-free: the lanes of the workgroup are the iterations of FBR_DOPT_LANES, which the device runs one per thread with
// FBR_DOPT_SYNC = __syncthreads and the host one after the other.  Code outside those loops is uniform: every thread computes the same
// value from what the LDS held at the last barrier.  A lane loop reads of shared data only what was written before the barrier in front of it.
#pragma once
#include <float.h>
#include <math.h>

#include "../../include/fbr.h"
#include "fbr_math.h"

#define FBR_DOPT_NONFINITE 1
#define FBR_DOPT_NOT_POSITIVE 2
#define FBR_DOPT_SHARED (6 * FBR_MAX_DOPT_COLUMNS)  // doubles of LDS a workgroup needs

struct FbrDoptLanes {
    int lane0, lane1, nt;  // this caller runs lanes [lane0, lane1) of nt
};
#define FBR_DOPT_LANES(t) for (int t = L.lane0; t < L.lane1; t++)
#if defined(__HIP_DEVICE_COMPILE__)
#define FBR_DOPT_SYNC() __syncthreads()
#else
#define FBR_DOPT_SYNC() ((void)0)
#endif

struct FbrDoptIn {
    const double *G;      // [Pa][Pa] the candidate's Gram
    int Pa, n;
    const int *cols;      // [n]
    const double *prior;  // [n][n] or null
    double reg, scale;
};

// halvings of the bisection: the widened Gershgorin interval is shorter than 8 n (|A_ij| < 2), so 55 + ceil(log2(2 n)) halvings bring
// it below 2^-52
FBR_HD int fbr_dopt_halvings(int n)
{
    int lg = 0;
    while ((1 << lg) < 2 * n) lg++;
    return 55 + lg;
}

FBR_HD bool fbr_dopt_finite(double v) { return fabs(v) <= DBL_MAX; }

// entry (r, c) of M from the lower triangles of G and the prior
FBR_HD double fbr_dopt_entry(const FbrDoptIn &in, int r, int c)
{
#pragma clang fp contract(off)
    const int hi = r >= c ? r : c, lo = r >= c ? c : r;
    double v = in.G[(long)in.cols[hi] * in.Pa + in.cols[lo]];
    if (in.prior) v += in.prior[(long)hi * in.n + lo];
    return v;
}

// A = 2^k M + shift I, full and exactly symmetric (lane c writes column c)
FBR_HD void fbr_dopt_gather(const FbrDoptLanes &L, const FbrDoptIn &in, int k, double shift, double *A)
{
#pragma clang fp contract(off)
    const int n = in.n;
    FBR_DOPT_LANES(t)
    for (int c = t; c < n; c += L.nt)
        for (int r = 0; r < n; r++) {
            const double v = ldexp(fbr_dopt_entry(in, r, c), k);
            A[(long)r * n + c] = r == c ? v + shift : v;
        }
    FBR_DOPT_SYNC();
}

// Stage 1 (second half): A -> tridiagonal d [n], e [n - 1].  xs, vs, ps, ws: [n] of shared memory each.  taus ([n] of shared memory, or
// null): the reflectors are kept for fbr_dopt_form_qt -- tau_k in taus[k] (0: H_k = I) and v_k[k + 2 .. n) in row k of A beyond column
// k + 1, which nothing reads after step k (v_k[k + 1] = 1 is implicit).  d and e are the same bits with and without.
FBR_HD void fbr_dopt_tridiagonal(const FbrDoptLanes &L, int n, double *A, double *d, double *e, double *xs, double *vs, double *ps, double *ws,
                                 double *taus = nullptr)
{
#pragma clang fp contract(off)
    for (int k = 0; k + 2 < n; k++) {
        FBR_DOPT_LANES(t)
        for (int j = k + 1 + t; j < n; j += L.nt) xs[j] = A[(long)k * n + j];
        FBR_DOPT_SYNC();
        const double alpha = xs[k + 1];
        double sigma = 0.0;
        for (int j = k + 2; j < n; j++) sigma += xs[j] * xs[j];
        if (!(sigma > 0.0)) {  // the column is already tridiagonal: H = I
            FBR_DOPT_LANES(t)
            if (t == 0) {
                d[k] = A[(long)k * n + k], e[k] = alpha;
                if (taus) taus[k] = 0.0;
            }
            FBR_DOPT_SYNC();
            continue;
        }
        const double beta = -copysign(sqrt(alpha * alpha + sigma), alpha);
        const double tau = (beta - alpha) / beta, sc = 1.0 / (alpha - beta);
        FBR_DOPT_LANES(t)
        {
            for (int j = k + 1 + t; j < n; j += L.nt) vs[j] = j == k + 1 ? 1.0 : xs[j] * sc;
            if (t == 0) {
                d[k] = A[(long)k * n + k], e[k] = beta;
                if (taus) taus[k] = tau;
            }
        }
        FBR_DOPT_SYNC();
        FBR_DOPT_LANES(t)
        for (int i = k + 1 + t; i < n; i += L.nt) {  // p = tau A v: column i of the symmetric A, read as rows
            double s = 0.0;
            for (int j = k + 1; j < n; j++) s += A[(long)j * n + i] * vs[j];
            ps[i] = tau * s;
        }
        FBR_DOPT_SYNC();
        double pv = 0.0;
        for (int j = k + 1; j < n; j++) pv += ps[j] * vs[j];
        const double coef = 0.5 * tau * pv;
        FBR_DOPT_LANES(t)
        for (int i = k + 1 + t; i < n; i += L.nt) ws[i] = ps[i] - coef * vs[i];
        FBR_DOPT_SYNC();
        FBR_DOPT_LANES(t)
        for (int c = k + 1 + t; c < n; c += L.nt) {
            const double wc = ws[c], vc = vs[c];
            for (int r = k + 1; r < n; r++) A[(long)r * n + c] -= vs[r] * wc + ws[r] * vc;  // (a + b == b + a: A stays symmetric)
            if (taus && c >= k + 2) A[(long)k * n + c] = vc;
        }
        FBR_DOPT_SYNC();
    }
    FBR_DOPT_LANES(t)
    if (t == 0) {
        if (n >= 2) d[n - 2] = A[(long)(n - 2) * n + n - 2], e[n - 2] = A[(long)(n - 1) * n + n - 2];
        d[n - 1] = A[(long)(n - 1) * n + n - 1];
    }
    FBR_DOPT_SYNC();
}

// eigenvalues below x of the tridiagonal (d, e2 = e^2)
FBR_HD int fbr_dopt_sturm(int n, const double *d, const double *e2, double pivmin, double x)
{
#pragma clang fp contract(off)
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int cnt = q < 0.0;
    for (int i = 1; i < n; i++) {
        q = d[i] - x - e2[i - 1] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0;
    }
    return cnt;
}

// Stage 2: ascending eigenvalues of (d, e) into ev [n]; e2: [n] of shared memory
FBR_HD void fbr_dopt_bisect(const FbrDoptLanes &L, int n, const double *d, const double *e, double *e2, double *ev)
{
#pragma clang fp contract(off)
    double gl = d[0], gu = d[0], emax2 = 0.0;
    for (int i = 0; i < n; i++) {
        const double r = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < n ? fabs(e[i]) : 0.0);
        gl = fmin(gl, d[i] - r);
        gu = fmax(gu, d[i] + r);
        if (i + 1 < n) emax2 = fmax(emax2, e[i] * e[i]);
    }
    const double tnorm = fmax(fabs(gl), fabs(gu)), pivmin = DBL_MIN * fmax(1.0, emax2);
    const double fudge = 2.1 * tnorm * DBL_EPSILON * n + 4.2 * pivmin;
    gl -= fudge;
    gu += fudge;
    const int nbis = fbr_dopt_halvings(n);
    FBR_DOPT_LANES(t)
    for (int i = t; i + 1 < n; i += L.nt) e2[i] = e[i] * e[i];
    FBR_DOPT_SYNC();
    FBR_DOPT_LANES(t)
    for (int j = t; j < n; j += L.nt) {
        double lo = gl, hi = gu;
        for (int it = 0; it < nbis; it++) {
            const double mid = 0.5 * (lo + hi);
            if (fbr_dopt_sturm(n, d, e2, pivmin, mid) >= j + 1) hi = mid;
            else lo = mid;
        }
        ev[j] = tnorm == 0.0 ? 0.0 : 0.5 * (lo + hi);  // (the zero tridiagonal: exact)
    }
    FBR_DOPT_SYNC();
}

// Stage 3: A (= 2^k M + 2^k delta I, gathered) -> Cmat = -2 scale 2^k A^-1.  ud, c0, c1, ps: [n] of shared memory each.  Returns 0, or
// FBR_DOPT_NOT_POSITIVE with Cmat filled with NaN.
FBR_HD int fbr_dopt_inverse(const FbrDoptLanes &L, int n, int k2, double scale, double *A, double *ud, double *c0, double *c1, double *ps, double *Cmat)
{
#pragma clang fp contract(off)
    // U^T U = A by rows; uc = column k of U above the diagonal, staged a step ahead
    int fail = 0;
    for (int k = 0; k < n; k++) {
        const double *uc = (k & 1) ? c1 : c0;
        double *un = (k & 1) ? c0 : c1;
        FBR_DOPT_LANES(t)
        for (int i = k + t; i < n; i += L.nt) {
            double s = A[(long)k * n + i];
            for (int j = 0; j < k; j++) s -= uc[j] * A[(long)j * n + i];
            ps[i] = s;
        }
        FBR_DOPT_SYNC();
        const double piv = ps[k];
        if (!(piv > 0.0) || !fbr_dopt_finite(piv)) {
            fail = FBR_DOPT_NOT_POSITIVE;
            break;
        }
        const double r = sqrt(piv);
        FBR_DOPT_LANES(t)
        {
            for (int i = k + 1 + t; i < n; i += L.nt) A[(long)k * n + i] = ps[i] / r;
            if (k + 1 < n) {
                for (int j = t; j < k; j += L.nt) un[j] = A[(long)j * n + k + 1];
                if (t == 0) un[k] = ps[k + 1] / r;
            }
            if (t == 0) ud[k] = r;
        }
        FBR_DOPT_SYNC();
    }
    if (fail) {
        FBR_DOPT_LANES(t)
        for (int c = t; c < n; c += L.nt)
            for (int r = 0; r < n; r++) Cmat[(long)r * n + c] = NAN;
        FBR_DOPT_SYNC();
        return fail;
    }
    // W = U^-T (lower, diagonal included; U's diagonal is in ud) row by row: U^T W = I
    for (int i = 0; i < n; i++) {
        const double *uc = (i & 1) ? c1 : c0;  // U[0 .. i - 1][i]
        double *un = (i & 1) ? c0 : c1;
        const double ui = ud[i];
        FBR_DOPT_LANES(t)
        {
            for (int j = t; j <= i; j += L.nt) {
                if (j == i) {
                    A[(long)i * n + i] = 1.0 / ui;
                } else {
                    double s = 0.0;
                    for (int q = j; q < i; q++) s += uc[q] * A[(long)q * n + j];
                    A[(long)i * n + j] = -s / ui;
                }
            }
            if (i + 1 < n)
                for (int q = t; q <= i; q += L.nt) un[q] = A[(long)q * n + i + 1];
        }
        FBR_DOPT_SYNC();
    }
    // A^-1 = W^T W, row a from column a of W (staged a step ahead); both triangles from the same value
    FBR_DOPT_LANES(t)
    for (int q = t; q < n; q += L.nt) c0[q] = A[(long)q * n];
    FBR_DOPT_SYNC();
    for (int a = 0; a < n; a++) {
        const double *wa = (a & 1) ? c1 : c0;
        double *wn = (a & 1) ? c0 : c1;
        FBR_DOPT_LANES(t)
        {
            for (int b = t; b <= a; b += L.nt) {
                double s = 0.0;
                for (int q = a; q < n; q++) s += wa[q] * A[(long)q * n + b];
                const double v = ldexp(-2.0 * scale * s, k2);
                Cmat[(long)a * n + b] = v;
                Cmat[(long)b * n + a] = v;
            }
            if (a + 1 < n)
                for (int q = a + 1 + t; q < n; q += L.nt) wn[q] = A[(long)q * n + a + 1];
        }
        FBR_DOPT_SYNC();
    }
    return 0;
}

// One candidate.  A: [n][n] scratch; sh: FBR_DOPT_SHARED doubles of shared memory; terms [4]; status, eig [n], Cmat [n][n] may be null.
FBR_HD void fbr_dopt_candidate(const FbrDoptLanes &L, const FbrDoptIn &in, double *A, double *sh, double *terms, int *status, double *eig,
                               double *Cmat)
{
#pragma clang fp contract(off)
    const int n = in.n;
    double *d = sh, *e = sh + FBR_MAX_DOPT_COLUMNS, *xs = e + FBR_MAX_DOPT_COLUMNS, *vs = xs + FBR_MAX_DOPT_COLUMNS, *ps = vs + FBR_MAX_DOPT_COLUMNS,
           *ws = ps + FBR_MAX_DOPT_COLUMNS;
    // the largest |M_rc| of the lower triangle and whether every entry is finite: per-lane partials, then every lane folds them alike
    FBR_DOPT_LANES(t)
    {
        double am = 0.0, bad = 0.0;
        for (int r = t; r < n; r += L.nt)
            for (int c = 0; c <= r; c++) {
                const double v = fbr_dopt_entry(in, r, c);
                if (!fbr_dopt_finite(v)) bad = 1.0;
                am = fmax(am, fabs(v));
            }
        ps[t] = am;
        ws[t] = bad;
    }
    FBR_DOPT_SYNC();
    double amax = 0.0;
    bool bad = false;
    for (int t = 0; t < L.nt; t++) {
        amax = fmax(amax, ps[t]);
        bad = bad || ws[t] != 0.0;
    }
    FBR_DOPT_SYNC();  // (ps, ws are written again below)
    if (bad) {
        FBR_DOPT_LANES(t)
        {
            if (t == 0) {
                terms[0] = terms[1] = terms[2] = NAN;
                terms[3] = 0.0;
                if (status) *status = FBR_DOPT_NONFINITE;
            }
            if (eig)
                for (int j = t; j < n; j += L.nt) eig[j] = NAN;
            if (Cmat)
                for (int c = t; c < n; c += L.nt)
                    for (int r = 0; r < n; r++) Cmat[(long)r * n + c] = NAN;
        }
        return;
    }
    int k2 = 0;  // A = 2^k2 M
    if (amax > 0.0) {
        int ex;
        (void)frexp(amax, &ex);
        k2 = 1 - ex;
        if (k2 > 1022) k2 = 1022;  // (a subnormal maximum: as far as a double's exponent goes)
    }
    fbr_dopt_gather(L, in, k2, 0.0, A);
    fbr_dopt_tridiagonal(L, n, A, d, e, xs, vs, ps, ws);
    fbr_dopt_bisect(L, n, d, e, ws, xs);  // xs: the eigenvalues of A
    const double lmax = ldexp(xs[n - 1], -k2), delta = in.reg * fmax(lmax, 1e-30);
    FBR_DOPT_LANES(t)
    {
        if (t == 0) {
            double s = 0.0;
            int nobs = 0;
            for (int i = 0; i < n; i++) {
                const double ev = ldexp(xs[i], -k2);
                s += log(fmax(ev + delta, 1e-300));
                nobs += ev > delta;
            }
            terms[0] = -s, terms[1] = lmax, terms[2] = delta, terms[3] = (double)nobs;
        }
        if (eig)
            for (int j = t; j < n; j += L.nt) eig[j] = ldexp(xs[j], -k2);
    }
    int st = 0;
    if (Cmat) {
        FBR_DOPT_SYNC();  // (xs is read above and written below)
        fbr_dopt_gather(L, in, k2, ldexp(delta, k2), A);
        st = fbr_dopt_inverse(L, n, k2, in.scale, A, d, xs, vs, ps, Cmat);
    }
    FBR_DOPT_LANES(t)
    if (t == 0 && status) *status = st;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Eigenvectors and the observability analysis (fbr_dopt_observability, fbr.h; the reference's trajectory.py:225-264 on the Gram).
//   4. W = Q^T = H_{n-3} .. H_0 from the kept reflectors, one lane per column of W (fbr_dopt_form_qt): T = Q^T A Q, so the eigenvectors of
//      A are the ROWS of Z^T Q^T with Z those of T.  W is stored that way round -- the transpose of LAPACK's Z -- so that a plane rotation
//      of two eigenvectors touches two rows and consecutive lanes sit on consecutive addresses.
//   5. implicit QL with Wilkinson shifts on (d, e) (EISPACK tql2's recurrence, the block found again before every sweep as dsteqr does):
//      lane 0 runs the scalar recurrence of a sweep and stages its rotations in cs, sn; after a barrier lane r applies them to column r of
//      W.  An off-diagonal counts as zero below eps (|d_l| + |e_l|)_max: absolute accuracy eps |A|, which is what the residual is held to;
//      orthogonality is that of a product of rotations, of order n eps also inside clusters.  At most 30 n sweeps in all, a bound fixed
//      before the loop; past it FBR_DOPT_NO_CONVERGENCE and NaN vectors and energy (nothing spins).
//   6. the eigenvalues REPORTED stay those of the bisection, bit for bit what fbr_dopt_terms gives; the pairs of the QL run are ranked
//      ascending (ties by index) and paired with them by index.  Every vector's component of largest magnitude, the first at a tie, is
//      positive.
//   7. lm = max(eig_max, 0), cut = thr^2 lm; index i is unobservable iff max(eig_i, 0) < cut (S_i < thr S_0 with S^2 = max(eig, 0): the
//      zero matrix has nothing unobservable); energy[j] = sum over unobservable i, ascending, of V[j][i]^2; n_observable = n - their
//      number; margin = min_i |eig_i - cut| / cut (+inf when cut = 0).
// The limit of the Gram route: an eigenvalue of M is known to about band(n) eig_max, band(n) = max(128, n) 2^-52 (no smaller than the bar
// the eigenvalues are held to, tests/dopt_reference.py bar_lambda, for every n <= 512), i.e. a singular value of YBase only down to
// sqrt(band) S_0, about 2e-7 S_0.  An eigenvalue within band(n) lm of the cut sets FBR_DOPT_AMBIGUOUS: fp64 Gram arithmetic does not decide
// that index (the numbers are returned all the same), and the entry point refuses thr^2 < 8 band(n).  Agreement with an SVD of YBase for
// singular values between 1e-8 S_0 and the threshold is a property of the Gram, not of this kernel.
// ------------------------------------------------------------------------------------------------------------------------------------
#define FBR_DOPT_AMBIGUOUS 4
#define FBR_DOPT_NO_CONVERGENCE 8
#define FBR_DOPT_OBS_SHARED (9 * FBR_MAX_DOPT_COLUMNS)  // doubles of LDS a workgroup of the observability kernel needs

FBR_HD double fbr_dopt_band(int n) { return (n > 128 ? n : 128) * DBL_EPSILON; }

// sqrt(a^2 + b^2) without overflow, from +, *, /, sqrt alone (the same bits on the host and the device)
FBR_HD double fbr_dopt_pythag(double a, double b)
{
#pragma clang fp contract(off)
    const double x = fabs(a), y = fabs(b), hi = x > y ? x : y, lo = x > y ? y : x;
    if (hi == 0.0) return 0.0;
    const double q = lo / hi;
    return hi * sqrt(1.0 + q * q);
}

// Stage 4: W [n][n] = H_{n-3} .. H_0 from the reflectors fbr_dopt_tridiagonal kept in A and taus.  Lane c owns column c: no barrier inside.
FBR_HD void fbr_dopt_form_qt(const FbrDoptLanes &L, int n, const double *A, const double *taus, double *W)
{
#pragma clang fp contract(off)
    FBR_DOPT_LANES(t)
    for (int c = t; c < n; c += L.nt) {
        for (int r = 0; r < n; r++) W[(long)r * n + c] = r == c ? 1.0 : 0.0;
        for (int k = 0; k + 2 < n; k++) {
            const double tau = taus[k];
            if (tau == 0.0) continue;
            const double *v = A + (long)k * n;
            double s = W[(long)(k + 1) * n + c];
            for (int j = k + 2; j < n; j++) s += v[j] * W[(long)j * n + c];
            s *= tau;
            W[(long)(k + 1) * n + c] -= s;
            for (int j = k + 2; j < n; j++) W[(long)j * n + c] -= v[j] * s;
        }
    }
    FBR_DOPT_SYNC();
}

// Stage 5: implicit QL on (d, e [n], e[n - 1] unused on entry); the rows of W are rotated along: on return row i of W is the eigenvector
// of d[i] (unsorted).  cs, sn, ctl: [n] of shared memory each.  Returns 0 or FBR_DOPT_NO_CONVERGENCE.
FBR_HD int fbr_dopt_ql(const FbrDoptLanes &L, int n, double *d, double *e, double *cs, double *sn, double *ctl, double *W)
{
#pragma clang fp contract(off)
    const int maxit = 30 * n;  // sweeps in all
    int l = 0;                 // (lane 0's: the row being worked on, the sum of the shifts, the running magnitude)
    double f = 0.0, tst1 = 0.0;
    bool fresh = true;
    int fail = 0;
    for (int it = 0; it <= maxit; it++) {
        FBR_DOPT_LANES(t)
        if (t == 0) {
            if (it == 0) e[n - 1] = 0.0;
            int m = l;
            while (l < n) {
                if (fresh) tst1 = fmax(tst1, fabs(d[l]) + fabs(e[l])), fresh = false;
                for (m = l; m < n - 1; m++)
                    if (fabs(e[m]) <= DBL_EPSILON * tst1) break;
                if (m > l) break;
                d[l] += f;
                l++, fresh = true;
            }
            if (l >= n) {
                ctl[0] = -1.0;
            } else if (it == maxit) {
                ctl[0] = -2.0;
            } else {
                // the shift
                double g = d[l], p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = fbr_dopt_pythag(p, 1.0);
                if (p < 0.0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; i++) d[i] -= h;
                f += h;
                // the sweep, from the bottom of the block up
                p = d[m];
                double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; i--) {
                    c3 = c2, c2 = c, s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = fbr_dopt_pythag(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    cs[i] = c, sn[i] = s;
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
                ctl[0] = (double)l, ctl[1] = (double)m;
            }
        }
        FBR_DOPT_SYNC();
        const double c0 = ctl[0];
        if (c0 < 0.0) {
            fail = c0 < -1.5 ? FBR_DOPT_NO_CONVERGENCE : 0;
            break;
        }
        const int lo = (int)c0, hi = (int)ctl[1];
        FBR_DOPT_LANES(t)
        for (int r = t; r < n; r += L.nt) {
            double up = W[(long)hi * n + r];  // row i + 1, as the rotations above it left it
            for (int i = hi - 1; i >= lo; i--) {
                const double c = cs[i], s = sn[i], w = W[(long)i * n + r];
                W[(long)(i + 1) * n + r] = s * w + c * up;
                up = c * w - s * up;
            }
            W[(long)lo * n + r] = up;
        }
        FBR_DOPT_SYNC();
    }
    FBR_DOPT_SYNC();  // (ctl is written again by the caller)
    return fail;
}

struct FbrDoptObsOut {
    int *n_observable;  // [1]
    double *energy;     // [n]
    double *margin;     // [1] or null
    double *eig;        // [n] or null
    double *vec;        // [n][n] or null: vec[j][i] = component j of the eigenvector of eig[i]
    int *status;        // [1] or null
};

// One candidate of fbr_dopt_observability.  A, W: [n][n] scratch each; sh: FBR_DOPT_OBS_SHARED doubles of shared memory.
FBR_HD void fbr_dopt_obs_candidate(const FbrDoptLanes &L, const FbrDoptIn &in, double thr, double *A, double *W, double *sh, const FbrDoptObsOut &o)
{
#pragma clang fp contract(off)
    const int n = in.n;
    double *d = sh, *e = sh + FBR_MAX_DOPT_COLUMNS, *xs = e + FBR_MAX_DOPT_COLUMNS, *vs = xs + FBR_MAX_DOPT_COLUMNS, *ps = vs + FBR_MAX_DOPT_COLUMNS,
           *ws = ps + FBR_MAX_DOPT_COLUMNS, *taus = ws + FBR_MAX_DOPT_COLUMNS, *cs = taus + FBR_MAX_DOPT_COLUMNS, *sn = cs + FBR_MAX_DOPT_COLUMNS;
    // (the scan and the scaling are those of fbr_dopt_candidate, so that eig is bit for bit what fbr_dopt_terms reports)
    FBR_DOPT_LANES(t)
    {
        double am = 0.0, bad = 0.0;
        for (int r = t; r < n; r += L.nt)
            for (int c = 0; c <= r; c++) {
                const double v = fbr_dopt_entry(in, r, c);
                if (!fbr_dopt_finite(v)) bad = 1.0;
                am = fmax(am, fabs(v));
            }
        ps[t] = am;
        ws[t] = bad;
    }
    FBR_DOPT_SYNC();
    double amax = 0.0;
    bool bad = false;
    for (int t = 0; t < L.nt; t++) {
        amax = fmax(amax, ps[t]);
        bad = bad || ws[t] != 0.0;
    }
    FBR_DOPT_SYNC();
    if (bad) {
        FBR_DOPT_LANES(t)
        {
            if (t == 0) {
                *o.n_observable = 0;
                if (o.margin) *o.margin = NAN;
                if (o.status) *o.status = FBR_DOPT_NONFINITE;
            }
            for (int j = t; j < n; j += L.nt) {
                o.energy[j] = NAN;
                if (o.eig) o.eig[j] = NAN;
                if (o.vec)
                    for (int r = 0; r < n; r++) o.vec[(long)r * n + j] = NAN;
            }
        }
        return;
    }
    int k2 = 0;
    if (amax > 0.0) {
        int ex;
        (void)frexp(amax, &ex);
        k2 = 1 - ex;
        if (k2 > 1022) k2 = 1022;
    }
    fbr_dopt_gather(L, in, k2, 0.0, A);
    fbr_dopt_tridiagonal(L, n, A, d, e, xs, vs, ps, ws, taus);
    fbr_dopt_bisect(L, n, d, e, ws, xs);  // xs: the eigenvalues of A, kept to the end
    fbr_dopt_form_qt(L, n, A, taus, W);
    const int fail = fbr_dopt_ql(L, n, d, e, cs, sn, ps, W);
    // rank of every QL eigenvalue (ties by index) -> vs[rank] = its row of W; ws[row] = the sign that makes its largest component positive
    FBR_DOPT_LANES(t)
    for (int i = t; i < n; i += L.nt) {
        const double di = d[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += d[j] < di || (d[j] == di && j < i);
        vs[rank] = (double)i;
        const double *w = W + (long)i * n;
        double big = 0.0, sg = 1.0;
        for (int j = 0; j < n; j++)
            if (fabs(w[j]) > big) big = fabs(w[j]), sg = w[j] < 0.0 ? -1.0 : 1.0;
        ws[i] = sg;
    }
    FBR_DOPT_SYNC();
    const double lmax = ldexp(xs[n - 1], -k2), lm = fmax(lmax, 0.0), cut = thr * thr * lm, band = fbr_dopt_band(n) * lm;
    int nun = 0, amb = 0;
    double mg = INFINITY;
    for (int i = 0; i < n; i++) {
        const double ev = ldexp(xs[i], -k2), dist = fabs(ev - cut);
        nun += fmax(ev, 0.0) < cut;
        if (cut > 0.0) mg = fmin(mg, dist / cut);
        if (dist < band) amb = FBR_DOPT_AMBIGUOUS;
    }
    FBR_DOPT_LANES(t)
    {
        if (t == 0) {
            *o.n_observable = n - nun;
            if (o.margin) *o.margin = mg;
            if (o.status) *o.status = amb | fail;
        }
        for (int j = t; j < n; j += L.nt) {
            double s = 0.0;
            for (int i = 0; i < nun; i++) {
                const double v = W[(long)vs[i] * n + j];
                s += v * v;
            }
            o.energy[j] = fail ? NAN : s;
            if (o.eig) o.eig[j] = ldexp(xs[j], -k2);
            if (o.vec)
                for (int i = 0; i < n; i++) {
                    const int row = (int)vs[i];
                    o.vec[(long)j * n + i] = fail ? NAN : ws[row] * W[(long)row * n + j];
                }
        }
    }
}

#if defined(__HIPCC__)
struct DevDoptObs {
    const double *G;      // [ngroups of the launch][Pa][Pa]
    const double *prior;  // [n][n] or null
    const int *cols;      // [n]
    double *A;            // scratch [ngroups of the launch][2][n][n]
    double *energy, *margin, *eig, *vec;
    int *n_observable, *status;
    int Pa, n;
    double thr;
};

// (a kernel of its own: the terms-only launch below keeps its registers and its 24 KB of LDS)
__global__ __launch_bounds__(256) void fbr_dopt_obs_kernel(DevDoptObs p)
{
    __shared__ double sh[FBR_DOPT_OBS_SHARED];
    const long c = blockIdx.x, n = p.n;
    const FbrDoptLanes L = {(int)threadIdx.x, (int)threadIdx.x + 1, (int)blockDim.x};
    const FbrDoptIn in = {p.G + c * p.Pa * p.Pa, p.Pa, p.n, p.cols, p.prior, 0.0, 1.0};
    const FbrDoptObsOut o = {p.n_observable + c, p.energy + c * n, p.margin ? p.margin + c : nullptr, p.eig ? p.eig + c * n : nullptr,
                             p.vec ? p.vec + c * n * n : nullptr, p.status ? p.status + c : nullptr};
    fbr_dopt_obs_candidate(L, in, p.thr, p.A + 2 * c * n * n, p.A + (2 * c + 1) * n * n, sh, o);
}

struct DevDopt {
    const double *G;      // [ngroups of the launch][Pa][Pa]
    const double *prior;  // [n][n] or null
    const int *cols;      // [n]
    const double *scale;  // [ngroups of the launch] or null
    double *A;            // scratch [ngroups of the launch][n][n]
    double *terms, *eig, *Cmat;
    int *status;
    int Pa, n;
    double reg;
};

__global__ __launch_bounds__(256) void fbr_dopt_kernel(DevDopt p)
{
    __shared__ double sh[FBR_DOPT_SHARED];
    const long c = blockIdx.x, n = p.n;
    const FbrDoptLanes L = {(int)threadIdx.x, (int)threadIdx.x + 1, (int)blockDim.x};
    const FbrDoptIn in = {p.G + c * p.Pa * p.Pa, p.Pa, p.n, p.cols, p.prior, p.reg, p.scale ? p.scale[c] : 1.0};
    fbr_dopt_candidate(L, in, p.A + c * n * n, sh, p.terms + 4 * c, p.status ? p.status + c : nullptr, p.eig ? p.eig + c * n : nullptr,
                       p.Cmat ? p.Cmat + c * n * n : nullptr);
}
#endif
