// fbr_weights.h -- D-optimality weight rows W = Y[:, cols] . C_g of the analytical trajectory gradient (fbr_regressor_weights, fbr.h).
//
// The reference forms W_std = R_dopt Pb^T on the host from the stacked YBase of ONE trajectory (excitation/analyticalGradient.py:538-565)
// and hands its rows to the finite-difference workers.  With YBase = Y[:, cols] Pb (or Y B) that product is Y[:, cols] . C with a constant
// ncols x ncols matrix per candidate, C = -2 scale Pb (Pb^T G Pb + delta I)^-1 Pb^T: a tall-skinny fp64 GEMM whose left operand the
// regressor kernel has just written into the caller's W buffer.  This kernel transforms that buffer IN PLACE, one row tile at a time.
//
// Tiling.  The stacked rows of a launch are global rows [R0, R1) of the S * rows regressor rows; group g owns rows [g Rg, (g + 1) Rg).  Row
// tiles of TM = 16 MT rows start at the beginning of every group segment of the launch, so a tile never mixes two groups (two matrices C)
// and the last tile of a segment is masked.  One workgroup (4 waves) per tile, one-dimensional grid:
//   1. the tile's rows of Y[:, cols] are gathered into the LDS, [TM][ldk], zero padded to a multiple of 4 columns and to TM rows.  ldk / 4 is
//      odd, so the 16 rows x 4 k-columns of an A operand read fall on all 32 bank pairs (2 lanes per bank pair: the minimum for 512 bytes);
//   2. barrier: from here on nothing reads W of this tile any more -- what makes in place safe (tiles own disjoint rows);
//   3. the columns NOT selected are overwritten with exact zeros;
//   4. wave w takes the column tiles w, w + 4, ... of the result (N tiling: C_g never has to fit the LDS -- WALK-MAN's 213 x 213 matrix is
//      363 KB -- its B operands are read straight from global memory, 16 consecutive doubles per k row, and stay in the L2 for the other
//      tiles of the group), runs ceil(ncols / 4) k-steps of v_mfma_f64_16x16x4_f64 on MT accumulators that share each B operand, and
//      scatters the 16 x 16 results to W[:, cols].  k and column remainders (213 = 53 * 4 + 1 = 13 * 16 + 5) are masked to zero operands.
// Operand maps of the instruction (lane l): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D[i = (l >> 4) + 4 reg][j = l & 15].
// A row of the result depends on nothing but its own row of Y and C_g, accumulated over k in ascending order: the bits do not depend on the
// tiling, the chunking or the run.
#pragma once

struct DevWeights {
    long R0, R1;  // global regressor rows [R0, R1) of this launch; W points at row R0
    long Rg;      // rows per group
    long t0, tpg; // tiles of the launch's first group segment (it may start inside a group), tiles of a whole group
    int P, ncols, ldk;
    int nunsel;
    const int *cols;   // [ncols], nullptr: every column
    const int *unsel;  // [nunsel] the columns that are not selected
    const double *C;   // [ngroups][ncols][ncols]
};

// LDS row stride of the staged tile: ncols rounded up to a multiple of 4 whose quarter is odd
static inline int fbr_weights_ldk(int ncols)
{
    const int k4 = (ncols + 3) / 4;
    return 4 * (k4 | 1);
}
#define FBR_WEIGHTS_MAX_LDS (150 * 1024)  // one 16-row tile must fit: ncols <= 1196
// row sub-tiles per workgroup: the largest of 4, 2, 1 whose tile leaves room for two workgroups per CU (72 KB each); 0: over the limit
static inline int fbr_weights_mt(int ncols)
{
    const size_t row16 = (size_t)16 * fbr_weights_ldk(ncols) * sizeof(double);
    for (int mt = 4; mt >= 1; mt >>= 1)
        if (row16 * mt <= (size_t)72 * 1024) return mt;
    return row16 <= (size_t)FBR_WEIGHTS_MAX_LDS ? 1 : 0;
}
// tiles of a launch over rows [R0, R1) (fills t0 / tpg)
static inline long fbr_weights_tiles(DevWeights *w, int mt)
{
    const long TM = 16L * mt, g0 = w->R0 / w->Rg;
    const long e0 = std::min(w->R1, (g0 + 1) * w->Rg);
    w->t0 = (e0 - w->R0 + TM - 1) / TM;
    w->tpg = (w->Rg + TM - 1) / TM;
    long tiles = w->t0;
    if (w->R1 > e0) {
        const long nfull = (w->R1 - e0) / w->Rg, rem = (w->R1 - e0) - nfull * w->Rg;
        tiles += nfull * w->tpg + (rem + TM - 1) / TM;
    }
    return tiles;
}

#if defined(__HIPCC__) && defined(FBR_KERNELS_CORE)
typedef double fbr_w4 __attribute__((ext_vector_type(4)));

template <int MT> __global__ __launch_bounds__(256) void fbr_weights_kernel(DevWeights p, double *__restrict__ W)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];  // [16 MT][ldk]
    constexpr int TM = 16 * MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x, g0 = p.R0 / p.Rg;
    long g, r0;
    if (b < p.t0) {
        g = g0;
        r0 = p.R0 + b * TM;
    } else {
        const long bb = b - p.t0;
        g = g0 + 1 + bb / p.tpg;
        r0 = g * p.Rg + (bb % p.tpg) * TM;
    }
    const long r1 = min(p.R1, (g + 1) * p.Rg);
    if (r0 >= r1) return;  // (never: the host counts exactly the tiles that hold rows)
    const int nr = (int)min((long)TM, r1 - r0), ncols = p.ncols, ldk = p.ldk, P = p.P;
    double *Wt = W + (r0 - p.R0) * (long)P;
    const int k4 = 4 * ((ncols + 3) >> 2);
    for (int i = tid; i < TM * k4; i += 256) {
        const int r = i / k4, k = i - r * k4;
        double v = 0.0;
        if (r < nr && k < ncols) v = Wt[(long)r * P + (p.cols ? p.cols[k] : k)];
        smem[r * ldk + k] = v;
    }
    __syncthreads();
    for (int i = tid; i < nr * p.nunsel; i += 256) {
        const int r = i / p.nunsel, u = i - r * p.nunsel;
        Wt[(long)r * P + p.unsel[u]] = 0.0;
    }
    const double *__restrict__ Cg = p.C + g * (long)ncols * ncols;
    const int li = lane & 15, kq = lane >> 4, NT = (ncols + 15) >> 4, KS = k4 >> 2;
    for (int nt = wave; nt < NT; nt += 4) {
        const int j = 16 * nt + li;
        const bool jok = j < ncols;
        fbr_w4 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) acc[mt] = (fbr_w4){0.0, 0.0, 0.0, 0.0};
        const double *cb = Cg + j;
        const double *ab = smem + li * ldk + kq;
        int ks = 0;
        for (; ks + 4 <= KS; ks += 4) {  // four B operands in flight before their MFMAs
            double bv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int k = 4 * (ks + u) + kq;
                bv[u] = (jok && k < ncols) ? cb[(long)k * ncols] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ab[mt * 16 * ldk + 4 * (ks + u)], bv[u], acc[mt], 0, 0, 0);
        }
        for (; ks < KS; ks++) {
            const int k = 4 * ks + kq;
            const double bv = (jok && k < ncols) ? cb[(long)k * ncols] : 0.0;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ab[mt * 16 * ldk + 4 * ks], bv, acc[mt], 0, 0, 0);
        }
        if (jok) {
            const int co = p.cols ? p.cols[j] : j;
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int r = 16 * mt + kq + 4 * reg;
                    if (r < nr) Wt[(long)r * P + co] = acc[mt][reg];
                }
        }
    }
}
#endif
