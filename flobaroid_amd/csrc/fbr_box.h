// fbr_box.h -- oriented-box collision distances of candidate trajectories (fbr_candidate_box_distances).
//
// Covers the pairs of the trajectory optimiser's collision block that its capsule routine does not serve and that need no mesh: every pair
// of collisionMode "box", and in collisionMode "capsule" every pair with a world link or a capsule-less robot link
// (excitation/trajectoryOptimizer.py "check collision constraints": fcl.distance on the boxes of optimizer.py _getLinkCollisionGeometry).
// A box is a rotation (columns: the box axes), a centre and three half extents.  fbr_box_distance returns
//   * the largest gap over the 15 separating axes when that is <= 0 (the boxes touch or overlap: the negated minimum translation), else
//   * the exact Euclidean distance: the minimum over vertices of one box against the other (solid) box and over the 144 edge pairs.
// The reference's FCL returns a GJK distance (tolerance 1e-6) when separated and a build-dependent negative number when not: the sign
// agrees, the value is unpinned there ("box distances").
//
// Two kernels and the capsules' finishing pass:
//   fbr_box_frames_kernel  one lane per CHECKED sample: the positions-only walk of fbr_capsule.h, R | centre of every robot-link box written
//                          lane-interleaved to a device temporary [block][box][12][64];
//   fbr_box_pairs_kernel   one wave per (block of 64 checked samples, batch of FBR_BOX_BATCH pairs), one lane per sample; a world box is a
//                          constant of the set read with scalar loads; the 64 distances of a pair staged in the LDS and scanned in sample
//                          order (strict <: the first sample wins a tie, a NaN never wins);
//   fbr_capsule_finish_kernel  unchanged.
//
// fbr_box_distance is HIP-free: tests/emul/box_emul.cpp compiles the same text with g++.
#pragma once
#include "fbr_capsule.h"

#define FBR_BOX_PARALLEL 1e-12  // |a_i x b_j|^2 below this: the cross axis is skipped, the edge pair takes s = 0

// (x0, x1, x2) <- (x1, x2, x0): the loops below stay rolled and always work on axis 0 -- no register array is indexed by a loop counter
#define FBR_BOX_ROT(x0, x1, x2) \
    {                           \
        const double r_ = x0;   \
        x0 = x1;                \
        x1 = x2;                \
        x2 = r_;                \
    }

// Signed distance of the boxes (RA, cA, hA) and (RB, cB, hB): R [9] row-major, its columns the box axes (orthonormal); c [3] the centre;
// h [3] the half extents (positive).  A NaN or an infinity among the inputs gives a NaN.
FBR_HD double fbr_box_distance(const double *RA, const double *cA, const double *hA_, const double *RB, const double *cB, const double *hB_)
{
    // B in the frame of A: C_ij = a_i . b_j, t = RA^T (cB - cA).  A is then the axis-aligned box [-hA, hA].
    const double d0 = cB[0] - cA[0], d1 = cB[1] - cA[1], d2 = cB[2] - cA[2];
    double t0 = RA[0] * d0 + RA[3] * d1 + RA[6] * d2, t1 = RA[1] * d0 + RA[4] * d1 + RA[7] * d2, t2 = RA[2] * d0 + RA[5] * d1 + RA[8] * d2;
    double C00 = RA[0] * RB[0] + RA[3] * RB[3] + RA[6] * RB[6], C01 = RA[0] * RB[1] + RA[3] * RB[4] + RA[6] * RB[7],
           C02 = RA[0] * RB[2] + RA[3] * RB[5] + RA[6] * RB[8];
    double C10 = RA[1] * RB[0] + RA[4] * RB[3] + RA[7] * RB[6], C11 = RA[1] * RB[1] + RA[4] * RB[4] + RA[7] * RB[7],
           C12 = RA[1] * RB[2] + RA[4] * RB[5] + RA[7] * RB[8];
    double C20 = RA[2] * RB[0] + RA[5] * RB[3] + RA[8] * RB[6], C21 = RA[2] * RB[1] + RA[5] * RB[4] + RA[8] * RB[7],
           C22 = RA[2] * RB[2] + RA[5] * RB[5] + RA[8] * RB[8];
    double hA0 = hA_[0], hA1 = hA_[1], hA2 = hA_[2], hB0 = hB_[0], hB1 = hB_[1], hB2 = hB_[2];
    const double chk = ((t0 + t1 + t2) + (C00 + C01 + C02) + (C10 + C11 + C12) + (C20 + C21 + C22)) + ((hA0 + hA1 + hA2) + (hB0 + hB1 + hB2));
    if (!(chk - chk == 0.0)) return chk - chk;  // (a NaN pose never wins a minimum)

    // ---- the 15 separating axes: gap = max over the axes of |ax . t| - r_A(ax) - r_B(ax)
    double gap = -1e300;
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        {  // the face normal a_0
            const double g = fabs(t0) - hA0 - (fabs(C00) * hB0 + fabs(C01) * hB1 + fabs(C02) * hB2);
            gap = g > gap ? g : gap;
        }
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            if (i == 0) {  // the face normal b_0
                const double g = fabs(t0 * C00 + t1 * C10 + t2 * C20) - hB0 - (hA0 * fabs(C00) + hA1 * fabs(C10) + hA2 * fabs(C20));
                gap = g > gap ? g : gap;
            }
            // a_0 x b_0 = (0, -C20, C10) in A's frame; its products with the other axes are entries of C (both frames are orthonormal)
            const double len2 = C10 * C10 + C20 * C20;
            if (len2 >= FBR_BOX_PARALLEL) {
                const double g = (fabs(t2 * C10 - t1 * C20) - (hA1 * fabs(C20) + hA2 * fabs(C10)) - (hB1 * fabs(C02) + hB2 * fabs(C01))) / sqrt(len2);
                gap = g > gap ? g : gap;
            }
            FBR_BOX_ROT(C00, C01, C02)  // the axes of B, one on
            FBR_BOX_ROT(C10, C11, C12)
            FBR_BOX_ROT(C20, C21, C22)
            FBR_BOX_ROT(hB0, hB1, hB2)
        }
        FBR_BOX_ROT(C00, C10, C20)  // the axes of A, one on
        FBR_BOX_ROT(C01, C11, C21)
        FBR_BOX_ROT(C02, C12, C22)
        FBR_BOX_ROT(t0, t1, t2)
        FBR_BOX_ROT(hA0, hA1, hA2)
    }
    if (gap <= 0.0) return gap;

    // ---- separated: the smallest squared distance over the feature pairs
    double best = 1e300;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {  // the vertices of B against the solid A
        const double s0 = (k & 1) ? hB0 : -hB0, s1 = (k & 2) ? hB1 : -hB1, s2 = (k & 4) ? hB2 : -hB2;
        double e0 = fabs(t0 + (C00 * s0 + C01 * s1 + C02 * s2)) - hA0, e1 = fabs(t1 + (C10 * s0 + C11 * s1 + C12 * s2)) - hA1,
               e2 = fabs(t2 + (C20 * s0 + C21 * s1 + C22 * s2)) - hA2;
        e0 = e0 > 0.0 ? e0 : 0.0;
        e1 = e1 > 0.0 ? e1 : 0.0;
        e2 = e2 > 0.0 ? e2 : 0.0;
        const double dd = e0 * e0 + e1 * e1 + e2 * e2;
        best = dd < best ? dd : best;
    }
#pragma unroll 1
    for (int k = 0; k < 8; k++) {  // the vertices of A against the solid B
        const double w0 = ((k & 1) ? hA0 : -hA0) - t0, w1 = ((k & 2) ? hA1 : -hA1) - t1, w2 = ((k & 4) ? hA2 : -hA2) - t2;
        double e0 = fabs(w0 * C00 + w1 * C10 + w2 * C20) - hB0, e1 = fabs(w0 * C01 + w1 * C11 + w2 * C21) - hB1,
               e2 = fabs(w0 * C02 + w1 * C12 + w2 * C22) - hB2;
        e0 = e0 > 0.0 ? e0 : 0.0;
        e1 = e1 > 0.0 ? e1 : 0.0;
        e2 = e2 > 0.0 ? e2 : 0.0;
        const double dd = e0 * e0 + e1 * e1 + e2 * e2;
        best = dd < best ? dd : best;
    }
    // The 144 edge pairs, by the 9 pairs of directions (a_0, b_0): an edge of A runs from (-hA0, +-hA1, +-hA2) along 2 hA0 e_0, an edge of B
    // from t - hB0 b_0 +- hB1 b_1 +- hB2 b_2 along 2 hB0 b_0.  Segment against segment with clamping (Ericson 5.1.9) WITHOUT the thresholds
    // of fbr_segment_distance; (nearly) parallel directions take s = 0 and the clamp of t -- any (s, t) in the unit square is a distance
    // between points of the two boxes, and the closest points of parallel edges include a vertex, which the loops above have seen.
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
#pragma unroll 1
        for (int j = 0; j < 3; j++) {
            const double u0 = 2.0 * hB0 * C00, u1 = 2.0 * hB0 * C10, u2 = 2.0 * hB0 * C20, la = 2.0 * hA0;
            const double a = la * la, e = u0 * u0 + u1 * u1 + u2 * u2, b = la * u0, den = a * e - b * b;
            const bool par = !(den > FBR_BOX_PARALLEL * (a * e));
            const double ia = 1.0 / a, ie = 1.0 / e, iden = par ? 0.0 : 1.0 / den;
            const double m0 = t0 - hB0 * C00, m1 = t1 - hB0 * C10, m2 = t2 - hB0 * C20;
#pragma unroll 1
            for (int k = 0; k < 16; k++) {
                const double sa = (k & 1) ? hA1 : -hA1, sb = (k & 2) ? hA2 : -hA2, sc = (k & 4) ? hB1 : -hB1, sd = (k & 8) ? hB2 : -hB2;
                const double r0 = -hA0 - (m0 + (sc * C01 + sd * C02)), r1 = sa - (m1 + (sc * C11 + sd * C12)), r2 = sb - (m2 + (sc * C21 + sd * C22));
                const double c = la * r0, f = u0 * r0 + u1 * r1 + u2 * r2;
                double s = par ? 0.0 : fbr_clip01((b * f - c * e) * iden);
                double tt = (b * s + f) * ie;
                if (tt < 0.0) {
                    tt = 0.0;
                    s = fbr_clip01(-c * ia);
                } else if (tt > 1.0) {
                    tt = 1.0;
                    s = fbr_clip01((b - c) * ia);
                }
                const double v0 = (r0 + s * la) - tt * u0, v1 = r1 - tt * u1, v2 = r2 - tt * u2;
                const double dd = v0 * v0 + v1 * v1 + v2 * v2;
                best = dd < best ? dd : best;
            }
            FBR_BOX_ROT(C00, C01, C02)
            FBR_BOX_ROT(C10, C11, C12)
            FBR_BOX_ROT(C20, C21, C22)
            FBR_BOX_ROT(hB0, hB1, hB2)
        }
        FBR_BOX_ROT(C00, C10, C20)
        FBR_BOX_ROT(C01, C11, C21)
        FBR_BOX_ROT(C02, C12, C22)
        FBR_BOX_ROT(t0, t1, t2)
        FBR_BOX_ROT(hA0, hA1, hA2)
    }
    return sqrt(best);
}

// centre of a robot-link box: mode 0: p + c (the offset added in world axes: the reference's Transform(rot, pos + offset)); 1: p + R c
FBR_HD void fbr_box_centre(int mode, const double *R, const double *p, const double *c, double *w)
{
    if (mode) {
        fbr_capsule_point(R, p, c, w);
    } else {
        for (int i = 0; i < 3; i++) w[i] = p[i] + c[i];
    }
}

#if defined(__HIPCC__)
#define FBR_BOX_BATCH 16  // pairs whose 64 distances a wave stages in the LDS: 8.3 KB a wave, the LDS never holds fewer waves than the registers

struct DevBoxes {
    int nsteps, nslots, nrob, nworld, npairs, cmode;
    const int *steps;     // [nsteps][FBR_KINID_STEP]
    const int *boxbeg;    // [nsteps + 1] robot-box slots of every step
    const int *boxid;     // [nrob] slot -> robot-box number (the caller's order among the boxes with a link)
    const double *cen;    // [nrob][3] centre in the link frame, by slot
    const double *half;   // [nrob][3] half extents, by robot-box number
    const double *world;  // [nworld][15] R | centre | half extents of the world boxes
    const int2 *pairs;    // [npairs] each entry: a robot-box number, or -1 - (world-box number)
};

#if defined(FBR_KERNELS_COLLISION)
// blocks [blk0, blk0 + nb) of the tiling; fr [nb][nrob][12][64]: R (row-major) | centre; the other arguments as for fbr_capsule_points_kernel
// (The walk is fbr_capsule_points_kernel's, written out a second time: on a shared body this kernel measured 2 % slower on a 9-link
// robot on an MI355X -- DESIGN.md, "collision layout".)
__global__ __launch_bounds__(64) void fbr_box_frames_kernel(DevModel m, DevBoxes bx, DevCapTiles tl, long blk0, long nb, int stage, int ldn,
                                                            const double *__restrict__ q, const double *__restrict__ rpy,
                                                            const double *__restrict__ bpos, double *__restrict__ fr, double *__restrict__ scratch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x, n = m.n;
    double *scr = scratch + (long)blockIdx.x * bx.nslots * 12 * 64 + lane;
    for (long b = blockIdx.x; b < nb; b += gridDim.x) {
        const long blk = blk0 + b, c = blk / tl.tiles, i0 = (blk - c * tl.tiles) << 6;
        const int valid = (int)min(64L, tl.Tc - i0);
        if (stage) {
            __syncthreads();  // (the block before has read its rows)
            for (int i = lane; i < valid * n; i += 64) {
                const int r = i / n, d = i - r * n;
                smem[r * ldn + d] = q[(c * tl.T + (i0 + r) * tl.step) * n + d];
            }
            __syncthreads();
        }
        const int ls = min(lane, valid - 1);  // lanes behind the last checked sample repeat it and store nothing
        const long s = c * tl.T + (i0 + ls) * tl.step;
        const bool live = lane < valid;
        const double *myq = stage ? smem + ls * ldn : q + s * n;
        double *out = fr + b * (long)bx.nrob * 12 * 64 + lane;
        auto qf = [&](int d) { return myq[d]; };
        auto basef = [&](double *e3, double *b3) {
            for (int i = 0; i < 3; i++) {
                e3[i] = rpy ? rpy[s * 3 + i] : 0.0;
                b3[i] = bpos ? bpos[s * 3 + i] : 0.0;
            }
        };
        auto save = [&](int sl, int i, double v) { scr[(sl * 12 + i) * 64] = v; };
        auto load = [&](int sl, int i) { return scr[(sl * 12 + i) * 64]; };
        auto consts = [&](int l, double *rR, double *rp, double *ax) {  // (l is wave-uniform: scalar loads through the constant address space)
            const fbr_cdouble_ptr cR = (fbr_cdouble_ptr)(unsigned long)m.restR, cq = (fbr_cdouble_ptr)(unsigned long)m.restp,
                                  ca = (fbr_cdouble_ptr)(unsigned long)m.axis;
            for (int i = 0; i < 9; i++) rR[i] = cR[9 * l + i];
            for (int i = 0; i < 3; i++) {
                rp[i] = cq[3 * l + i];
                ax[i] = ca[3 * l + i];
            }
        };
        auto box = [&](int bs, const double *R, const double *p) {
            const fbr_cdouble_ptr cc = (fbr_cdouble_ptr)(unsigned long)(bx.cen + 3 * bs);
            const int id = FBR_UNI(((fbr_cint_ptr)(unsigned long)bx.boxid)[bs]);
            const double cl[3] = {cc[0], cc[1], cc[2]};
            double w[3];
            fbr_box_centre(bx.cmode, R, p, cl, w);
            if (live) {
                for (int i = 0; i < 9; i++) out[((long)id * 12 + i) * 64] = R[i];
                for (int i = 0; i < 3; i++) out[((long)id * 12 + 9 + i) * 64] = w[i];
            }
        };
        fbr_capsule_lane(bx.nsteps, bx.steps, bx.boxbeg, m.floating && rpy != nullptr, qf, basef, save, load, consts, box);
    }
}

// one box of a pair into registers: id >= 0: robot box `id` of this lane's sample; id < 0: world box -1 - id (wave-uniform loads)
__device__ __forceinline__ void fbr_box_fetch(const DevBoxes &bx, int id, const double *f, double *R, double *c, double *h)
{
    if (id >= 0) {
        for (int i = 0; i < 9; i++) R[i] = f[((long)id * 12 + i) * 64];
        for (int i = 0; i < 3; i++) c[i] = f[((long)id * 12 + 9 + i) * 64];
        const fbr_cdouble_ptr hh = (fbr_cdouble_ptr)(unsigned long)(bx.half + 3 * id);
        for (int i = 0; i < 3; i++) h[i] = hh[i];
    } else {
        const fbr_cdouble_ptr w = (fbr_cdouble_ptr)(unsigned long)(bx.world + 15 * (long)(-1 - id));
        for (int i = 0; i < 9; i++) R[i] = w[i];
        for (int i = 0; i < 3; i++) {
            c[i] = w[9 + i];
            h[i] = w[12 + i];
        }
    }
}

// work items (block, batch of FBR_BOX_BATCH pairs), one wave each; pval / pidx [nb][npairs] as for fbr_capsule_pairs_kernel
__global__ __launch_bounds__(64) void fbr_box_pairs_kernel(DevBoxes bx, DevCapTiles tl, long blk0, long nb, const double *__restrict__ fr,
                                                           double *__restrict__ pval, long *__restrict__ pidx)
{
    __shared__ double sd[FBR_BOX_BATCH * 65];
    const int lane = threadIdx.x;
    const long nbatch = (bx.npairs + FBR_BOX_BATCH - 1) / FBR_BOX_BATCH, items = nb * nbatch;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrPairItem w = fbr_pair_item(it, nbatch, FBR_BOX_BATCH, bx.npairs, tl, blk0);
        const double *f = fr + w.b * (long)bx.nrob * 12 * 64 + lane;  // (lanes behind the last checked sample read what an earlier call left: never scanned)
        int cura = 0;
        bool have = false;
        double RA[9], cA[3], hA[3];
        for (int i = 0; i < 9; i++) RA[i] = 0.0;
        for (int i = 0; i < 3; i++) cA[i] = hA[i] = 0.0;
        __syncthreads();  // (the item before has been scanned)
#pragma unroll 1
        for (int j = 0; j < w.cnt; j++) {
            const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(bx.pairs + w.k0 + j);
            const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
            if (!have || ia != cura) {  // (pair lists come sorted by their first box: it stays in registers)
                fbr_box_fetch(bx, ia, f, RA, cA, hA);
                cura = ia;
                have = true;
            }
            double RB[9], cB[3], hB[3];
            fbr_box_fetch(bx, ib, f, RB, cB, hB);
            sd[j * 65 + lane] = fbr_box_distance(RA, cA, hA, RB, cB, hB);
        }
        __syncthreads();
        fbr_pair_scan_store(sd, w, lane, tl, bx.npairs, [](int k) { return k; }, pval, pidx);
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
