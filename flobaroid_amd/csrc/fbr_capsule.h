// fbr_capsule.h -- capsule collision distances of candidate trajectories (fbr_candidate_capsule_distances).
//
// Replaces the collision block of the trajectory optimiser's objective in its capsule mode (excitation/trajectoryOptimizer.py "check collision
// constraints": per checked sample one setRobotState, per link pair one Python call of excitation/capsule.py capsule_distance).  A capsule is a
// segment in a link's frame plus a radius; the distance of two capsules is the closed-form distance of their segments (Ericson, Real-Time
// Collision Detection 5.1.9) minus the radii.
//
// Two kernels and a finishing pass ("capsule distances"):
//   fbr_capsule_points_kernel  one lane per CHECKED sample: walks the tree parents first composing R_l, p_l only (no velocities, no
//                              accelerations), transforms the capsule endpoints and writes them lane-interleaved to a device temporary
//                              [block][capsule][6][64] (512-byte coalesced lines, like the branch-point scratch of fbr_kinid.h);
//   fbr_capsule_pairs_kernel   one wave per (block of 64 checked samples, batch of 32 pairs), one lane per sample: the segment routine per pair,
//                              the 64 distances of a pair staged in the LDS, then one lane per pair scans them in sample order (strict <: the
//                              first sample wins a tie, a NaN never wins) and writes the block's partial (value, index);
//   fbr_capsule_finish_kernel  the partials of a candidate's blocks reduced in block order (no atomics: the same bits every run).
// A block of 64 checked samples never spans two candidates.
//
// The arithmetic (fbr_segment_distance, fbr_pose_base / fbr_pose_child, fbr_capsule_lane) is HIP-free: tests/emul/capsule_emul.cpp compiles
// the same text with g++ and the tests hold it against the reference's recorded outputs.
#pragma once
#include "fbr_kinid.h"
#include "fbr_math.h"

// np.clip(x, 0, 1) (a NaN stays a NaN)
FBR_HD double fbr_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// Distance of the segments A(s) = a0 + s (a1 - a0) and B(t) = b0 + t (b1 - b0), s, t in [0, 1], and the parameters of the closest points --
// the reference's segment_segment_distance (excitation/capsule.py) branch for branch: the distance jumps where a squared length or
// a e - b^2 crosses 1e-10, so the thresholds, the s = 0 of parallel segments and the clamp-and-recompute of t are part of the function.
FBR_HD double fbr_segment_distance(const double *a0, const double *a1, const double *b0, const double *b1, double *s_out, double *t_out)
{
    const double EPSILON = 1e-10;
    double d1[3], d2[3], r[3];
    for (int i = 0; i < 3; i++) {
        d1[i] = a1[i] - a0[i];
        d2[i] = b1[i] - b0[i];
        r[i] = a0[i] - b0[i];
    }
    const double a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
    const double e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
    const double f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
    double s, t;
    if (a <= EPSILON && e <= EPSILON) {  // both segments are points
        *s_out = 0.0;
        *t_out = 0.0;
        return sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    if (a <= EPSILON) {  // A is a point
        s = 0.0;
        t = fbr_clip01(f / e);
    } else {
        const double c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
        if (e <= EPSILON) {  // B is a point
            t = 0.0;
            s = fbr_clip01(-c / a);
        } else {
            const double b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
            const double denom = a * e - b * b;
            // not parallel: the point of line A closest to line B, clamped to the segment; parallel: s = 0
            s = denom > EPSILON ? fbr_clip01((b * f - c * e) / denom) : 0.0;
            t = (b * s + f) / e;  // the point of line B closest to A(s)
            if (t < 0.0) {
                t = 0.0;
                s = fbr_clip01(-c / a);
            } else if (t > 1.0) {
                t = 1.0;
                s = fbr_clip01((b - c) / a);
            }
        }
    }
    double dd = 0.0;
    for (int i = 0; i < 3; i++) {
        const double v = (a0[i] + s * d1[i]) - (b0[i] + t * d2[i]);
        dd += v * v;
    }
    *s_out = s;
    *t_out = t;
    return sqrt(dd);
}

// Pose of the base link: world_T_base = Transform(RPY(rpy).inverse(), base_position) (the reference's setCollisionRobotState); fixed base:
// identity.  R as fbr_kin_base forms it.
FBR_HD void fbr_pose_base(int floating, const double *rpy, const double *bpos, double *R, double *p)
{
    if (floating) {
        const double cr = cos(rpy[0]), sr = sin(rpy[0]);
        const double cp = cos(rpy[1]), sp = sin(rpy[1]);
        const double cy = cos(rpy[2]), sy = sin(rpy[2]);
        R[0] = cy * cp;
        R[3] = cy * sp * sr - sy * cr;
        R[6] = cy * sp * cr + sy * sr;
        R[1] = sy * cp;
        R[4] = sy * sp * sr + cy * cr;
        R[7] = sy * sp * cr - cy * sr;
        R[2] = -sp;
        R[5] = cp * sr;
        R[8] = cp * cr;
        for (int i = 0; i < 3; i++) p[i] = bpos[i];
    } else {
        R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
        p[0] = p[1] = p[2] = 0.0;
    }
}

// Pose of a child link from its parent's: the orientation and origin of fbr_kin_child (the same expressions), nothing else.
// jt: 0 fixed, 1 revolute about `s` (unit, child frame) by q, 2 prismatic along `s` by q.
FBR_HD void fbr_pose_child(const double *Rp, const double *pp, const double *restR, const double *r0, const double *s, int jt, double q,
                           double *R, double *p)
{
    double Rj[9], r[3] = {r0[0], r0[1], r0[2]};
    if (jt == 1) {
        const double c = cos(q), sn = sin(q), v = 1.0 - c;
        double Rq[9];
        Rq[0] = c + s[0] * s[0] * v;
        Rq[1] = s[0] * s[1] * v - s[2] * sn;
        Rq[2] = s[0] * s[2] * v + s[1] * sn;
        Rq[3] = s[1] * s[0] * v + s[2] * sn;
        Rq[4] = c + s[1] * s[1] * v;
        Rq[5] = s[1] * s[2] * v - s[0] * sn;
        Rq[6] = s[2] * s[0] * v - s[1] * sn;
        Rq[7] = s[2] * s[1] * v + s[0] * sn;
        Rq[8] = c + s[2] * s[2] * v;
        fbr_mm(restR, Rq, Rj);
    } else {
        for (int i = 0; i < 9; i++) Rj[i] = restR[i];
        if (jt == 2) {
            double sp[3];
            fbr_mv(restR, s, sp);
            for (int i = 0; i < 3; i++) r[i] += sp[i] * q;
        }
    }
    fbr_mm(Rp, Rj, R);
    double t[3];
    fbr_mv(Rp, r, t);
    for (int i = 0; i < 3; i++) p[i] = pp[i] + t[i];
}

// world point of a point given in a link's frame: both endpoints of a capsule go through this one expression, so that a sphere
// (p0 == p1) has a squared length of exactly 0
FBR_HD void fbr_capsule_point(const double *R, const double *p, const double *local, double *w)
{
    fbr_mv(R, local, w);
    for (int i = 0; i < 3; i++) w[i] += p[i];
}

// One lane = one checked sample: the step program of fbr_kinid_build (entries link, psrc, psave, jtype, dof of every step) walked for the
// poses only.  QFn(d): position of dof d; BaseFn(rpy3, pos3): base pose inputs (floating base); save(b, i, v) / load(b, i): slot b of the
// branch-point poses (12 doubles: R, p); ConstFn(l, restR, restp, axis); CapFn(c, R, p): capsule slot c (capsules sorted by the step of
// their link, capbeg [nsteps + 1]) sits on the link whose pose is (R, p).
template <class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class CapFn>
FBR_HD void fbr_capsule_lane(int nsteps, const int *steps, const int *capbeg, int floating, QFn qf, BaseFn basef, SlotSave save, SlotLoad load,
                             ConstFn consts, CapFn cap)
{
    double P[12];
    for (int i = 0; i < 12; i++) P[i] = 0.0;
    for (int k = 0; k < nsteps; k++) {
#if defined(__HIP_DEVICE_COMPILE__)
        const fbr_cint_ptr st = (fbr_cint_ptr)(unsigned long)(steps + k * FBR_KINID_STEP);  // (the step program: scalar loads)
        const fbr_cint_ptr cb = (fbr_cint_ptr)(unsigned long)(capbeg + k);
#else
        const int *st = steps + k * FBR_KINID_STEP, *cb = capbeg + k;
#endif
        const int l = FBR_UNI(st[0]), psrc = FBR_UNI(st[1]), psave = FBR_UNI(st[2]), jt = FBR_UNI(st[3]), d = FBR_UNI(st[4]);
        const int c0 = FBR_UNI(cb[0]), c1 = FBR_UNI(cb[1]);
        double out[12];
        if (psrc < 0) {
            double e3[3] = {0, 0, 0}, b3[3] = {0, 0, 0};
            if (floating) basef(e3, b3);
            fbr_pose_base(floating, e3, b3, out, out + 9);
        } else {
            if (psrc > 0)
                for (int i = 0; i < 12; i++) P[i] = load(psrc - 1, i);
            double rR[9], rp[3], ax[3];
            consts(l, rR, rp, ax);
            const double qv = d >= 0 ? qf(d) : 0.0;
            fbr_pose_child(P, P + 9, rR, rp, ax, jt, qv, out, out + 9);
        }
        if (psave >= 0)
            for (int i = 0; i < 12; i++) save(psave, i, out[i]);
        for (int i = 0; i < 12; i++) P[i] = out[i];
        for (int c = c0; c < c1; c++) cap(c, out, out + 9);
    }
}

// does a later sample's (or block's) distance a replace the running minimum b?  The reference's `d < g`: strict, a NaN never wins
FBR_HD bool fbr_capsule_take(double a, double b) { return a < b; }
#define FBR_CAPSULE_NONE 1e10  // the reference's initial g: what a pair keeps (with index -1) when no sample wins

#if defined(__HIPCC__)
#define FBR_CAPSULE_BATCH 32  // pairs whose 64 distances a wave stages in the LDS before one lane per pair scans them

struct DevCapsules {
    int nsteps, nslots, ncaps, npairs;
    const int *steps;      // [nsteps][FBR_KINID_STEP]
    const int *capbeg;     // [nsteps + 1] capsule slots of every step
    const int *capid;      // [ncaps] slot -> the caller's capsule index
    const double *seg;     // [ncaps][6] p0 | p1 in the link frame, by slot
    const double *radius;  // [ncaps] by the caller's index
    const int2 *pairs;     // [npairs] the caller's capsule indices
};
// C candidates of T consecutive samples, of which every step-th is checked: Tc = ceil(T / step) checked samples per candidate, cut into
// tiles of 64 that never span two candidates (block b = candidate b / tiles)
struct DevCapTiles {
    long T, step, Tc, tiles, nblk;
};

#if defined(FBR_KERNELS_COLLISION)
// ---- what fbr_capsule_pairs_kernel, fbr_box_pairs_kernel and fbr_mesh_pairs_kernel share ("collision layout") ------------------
// Work item `it` of a pairs kernel, one wave: block b of the launch (its first checked sample i0 inside the candidate, `valid` of them) and
// the batch of cnt pairs from k0.
struct FbrPairItem {
    long b, i0;
    int k0, cnt, valid;
};
__device__ __forceinline__ FbrPairItem fbr_pair_item(long it, long nbatch, int batch, int npairs, const DevCapTiles &tl, long blk0)
{
    FbrPairItem w;
    w.b = it / nbatch;
    w.k0 = (int)(it - w.b * nbatch) * batch;
    w.cnt = min(batch, npairs - w.k0);
    const long blk = blk0 + w.b, c = blk / tl.tiles;
    w.i0 = (blk - c * tl.tiles) << 6;
    w.valid = (int)min(64L, tl.Tc - w.i0);
    return w;
}
// The tail of a pairs kernel: sd [pair of the batch][sample], rows 65 apart (the scan's lanes hit different banks); one lane per pair scans
// the item's samples in order (strict <: the first sample wins a tie, a NaN never wins) and writes the block's partial into column
// col(pair) of pval / pidx [nb][ldp] (FBR_CAPSULE_NONE / -1: no sample won).
template <class ColFn>
__device__ __forceinline__ void fbr_pair_scan_store(const double *sd, const FbrPairItem &w, int lane, const DevCapTiles &tl, long ldp, ColFn col,
                                                    double *pval, long *pidx)
{
    if (lane >= w.cnt) return;
    double best = FBR_CAPSULE_NONE;
    int ibest = -1;
    for (int r = 0; r < w.valid; r++) {
        const double a = sd[lane * 65 + r];
        if (fbr_capsule_take(a, best)) best = a, ibest = r;
    }
    const long o = w.b * ldp + col(w.k0 + lane);
    pval[o] = best;
    pidx[o] = ibest < 0 ? -1 : (w.i0 + ibest) * tl.step;
}

// blocks [blk0, blk0 + nb) of the tiling; ep [nb][ncaps][6][64]; dynamic LDS (stage != 0): the q rows of the block's samples, [64][ldn];
// scratch [gridDim.x][nslots][12][64]
__global__ __launch_bounds__(64) void fbr_capsule_points_kernel(DevModel m, DevCapsules cp, DevCapTiles tl, long blk0, long nb, int stage, int ldn,
                                                                const double *__restrict__ q, const double *__restrict__ rpy,
                                                                const double *__restrict__ bpos, double *__restrict__ ep, double *__restrict__ scratch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x, n = m.n;
    double *scr = scratch + (long)blockIdx.x * cp.nslots * 12 * 64 + lane;
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
        double *out = ep + b * (long)cp.ncaps * 6 * 64 + lane;
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
        auto cap = [&](int cs, const double *R, const double *p) {
            const fbr_cdouble_ptr sg = (fbr_cdouble_ptr)(unsigned long)(cp.seg + 6 * cs);
            const int id = FBR_UNI(((fbr_cint_ptr)(unsigned long)cp.capid)[cs]);
            const double l0[3] = {sg[0], sg[1], sg[2]}, l1[3] = {sg[3], sg[4], sg[5]};
            double w0[3], w1[3];
            fbr_capsule_point(R, p, l0, w0);
            fbr_capsule_point(R, p, l1, w1);
            if (live)
                for (int i = 0; i < 3; i++) {
                    out[((long)id * 6 + i) * 64] = w0[i];
                    out[((long)id * 6 + 3 + i) * 64] = w1[i];
                }
        };
        fbr_capsule_lane(cp.nsteps, cp.steps, cp.capbeg, m.floating && rpy != nullptr, qf, basef, save, load, consts, cap);
    }
}

// work items (block, batch of FBR_CAPSULE_BATCH pairs), one wave each; pval / pidx [nb][npairs]: the block's minimum of every pair and the
// sample index inside the candidate where it is reached
__global__ __launch_bounds__(64) void fbr_capsule_pairs_kernel(DevCapsules cp, DevCapTiles tl, long blk0, long nb, const double *__restrict__ ep,
                                                               double *__restrict__ pval, long *__restrict__ pidx)
{
    __shared__ double sd[FBR_CAPSULE_BATCH * 65];
    const int lane = threadIdx.x;
    const long nbatch = (cp.npairs + FBR_CAPSULE_BATCH - 1) / FBR_CAPSULE_BATCH, items = nb * nbatch;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrPairItem w = fbr_pair_item(it, nbatch, FBR_CAPSULE_BATCH, cp.npairs, tl, blk0);
        const double *e = ep + w.b * (long)cp.ncaps * 6 * 64 + lane;  // (lanes behind the last checked sample read what an earlier call left: never scanned)
        int cura = -1;
        double a0[3] = {0, 0, 0}, a1[3] = {0, 0, 0}, ra = 0.0;
        __syncthreads();  // (the item before has been scanned)
        for (int j = 0; j < w.cnt; j++) {
            const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(cp.pairs + w.k0 + j);
            const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
            if (ia != cura) {  // (pair lists come sorted by their first capsule: its endpoints stay in registers)
                for (int i = 0; i < 3; i++) {
                    a0[i] = e[((long)ia * 6 + i) * 64];
                    a1[i] = e[((long)ia * 6 + 3 + i) * 64];
                }
                ra = ((fbr_cdouble_ptr)(unsigned long)cp.radius)[ia];
                cura = ia;
            }
            double b0[3], b1[3], s, t;
            for (int i = 0; i < 3; i++) {
                b0[i] = e[((long)ib * 6 + i) * 64];
                b1[i] = e[((long)ib * 6 + 3 + i) * 64];
            }
            const double rb = ((fbr_cdouble_ptr)(unsigned long)cp.radius)[ib];
            sd[j * 65 + lane] = fbr_segment_distance(a0, a1, b0, b1, &s, &t) - ra - rb;
        }
        __syncthreads();
        fbr_pair_scan_store(sd, w, lane, tl, cp.npairs, [](int k) { return k; }, pval, pidx);
    }
}

// The partials of blocks [blk0, blk0 + nb) folded, in block order, into val / idx [C][npairs]: one thread per (candidate with a block in
// the range, pair).  A candidate whose first block lies in the range starts from (FBR_CAPSULE_NONE, -1), one that an earlier range began
// from what that range left.
__global__ __launch_bounds__(256) void fbr_capsule_finish_kernel(DevCapTiles tl, int npairs, long blk0, long nb, const double *__restrict__ pval,
                                                                 const long *__restrict__ pidx, double *__restrict__ val, long *__restrict__ idx)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long c0 = blk0 / tl.tiles, c1 = (blk0 + nb - 1) / tl.tiles;
    const long c = c0 + t / npairs;
    if (c > c1) return;
    const int k = (int)(t % npairs);
    const long j0 = max(c * tl.tiles, blk0), j1 = min((c + 1) * tl.tiles, blk0 + nb);
    const bool fresh = j0 == c * tl.tiles;
    double best = fresh ? FBR_CAPSULE_NONE : val[c * npairs + k];
    long ibest = fresh ? -1 : idx[c * npairs + k];
    for (long j = j0; j < j1; j++) {
        const double a = pval[(j - blk0) * npairs + k];
        if (fbr_capsule_take(a, best)) best = a, ibest = pidx[(j - blk0) * npairs + k];
    }
    val[c * npairs + k] = best;
    idx[c * npairs + k] = ibest;
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
