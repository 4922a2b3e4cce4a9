// fbr_capsule_grad.h -- capsule distance and its derivative with respect to the joint positions at chosen configurations of candidate
// trajectories (fbr_capsule_distance_gradients).
//
// Replaces the collision block of the reference's analytical gradient (excitation/analyticalGradient.py:955-1027: per collision pair two
// iDynTree Jacobians and capsule.py capsule_distance_and_gradient).  With p_A, p_B the closest points of the two segments and
// n = (p_A - p_B) / |p_A - p_B| (zero below 1e-12, the reference's rule),
//     d dist / d q_j = n . (d p_A / d q_j - d p_B / d q_j),
// every point moving rigidly with its link: d p / d q_j = z_j x (p - o_j) for a revolute joint j above p's link (world axis z_j through
// o_j), z_j for a prismatic one, 0 for every other joint.  This is v + omega x r; the reference's _point_jacobian forms v + r x omega
// (INTEGRATION 2 has the finite-difference evidence).  A joint above BOTH links moves p_A and p_B alike and n . (z x (p_A - p_B)) = 0, so
// only the joints on the tree path between the two links are evaluated; every other entry of a row is an exact 0.
//
// One kernel, one lane per (pair, candidate), pair-major: the 64 lanes of a wave are 64 candidates of ONE pair, so the two links, their
// ancestor sets (a bit per step of the program of fbr_kinid_build, per link) and the path joints are wave-uniform scalars; only q differs
// between lanes.  A lane walks the steps that are ancestors of either link twice: first for the two link poses (closest points, n, the
// distance), then again for the world axis and origin of every path joint, whose entry it stores at once -- nothing is parked between the
// walks but the branch-point poses of the lane-interleaved scratch ("capsule distance gradients").
//
// The arithmetic (fbr_capgrad_walk, fbr_capgrad_item) is HIP-free: tests/emul/capsule_grad_emul.cpp compiles the same text with g++.
#pragma once
#include "fbr_capsule.h"

#define FBR_CAPGRAD_COINCIDENT 1e-12  // |p_A - p_B| below this: the direction is undefined, the row is zero (capsule.py)

// The step program walked for the poses of the steps k < kend with mask(k) != 0 only (mask: bit 0 the step is the first link or above it,
// bit 1 the same for the second link).  Such a set is closed under parents, so a step whose parent is "the step before" (psrc 0) finds it in
// registers, and a slot is read only after the parent, itself in the set, has saved it.  QFn, BaseFn, SlotSave, SlotLoad, ConstFn as for
// fbr_capsule_lane; LinkFn(k, mk, jt, d, axis, R, p): step k, its mask, joint type, dof, joint axis in the link's frame, world pose.
template <class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class LinkFn>
FBR_HD void fbr_capgrad_walk(int kend, const int *steps, int floating, MaskFn mask, QFn qf, BaseFn basef, SlotSave save, SlotLoad load,
                             ConstFn consts, LinkFn link)
{
    double P[12];
    for (int i = 0; i < 12; i++) P[i] = 0.0;
    for (int k = 0; k < kend; k++) {
        const int mk = mask(k);
        if (!mk) continue;
#if defined(__HIP_DEVICE_COMPILE__)
        const fbr_cint_ptr st = (fbr_cint_ptr)(unsigned long)(steps + k * FBR_KINID_STEP);  // (the step program: scalar loads)
#else
        const int *st = steps + k * FBR_KINID_STEP;
#endif
        const int l = FBR_UNI(st[0]), psrc = FBR_UNI(st[1]), psave = FBR_UNI(st[2]), jt = FBR_UNI(st[3]), d = FBR_UNI(st[4]);
        double out[12], ax[3] = {0, 0, 0};
        if (psrc < 0) {
            double e3[3] = {0, 0, 0}, b3[3] = {0, 0, 0};
            if (floating) basef(e3, b3);
            fbr_pose_base(floating, e3, b3, out, out + 9);
        } else {
            if (psrc > 0)
                for (int i = 0; i < 12; i++) P[i] = load(psrc - 1, i);
            double rR[9], rp[3];
            consts(l, rR, rp, ax);
            const double qv = d >= 0 ? qf(d) : 0.0;
            fbr_pose_child(P, P + 9, rR, rp, ax, jt, qv, out, out + 9);
        }
        if (psave >= 0)
            for (int i = 0; i < 12; i++) save(psave, i, out[i]);
        for (int i = 0; i < 12; i++) P[i] = out[i];
        link(k, mk, psrc < 0 ? 0 : jt, d, ax, out, out + 9);
    }
}

// One (pair, configuration): the segment distance of the capsules sa (on the link of step ka) and sb (step kb), p0 | p1 in the link's
// frame, returned WITHOUT the radii, and through grad(d, v) the entry of every path joint d.  A NaN pose gives NaN in the distance and in
// the path joints' entries.
template <class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class GradFn>
FBR_HD double fbr_capgrad_item(int ka, int kb, const double *sa, const double *sb, const int *steps, int floating, MaskFn mask, QFn qf,
                               BaseFn basef, SlotSave save, SlotLoad load, ConstFn consts, GradFn grad)
{
    const int kend = (ka > kb ? ka : kb) + 1;
    double a0[3] = {0, 0, 0}, a1[3] = {0, 0, 0}, b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
    fbr_capgrad_walk(kend, steps, floating, mask, qf, basef, save, load, consts,
                     [&](int k, int, int, int, const double *, const double *R, const double *p) {
                         if (k == ka) {
                             fbr_capsule_point(R, p, sa, a0);
                             fbr_capsule_point(R, p, sa + 3, a1);
                         }
                         if (k == kb) {
                             fbr_capsule_point(R, p, sb, b0);
                             fbr_capsule_point(R, p, sb + 3, b1);
                         }
                     });
    double s, t;
    const double dist = fbr_segment_distance(a0, a1, b0, b1, &s, &t);
    double pa[3], pb[3], nv[3];
    for (int i = 0; i < 3; i++) {
        pa[i] = a0[i] + s * (a1[i] - a0[i]);
        pb[i] = b0[i] + t * (b1[i] - b0[i]);
        nv[i] = dist < FBR_CAPGRAD_COINCIDENT ? 0.0 : (pa[i] - pb[i]) / dist;
    }
    fbr_capgrad_walk(kend, steps, floating, mask, qf, basef, save, load, consts,
                     [&](int, int mk, int jt, int d, const double *ax, const double *R, const double *p) {
                         if (mk == 3 || jt == 0 || d < 0) return;  // above both links (the two shares cancel), or no joint variable
                         double z[3], g;
                         fbr_mv(R, ax, z);
                         if (jt == 1) {
                             const double *pt = mk == 1 ? pa : pb;
                             const double r[3] = {pt[0] - p[0], pt[1] - p[1], pt[2] - p[2]};
                             double c[3];
                             fbr_cross(z, r, c);
                             g = nv[0] * c[0] + nv[1] * c[1] + nv[2] * c[2];
                         } else {
                             g = nv[0] * z[0] + nv[1] * z[1] + nv[2] * z[2];
                         }
                         grad(d, mk == 1 ? g : -g);
                     });
    return dist;
}

// Host side of the tables: anc [nsteps][W] (W = words of 32 steps): bit j of row k is set when step j is step k's link or above it.
static inline int fbr_capgrad_words(int nsteps) { return (nsteps + 31) / 32; }
static inline void fbr_capgrad_ancestors(const FbrHostModel &hm, const FbrKinIdProgram &prog, std::vector<int> &stepof, std::vector<int> &anc)
{
    const int W = fbr_capgrad_words(prog.nsteps);
    stepof.assign(hm.L, 0);
    for (int k = 0; k < prog.nsteps; k++) stepof[prog.steps[(size_t)k * FBR_KINID_STEP]] = k;
    anc.assign((size_t)std::max(prog.nsteps, 1) * W, 0);
    for (int k = 0; k < prog.nsteps; k++)
        for (int l = prog.steps[(size_t)k * FBR_KINID_STEP]; l >= 0; l = hm.parent[l]) {
            const int j = stepof[l];
            anc[(size_t)k * W + (j >> 5)] |= (int)(1u << (j & 31));
        }
}
FBR_HD int fbr_capgrad_mask(const int *anc, int W, int ka, int kb, int k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const fbr_cint_ptr ca = (fbr_cint_ptr)(unsigned long)anc;  // (ka, kb, k are wave-uniform: scalar loads)
#else
    const int *ca = anc;
#endif
    const unsigned wa = (unsigned)FBR_UNI(ca[(long)ka * W + (k >> 5)]), wb = (unsigned)FBR_UNI(ca[(long)kb * W + (k >> 5)]);
    return (int)((wa >> (k & 31)) & 1u) | (int)(((wb >> (k & 31)) & 1u) << 1);
}

#if defined(__HIPCC__)
// The table of a set's gradient call (fbr_collision_grad_table), the same for capsules, boxes and hulls.
struct DevPairGrad {
    int W;             // words per row of anc
    const int *anc;    // [nsteps][W] (fbr_capgrad_ancestors)
    const int4 *pair;  // [npairs] step of the first member's link (-1: a world member), of the second's, slot of the first member (DevCapsules.seg,
                       // DevBoxes.cen, DevHulls.fr.cen; a world member: its number), of the second
};

#if defined(FBR_KERNELS_COLLISION)
// ---- what fbr_capsule_grad_kernel and fbr_mesh_grad_frames_kernel share ("collision layout"; the box and the hull gradient
// kernel have the same things written out) --------------------------------------------------------------------------------------------
// The callbacks that the gradient items (fbr_capgrad_item, fbr_meshgrad_frames_item) take besides the kernel's own.  qf: the joint
// positions of the lane's configuration, row q, times the item's scale; basef: the base pose inputs of row s; save / load: the lane's
// column of the branch-point scratch; consts: the constants of link l (l is wave-uniform: scalar loads through the constant address space).
struct FbrLaneQ {
    const double *q;
    double sc;
    __device__ __forceinline__ double operator()(int d) const { return sc * q[d]; }
};
struct FbrLaneBase {
    const double *rpy, *bpos;
    long s;
    __device__ __forceinline__ void operator()(double *e3, double *b3) const
    {
        for (int i = 0; i < 3; i++) {
            e3[i] = rpy ? rpy[s * 3 + i] : 0.0;
            b3[i] = bpos ? bpos[s * 3 + i] : 0.0;
        }
    }
};
struct FbrLaneSave {
    double *scr;
    __device__ __forceinline__ void operator()(int sl, int i, double v) const { scr[(sl * 12 + i) * 64] = v; }
};
struct FbrLaneLoad {
    const double *scr;
    __device__ __forceinline__ double operator()(int sl, int i) const { return scr[(sl * 12 + i) * 64]; }
};
struct FbrLaneConsts {
    fbr_cdouble_ptr cR, cq, ca;
    __device__ __forceinline__ void operator()(int l, double *rR, double *rp, double *ax) const
    {
        for (int i = 0; i < 9; i++) rR[i] = cR[9 * l + i];
        for (int i = 0; i < 3; i++) {
            rp[i] = cq[3 * l + i];
            ax[i] = ca[3 * l + i];
        }
    }
};
struct FbrLaneIO {
    FbrLaneQ qf;
    FbrLaneBase basef;
    FbrLaneSave save;
    FbrLaneLoad load;
    FbrLaneConsts consts;
};
// scr: the lane's column of the wave's scratch [nslots][12][64]
__device__ __forceinline__ FbrLaneIO fbr_lane_io(const DevModel &m, const double *qrow, double sc, const double *rpy, const double *bpos, long s,
                                                 double *scr)
{
    return {{qrow, sc},
            {rpy, bpos, s},
            {scr},
            {scr},
            {(fbr_cdouble_ptr)(unsigned long)m.restR, (fbr_cdouble_ptr)(unsigned long)m.restp, (fbr_cdouble_ptr)(unsigned long)m.axis}};
}

// The head of work item `it` = (pair k of the launch, tile of 64 candidates), pair-major, one lane per candidate.  sample / scale / pose
// [C][ld] (scale, pose may be NULL), the pair's column col(k) among the ld; pair: the set's table, by column.  Lanes behind the last
// candidate repeat it and store nothing (live); a sample or pose index outside -1 .. T - 1 sets *flag and is read clamped (nothing
// faults); eval: the lane has a sample to evaluate.
struct FbrGradItem {
    long k, c, e;        // pair of the launch, candidate, entry c * ld + col
    int col;             // the pair's column
    long sr, pr;         // rows of q and of the base pose
    bool live, eval;
    double sc;
    int ka, kb, sla, slb;  // the pair's record: steps of the two members' links (-1: a world member), their slots (a world member: its number)
};
template <class ColFn>
__device__ __forceinline__ FbrGradItem fbr_grad_item_head(long it, long tiles, long C, long T, long ld, ColFn col, const long *sample, const double *scale,
                                                          const long *pose, const int4 *pair, int *flag)
{
    FbrGradItem w;
    const int lane = threadIdx.x;
    w.k = it / tiles;
    const long c0 = (it - w.k * tiles) << 6;
    const int valid = (int)min(64L, C - c0);
    w.col = col(w.k);
    w.c = c0 + min(lane, valid - 1);
    w.live = lane < valid;
    w.e = w.c * ld + w.col;
    const long s = sample[w.e], ps0 = pose ? pose[w.e] : s, ps = ps0 < 0 ? s : ps0;
    const bool bad = s < -1 || s >= T || ps0 < -1 || ps0 >= T;
    if (bad && w.live) *flag = 1;
    w.eval = w.live && s >= 0 && !bad;
    w.sr = w.c * T + min(max(s, 0L), T - 1);
    w.pr = w.c * T + min(max(ps, 0L), T - 1);
    w.sc = scale ? scale[w.e] : 1.0;
    const int4 pt = pair[w.col];
    w.ka = FBR_UNI(pt.x), w.kb = FBR_UNI(pt.y), w.sla = FBR_UNI(pt.z), w.slb = FBR_UNI(pt.w);
    return w;
}
// which of a pair's two members step st lies above (fbr_capgrad_mask), cut to `keep`: 3 for capsules, less in fbr_mesh_grad_frames_kernel
// where a world member owns no step
struct FbrGradMask {
    const int *anc;
    int W, ka, kb, keep;
    __device__ __forceinline__ int operator()(int st) const { return fbr_capgrad_mask(anc, W, ka, kb, st) & keep; }
};

// Work items (pair, tile of 64 candidates), one wave each, pair-major; C candidates of T samples; sample / scale / pose [C][npairs] (scale,
// pose may be NULL).  dist [C][npairs]; grad [C][npairs][n], ZEROED by the caller: only the path joints of evaluated items are stored.
// scratch [gridDim.x][nslots][12][64].  flag: set when a sample or pose index lies outside -1 .. T - 1 (read clamped: nothing faults).
__global__ __launch_bounds__(64) void fbr_capsule_grad_kernel(DevModel m, DevCapsules cp, DevPairGrad cg, long C, long T, const double *__restrict__ q,
                                                              const double *__restrict__ rpy, const double *__restrict__ bpos,
                                                              const long *__restrict__ sample, const double *__restrict__ scale,
                                                              const long *__restrict__ pose, double *__restrict__ dist, double *__restrict__ grad,
                                                              double *__restrict__ scratch, int *__restrict__ flag)
{
    const int lane = threadIdx.x, n = m.n;
    const long P = cp.npairs, tiles = (C + 63) >> 6, items = P * tiles;
    double *scr = scratch + (long)blockIdx.x * cp.nslots * 12 * 64 + lane;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrGradItem w = fbr_grad_item_head(it, tiles, C, T, P, [](long k) { return (int)k; }, sample, scale, pose, cg.pair, flag);
        // (the capsules' own: both members sit on links, and their constants are the segments by slot and the radii by number)
        const int2 ids = cp.pairs[w.k];
        const fbr_cdouble_ptr crad = (fbr_cdouble_ptr)(unsigned long)cp.radius, cseg = (fbr_cdouble_ptr)(unsigned long)cp.seg;
        const double ra = crad[FBR_UNI(ids.x)], rb = crad[FBR_UNI(ids.y)];
        double sa[6], sb[6];
        for (int i = 0; i < 6; i++) {
            sa[i] = cseg[6 * w.sla + i];
            sb[i] = cseg[6 * w.slb + i];
        }
        const FbrLaneIO io = fbr_lane_io(m, q + w.sr * n, w.sc, rpy, bpos, w.pr, scr);
        auto gst = [g = grad + w.e * n, eval = w.eval](int d, double v) {
            if (eval) g[d] = v;
        };
        const double dd = fbr_capgrad_item(w.ka, w.kb, sa, sb, cp.steps, m.floating && rpy != nullptr, FbrGradMask{cg.anc, cg.W, w.ka, w.kb, 3}, io.qf, io.basef,
                                           io.save, io.load, io.consts, gst);
        if (w.live) dist[w.e] = w.eval ? dd - ra - rb : FBR_CAPSULE_NONE;
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
