// fbr_box_grad.h -- signed box distance and its central-difference derivative with respect to the joint positions at chosen configurations
// of candidate trajectories (fbr_box_distance_gradients).
//
// Replaces the box pairs of the collision block of the reference's analytical gradient (excitation/analyticalGradient.py
// _collision_fd_single_pair and the `else` branch of the collision block: per joint two whole-robot forward kinematics and two distance
// calls of its mesh library at q +- analyticalGradientEpsilon e_j).  The rule is kept -- (d(q + eps e_j) - d(q - eps e_j)) / (2 eps) of the
// box distance of fbr_box.h -- but the robot is not walked again for every joint: adding eps to q_j moves everything below joint j
// rigidly, by a rotation of eps about the joint's world axis z_j through its origin o_j (revolute) or by the translation eps z_j
// (prismatic).  With v a vector fixed to the moved link,
//     Rot(v) = v + sin(eps) (z x v) + (1 - cos(eps)) (z (z . v) - v),     1 - cos(eps) = 2 sin^2(eps / 2),
// the link's R' = Rot(R) column by column and p' = o + Rot(p - o).  The box centre follows its mode: p' + c (the offset stays in world
// axes and does NOT turn with the link) or p' + R' c.  Fixed joints and joints above neither link move nothing, and a joint above BOTH
// links moves the two boxes alike when the centres turn with their links or the joint is prismatic: those entries of a row are exact
// zeros, never evaluated.  With the offsets in world axes a revolute joint above both links turns the two links but not the offsets, so the
// pair is NOT moved rigidly and the entry is evaluated: the distance is invariant under a common rigid motion, so instead of turning both
// links the two offsets are turned the other way, c' = p + Rot^-1(c) -- only the centres change.  A world box never moves, so every moving
// joint above the robot link is evaluated.
//
// One kernel, one lane per (pair, candidate), pair-major, as fbr_capsule_grad_kernel: the links, masks, path joints and which box moves
// are wave-uniform.  A lane walks the steps above either link twice (fbr_capgrad_walk): once for the poses of the two links, then again
// for z_j and o_j of every path joint, where it forms the moved copy of the box on that joint's side twice, evaluates fbr_box_distance
// on each and stores the quotient at once.  fbr_box_distance has ONE call site, inside a rolled loop over (centre, +, -): the unmoved
// distance is the first evaluation of the second walk, at its first step ("box distance gradients").
//
// The arithmetic (fbr_boxgrad_move, fbr_rigidgrad_item, fbr_boxgrad_item) is HIP-free: tests/emul/box_grad_emul.cpp compiles the same text
// with g++.  fbr_rigidgrad_item takes the distance routine as a functor: the hulls (fbr_hull_grad.h) instantiate it a second time.
#pragma once
#include "fbr_box.h"
#include "fbr_capsule_grad.h"

// sin(eps) and 1 - cos(eps) of the stencil, formed once on the host (wave-uniform kernel arguments)
static inline void fbr_boxgrad_trig(double eps, double *se, double *omc)
{
    const double h = sin(0.5 * eps);
    *se = sin(eps);
    *omc = 2.0 * h * h;
}

// w <- Rot(v): v turned about the unit axis z through the angle whose sine is sn and whose 1 - cosine is omc
FBR_HD void fbr_boxgrad_rot(double sn, double omc, const double *z, double v0, double v1, double v2, double *w0, double *w1, double *w2)
{
    const double zv = z[0] * v0 + z[1] * v1 + z[2] * v2;
    *w0 = v0 + (sn * (z[1] * v2 - z[2] * v1) + omc * (z[0] * zv - v0));
    *w1 = v1 + (sn * (z[2] * v0 - z[0] * v2) + omc * (z[1] * zv - v1));
    *w2 = v2 + (sn * (z[0] * v1 - z[1] * v0) + omc * (z[2] * zv - v2));
}

// The link pose (R, p) moved by joint (jt, world axis z, origin o) through sg * eps (sg = +-1; se, omc: fbr_boxgrad_trig), and the box
// whose centre offset is `off`: X [12] <- R' | centre.
FBR_HD void fbr_boxgrad_move(int cmode, int jt, double sg, double eps, double se, double omc, const double *z, const double *o, const double *R,
                             const double *p, const double *off, double *X)
{
    double pn[3];
    if (jt == 1) {
        const double sn = sg * se;
        fbr_boxgrad_rot(sn, omc, z, R[0], R[3], R[6], X + 0, X + 3, X + 6);  // the three columns of R, then p - o
        fbr_boxgrad_rot(sn, omc, z, R[1], R[4], R[7], X + 1, X + 4, X + 7);
        fbr_boxgrad_rot(sn, omc, z, R[2], R[5], R[8], X + 2, X + 5, X + 8);
        fbr_boxgrad_rot(sn, omc, z, p[0] - o[0], p[1] - o[1], p[2] - o[2], pn + 0, pn + 1, pn + 2);
        for (int i = 0; i < 3; i++) pn[i] += o[i];
    } else {
        for (int i = 0; i < 9; i++) X[i] = R[i];
        for (int i = 0; i < 3; i++) pn[i] = p[i] + (sg * eps) * z[i];
    }
    fbr_box_centre(cmode, X, pn, off, X + 9);
}

// centre of a box whose world-axes offset `off` is turned by sn = +-sin(eps) about z: c <- p + Rot(off)
FBR_HD void fbr_boxgrad_turn(double sn, double omc, const double *z, const double *p, const double *off, double *c)
{
    fbr_boxgrad_rot(sn, omc, z, off[0], off[1], off[2], c + 0, c + 1, c + 2);
    for (int i = 0; i < 3; i++) c[i] += p[i];
}

// One (pair, configuration) of two rigid bodies placed as boxes are: R_link | p_link + offset (fbr_box_centre).  Member A sits on the link of
// step ka (ka < 0: a world member), B on that of kb; at most one is a world member.  A robot member's `xa` holds its centre offset (3), a
// world member's R | centre (12).  distf(X, Y): the signed distance of the two bodies at the frames X, Y [12] (R | centre) -- the boxes'
// fbr_box_distance, the hulls' fbr_hull_distance (fbr_hull_grad.h); it has ONE call site.  Returns the distance and, through grad(d, v), the
// central difference over +- eps of every evaluated joint d.  A NaN pose gives NaN in the distance and in the evaluated joints' entries.
// mask(k) must leave the bit of a world member clear.  base_of_pose(e3, b3): the caller's base pose (rpy, position); it is asked only
// where the pair depends on it (below).
template <class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class GradFn, class DistFn>
FBR_HD double fbr_rigidgrad_item(int ka, int kb, int cmode, const double *xa, const double *xb, double eps, double se, double omc, const int *steps,
                                 int floating, MaskFn mask, QFn qf, BaseFn base_of_pose, SlotSave save, SlotLoad load, ConstFn consts,
                                 GradFn grad, DistFn distf)
{
    const int kend = (ka > kb ? ka : kb) + 1;
    // Two robot members whose offsets turn with their links: the base moves the pair rigidly, so its distance and its row do not depend on
    // the base pose.  Such a pair is walked from an identity base (wave-uniform), and returns the bits of a stationary base whatever the
    // base does.  With the offsets in world axes, or against a world member, the base pose counts and is the caller's.
    const bool rel = ka >= 0 && kb >= 0 && cmode != 0;
    auto basef = [&](double *e3, double *b3) {
        if (rel) {
            for (int i = 0; i < 3; i++) e3[i] = b3[i] = 0.0;
        } else {
            base_of_pose(e3, b3);
        }
    };
    double A[12], pA[3] = {0, 0, 0}, B[12], pB[3] = {0, 0, 0};  // the boxes R | centre (a robot box has its link's R) and the link origins
    for (int i = 0; i < 12; i++) {
        A[i] = ka < 0 ? xa[i] : 0.0;
        B[i] = kb < 0 ? xb[i] : 0.0;
    }
    fbr_capgrad_walk(kend, steps, floating, mask, qf, basef, save, load, consts,
                     [&](int k, int, int, int, const double *, const double *R, const double *p) {
                         if (k == ka) {
                             for (int i = 0; i < 9; i++) A[i] = R[i];
                             for (int i = 0; i < 3; i++) pA[i] = p[i];
                             fbr_box_centre(cmode, R, p, xa, A + 9);
                         }
                         if (k == kb) {
                             for (int i = 0; i < 9; i++) B[i] = R[i];
                             for (int i = 0; i < 3; i++) pB[i] = p[i];
                             fbr_box_centre(cmode, R, p, xb, B + 9);
                         }
                     });
    double dist = 0.0;
    bool first = true;
    fbr_capgrad_walk(kend, steps, floating, mask, qf, basef, save, load, consts,
                     [&](int, int mk, int jt, int d, const double *ax, const double *R, const double *p) {
                         // no joint variable; above both links: the boxes move together unless the offsets keep their world direction
                         const bool pj = jt != 0 && d >= 0 && (mk != 3 || (cmode == 0 && jt == 1));
                         const int e0 = first ? 0 : 1;
                         first = false;
                         if (!pj && e0) return;
                         // the moved copies are formed in X | Y beside the pair's boxes and die once the distance routine below, called on
                         // (X, Y) whatever moves, has taken its frame from them: in its body only the pair's own two boxes stay live
                         double z[3] = {0, 0, 0}, dplus = 0.0;
                         if (pj) fbr_mv(R, ax, z);
#pragma unroll 1
                         for (int e = e0; e < (pj ? 3 : 1); e++) {  // the unmoved pair (once), then q_d + eps, q_d - eps
                             double X[12], Y[12];
                             for (int i = 0; i < 12; i++) {
                                 X[i] = A[i];
                                 Y[i] = B[i];
                             }
                             if (e) {
                                 const double sg = e == 1 ? 1.0 : -1.0;
                                 if (mk == 1) {
                                     fbr_boxgrad_move(cmode, jt, sg, eps, se, omc, z, p, A, pA, xa, X);
                                 } else if (mk == 2) {
                                     fbr_boxgrad_move(cmode, jt, sg, eps, se, omc, z, p, B, pB, xb, Y);
                                 } else {
                                     fbr_boxgrad_turn(-sg * se, omc, z, pA, xa, X + 9);
                                     fbr_boxgrad_turn(-sg * se, omc, z, pB, xb, Y + 9);
                                 }
                             }
                             const double v = distf(X, Y);
                             if (e == 0)
                                 dist = v;
                             else if (e == 1)
                                 dplus = v;
                             else
                                 grad(d, (dplus - v) / (2.0 * eps));
                         }
                     });
    return dist;
}

// the box pair: ha, hb the half extents of the two members
template <class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class GradFn>
FBR_HD double fbr_boxgrad_item(int ka, int kb, int cmode, const double *xa, const double *ha, const double *xb, const double *hb, double eps, double se,
                               double omc, const int *steps, int floating, MaskFn mask, QFn qf, BaseFn basef, SlotSave save, SlotLoad load,
                               ConstFn consts, GradFn grad)
{
    return fbr_rigidgrad_item(ka, kb, cmode, xa, xb, eps, se, omc, steps, floating, mask, qf, basef, save, load, consts, grad,
                              [&](const double *X, const double *Y) { return fbr_box_distance(X, X + 9, ha, Y, Y + 9, hb); });
}

#if defined(__HIPCC__)
#if defined(FBR_KERNELS_COLLISION)
// (This kernel and fbr_hull_grad_kernel keep their item preamble and their callbacks written out: with the shared helpers of
// fbr_capsule.h / fbr_capsule_grad.h their code came out a little different and 1 to 2 % slower on an MI355X -- DESIGN.md, "collision
// layout".)
// Work items (pair, tile of 64 candidates), one wave each, pair-major; the arguments as for fbr_capsule_grad_kernel.  eps, se, omc: the
// stencil step and fbr_boxgrad_trig of it.
__global__ __launch_bounds__(64) void fbr_box_grad_kernel(DevModel m, DevBoxes bx, DevPairGrad bg, long C, long T, const double *__restrict__ q,
                                                          const double *__restrict__ rpy, const double *__restrict__ bpos,
                                                          const long *__restrict__ sample, const double *__restrict__ scale,
                                                          const long *__restrict__ pose, double eps, double se, double omc,
                                                          double *__restrict__ dist, double *__restrict__ grad, double *__restrict__ scratch,
                                                          int *__restrict__ flag)
{
    const int lane = threadIdx.x, n = m.n;
    const long P = bx.npairs, tiles = (C + 63) >> 6, items = P * tiles;
    double *scr = scratch + (long)blockIdx.x * bx.nslots * 12 * 64 + lane;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long k = it / tiles, c0 = (it - k * tiles) << 6;
        const int valid = (int)min(64L, C - c0);
        const long c = c0 + min(lane, valid - 1);  // lanes behind the last candidate repeat it and store nothing
        const bool live = lane < valid;
        const long e = c * P + k;
        const long s = sample[e], ps0 = pose ? pose[e] : s, ps = ps0 < 0 ? s : ps0;
        const bool bad = s < -1 || s >= T || ps0 < -1 || ps0 >= T;
        if (bad && live) *flag = 1;
        const bool eval = live && s >= 0 && !bad;
        const long sr = c * T + min(max(s, 0L), T - 1), pr = c * T + min(max(ps, 0L), T - 1);
        const double sc = scale ? scale[e] : 1.0;
        const int4 pt = bg.pair[k];
        const int ka = FBR_UNI(pt.x), kb = FBR_UNI(pt.y), sla = FBR_UNI(pt.z), slb = FBR_UNI(pt.w);
        const int2 ids = bx.pairs[k];
        const int ia = FBR_UNI(ids.x), ib = FBR_UNI(ids.y);
        // the constants of the two members (wave-uniform loads): a robot box's centre offset by slot and half extents by number, a world
        // box's R | centre | half extents
        const fbr_cdouble_ptr ccen = (fbr_cdouble_ptr)(unsigned long)bx.cen, chalf = (fbr_cdouble_ptr)(unsigned long)bx.half,
                              cworld = (fbr_cdouble_ptr)(unsigned long)bx.world;
        double xa[12], ha[3], xb[12], hb[3];
        for (int i = 0; i < 12; i++) xa[i] = xb[i] = 0.0;
        if (ka >= 0) {
            for (int i = 0; i < 3; i++) {
                xa[i] = ccen[3 * sla + i];
                ha[i] = chalf[3 * ia + i];
            }
        } else {
            for (int i = 0; i < 12; i++) xa[i] = cworld[15 * sla + i];
            for (int i = 0; i < 3; i++) ha[i] = cworld[15 * sla + 12 + i];
        }
        if (kb >= 0) {
            for (int i = 0; i < 3; i++) {
                xb[i] = ccen[3 * slb + i];
                hb[i] = chalf[3 * ib + i];
            }
        } else {
            for (int i = 0; i < 12; i++) xb[i] = cworld[15 * slb + i];
            for (int i = 0; i < 3; i++) hb[i] = cworld[15 * slb + 12 + i];
        }
        const double *myq = q + sr * n;
        double *g = grad + e * n;
        const int kam = ka < 0 ? 0 : ka, kbm = kb < 0 ? 0 : kb, keep = (ka < 0 ? 0 : 1) | (kb < 0 ? 0 : 2);
        auto mask = [&](int st) { return fbr_capgrad_mask(bg.anc, bg.W, kam, kbm, st) & keep; };  // (a world member owns no step)
        auto qf = [&](int d) { return sc * myq[d]; };
        auto basef = [&](double *e3, double *b3) {
            for (int i = 0; i < 3; i++) {
                e3[i] = rpy ? rpy[pr * 3 + i] : 0.0;
                b3[i] = bpos ? bpos[pr * 3 + i] : 0.0;
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
        auto gst = [&](int d, double v) {
            if (eval) g[d] = v;
        };
        const double dd = fbr_boxgrad_item(ka, kb, bx.cmode, xa, ha, xb, hb, eps, se, omc, bx.steps, m.floating && rpy != nullptr, mask, qf, basef, save,
                                           load, consts, gst);
        if (live) dist[e] = eval ? dd : FBR_CAPSULE_NONE;
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
