// fbr_hull_grad.h -- signed convex-hull distance and its central-difference derivative with respect to the joint positions at chosen
// configurations of candidate trajectories (fbr_hull_distance_gradients).
//
// Replaces the collision block of the reference's analytical gradient in its default collisionMode "convex"
// (excitation/analyticalGradient.py, the `else` branch of the collision block: per joint two whole-robot forward kinematics and two
// distance calls of its mesh library at q +- analyticalGradientEpsilon e_j).  The rule is kept -- (d(q + eps e_j) - d(q - eps e_j)) / (2 eps)
// of fbr_hull_distance (fbr_hull.h) -- and the stencil is the boxes' (fbr_box_grad.h): a hull's frame is what a box's is, R_link | p_link +
// offset, offset_in_link_axes in the place of center_in_link_axes, a world hull a constant rot | position.  So the two walks, the moved
// copies (fbr_boxgrad_move, fbr_boxgrad_turn) and the zero rules are fbr_rigidgrad_item's, instantiated here with the hull distance:
// fixed joints, joints above neither link and joints above both links that move the pair rigidly (always with the offsets in link axes,
// prismatic joints with the offsets in world axes) are exact zeros, never evaluated; with the offsets in world axes a revolute joint above
// both links is evaluated by turning the two offsets the other way; with a world hull every moving joint above the robot link is evaluated.
//
// fbr_hull_distance has ONE call site, in fbr_rigidgrad_item's rolled loop over (centre, +, -).  Its loops vote over the wave
// (FBR_HULL_ANY): the call sits in control flow that depends on the pair alone, and a wave holds one pair -- lanes behind the last
// candidate repeat it, lanes without a sample evaluate a clamped one and store nothing.
//
// The arithmetic (fbr_hullgrad_item) is HIP-free: tests/emul/hull_grad_emul.cpp compiles the same text with g++.
#pragma once
#include "fbr_box_grad.h"
#include "fbr_hull.h"

// One (pair, configuration): the hulls HA on the link of step ka (ka < 0: a world hull) and HB on that of kb; xa, xb and the callbacks as
// for fbr_rigidgrad_item.
template <class DP, class IP, class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class GradFn>
FBR_HD double fbr_hullgrad_item(int ka, int kb, int cmode, const double *xa, const FbrHullT<DP, IP> &HA, const double *xb, const FbrHullT<DP, IP> &HB,
                                double eps, double se, double omc, const int *steps, int floating, MaskFn mask, QFn qf, BaseFn basef, SlotSave save,
                                SlotLoad load, ConstFn consts, GradFn grad)
{
    return fbr_rigidgrad_item(ka, kb, cmode, xa, xb, eps, se, omc, steps, floating, mask, qf, basef, save, load, consts, grad,
                              [&](const double *X, const double *Y) { return fbr_hull_distance(X, X + 9, HA, Y, Y + 9, HB, (int *)nullptr); });
}

#if defined(__HIPCC__)
#if defined(FBR_KERNELS_COLLISION)
// the tables of hull h (wave-uniform), as fbr_hull_fetch reads them
__device__ __forceinline__ void fbr_hullgrad_tables(const DevHulls &hs, int h, FbrDevHull *H)
{
    const fbr_cint_ptr tb = (fbr_cint_ptr)(unsigned long)(hs.tab + 8 * (long)h);
    H->nv = FBR_UNI(tb[2]);
    H->nf = FBR_UNI(tb[4]);
    H->ne = FBR_UNI(tb[6]);
    H->verts = (fbr_cdouble_ptr)(unsigned long)(hs.verts + 3 * (long)FBR_UNI(tb[1]));
    H->planes = (fbr_cdouble_ptr)(unsigned long)(hs.planes + 4 * (long)FBR_UNI(tb[3]));
    H->edges = (fbr_cint_ptr)(unsigned long)(hs.edges + 4 * (long)FBR_UNI(tb[5]));
    H->diam = ((fbr_cdouble_ptr)(unsigned long)hs.diam)[h];
}

// Work items (pair, tile of 64 candidates), one wave each, pair-major; the arguments as for fbr_box_grad_kernel.  hs: the set, or the plain
// pairs of a set with meshes attached (hs.col: their columns among the hs.ldp pairs of the whole set, which sample / scale / pose, dist
// and grad are laid out by, as hg.pair is; fbr_mesh_grad.h has the other pairs).
__global__ __launch_bounds__(64) void fbr_hull_grad_kernel(DevModel m, DevHulls hs, DevPairGrad hg, long C, long T, const double *__restrict__ q,
                                                           const double *__restrict__ rpy, const double *__restrict__ bpos,
                                                           const long *__restrict__ sample, const double *__restrict__ scale,
                                                           const long *__restrict__ pose, double eps, double se, double omc,
                                                           double *__restrict__ dist, double *__restrict__ grad, double *__restrict__ scratch,
                                                           int *__restrict__ flag)
{
    const int lane = threadIdx.x, n = m.n;
    const long P = hs.npairs, tiles = (C + 63) >> 6, items = P * tiles;
    double *scr = scratch + (long)blockIdx.x * hs.fr.nslots * 12 * 64 + lane;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long k = it / tiles, c0 = (it - k * tiles) << 6;
        const int valid = (int)min(64L, C - c0);
        const long c = c0 + min(lane, valid - 1);  // lanes behind the last candidate repeat it and store nothing
        const bool live = lane < valid;
        const int col = hs.col ? FBR_UNI(hs.col[k]) : (int)k;  // (a set split by fbr_model_set_hull_meshes: the pair's column among all pairs)
        const long e = c * hs.ldp + col;
        const long s = sample[e], ps0 = pose ? pose[e] : s, ps = ps0 < 0 ? s : ps0;
        const bool bad = s < -1 || s >= T || ps0 < -1 || ps0 >= T;
        if (bad && live) *flag = 1;
        const bool eval = live && s >= 0 && !bad;
        const long sr = c * T + min(max(s, 0L), T - 1), pr = c * T + min(max(ps, 0L), T - 1);
        const double sc = scale ? scale[e] : 1.0;
        const int4 pt = hg.pair[col];
        const int ka = FBR_UNI(pt.x), kb = FBR_UNI(pt.y), sla = FBR_UNI(pt.z), slb = FBR_UNI(pt.w);
        const int2 ids = hs.pairs[k];
        const int ia = FBR_UNI(ids.x), ib = FBR_UNI(ids.y);
        // the constants of the two members (wave-uniform loads): a robot hull's offset by slot, a world hull's R | position; the tables by
        // the caller's number
        const fbr_cdouble_ptr ccen = (fbr_cdouble_ptr)(unsigned long)hs.fr.cen, cworld = (fbr_cdouble_ptr)(unsigned long)hs.world;
        double xa[12], xb[12];
        for (int i = 0; i < 12; i++) xa[i] = xb[i] = 0.0;
        if (ka >= 0) {
            for (int i = 0; i < 3; i++) xa[i] = ccen[3 * sla + i];
        } else {
            for (int i = 0; i < 12; i++) xa[i] = cworld[12 * sla + i];
        }
        if (kb >= 0) {
            for (int i = 0; i < 3; i++) xb[i] = ccen[3 * slb + i];
        } else {
            for (int i = 0; i < 12; i++) xb[i] = cworld[12 * slb + i];
        }
        FbrDevHull HA, HB;
        fbr_hullgrad_tables(hs, ia, &HA);
        fbr_hullgrad_tables(hs, ib, &HB);
        const double *myq = q + sr * n;
        double *g = grad + e * n;
        const int kam = ka < 0 ? 0 : ka, kbm = kb < 0 ? 0 : kb, keep = (ka < 0 ? 0 : 1) | (kb < 0 ? 0 : 2);
        auto mask = [&](int st) { return fbr_capgrad_mask(hg.anc, hg.W, kam, kbm, st) & keep; };  // (a world member owns no step)
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
        const double dd = fbr_hullgrad_item(ka, kb, hs.fr.cmode, xa, HA, xb, HB, eps, se, omc, hs.fr.steps, m.floating && rpy != nullptr, mask, qf, basef,
                                            save, load, consts, gst);
        if (live) dist[e] = eval ? dd : FBR_CAPSULE_NONE;
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
