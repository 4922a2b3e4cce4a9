// fbr_mesh_grad.h -- triangle-mesh distance and its central-difference derivative with respect to the joint positions at chosen
// configurations of candidate trajectories (fbr_mesh_distance_gradients): the gradient half of fullMeshLinks and collisionMode "full".
//
// The reference has no rule of its own for meshes (excitation/analyticalGradient.py, the `else` branch of the collision block): per joint
// (d(q + eps e_j) - d(q - eps e_j)) / (2 eps) of the distance its mesh library gives, whatever geometry the link carries.  The rule is kept,
// with the stencil of the rigid bodies (fbr_rigidgrad_item, fbr_box_grad.h) and the mesh distance of fbr_mesh.h -- but NOT in the launch
// shape of the hull gradient, whose wave evaluates all 1 + 2 J stencil points of its pair one after the other: a mesh pair is 1e2 to 1e4
// hull evaluations a stencil point.  Three stages instead, for the pairs of the set with a mesh on either side (the others go through
// fbr_hull_grad_kernel, which takes the split set's pair list and columns):
//   A  fbr_mesh_grad_frames_kernel: (mesh pair, tile of 64 candidates), one wave each -- the hull gradient's launch.  fbr_rigidgrad_item a
//      third time, its "distance" a functor that RECORDS the relative pose (FbrHullRel, the meshed hull first, as fbr_mesh_distance orders
//      it) of the two frames it is handed and returns 0.0.  The walks, the moved copies and the zero rules are fbr_rigidgrad_item's text; the
//      functor has its one call site, so its calls number the stencil points: slot 0 the centre, then + eps, - eps of every evaluated
//      joint in walk order.  S_k = 1 + 2 J_k and the joint of every slot depend on the pair alone: fbr_meshgrad_slots, on the host.
//   B  fbr_mesh_grad_dist_kernel: (mesh pair, slot, tile of 64 candidates), ONE WAVE PER ITEM, pair-major.  A lane reads its candidate's
//      recorded pose, calls fbr_mesh_distance_oriented<true> and stores one double.  The call sits in control flow that depends on
//      (pair, slot) alone; its loops vote over the wave (FBR_HULL_ANY).  Lanes behind the last candidate repeat the last one and store
//      nothing; a lane without a sample evaluates the pose stage A made of the clamped sample, and stage C drops the value.
//   C  fbr_mesh_grad_quot_kernel: per (candidate, mesh pair) dist = d[0], grad[joint(s)] = (d[s+] - d[s-]) / (2.0 * eps), the expression of
//      fbr_rigidgrad_item.  Entries never evaluated stay the zeros of the caller's memset.
//
// Semantics.  A mesh distance is never negative and exactly 0.0 on contact (fbr_mesh.h), so an entry whose two stencil values are both
// 0.0 is exactly 0.0: a mesh carries no penetration depth, and a pair in intersection gives the optimiser no direction out of it (the
// reference's BVH gives it the same zeros).  A NaN pose gives NaN in the distance and in the evaluated entries only.
//
// The arithmetic (fbr_meshgrad_frames_item, fbr_meshgrad_slots, fbr_meshgrad_quotients) is HIP-free: tests/emul/mesh_grad_emul.cpp compiles
// the same text with g++ and holds it, bit for bit, to the single pass -- fbr_rigidgrad_item with fbr_mesh_distance as its functor.
#pragma once
#include "fbr_hull_grad.h"
#include "fbr_mesh.h"

#define FBR_MESHGRAD_REL 13  // the doubles of an FbrHullRel

// Stage A of one (pair, configuration): arguments as for fbr_rigidgrad_item; swap: the second member carries the pair's (only) mesh, so
// the pose recorded is that of the first relative to the second.  rec(s, rel): stencil point s.  Returns the number of stencil points.
template <class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class RecFn>
FBR_HD int fbr_meshgrad_frames_item(int ka, int kb, int cmode, const double *xa, const double *xb, bool swap, double eps, double se, double omc,
                                    const int *steps, int floating, MaskFn mask, QFn qf, BaseFn basef, SlotSave save, SlotLoad load, ConstFn consts,
                                    RecFn rec)
{
    int s = 0;
    fbr_rigidgrad_item(
        ka, kb, cmode, xa, xb, eps, se, omc, steps, floating, mask, qf, basef, save, load, consts, [](int, double) {},
        [&](const double *X, const double *Y) {
            FbrHullRel r;
            if (swap)
                fbr_hull_relative(Y, Y + 9, X, X + 9, &r);
            else
                fbr_hull_relative(X, X + 9, Y, Y + 9, &r);
            rec(s++, r);
            return 0.0;
        });
    return s;
}

// The joints of the stencil points of a pair (host): joint[0] = -1 (the centre), then twice the dof of every joint fbr_rigidgrad_item
// evaluates, in walk order.  ka, kb, cmode as there; steps, anc, W: the step program and the ancestor masks (fbr_capgrad_ancestors).
static inline void fbr_meshgrad_slots(int ka, int kb, int cmode, const int *steps, const int *anc, int W, std::vector<int> &joint)
{
    joint.assign(1, -1);
    const int kam = ka < 0 ? 0 : ka, kbm = kb < 0 ? 0 : kb, keep = (ka < 0 ? 0 : 1) | (kb < 0 ? 0 : 2), kend = (ka > kb ? ka : kb) + 1;
    for (int k = 0; k < kend; k++) {
        const int mk = fbr_capgrad_mask(anc, W, kam, kbm, k) & keep;
        if (!mk) continue;
        const int *st = steps + (size_t)k * FBR_KINID_STEP;
        const int jt = st[1] < 0 ? 0 : st[3], d = st[4];
        if (jt != 0 && d >= 0 && (mk != 3 || (cmode == 0 && jt == 1))) {
            joint.push_back(d);
            joint.push_back(d);
        }
    }
}

// Stage C of one (pair, configuration): S stencil values dv(s), joint [S] as fbr_meshgrad_slots made them.  Returns the centre distance and
// stores, through grad(d, v), the quotient of every evaluated joint -- the expression of fbr_rigidgrad_item.
template <class JointFn, class DistFn, class GradFn>
FBR_HD double fbr_meshgrad_quotients(int S, JointFn joint, DistFn dv, double eps, GradFn grad)
{
    for (int s = 1; s + 1 < S; s += 2) {
        const double dplus = dv(s), v = dv(s + 1);
        grad(joint(s), (dplus - v) / (2.0 * eps));
    }
    return dv(0);
}

#if defined(__HIPCC__)
struct DevMeshGrad {
    int nitems;         // stencil points of all mesh pairs (the sum of S_k)
    int smax;           // the largest S_k
    const int *sbeg;    // [DevMeshes.npairs + 1] the first stencil point of a mesh pair
    const int *spair;   // [nitems] the mesh pair of a stencil point
    const int *sjoint;  // [nitems] the joint it moves (-1: the centre)
};

#if defined(FBR_KERNELS_COLLISION)
// Stage A.  Work items (mesh pair, tile of 64 candidates), one wave each, pair-major; hs: the WHOLE set (sample / scale / pose
// [C][hs.npairs], the pair's column from ms.col); the other arguments as for fbr_hull_grad_kernel.  rel [mg.nitems][13][C].
__global__ __launch_bounds__(64) void fbr_mesh_grad_frames_kernel(DevModel m, DevHulls hs, DevPairGrad hg, DevMeshes ms, DevMeshGrad mg, long C, long T,
                                                                  const double *__restrict__ q, const double *__restrict__ rpy,
                                                                  const double *__restrict__ bpos, const long *__restrict__ sample,
                                                                  const double *__restrict__ scale, const long *__restrict__ pose, double eps, double se,
                                                                  double omc, double *__restrict__ rel, double *__restrict__ scratch,
                                                                  int *__restrict__ flag)
{
    const int lane = threadIdx.x, n = m.n;
    const long P = hs.npairs, tiles = (C + 63) >> 6, items = ms.npairs * tiles;
    double *scr = scratch + (long)blockIdx.x * hs.fr.nslots * 12 * 64 + lane;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrGradItem w = fbr_grad_item_head(it, tiles, C, T, P, [&](long k) { return FBR_UNI(((fbr_cint_ptr)(unsigned long)ms.col)[k]); }, sample, scale,
                                                 pose, hg.pair, flag);
        const fbr_cint_ptr sb = (fbr_cint_ptr)(unsigned long)(mg.sbeg + w.k);
        const int s0 = FBR_UNI(sb[0]), sk = FBR_UNI(sb[1]) - s0;
        const int ia = FBR_UNI(((fbr_cint_ptr)(unsigned long)hs.pairs)[2 * (long)w.col]);
        const bool swap = FBR_UNI(((fbr_cint_ptr)(unsigned long)ms.mtab)[2 * (long)ia + 1]) == 0;  // (the mesh is the second member's)
        // the constants of the two hulls (wave-uniform loads): a robot hull's offset by slot, a world hull's R | position
        const fbr_cdouble_ptr ccen = (fbr_cdouble_ptr)(unsigned long)hs.fr.cen, cworld = (fbr_cdouble_ptr)(unsigned long)hs.world;
        double xa[12], xb[12];
        for (int i = 0; i < 12; i++) xa[i] = xb[i] = 0.0;
        if (w.ka >= 0) {
            for (int i = 0; i < 3; i++) xa[i] = ccen[3 * w.sla + i];
        } else {
            for (int i = 0; i < 12; i++) xa[i] = cworld[12 * w.sla + i];
        }
        if (w.kb >= 0) {
            for (int i = 0; i < 3; i++) xb[i] = ccen[3 * w.slb + i];
        } else {
            for (int i = 0; i < 12; i++) xb[i] = cworld[12 * w.slb + i];
        }
        // (a world member, step -1, owns no step)
        const FbrGradMask mask = {hg.anc, hg.W, w.ka < 0 ? 0 : w.ka, w.kb < 0 ? 0 : w.kb, (w.ka < 0 ? 0 : 1) | (w.kb < 0 ? 0 : 2)};
        const FbrLaneIO io = fbr_lane_io(m, q + w.sr * n, w.sc, rpy, bpos, w.pr, scr);
        auto rec = [&](int sp, const FbrHullRel &r) {
            if (!w.live || sp >= sk) return;  // (the host's table has the walk's count: nothing is stored past the pair's slots)
            double *o = rel + (long)(s0 + sp) * FBR_MESHGRAD_REL * C + w.c;
            const double v[FBR_MESHGRAD_REL] = {r.t0, r.t1, r.t2, r.C00, r.C01, r.C02, r.C10, r.C11, r.C12, r.C20, r.C21, r.C22, r.chk};
            for (int i = 0; i < FBR_MESHGRAD_REL; i++) o[i * C] = v[i];
        };
        fbr_meshgrad_frames_item(w.ka, w.kb, hs.fr.cmode, xa, xb, swap, eps, se, omc, hs.fr.steps, m.floating && rpy != nullptr, mask, io.qf,
                                 io.basef, io.save, io.load, io.consts, rec);
    }
}

// Stage B.  Work items (stencil point of a mesh pair, tile of 64 candidates), one wave each, pair-major.  rel as stage A left it;
// d [mg.nitems][C].
__global__ __launch_bounds__(64) void fbr_mesh_grad_dist_kernel(DevHulls hs, DevMeshes ms, DevMeshGrad mg, long C, const double *__restrict__ rel,
                                                                double *__restrict__ d)
{
    const int lane = threadIdx.x;
    const long tiles = (C + 63) >> 6, items = mg.nitems * tiles;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long idx = it / tiles, c0 = (it - idx * tiles) << 6;
        const int valid = (int)min(64L, C - c0);
        const long c = c0 + min(lane, valid - 1);  // lanes behind the last candidate repeat its pose and store nothing
        const int k = FBR_UNI(((fbr_cint_ptr)(unsigned long)mg.spair)[idx]);
        const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(ms.pairs + k);
        const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);  // (the meshed hull first)
        FbrDevHull HA, HB;
        fbr_hullgrad_tables(hs, ia, &HA);
        fbr_hullgrad_tables(hs, ib, &HB);
        const fbr_cint_ptr ma = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ia), mb = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ib);
        const long ta0 = FBR_UNI(ma[0]), tb0 = FBR_UNI(mb[0]);
        const FbrMeshT<fbr_cdouble_ptr> MA = {FBR_UNI(ma[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * ta0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * ta0)};
        const FbrMeshT<fbr_cdouble_ptr> MB = {FBR_UNI(mb[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * tb0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * tb0)};
        const double *w = rel + idx * FBR_MESHGRAD_REL * C + c;
        const FbrHullRel r = {w[0], w[C], w[2 * C], w[3 * C], w[4 * C], w[5 * C], w[6 * C], w[7 * C], w[8 * C], w[9 * C], w[10 * C], w[11 * C], w[12 * C]};
        const double dd = fbr_mesh_distance_oriented<true>(r, HA, MA, HB, MB, (fbr_cdouble_ptr)(unsigned long)(ms.sph + 4 * (long)ib), (FbrMeshStats *)nullptr);
        if (lane < valid) d[idx * C + c] = dd;
    }
}

// Stage C.  One lane per (mesh pair, candidate), the candidate fastest; sample / pose and the outputs as for fbr_hull_grad_kernel.
__global__ __launch_bounds__(256) void fbr_mesh_grad_quot_kernel(DevHulls hs, DevMeshes ms, DevMeshGrad mg, int n, long C, long T,
                                                                 const long *__restrict__ sample, const long *__restrict__ pose, double eps,
                                                                 const double *__restrict__ d, double *__restrict__ dist, double *__restrict__ grad)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * ms.npairs) return;
    const long k = i / C, c = i - k * C, e = c * hs.npairs + ms.col[k];
    const long s = sample[e], ps0 = pose ? pose[e] : s;
    const bool bad = s < -1 || s >= T || ps0 < -1 || ps0 >= T;
    if (s < 0 || bad) {
        dist[e] = FBR_CAPSULE_NONE;
        return;
    }
    const int s0 = mg.sbeg[k], sk = mg.sbeg[k + 1] - s0;
    double *g = grad + e * n;
    dist[e] = fbr_meshgrad_quotients(
        sk, [&](int sp) { return mg.sjoint[s0 + sp]; }, [&](int sp) { return d[(long)(s0 + sp) * C + c]; }, eps, [&](int j, double v) { g[j] = v; });
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
