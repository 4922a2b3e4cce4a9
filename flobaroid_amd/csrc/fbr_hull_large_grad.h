// fbr_hull_large_grad.h -- signed distance of convex hulls of 129 to FBR_MAX_LARGE_HULL_VERTICES vertices and its central-difference
// derivative with respect to the joint positions at chosen configurations of candidate trajectories (fbr_large_hull_distance_gradients):
// the gradient half of fbr_model_set_large_hulls, KUKA LWR4 in the reference's default collisionMode "convex".
//
// The rule is the hulls' (excitation/analyticalGradient.py, the `else` branch of the collision block): per joint
// (d(q + eps e_j) - d(q - eps e_j)) / (2 eps), the stencil of the rigid bodies (fbr_rigidgrad_item, fbr_box_grad.h).  The launch shape is
// NOT the hull gradient's, whose lane evaluates all 1 + 2 J stencil points of its pair one after the other: a stencil spans +- 1e-7 rad, so
// it touches at every point when its centre touches, and a touching large pair is up to 4.1e6 arc tests a facet pass.  The three stages of
// the mesh gradient (fbr_mesh_grad.h) instead, for the LARGE pairs of the set -- those with a hull above FBR_MAX_HULL_VERTICES vertices, or
// every pair with option hull_large_all = 1; the others go through fbr_hull_grad_kernel into their own columns:
//   A  fbr_hull_large_grad_frames_kernel: (large pair, tile of 64 candidates), one wave each.  fbr_rigidgrad_item with the recording functor
//      of fbr_meshgrad_frames_item: slot 0 the centre, then + eps, - eps of every evaluated joint in walk order.  The members keep the pair's
//      own order (no swap).  The slot tables (fbr_stencil_table: sbeg, spair, sjoint) are built with the set, for both arrangements of
//      hull_large_all.
//   B  fbr_hull_large_grad_dist_kernel: work items belong to one large pair; their lanes are the flattened (stencil point, candidate)
//      entries of that pair, [sbeg[k] C, sbeg[k + 1] C) in the [nitems][C] layout of the stencil distances, `width` live lanes an item
//      (a power of two, 1 .. 64: option hull_grad_tile, 0: fbr_hull_large_grad_width, the widest that leaves 12 items a CU).  A lane
//      loads its recorded pose and runs fbr_hull_gjk; then the wave ballots the touching live lanes and takes them in ascending order as fbr_hull_large_pairs_kernel does:
//      the pose of lane s broadcast exactly, lane l on fbr_hull_facets(q_s, A, B, l, 64), the 64 partial maxima joined in lane order with
//      g > gap, lane s keeps the result.  Lanes behind the last entry repeat it, are not balloted and store nothing.  No atomics; every loop
//      is bounded by the tables, the 64 bits of the ballot and FBR_HULL_MAX_ITER.  An entry's value depends on its pose alone, not on the
//      width.
//   C  fbr_hull_large_grad_quot_kernel: fbr_meshgrad_quotients per (candidate, large pair).  Entries never evaluated stay the zeros of the
//      caller's memset.
//
// The arithmetic is HIP-free: fbr_hull_large_entry and fbr_hull_large_grad_item restate the three stages on the host, and
// tests/emul/hull_large_grad_emul.cpp holds them, bit for bit, to the single pass -- fbr_rigidgrad_item with fbr_hull_large_distance as
// its functor.
#pragma once
#include "fbr_hull_large.h"
#include "fbr_mesh_grad.h"

// stage B of one entry: the distance of fbr_hull_large_distance on a recorded pose.  facet (may be null): counts the entries that enter the
// facet pass
template <class DP, class IP>
inline double fbr_hull_large_entry(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrHullT<DP, IP> &B, long *facet)
{
    bool touching;
    int it;
    const double res = fbr_hull_gjk(q, A, B, false, &touching, &it);
    if (touching && facet) ++*facet;
    return touching ? fbr_hull_facets_wave(q, A, B) : res;
}

// The three stages of one (pair, configuration) on the host; arguments as for fbr_hullgrad_item, anc / W: the ancestor masks the slot
// table is made from.  nslots: the stencil points of the item, -1 when the recorded poses do not number what fbr_meshgrad_slots says (the
// return value then means nothing).
template <class DP, class IP, class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class GradFn>
inline double fbr_hull_large_grad_item(int ka, int kb, int cmode, const double *xa, const FbrHullT<DP, IP> &HA, const double *xb,
                                       const FbrHullT<DP, IP> &HB, double eps, double se, double omc, const int *steps, const int *anc, int W,
                                       int floating, MaskFn mask, QFn qf, BaseFn basef, SlotSave save, SlotLoad load, ConstFn consts, GradFn grad,
                                       int *nslots, long *facet)
{
    std::vector<int> joint;
    fbr_meshgrad_slots(ka, kb, cmode, steps, anc, W, joint);
    std::vector<FbrHullRel> rel;
    const int S = fbr_meshgrad_frames_item(ka, kb, cmode, xa, xb, false, eps, se, omc, steps, floating, mask, qf, basef, save, load, consts,
                                           [&](int s, const FbrHullRel &r) {
                                               if ((int)rel.size() == s) rel.push_back(r);
                                           });
    if (S != (int)joint.size() || S != (int)rel.size()) {
        *nslots = -1;
        return 0.0;
    }
    *nslots = S;
    std::vector<double> dv((size_t)S);
    for (int s = 0; s < S; s++) dv[s] = fbr_hull_large_entry(rel[s], HA, HB, facet);
    return fbr_meshgrad_quotients(
        S, [&](int s) { return joint[s]; }, [&](int s) { return dv[s]; }, eps, grad);
}

// The live lanes of an item of stage B when option hull_grad_tile is 0: a touching centre makes nearly every lane of its item touch, and the
// wave runs their facet passes one after the other, so a wider item only saves GJK lanes once every wave slot of the card has an item: the
// widest power of two that still leaves `want` items -- the waves the card holds at the kernel's 152 VGPRs, 3 a SIMD --, 1 where the
// entries do not allow it (measured: DESIGN.md, "Large convex hulls").  sbeg [npairs + 1]: the first stencil point of a large pair; C
// candidates.
#define FBR_HULL_LARGE_GRAD_WAVES_PER_CU 12
static inline int fbr_hull_large_grad_width(const int *sbeg, int npairs, long C, long want)
{
    for (int w = 64; w > 1; w >>= 1) {
        long items = 0;
        for (int k = 0; k < npairs; k++) items += ((long)(sbeg[k + 1] - sbeg[k]) * C + w - 1) / w;
        if (items >= want) return w;
    }
    return 1;
}

#if defined(__HIPCC__)
#if defined(FBR_KERNELS_COLLISION)
// Stage A.  Work items (large pair, tile of 64 candidates), one wave each, pair-major.  hs: the view of the large pairs (hs.pairs, hs.col:
// their columns among the hs.ldp pairs of the whole set, null: their own numbers), which sample / scale / pose [C][hs.ldp] and hg.pair are
// laid out by; lg: the slot tables of that view; the other arguments as for fbr_hull_grad_kernel.  rel [lg.nitems][13][C].
__global__ __launch_bounds__(64) void fbr_hull_large_grad_frames_kernel(DevModel m, DevHulls hs, DevPairGrad hg, DevMeshGrad lg, long C, long T,
                                                                        const double *__restrict__ q, const double *__restrict__ rpy,
                                                                        const double *__restrict__ bpos, const long *__restrict__ sample,
                                                                        const double *__restrict__ scale, const long *__restrict__ pose, double eps,
                                                                        double se, double omc, double *__restrict__ rel, double *__restrict__ scratch,
                                                                        int *__restrict__ flag)
{
    const int lane = threadIdx.x, n = m.n;
    const long tiles = (C + 63) >> 6, items = hs.npairs * tiles;
    double *scr = scratch + (long)blockIdx.x * hs.fr.nslots * 12 * 64 + lane;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrGradItem w = fbr_grad_item_head(
            it, tiles, C, T, (long)hs.ldp, [&](long k) { return hs.col ? FBR_UNI(((fbr_cint_ptr)(unsigned long)hs.col)[k]) : (int)k; }, sample, scale, pose,
            hg.pair, flag);
        const fbr_cint_ptr sb = (fbr_cint_ptr)(unsigned long)(lg.sbeg + w.k);
        const int s0 = FBR_UNI(sb[0]), sk = FBR_UNI(sb[1]) - s0;
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
        fbr_meshgrad_frames_item(w.ka, w.kb, hs.fr.cmode, xa, xb, false, eps, se, omc, hs.fr.steps, m.floating && rpy != nullptr, mask, io.qf, io.basef,
                                 io.save, io.load, io.consts, rec);
    }
}

// Stage B.  Work items (large pair, tile of `width` entries of that pair), one wave each, pair-major, tpp tiles a pair (those behind a
// pair's last entry are empty); rel as stage A left it; d [lg.nitems][C].
__global__ __launch_bounds__(64) void fbr_hull_large_grad_dist_kernel(DevHulls hs, DevMeshGrad lg, long C, int width, long tpp,
                                                                      const double *__restrict__ rel, double *__restrict__ d)
{
    const int lane = threadIdx.x;
    const long items = hs.npairs * tpp;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long k = it / tpp, e0 = (it - k * tpp) * width;
        const fbr_cint_ptr sb = (fbr_cint_ptr)(unsigned long)(lg.sbeg + k);
        const int s0 = FBR_UNI(sb[0]), sk = FBR_UNI(sb[1]) - s0;
        const long E = (long)sk * C;
        if (e0 >= E) continue;
        const int valid = (int)min((long)width, E - e0);
        const long f = (long)s0 * C + e0 + min(lane, valid - 1);  // lanes behind the last entry repeat its pose and store nothing
        const long s = f / C, c = f - s * C;
        const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(hs.pairs + k);
        const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
        FbrDevHull HA, HB;
        fbr_hullgrad_tables(hs, ia, &HA);
        fbr_hullgrad_tables(hs, ib, &HB);
        const double *w = rel + s * FBR_MESHGRAD_REL * C + c;
        const FbrHullRel q = {w[0], w[C], w[2 * C], w[3 * C], w[4 * C], w[5 * C], w[6 * C], w[7 * C], w[8 * C], w[9 * C], w[10 * C], w[11 * C], w[12 * C]};
        bool touching;
        int iters;
        double dd = fbr_hull_gjk(q, HA, HB, false, &touching, &iters);
        // the touching entries, one after the other (the repeats behind the last entry are not counted)
        const unsigned long todo = __builtin_amdgcn_ballot_w64(touching && lane < valid);
        dd = fbr_hull_large_touching(todo, q, HA, HB, lane, dd);
        if (lane < valid) d[f] = dd;
    }
}

// Stage C.  One lane per (large pair, candidate), the candidate fastest; sample / pose and the outputs as for fbr_hull_grad_kernel.
__global__ __launch_bounds__(256) void fbr_hull_large_grad_quot_kernel(DevHulls hs, DevMeshGrad lg, int n, long C, long T,
                                                                       const long *__restrict__ sample, const long *__restrict__ pose, double eps,
                                                                       const double *__restrict__ d, double *__restrict__ dist,
                                                                       double *__restrict__ grad)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * hs.npairs) return;
    const long k = i / C, c = i - k * C, e = c * hs.ldp + (hs.col ? hs.col[k] : (int)k);
    const long s = sample[e], ps0 = pose ? pose[e] : s;
    const bool bad = s < -1 || s >= T || ps0 < -1 || ps0 >= T;
    if (s < 0 || bad) {
        dist[e] = FBR_CAPSULE_NONE;
        return;
    }
    const int s0 = lg.sbeg[k], sk = lg.sbeg[k + 1] - s0;
    double *g = grad + e * n;
    dist[e] = fbr_meshgrad_quotients(
        sk, [&](int sp) { return lg.sjoint[s0 + sp]; }, [&](int sp) { return d[(long)(s0 + sp) * C + c]; }, eps, [&](int j, double v) { g[j] = v; });
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
