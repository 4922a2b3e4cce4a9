// fbr_mesh_bvh_grad.h -- distance of triangle meshes behind a tree (fbr_mesh_bvh.h, fbr_model_set_large_hull_meshes) and its
// central-difference derivative with respect to the joint positions at chosen configurations of candidate trajectories
// (fbr_large_mesh_distance_gradients): the gradient half of KUKA LWR4's collisionMode "full".
//
// The rule is the meshes' (fbr_mesh_grad.h): per joint (d(q + eps e_j) - d(q - eps e_j)) / (2 eps) over the stencil of fbr_rigidgrad_item, in
// three stages.  Stages A and C do not depend on the size of a mesh and are the kernels of fbr_mesh_grad.h, their text unchanged
// (fbr_mesh_grad_frames_kernel, fbr_mesh_grad_quot_kernel) on the MESH view and the stencil table of a tree attachment.  Stage B is new:
//   B  fbr_mesh_bvh_grad_dist_kernel: one wave per work item, the wave's node-pair stack in the LDS as in fbr_mesh_bvh_pairs_kernel.  A lane
//      loads its recorded pose, calls fbr_mesh_bvh_distance<1> -- the traversal's text is not changed, so its proof that no skip changes a
//      bit carries over and every stencil value has the bits fbr_mesh_distance_oriented<true> returns for that pose -- and stores one
//      double.
// Which 64 entries share a wave.  The traversal is the wave's: a node pair is visited when ANY live lane wants it, so a wave pays for the
// union of its lanes' walks.  The candidates of one stencil point sit at unrelated winning configurations; the S_k = 1 + 2 J_k stencil
// points of one (pair, candidate) differ by +- eps in one joint and walk the same walk.  So the lanes are the flattened entries of ONE
// mesh pair, an item 64 consecutive entries (as fbr_hull_large_grad_dist_kernel flattens its own), in one of two orders
// (fbr_mesh_bvh_grad_entry; option mesh_grad_order, 0: FBR_MESH_GRAD_ORDER_DEFAULT, decided by measurement: DESIGN.md):
//   candidate-major  e = c S_k + s: a wave holds all stencil points of about 64 / S_k candidates (S_k > 64: they run on into the next item);
//   slot-major       e = s C + c:   a wave holds one stencil point of 64 candidates where C allows.
// Lanes behind the last entry of the pair repeat it and store nothing: they add nothing to the union.  A lane whose candidate has no sample
// evaluates the clamped pose stage A recorded, and stage C drops it.  All control flow around the call depends on the item alone.  An
// entry's value depends on its pose alone, never on the order.
//
// The arithmetic is HIP-free: fbr_mesh_bvh_grad_entry (the mapping the kernel and the host share) and fbr_mesh_bvh_grad_item restate the
// three stages on the host, and tests/emul/mesh_bvh_grad_emul.cpp holds them, bit for bit, to the single pass -- fbr_rigidgrad_item with
// the brute-force fbr_mesh_distance as its functor.
#pragma once
#include "fbr_mesh_bvh.h"
#include "fbr_mesh_grad.h"

enum { FBR_MESH_GRAD_CANDIDATE_MAJOR = 1, FBR_MESH_GRAD_SLOT_MAJOR = 2 };
#define FBR_MESH_GRAD_ORDER_DEFAULT FBR_MESH_GRAD_CANDIDATE_MAJOR  // what option mesh_grad_order = 0 means (measured: DESIGN.md)

// Entry e of a pair with S stencil points and C candidates -> its stencil point *s and candidate *c; order: one of the two above.
FBR_HD void fbr_mesh_bvh_grad_entry(int order, long e, int S, long C, int *s, long *c)
{
    if (order == FBR_MESH_GRAD_SLOT_MAJOR) {
        const long sl = e / C;
        *s = (int)sl, *c = e - sl * C;
    } else {
        const long cl = e / S;
        *c = cl, *s = (int)(e - cl * S);
    }
}

// the inverse: the entry of (stencil point s, candidate c)
FBR_HD long fbr_mesh_bvh_grad_entry_of(int order, int s, long c, int S, long C)
{
    return order == FBR_MESH_GRAD_SLOT_MAJOR ? (long)s * C + c : c * (long)S + s;
}

// Tile t of a pair with E = S C entries, 64 consecutive entries a tile: its first entry *e0; returns its entries, 1 .. 64, or 0 for a tile
// behind the pair's last entry.  Lane l of the tile takes entry *e0 + min(l, entries - 1): no lane leaves [0, E).
FBR_HD int fbr_mesh_bvh_grad_tile(long t, long E, long *e0)
{
    *e0 = t << 6;
    if (*e0 >= E) return 0;
    return E - *e0 < 64 ? (int)(E - *e0) : 64;
}

// stage B of one entry: fbr_mesh_bvh_distance of one pose, the meshed hull A first (B: a mesh with its tree, or MB.nt == 0: the solid
// hull with the sphere sphB).  stk [2 FBR_MESH_BVH_STACK]
template <class DP, class IP>
inline double fbr_mesh_bvh_grad_value(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrMeshT<DP> &MA, IP nodeA, DP volA,
                                      const FbrHullT<DP, IP> &B, const FbrMeshT<DP> &MB, IP nodeB, DP volB, DP sphB, int *stk, FbrMeshBvhStats *stats)
{
    double out;
    fbr_mesh_bvh_distance<1>(1, &q, A, MA, nodeA, volA, B, MB, nodeB, volB, sphB, stk, &out, stats);
    return out;
}

// One member of a pair as the restatement takes it: the hull, its mesh in tree order (nt == 0: none), the tree and the sphere of the table
// sph (fbr_mesh_point_sphere).
template <class DP, class IP> struct FbrMeshBvhMember {
    FbrHullT<DP, IP> hull;
    FbrMeshT<DP> mesh;
    IP node;
    DP vol, sph;
};

// The three stages of one (pair, configuration) on the host; arguments as for fbr_hull_large_grad_item, the members in the pair's own order
// (at least one carries a mesh: the recorded pose has the meshed one first, the first of two).  nslots: the stencil points of the item,
// -1 when the recorded poses do not number what fbr_meshgrad_slots says (the return value then means nothing).
template <class DP, class IP, class MaskFn, class QFn, class BaseFn, class SlotSave, class SlotLoad, class ConstFn, class GradFn>
inline double fbr_mesh_bvh_grad_item(int ka, int kb, int cmode, const double *xa, const FbrMeshBvhMember<DP, IP> &PA, const double *xb,
                                     const FbrMeshBvhMember<DP, IP> &PB, double eps, double se, double omc, const int *steps, const int *anc, int W,
                                     int floating, MaskFn mask, QFn qf, BaseFn basef, SlotSave save, SlotLoad load, ConstFn consts, GradFn grad,
                                     int *nslots, FbrMeshBvhStats *stats)
{
    std::vector<int> joint;
    fbr_meshgrad_slots(ka, kb, cmode, steps, anc, W, joint);
    std::vector<FbrHullRel> rel;
    const bool swap = PA.mesh.nt == 0;
    const int S = fbr_meshgrad_frames_item(ka, kb, cmode, xa, xb, swap, eps, se, omc, steps, floating, mask, qf, basef, save, load, consts,
                                           [&](int s, const FbrHullRel &r) {
                                               if ((int)rel.size() == s) rel.push_back(r);
                                           });
    if (S != (int)joint.size() || S != (int)rel.size()) {
        *nslots = -1;
        return 0.0;
    }
    *nslots = S;
    const FbrMeshBvhMember<DP, IP> &A = swap ? PB : PA, &B = swap ? PA : PB;
    int stk[2 * FBR_MESH_BVH_STACK];
    std::vector<double> dv((size_t)S);
    for (int s = 0; s < S; s++)
        dv[s] = fbr_mesh_bvh_grad_value(rel[s], A.hull, A.mesh, A.node, A.vol, B.hull, B.mesh, B.node, B.vol, B.sph, stk, stats);
    return fbr_meshgrad_quotients(
        S, [&](int s) { return joint[s]; }, [&](int s) { return dv[s]; }, eps, grad);
}

#if defined(__HIPCC__)
#if defined(FBR_KERNELS_COLLISION)
// Stage B.  Work items (mesh pair, tile of 64 entries of that pair), one wave each, pair-major, tpp tiles a pair (those behind a pair's last
// entry are empty); ms, bv: the tables of fbr_model_set_large_hull_meshes with the MESH view's pairs (the meshed hull first); mg: its stencil
// table; order: FBR_MESH_GRAD_CANDIDATE_MAJOR or FBR_MESH_GRAD_SLOT_MAJOR; rel [mg.nitems][13][C] as stage A left it; d [mg.nitems][C].
__global__ __launch_bounds__(64) void fbr_mesh_bvh_grad_dist_kernel(DevHulls hs, DevMeshes ms, DevMeshBvh bv, DevMeshGrad mg, long C, int order, long tpp,
                                                                    const double *__restrict__ rel, double *__restrict__ d)
{
    __shared__ int stk[2 * FBR_MESH_BVH_STACK];
    const int lane = threadIdx.x;
    const long items = ms.npairs * tpp;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long k = it / tpp;
        const fbr_cint_ptr sb = (fbr_cint_ptr)(unsigned long)(mg.sbeg + k);
        const int s0 = FBR_UNI(sb[0]), sk = FBR_UNI(sb[1]) - s0;
        const long E = (long)sk * C;
        long e0;
        const int valid = fbr_mesh_bvh_grad_tile(it - k * tpp, E, &e0);
        if (valid == 0) continue;
        int s;
        long c;
        fbr_mesh_bvh_grad_entry(order, e0 + min(lane, valid - 1), sk, C, &s, &c);  // lanes behind the last entry repeat its pose and store nothing
        const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(ms.pairs + k);
        const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);  // (the meshed hull first)
        FbrDevHull HA, HB;
        fbr_hullgrad_tables(hs, ia, &HA);
        fbr_hullgrad_tables(hs, ib, &HB);
        const fbr_cint_ptr ma = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ia), mb = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ib);
        const long ta0 = FBR_UNI(ma[0]), tb0 = FBR_UNI(mb[0]);
        const FbrMeshT<fbr_cdouble_ptr> MA = {FBR_UNI(ma[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * ta0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * ta0)};
        const FbrMeshT<fbr_cdouble_ptr> MB = {FBR_UNI(mb[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * tb0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * tb0)};
        const fbr_cint_ptr nbeg = (fbr_cint_ptr)(unsigned long)bv.nbeg;
        const long na0 = FBR_UNI(nbeg[ia]), nb0 = FBR_UNI(nbeg[ib]);
        const long f = (long)(s0 + s) * C + c;
        const double *w = rel + (long)(s0 + s) * FBR_MESHGRAD_REL * C + c;
        const FbrHullRel q = {w[0], w[C], w[2 * C], w[3 * C], w[4 * C], w[5 * C], w[6 * C], w[7 * C], w[8 * C], w[9 * C], w[10 * C], w[11 * C], w[12 * C]};
        double dd;
        fbr_mesh_bvh_distance<1>(1, &q, HA, MA, (fbr_cint_ptr)(unsigned long)(bv.node + 4 * na0), (fbr_cdouble_ptr)(unsigned long)(bv.vol + 4 * na0), HB, MB,
                                 (fbr_cint_ptr)(unsigned long)(bv.node + 4 * nb0), (fbr_cdouble_ptr)(unsigned long)(bv.vol + 4 * nb0),
                                 (fbr_cdouble_ptr)(unsigned long)(ms.sph + 4 * (long)ib), stk, &dd, (FbrMeshBvhStats *)nullptr);
        if (lane < valid) d[f] = dd;
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
