// fbr_mesh.h -- triangle-mesh collision distances of candidate trajectories: the reference's fullMeshLinks and collisionMode "full"
// (optimizer.py _getLinkCollisionGeometry gives such a link an FCL BVH of triangles instead of a convex hull: cages and other concave shapes).
//
// A mesh is a set of triangles in the axes of its hull (fbr_hull.h: the convex hull of the mesh's vertices stays in the hull tables).  Its
// distance to a geometry X -- a solid convex hull, or a triangle of another mesh -- is the minimum over its triangles of dist(triangle, X);
// dist is the Euclidean distance when the two are apart and EXACTLY 0.0 when they touch or intersect, so a mesh distance is never
// negative (FCL's BVH behaves the same way), and a geometry wholly inside a closed mesh, not touching its surface, has a positive one.
// Brute force: the WALK-MAN simple/ meshes have 30 to 170 triangles.  A triangle is an FbrHullT of nv = 3, nf = ne = 0 whose verts point
// at nine doubles of the table tris [T][9] (expanded: no index indirection, scalar loads, wave-uniform counters) and whose diam is its
// longest edge; the GJK is fbr_hull_gjk, the one of fbr_hull_distance, and where that routine would enter its facet pass this one
// takes 0.0.  Two triangles have a flat Minkowski difference (coplanar or zero-area ones a flatter one still): the tetrahedron test of the
// GJK then never says "inside", and its exits (c) no closer, (d) the iteration cap and |v| <= floor carry these cases.
//
// Culling.  aux [T][5] holds per triangle a bounding sphere (centre | radius, inflated by 4 eps) and the longest edge, sph [nhulls][4] a
// bounding sphere per hull -- over the hull's vertices AND the vertices of the mesh attached to it, which fbr_mesh_validate lets lie 1e-9 x
// the diameter outside the hull's planes: the sphere holds the mesh whatever the caller's tolerance used up --, both computed on the host
// at set time.  A triangle (pair) whose sphere bound |c_A - c_B| - r_A - r_B, deflated
// by FBR_MESH_CULL_K eps scale (scale = |cB - cA| + diam hull A + diam hull B), is not below the lane's best so far is skipped.  Why no
// bit changes: the GJK returns |v| of a point v of the computed Minkowski difference, whose coordinates carry a few eps x scale of
// rounding, so a computed distance is at least the true one - 16 eps scale; the computed bound is at most the true one + 8 eps scale, and
// the true bound is at most the true distance.  A skipped evaluation would therefore have returned more than best + 40 eps scale: it
// could not have won the strict minimum.  The loops stay wave-uniform (FBR_HULL_ANY): a lane that skips is predicated off, a triangle
// that all 64 lanes skip costs no GJK.  Once a lane's best is 0.0 nothing can undercut it and the lane is done.
#pragma once
#include "fbr_hull.h"

#define FBR_MESH_CULL_K 64.0
#define FBR_MESH_EPS 2.220446049250313e-16
#define FBR_MESH_HULL_TOL 1e-9  // x the hull's diameter: how far outside its hull's planes a triangle vertex may lie

template <class DP>
struct FbrMeshT {
    int nt;    // 0: no mesh attached, the hull itself
    DP tris;   // [nt][9]
    DP aux;    // [nt][5] sphere centre | radius | longest edge
};

struct FbrMeshStats {  // (host only: tests/emul/mesh_emul.cpp)
    long evals, culled;
    int max_iter;
};

// bounding sphere and longest edge of the triangle t [9]: the centre is the centroid
inline void fbr_mesh_triangle_aux(const double *t, double *aux)
{
    double r = 0.0, e = 0.0;
    for (int k = 0; k < 3; k++) aux[k] = (t[k] + t[3 + k] + t[6 + k]) / 3.0;
    for (int i = 0; i < 3; i++) {
        const double *a = t + 3 * i, *b = t + 3 * ((i + 1) % 3);
        r = std::max(r, std::sqrt((a[0] - aux[0]) * (a[0] - aux[0]) + (a[1] - aux[1]) * (a[1] - aux[1]) + (a[2] - aux[2]) * (a[2] - aux[2])));
        e = std::max(e, std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])));
    }
    aux[3] = r * (1.0 + 4.0 * FBR_MESH_EPS);
    aux[4] = e;
}

// bounding sphere of the points v [nv][3] -- a hull's vertices -- and of the ne points e [ne][3] -- the vertices of the mesh attached to
// it, which fbr_mesh_validate lets lie 1e-9 x the diameter outside the hull's planes: the middle of the bounding box of v, the largest
// distance of a point of either set from it
inline void fbr_mesh_point_sphere(long nv, const double *v, long ne, const double *e, double *sph)
{
    for (int k = 0; k < 3; k++) {
        double lo = v[k], hi = v[k];
        for (long i = 1; i < nv; i++) lo = std::min(lo, v[3 * i + k]), hi = std::max(hi, v[3 * i + k]);
        sph[k] = 0.5 * (lo + hi);
    }
    double r = 0.0;
    for (long i = 0; i < nv + ne; i++) {
        const double *p = i < nv ? v + 3 * i : e + 3 * (i - nv);
        const double a = p[0] - sph[0], b = p[1] - sph[1], c = p[2] - sph[2];
        r = std::max(r, std::sqrt(a * a + b * b + c * c));
    }
    sph[3] = r * (1.0 + 4.0 * FBR_MESH_EPS);
}

// The triangles of MA (in the axes of hull A; MA.nt >= 1) against B -- the triangles of MB when MB.nt >= 1, else the solid hull B -- folded
// into *best: the body of fbr_mesh_distance_oriented, and of a leaf pair of csrc/fbr_mesh_bvh.h, where MA and MB are the leaves' ranges.
// q: B relative to A; (hb0, hb1, hb2 | hbr): a sphere, in the axes of A, that holds everything of B the call looks at; off: this lane takes
// no part (a NaN pose, or a lane of the wave that does not want this range); slack: the deflation of the bounds.
template <bool CULL, class DP, class IP>
FBR_HD void fbr_mesh_range_oriented(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrMeshT<DP> &MA, const FbrHullT<DP, IP> &B,
                                    const FbrMeshT<DP> &MB, double hb0, double hb1, double hb2, double hbr, double slack, bool off, double *bestp,
                                    FbrMeshStats *stats)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool dead = off;
    double best = *bestp;
    const int nb = MB.nt > 0 ? MB.nt : 1;
#pragma unroll 1
    for (int ta = 0; ta < MA.nt; ta++) {
        if (!FBR_HULL_ANY(!dead && best != 0.0)) break;
        const DP ua = MA.aux + 5 * ta;
        const double a0 = ua[0], a1 = ua[1], a2 = ua[2], ar = ua[3];
        const FbrHullT<DP, IP> TA = {3, 0, 0, MA.tris + 9 * ta, DP(), IP(), ua[4]};
        bool outer = !dead && best != 0.0;
        if (CULL) {
            const double x = a0 - hb0, y = a1 - hb1, z = a2 - hb2;
            outer = outer && (sqrt(x * x + y * y + z * z) - ar - hbr) - slack < best;
        }
        if (!FBR_HULL_ANY(outer)) {
            if (stats) stats->culled += nb;
            continue;
        }
#pragma unroll 1
        for (int tb = 0; tb < nb; tb++) {
            FbrHullT<DP, IP> G = B;
            bool want = outer && best != 0.0;
            if (MB.nt > 0) {
                const DP ub = MB.aux + 5 * tb;
                G = FbrHullT<DP, IP>{3, 0, 0, MB.tris + 9 * tb, DP(), IP(), ub[4]};
                if (CULL) {
                    const double x = a0 - ((q.C00 * ub[0] + q.C01 * ub[1] + q.C02 * ub[2]) + q.t0), y = a1 - ((q.C10 * ub[0] + q.C11 * ub[1] + q.C12 * ub[2]) + q.t1),
                                 z = a2 - ((q.C20 * ub[0] + q.C21 * ub[1] + q.C22 * ub[2]) + q.t2);
                    want = want && (sqrt(x * x + y * y + z * z) - ar - ub[3]) - slack < best;
                }
            }
            if (!FBR_HULL_ANY(want)) {
                if (stats) stats->culled++;
                continue;
            }
            bool touch;
            int it;
            const double d = fbr_hull_gjk(q, TA, G, !want, &touch, &it);
            if (stats) {
                stats->evals++;
                stats->max_iter = it > stats->max_iter ? it : stats->max_iter;
            }
            if (want && d < best) best = d;  // (touching: the GJK returns 0.0)
        }
    }
    *bestp = best;
}

// the deflation of a sphere bound of the pose q between the hulls A and B: FBR_MESH_CULL_K eps x scale
template <class DP, class IP>
FBR_HD double fbr_mesh_slack(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrHullT<DP, IP> &B)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (FBR_MESH_CULL_K * FBR_MESH_EPS) * (sqrt(q.t0 * q.t0 + q.t1 * q.t1 + q.t2 * q.t2) + A.diam + B.diam);
}

// Distance of the mesh MA (in the axes of hull A; MA.nt >= 1) to B: to the triangles of MB when MB.nt >= 1, else to the solid hull B.
// q: B relative to A (fbr_hull_relative); sphB [4]: the bounding sphere of hull B in its axes.  A NaN pose gives a NaN.
template <bool CULL, class DP, class IP>
FBR_HD double fbr_mesh_distance_oriented(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrMeshT<DP> &MA, const FbrHullT<DP, IP> &B,
                                         const FbrMeshT<DP> &MB, DP sphB, FbrMeshStats *stats)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double nan0 = q.chk - q.chk;
    const bool dead = !(nan0 == 0.0);
    double best = FBR_CAPSULE_NONE;
    const double slack = fbr_mesh_slack(q, A, B);
    // the sphere of hull B in the axes of A
    const double hb0 = (q.C00 * sphB[0] + q.C01 * sphB[1] + q.C02 * sphB[2]) + q.t0, hb1 = (q.C10 * sphB[0] + q.C11 * sphB[1] + q.C12 * sphB[2]) + q.t1,
                 hb2 = (q.C20 * sphB[0] + q.C21 * sphB[1] + q.C22 * sphB[2]) + q.t2, hbr = sphB[3];
    fbr_mesh_range_oriented<CULL>(q, A, MA, B, MB, hb0, hb1, hb2, hbr, slack, dead, &best, stats);
    return dead ? nan0 : best;
}

// Distance of the geometries of two hulls of which one at least carries a mesh: dist(mesh_A, hull_B) when only A has one, the same with the
// roles swapped when only B has one, the triangle-triangle minimum when both have.  sphA, sphB: the hulls' bounding spheres.
template <bool CULL, class DP, class IP>
FBR_HD double fbr_mesh_distance(const double *RA, const double *cA, const FbrHullT<DP, IP> &A, const FbrMeshT<DP> &MA, DP sphA, const double *RB,
                                const double *cB, const FbrHullT<DP, IP> &B, const FbrMeshT<DP> &MB, DP sphB, FbrMeshStats *stats)
{
    FbrHullRel q;
    if (MA.nt > 0) {
        fbr_hull_relative(RA, cA, RB, cB, &q);
        return fbr_mesh_distance_oriented<CULL>(q, A, MA, B, MB, sphB, stats);
    }
    fbr_hull_relative(RB, cB, RA, cA, &q);
    return fbr_mesh_distance_oriented<CULL>(q, B, MB, A, MA, sphA, stats);
}

// ---- what fbr_model_set_hull_meshes takes, checked on the host against the hull set in place (HIP-free: tests/emul/mesh_emul.cpp runs the
// same text).  Returns "" when acceptable, else what is wrong.  link, vbeg, fbeg, planes, diam, pairs: the hull set.
inline std::string fbr_mesh_validate(int nhulls, const int32_t *link, const int32_t *fbeg, const double *planes, const double *diam, int npairs,
                                     const int32_t *pairs, int max_triangles, long max_pair_work, int nmesh, const int32_t *hull, const int32_t *tbeg,
                                     const double *tris)
{
    const auto S = [](long v) { return std::to_string(v); };
    if (nhulls <= 0) return "hull meshes: no hull set (fbr_model_set_hulls)";
    if (nmesh < 0 || nmesh > nhulls) return "hull meshes: between 0 and the number of hulls";
    if (nmesh == 0) return "";
    if (!hull || !tbeg || !tris) return "hull meshes: null array";
    if (tbeg[0] != 0) return "hull meshes: tbeg starts at 0";
    std::vector<long> nt((size_t)nhulls, 0);
    for (int i = 0; i < nmesh; i++) {
        const std::string who = "mesh " + S(i) + ": ";
        const int h = hull[i];
        if (h < 0 || h >= nhulls) return who + "hull index out of range";
        if (nt[h] != 0) return who + "hull " + S(h) + " given twice";
        if (link[h] < 0) return who + "hull " + S(h) + " is a world hull (world links are never meshed)";
        const long n = (long)tbeg[i + 1] - tbeg[i];
        if (n < 0) return who + "tbeg not ascending";
        if (n == 0) return who + "no triangle";
        if (n > max_triangles) return who + S(n) + " triangles on hull " + S(h) + ", more than " + S(max_triangles);
        nt[h] = n;
        const double *t = tris + 9 * (size_t)tbeg[i], *Pl = planes + 4 * (size_t)fbeg[h];
        for (long k = 0; k < 9 * n; k++)
            if (!std::isfinite(t[k])) return who + "non-finite triangle";
        for (long f = 0; f < (long)fbeg[h + 1] - fbeg[h]; f++)
            for (long k = 0; k < 3 * n; k++)
                if (Pl[4 * f] * t[3 * k] + Pl[4 * f + 1] * t[3 * k + 1] + Pl[4 * f + 2] * t[3 * k + 2] - Pl[4 * f + 3] > FBR_MESH_HULL_TOL * diam[h])
                    return who + "a vertex of triangle " + S(k / 3) + " lies outside face " + S(f) + " of hull " + S(h) + " by more than 1e-9 x the diameter";
    }
    for (int k = 0; k < npairs; k++) {
        const long a = nt[pairs[2 * k]], b = nt[pairs[2 * k + 1]];
        if (a * b > max_pair_work)
            return "hull pair " + S(k) + ": " + S(a) + " x " + S(b) + " triangle pairs, more than " + S(max_pair_work);
    }
    return "";
}

#if defined(__HIPCC__)
#define FBR_MESH_BATCH 4  // pairs a wave stages in the LDS: a mesh pair is 1e2 to 1e4 hull pairs' work, small batches spread it over the CUs

struct DevMeshes {
    int npairs;          // the pairs of the set with a mesh on either side
    const int *mtab;     // [nhulls][2] tbeg | nt (0: no mesh), by the caller's hull number
    const double *sph;   // [nhulls][4]
    const double *tris;  // [][9]
    const double *aux;   // [][5]
    const int2 *pairs;   // [npairs] hull numbers, the meshed hull first (both meshed: the caller's order), sorted by the first
    const int *col;      // [npairs] the pair's column among the caller's pairs
};

#if defined(FBR_KERNELS_COLLISION)
// work items (block, batch of FBR_MESH_BATCH mesh pairs), one wave each; pval / pidx [nb][hs.ldp]: the columns of ALL pairs of the set (hs: the whole set)
__global__ __launch_bounds__(64) void fbr_mesh_pairs_kernel(DevHulls hs, DevMeshes ms, DevCapTiles tl, long blk0, long nb, const double *__restrict__ fr,
                                                            double *__restrict__ pval, long *__restrict__ pidx)
{
    __shared__ double sd[FBR_MESH_BATCH * 65];
    const int lane = threadIdx.x;
    const long nbatch = (ms.npairs + FBR_MESH_BATCH - 1) / FBR_MESH_BATCH, items = nb * nbatch;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrPairItem w = fbr_pair_item(it, nbatch, FBR_MESH_BATCH, ms.npairs, tl, blk0);
        // lanes behind the last checked sample repeat it, as in fbr_hull_pairs_kernel
        const double *f = fr + w.b * (long)hs.fr.nrob * 12 * 64 + min(lane, w.valid - 1);
        int cura = 0;
        bool have = false;
        double RA[9], cA[3];
        FbrDevHull HA = {0, 0, 0, nullptr, nullptr, nullptr, 0.0};
        for (int i = 0; i < 9; i++) RA[i] = 0.0;
        for (int i = 0; i < 3; i++) cA[i] = 0.0;
        __syncthreads();  // (the item before has been scanned)
#pragma unroll 1
        for (int j = 0; j < w.cnt; j++) {
            const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(ms.pairs + w.k0 + j);
            const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
            if (!have || ia != cura) {
                fbr_hull_fetch(hs, ia, f, RA, cA, &HA);
                cura = ia;
                have = true;
            }
            double RB[9], cB[3];
            FbrDevHull HB;
            fbr_hull_fetch(hs, ib, f, RB, cB, &HB);
            const fbr_cint_ptr ma = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ia), mb = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ib);
            const long ta0 = FBR_UNI(ma[0]), tb0 = FBR_UNI(mb[0]);
            const FbrMeshT<fbr_cdouble_ptr> MA = {FBR_UNI(ma[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * ta0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * ta0)};
            const FbrMeshT<fbr_cdouble_ptr> MB = {FBR_UNI(mb[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * tb0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * tb0)};
            FbrHullRel q;
            fbr_hull_relative(RA, cA, RB, cB, &q);
            sd[j * 65 + lane] = fbr_mesh_distance_oriented<true>(q, HA, MA, HB, MB, (fbr_cdouble_ptr)(unsigned long)(ms.sph + 4 * (long)ib), (FbrMeshStats *)nullptr);
        }
        __syncthreads();
        fbr_pair_scan_store(sd, w, lane, tl, hs.ldp, [&](int k) { return ms.col[k]; }, pval, pidx);
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
