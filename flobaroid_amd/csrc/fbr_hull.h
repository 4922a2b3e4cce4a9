// fbr_hull.h -- convex-hull collision distances of candidate trajectories (fbr_candidate_hull_distances).
//
// Covers the reference's default collisionMode "convex": every pair of the collision block goes to fcl.distance on the convex hull of the
// link's mesh (optimizer.py _getLinkCollisionGeometry: collision mesh, else visual mesh, times the URDF scale; links without a mesh and all
// world links fall back to a box, here a hull of 8 vertices).  A hull is a rotation, a centre (p_link + offset) and three wave-uniform tables
// in the hull's own axes: vertices [V][3], merged faces [F][4] (unit outward normal | offset: n.x <= o inside) and edges [E][4] (two end
// vertices | the two faces that meet there).  fbr_hull_distance is fbr_box_distance's definition for general polytopes:
//   * separated: the Euclidean distance, by GJK on the Minkowski difference A - B in the frame of A.  The closest point of the simplex is
//     found in fp64 by Voronoi regions (segment, triangle; a tetrahedron: its three new faces, and the barycentric signs for "inside").  It
//     ends when the new support pair is already in the simplex (finite for polytopes, exact to rounding), when the duality gap
//     |v|^2 - v.w is below FBR_HULL_GAP_REL |v|^2 + FBR_HULL_NOISE |v| scale, when the simplex no longer comes closer, or at
//     FBR_HULL_MAX_ITER (it returns the current |v|);
//   * touching or overlapping (the simplex encloses the origin, or |v| <= FBR_HULL_NOISE scale): the largest signed gap over the facets of
//     the Minkowski difference -- the faces of A, the faces of B and the edge pairs that form a Minkowski face (Gauss-map arc test, O(1) a
//     pair).  <= 0: the negated minimum translation; should it come out positive, it is returned as it is.
// scale = |cB - cA| + diam A + diam B.  Contraction of a * b + c into an FMA is switched off in fbr_hull_distance: GJK takes discrete
// decisions, and the g++ emulation (tests/emul/hull_emul.cpp, -ffp-contract=off) then walks the same simplices as the device.
// The reference's FCL returns a GJK/EPA value of tolerance 1e-6, build-dependent when negative: only the sign is common ground.
//
// Frames: R_link | p_link + offset per checked sample is what fbr_box_frames_kernel writes for a box centre; the hull set carries a DevBoxes
// view (steps, slots, offsets) and that kernel is reused.  fbr_hull_pairs_kernel has the structure of fbr_box_pairs_kernel.
// The GJK loop (fbr_hull_gjk) and the relative pose (fbr_hull_relative) are functions of their own: fbr_mesh.h calls them on triangles.
// So is the facet pass (fbr_hull_facets), over every facet or over one part of them: fbr_hull_large.h deals the parts to the lanes of a wave
// for hulls of 129 to FBR_MAX_LARGE_HULL_VERTICES vertices (fbr_model_set_large_hulls).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "fbr_box.h"

#define FBR_HULL_MAX_ITER 64                     // GJK iterations of one evaluation (largest seen: DESIGN.md)
#define FBR_HULL_GAP_REL 1e-15                   // duality gap relative to |v|^2
#define FBR_HULL_NOISE (8.0 * 2.220446049250313e-16)  // x scale: below this |v| counts as touching; x |v| scale: the roundings of v.w
#define FBR_HULL_FLAT 1e-12                      // x scale^3: a tetrahedron of smaller volume (x 6) encloses nothing
#ifndef FBR_HULL_KEY_BITS                        // (tests/test_hulls_large.py builds the emulation once more with 8, the width of before)
#define FBR_HULL_KEY_BITS 10                     // a support pair's key is (ia << 10) | ib: unique up to FBR_MAX_LARGE_HULL_VERTICES = 1 << 10
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define FBR_HULL_ANY(p) (__builtin_amdgcn_ballot_w64(p) != 0)  // the wave's vote: the loops below are wave-uniform
#else
#define FBR_HULL_ANY(p) (p)
#endif

// tables of one hull; DP / IP: plain pointers on the host, constant-address-space pointers (scalar loads) on the device
template <class DP, class IP>
struct FbrHullT {
    int nv, nf, ne;
    DP verts;   // [nv][3]
    DP planes;  // [nf][4]
    IP edges;   // [ne][4]
    double diam;
};

// the vertex furthest along d; returns its index
template <class DP>
FBR_HD int fbr_hull_support(int nv, DP verts, double d0, double d1, double d2, double *p)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double best = -1e300;
    int ib = 0;
    p[0] = p[1] = p[2] = 0.0;
#pragma unroll 4
    for (int i = 0; i < nv; i++) {
        const double x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
        const double s = d0 * x + d1 * y + d2 * z;
        if (s > best) {
            best = s;
            ib = i;
            p[0] = x;
            p[1] = y;
            p[2] = z;
        }
    }
    return ib;
}

// the smallest d . v over the vertices
template <class DP>
FBR_HD double fbr_hull_low(int nv, DP verts, double d0, double d1, double d2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double low = 1e300;
#pragma unroll 4
    for (int i = 0; i < nv; i++) {
        const double s = d0 * verts[3 * i] + d1 * verts[3 * i + 1] + d2 * verts[3 * i + 2];
        low = s < low ? s : low;
    }
    return low;
}

// barycentric coordinates (la, lb, lc) of the point of the triangle a b c closest to the origin (Ericson, Real-Time Collision Detection 5.1.5)
FBR_HD void fbr_hull_triangle(const double *a, const double *b, const double *c, double *la, double *lb, double *lc)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2], ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const double d1 = -(ab0 * a[0] + ab1 * a[1] + ab2 * a[2]), d2 = -(ac0 * a[0] + ac1 * a[1] + ac2 * a[2]);
    const double d3 = -(ab0 * b[0] + ab1 * b[1] + ab2 * b[2]), d4 = -(ac0 * b[0] + ac1 * b[1] + ac2 * b[2]);
    const double d5 = -(ab0 * c[0] + ab1 * c[1] + ab2 * c[2]), d6 = -(ac0 * c[0] + ac1 * c[1] + ac2 * c[2]);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    double x = 1.0, y = 0.0, z = 0.0;
    if (d1 <= 0.0 && d2 <= 0.0) {  // the vertex a
    } else if (d3 >= 0.0 && d4 <= d3) {
        x = 0.0, y = 1.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // the edge a b
        y = d1 / (d1 - d3);
        x = 1.0 - y;
    } else if (d6 >= 0.0 && d5 <= d6) {
        x = 0.0, z = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // the edge a c
        z = d2 / (d2 - d6);
        x = 1.0 - z;
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {  // the edge b c
        z = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        y = 1.0 - z;
        x = 0.0;
    } else {  // the face
        const double den = 1.0 / (va + vb + vc);
        y = vb * den;
        z = vc * den;
        x = 1.0 - y - z;
    }
    *la = x;
    *lb = y;
    *lc = z;
}

// det(x - w, y - w, z - w)
FBR_HD double fbr_hull_det(const double *w, const double *x, const double *y, const double *z)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a0 = x[0] - w[0], a1 = x[1] - w[1], a2 = x[2] - w[2], b0 = y[0] - w[0], b1 = y[1] - w[1], b2 = y[2] - w[2];
    const double c0 = z[0] - w[0], c1 = z[1] - w[1], c2 = z[2] - w[2];
    return a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
}

// slots i and j of the simplex change places when i is empty and j is not (constant indices: the arrays stay in registers)
#define FBR_HULL_SINK(i, j)                          \
    if (lam[i] == 0.0 && lam[j] != 0.0) {            \
        for (int k_ = 0; k_ < 3; k_++) {             \
            const double r_ = P[i][k_];              \
            P[i][k_] = P[j][k_];                     \
            P[j][k_] = r_;                           \
        }                                            \
        const int q_ = id[i];                        \
        id[i] = id[j];                               \
        id[j] = q_;                                  \
        lam[i] = lam[j];                             \
        lam[j] = 0.0;                                \
    }

// B in the frame of A: C = RA^T RB, t = RA^T (cB - cA); chk - chk is 0.0 for finite poses and a NaN otherwise
struct FbrHullRel {
    double t0, t1, t2, C00, C01, C02, C10, C11, C12, C20, C21, C22, chk;
};

FBR_HD void fbr_hull_relative(const double *RA, const double *cA, const double *RB, const double *cB, FbrHullRel *q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d0 = cB[0] - cA[0], d1 = cB[1] - cA[1], d2 = cB[2] - cA[2];
    q->t0 = RA[0] * d0 + RA[3] * d1 + RA[6] * d2, q->t1 = RA[1] * d0 + RA[4] * d1 + RA[7] * d2, q->t2 = RA[2] * d0 + RA[5] * d1 + RA[8] * d2;
    q->C00 = RA[0] * RB[0] + RA[3] * RB[3] + RA[6] * RB[6], q->C01 = RA[0] * RB[1] + RA[3] * RB[4] + RA[6] * RB[7],
    q->C02 = RA[0] * RB[2] + RA[3] * RB[5] + RA[6] * RB[8];
    q->C10 = RA[1] * RB[0] + RA[4] * RB[3] + RA[7] * RB[6], q->C11 = RA[1] * RB[1] + RA[4] * RB[4] + RA[7] * RB[7],
    q->C12 = RA[1] * RB[2] + RA[4] * RB[5] + RA[7] * RB[8];
    q->C20 = RA[2] * RB[0] + RA[5] * RB[3] + RA[8] * RB[6], q->C21 = RA[2] * RB[1] + RA[5] * RB[4] + RA[8] * RB[7],
    q->C22 = RA[2] * RB[2] + RA[5] * RB[5] + RA[8] * RB[8];
    q->chk = (q->t0 + q->t1 + q->t2) + (q->C00 + q->C01 + q->C02) + (q->C10 + q->C11 + q->C12) + (q->C20 + q->C21 + q->C22);
}

// GJK on A - (C B + t), shared by fbr_hull_distance and fbr_mesh_distance (csrc/fbr_mesh.h: A or B may be a triangle, nv = 3, whose
// Minkowski difference with a triangle is flat -- then the tetrahedron never encloses the origin and the exits below carry the case).
// Returns |v| when the two are apart, a NaN for a NaN pose, and 0.0 with *touching set when the simplex encloses the origin or
// |v| <= FBR_HULL_NOISE scale.  skip: this lane takes no part (the loop is the wave's); its return value means nothing.
// *it: the iterations taken.
template <class DP, class IP>
FBR_HD double fbr_hull_gjk(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrHullT<DP, IP> &B, bool skip, bool *touch, int *itp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t0 = q.t0, t1 = q.t1, t2 = q.t2, C00 = q.C00, C01 = q.C01, C02 = q.C02, C10 = q.C10, C11 = q.C11, C12 = q.C12, C20 = q.C20,
                 C21 = q.C21, C22 = q.C22;
    double res = q.chk - q.chk;        // (a NaN pose never wins a minimum)
    bool done = !(res == 0.0) || skip, touching = false;
    const double scale = sqrt(t0 * t0 + t1 * t1 + t2 * t2) + A.diam + B.diam;
    const double floor2 = (FBR_HULL_NOISE * scale) * (FBR_HULL_NOISE * scale);

    // ---- GJK: the point v of A - (C B + t) closest to the origin.  The simplex: slots 0 .. n - 1 of P (n <= 3 between the iterations), the
    // new point in slot 3; id: the support pair of a slot.
    double P[4][3], lam[4] = {1.0, 0.0, 0.0, 0.0}, v0, v1, v2;
    int id[4] = {0, -1, -1, -1}, n = 1, it = 0;
    {
        const double bx = B.verts[0], by = B.verts[1], bz = B.verts[2];
        v0 = P[0][0] = A.verts[0] - ((C00 * bx + C01 * by + C02 * bz) + t0);
        v1 = P[0][1] = A.verts[1] - ((C10 * bx + C11 * by + C12 * bz) + t1);
        v2 = P[0][2] = A.verts[2] - ((C20 * bx + C21 * by + C22 * bz) + t2);
        for (int i = 1; i < 4; i++) P[i][0] = P[i][1] = P[i][2] = 0.0;
    }
    while (FBR_HULL_ANY(!done)) {
        if (!done) {
            const double vv = v0 * v0 + v1 * v1 + v2 * v2;
            if (vv <= floor2) {
                touching = done = true;
            } else {
                double pa[3], pb[3];
                const int ia = fbr_hull_support(A.nv, A.verts, -v0, -v1, -v2, pa);
                const int ib = fbr_hull_support(B.nv, B.verts, C00 * v0 + C10 * v1 + C20 * v2, C01 * v0 + C11 * v1 + C21 * v2,
                                                C02 * v0 + C12 * v1 + C22 * v2, pb);
                const int key = (ia << FBR_HULL_KEY_BITS) | ib;
                P[3][0] = pa[0] - ((C00 * pb[0] + C01 * pb[1] + C02 * pb[2]) + t0);
                P[3][1] = pa[1] - ((C10 * pb[0] + C11 * pb[1] + C12 * pb[2]) + t1);
                P[3][2] = pa[2] - ((C20 * pb[0] + C21 * pb[1] + C22 * pb[2]) + t2);
                id[3] = key;
                const double vw = v0 * P[3][0] + v1 * P[3][1] + v2 * P[3][2];
                const bool dup = id[0] == key || (n > 1 && id[1] == key) || (n > 2 && id[2] == key);
                if (dup || vv - vw <= FBR_HULL_GAP_REL * vv + FBR_HULL_NOISE * scale * sqrt(vv) || it >= FBR_HULL_MAX_ITER) {
                    res = sqrt(vv);
                    done = true;
                } else {
                    it++;
                    double bvv = 1e300;
                    lam[0] = lam[1] = lam[2] = lam[3] = 0.0;
                    if (n == 1) {  // the segment P0 P3
                        const double e0 = P[3][0] - P[0][0], e1 = P[3][1] - P[0][1], e2 = P[3][2] - P[0][2];
                        const double ee = e0 * e0 + e1 * e1 + e2 * e2;
                        const double s = ee > 0.0 ? fbr_clip01(-(P[0][0] * e0 + P[0][1] * e1 + P[0][2] * e2) / ee) : 0.0;
                        lam[0] = 1.0 - s;
                        lam[3] = s;
                    } else {
                        bool inside = false;
                        if (n == 3) {  // O = sum l_i P_i, sum l_i = 1: l_i = det with P_i replaced by O / det
                            const double O[3] = {0.0, 0.0, 0.0};
                            const double V = fbr_hull_det(P[0], P[1], P[2], P[3]);
                            const double s = V < 0.0 ? -1.0 : 1.0;
                            inside = fabs(V) > FBR_HULL_FLAT * scale * scale * scale && s * fbr_hull_det(O, P[1], P[2], P[3]) > 0.0 &&
                                     s * fbr_hull_det(P[0], O, P[2], P[3]) > 0.0 && s * fbr_hull_det(P[0], P[1], O, P[3]) > 0.0 &&
                                     s * fbr_hull_det(P[0], P[1], P[2], O) > 0.0;
                        }
                        if (inside) {
                            touching = done = true;
                        } else {
                            // the faces (P0, P1, P3), (P1, P2, P3), (P2, P0, P3): always slots 0 and 1, which rotate; with two old points
                            // only the first.  The best weights rotate with their points.
#pragma unroll 1
                            for (int f = 0; f < 3; f++) {
                                if (f == 0 || n == 3) {
                                    double x, y, z;
                                    fbr_hull_triangle(P[0], P[1], P[3], &x, &y, &z);
                                    const double w0 = (x * P[0][0] + y * P[1][0]) + z * P[3][0], w1 = (x * P[0][1] + y * P[1][1]) + z * P[3][1],
                                                 w2 = (x * P[0][2] + y * P[1][2]) + z * P[3][2];
                                    const double ww = w0 * w0 + w1 * w1 + w2 * w2;
                                    if (ww < bvv) {
                                        bvv = ww;
                                        lam[0] = x, lam[1] = y, lam[2] = 0.0, lam[3] = z;
                                    }
                                }
                                FBR_BOX_ROT(P[0][0], P[1][0], P[2][0])
                                FBR_BOX_ROT(P[0][1], P[1][1], P[2][1])
                                FBR_BOX_ROT(P[0][2], P[1][2], P[2][2])
                                FBR_BOX_ROT(lam[0], lam[1], lam[2])
                                {
                                    const int q_ = id[0];
                                    id[0] = id[1], id[1] = id[2], id[2] = q_;
                                }
                            }
                        }
                    }
                    if (!done) {
                        const double w0 = ((lam[0] * P[0][0] + lam[1] * P[1][0]) + lam[2] * P[2][0]) + lam[3] * P[3][0],
                                     w1 = ((lam[0] * P[0][1] + lam[1] * P[1][1]) + lam[2] * P[2][1]) + lam[3] * P[3][1],
                                     w2 = ((lam[0] * P[0][2] + lam[1] * P[1][2]) + lam[2] * P[2][2]) + lam[3] * P[3][2];
                        const double ww = w0 * w0 + w1 * w1 + w2 * w2;
                        if (!(ww < vv)) {  // no closer (or a NaN from a degenerate triangle): v stands
                            res = sqrt(vv);
                            done = true;
                        } else {
                            v0 = w0, v1 = w1, v2 = w2;
                            FBR_HULL_SINK(0, 1)
                            FBR_HULL_SINK(1, 2)
                            FBR_HULL_SINK(2, 3)
                            FBR_HULL_SINK(0, 1)
                            FBR_HULL_SINK(1, 2)
                            FBR_HULL_SINK(0, 1)
                            n = (lam[0] != 0.0) + (lam[1] != 0.0) + (lam[2] != 0.0) + (lam[3] != 0.0);
                            if (n == 4) {  // (weights of a face are never all four: kept for safety)
                                touching = done = true;
                            }
                        }
                    }
                }
            }
        }
    }
    *touch = touching;
    *itp = it;
    return res;
}

// The facet pass of a touching or overlapping pair: the largest signed gap over those facets of the Minkowski difference A - (C B + t) whose
// index is `part` modulo `nparts` -- the faces of A, the faces of B, and the edges of B, each against every edge of A (the inner loop stays
// whole).  (0, 1): all of them, what fbr_hull_distance returns for a touching pair.  A maximum: the parts may be taken in any order and
// joined with the same rule (g > gap: a NaN is never taken); only the sign of a zero may depend on the order.  -1e300 for an empty part.
// (csrc/fbr_hull_large.h shares one pass among the 64 lanes of a wave.)
template <class DP, class IP>
FBR_HD double fbr_hull_facets(const FbrHullRel &q, const FbrHullT<DP, IP> &A, const FbrHullT<DP, IP> &B, int part, int nparts)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t0 = q.t0, t1 = q.t1, t2 = q.t2, C00 = q.C00, C01 = q.C01, C02 = q.C02, C10 = q.C10, C11 = q.C11, C12 = q.C12, C20 = q.C20,
                 C21 = q.C21, C22 = q.C22;
    double gap = -1e300;
#pragma unroll 1
    for (int f = part; f < A.nf; f += nparts) {  // the faces of A: n . t - o + min over B of (C^T n) . v
        const double n0 = A.planes[4 * f], n1 = A.planes[4 * f + 1], n2 = A.planes[4 * f + 2], o = A.planes[4 * f + 3];
        const double low = fbr_hull_low(B.nv, B.verts, C00 * n0 + C10 * n1 + C20 * n2, C01 * n0 + C11 * n1 + C21 * n2,
                                        C02 * n0 + C12 * n1 + C22 * n2);
        const double g = ((n0 * t0 + n1 * t1 + n2 * t2) - o) + low;
        gap = g > gap ? g : gap;
    }
#pragma unroll 1
    for (int f = part; f < B.nf; f += nparts) {  // the faces of B, their normals C n in A's axes: min over A of (C n) . v - (C n) . t - o
        const double m0 = B.planes[4 * f], m1 = B.planes[4 * f + 1], m2 = B.planes[4 * f + 2], o = B.planes[4 * f + 3];
        const double n0 = C00 * m0 + C01 * m1 + C02 * m2, n1 = C10 * m0 + C11 * m1 + C12 * m2, n2 = C20 * m0 + C21 * m1 + C22 * m2;
        const double g = (fbr_hull_low(A.nv, A.verts, n0, n1, n2) - (n0 * t0 + n1 * t1 + n2 * t2)) - o;
        gap = g > gap ? g : gap;
    }
    // The edge pairs that form a face of the Minkowski difference: on the Gauss map the arc between the normals a, b of the two
    // faces at A's edge crosses the arc between the negated normals c, d at B's edge (Gregorius, "The Separating Axis Test between
    // Convex Polyhedra", GDC 2013).  The axis: the normalised cross product of the edges, turned out of A.
#pragma unroll 1
    for (int eb = part; eb < B.ne; eb += nparts) {
        const int bv0 = B.edges[4 * eb], bv1 = B.edges[4 * eb + 1], bf0 = B.edges[4 * eb + 2], bf1 = B.edges[4 * eb + 3];
        double c0, c1, c2, e0, e1, e2, q0, q1, q2, u0, u1, u2;
        {
            const double m0 = B.planes[4 * bf0], m1 = B.planes[4 * bf0 + 1], m2 = B.planes[4 * bf0 + 2];
            c0 = -(C00 * m0 + C01 * m1 + C02 * m2), c1 = -(C10 * m0 + C11 * m1 + C12 * m2), c2 = -(C20 * m0 + C21 * m1 + C22 * m2);
        }
        {
            const double m0 = B.planes[4 * bf1], m1 = B.planes[4 * bf1 + 1], m2 = B.planes[4 * bf1 + 2];
            e0 = -(C00 * m0 + C01 * m1 + C02 * m2), e1 = -(C10 * m0 + C11 * m1 + C12 * m2), e2 = -(C20 * m0 + C21 * m1 + C22 * m2);
        }
        {
            const double x = B.verts[3 * bv0], y = B.verts[3 * bv0 + 1], z = B.verts[3 * bv0 + 2];
            q0 = (C00 * x + C01 * y + C02 * z) + t0, q1 = (C10 * x + C11 * y + C12 * z) + t1, q2 = (C20 * x + C21 * y + C22 * z) + t2;
            const double dx = B.verts[3 * bv1] - x, dy = B.verts[3 * bv1 + 1] - y, dz = B.verts[3 * bv1 + 2] - z;
            u0 = C00 * dx + C01 * dy + C02 * dz, u1 = C10 * dx + C11 * dy + C12 * dz, u2 = C20 * dx + C21 * dy + C22 * dz;
        }
        const double x0 = e1 * c2 - e2 * c1, x1 = e2 * c0 - e0 * c2, x2 = e0 * c1 - e1 * c0;  // d x c
        const double uu = u0 * u0 + u1 * u1 + u2 * u2;
#pragma unroll 1
        for (int ea = 0; ea < A.ne; ea++) {
            const int af0 = A.edges[4 * ea + 2], af1 = A.edges[4 * ea + 3];
            const double a0 = A.planes[4 * af0], a1 = A.planes[4 * af0 + 1], a2 = A.planes[4 * af0 + 2];
            const double b0 = A.planes[4 * af1], b1 = A.planes[4 * af1 + 1], b2 = A.planes[4 * af1 + 2];
            const double y0 = b1 * a2 - b2 * a1, y1 = b2 * a0 - b0 * a2, y2 = b0 * a1 - b1 * a0;  // b x a
            const double cba = c0 * y0 + c1 * y1 + c2 * y2, dba = e0 * y0 + e1 * y1 + e2 * y2;
            const double adc = a0 * x0 + a1 * x1 + a2 * x2, bdc = b0 * x0 + b1 * x1 + b2 * x2;
            if (cba * dba < 0.0 && adc * bdc < 0.0 && cba * bdc > 0.0) {
                const int av0 = A.edges[4 * ea], av1 = A.edges[4 * ea + 1];
                const double p0 = A.verts[3 * av0], p1 = A.verts[3 * av0 + 1], p2 = A.verts[3 * av0 + 2];
                const double w0 = A.verts[3 * av1] - p0, w1 = A.verts[3 * av1 + 1] - p1, w2 = A.verts[3 * av1 + 2] - p2;
                double n0 = w1 * u2 - w2 * u1, n1 = w2 * u0 - w0 * u2, n2 = w0 * u1 - w1 * u0;
                const double len2 = n0 * n0 + n1 * n1 + n2 * n2;
                if (len2 >= FBR_BOX_PARALLEL * ((w0 * w0 + w1 * w1 + w2 * w2) * uu)) {
                    const double s = (n0 * (a0 + b0) + n1 * (a1 + b1) + n2 * (a2 + b2) < 0.0 ? -1.0 : 1.0) / sqrt(len2);
                    const double g = s * (n0 * (q0 - p0) + n1 * (q1 - p1) + n2 * (q2 - p2));
                    gap = g > gap ? g : gap;
                }
            }
        }
    }
    return gap;
}

// Signed distance of the hulls A at (RA, cA) and B at (RB, cB): R [9] row-major (orthonormal), c [3] the origin of the hull's axes in the
// world.  A NaN or an infinity among the poses gives a NaN.  iters (may be null): the GJK iterations taken, + 1000 when the facet pass ran.
template <class DP, class IP>
FBR_HD double fbr_hull_distance(const double *RA, const double *cA, const FbrHullT<DP, IP> &A, const double *RB, const double *cB,
                                const FbrHullT<DP, IP> &B, int *iters)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    FbrHullRel q;
    fbr_hull_relative(RA, cA, RB, cB, &q);
    bool touching;
    int it;
    double res = fbr_hull_gjk(q, A, B, false, &touching, &it);
    if (iters) *iters = it + (touching ? 1000 : 0);
    // ---- touching or overlapping: the largest signed gap over the facets of the Minkowski difference
    if (FBR_HULL_ANY(touching)) {
        if (touching) res = fbr_hull_facets(q, A, B, 0, 1);
    }
    return res;
}

// ---- the set as fbr_model_set_hulls takes it, checked on the host (HIP-free: tests/emul/hull_emul.cpp runs the same text) ---------------------
// Returns "" when the set is acceptable, else what is wrong.  L: the number of links; diam [nhulls] (may be null): the hulls' diameters.
inline std::string fbr_hull_validate(int L, int max_hulls, int max_pairs, int max_vertices, int nhulls, const int32_t *link, const double *offset,
                                     const double *rot, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes,
                                     const int32_t *ebeg, const int32_t *edges, int npairs, const int32_t *pairs, double *diam)
{
    const auto S = [](long v) { return std::to_string(v); };
    if (nhulls < 0 || npairs < 0 || nhulls > max_hulls || npairs > max_pairs)
        return "hull set: at most " + S(max_hulls) + " hulls and " + S(max_pairs) + " pairs";
    if ((nhulls > 0 && (!link || !offset || !vbeg || !verts || !fbeg || !planes || !ebeg || !edges)) || (npairs > 0 && !pairs)) return "hull set: null array";
    if (nhulls > 0 && (vbeg[0] != 0 || fbeg[0] != 0 || ebeg[0] != 0)) return "hull set: vbeg, fbeg and ebeg start at 0";
    for (int h = 0; h < nhulls; h++) {
        const std::string who = "hull " + S(h) + ": ";
        if (link[h] < -1 || link[h] >= L) return who + "link index out of range (-1: a world hull)";
        const long nv = (long)vbeg[h + 1] - vbeg[h], nf = (long)fbeg[h + 1] - fbeg[h], ne = (long)ebeg[h + 1] - ebeg[h];
        if (nv < 4 || nv > max_vertices) return who + S(nv) + " vertices (4 to " + S(max_vertices) + ")";
        if (nf < 4 || nf > 2 * nv - 4 || ne < 6 || ne > 3 * nv - 6) return who + "between 4 and 2 V - 4 faces, 6 and 3 V - 6 edges";
        for (int i = 0; i < 3; i++)
            if (!std::isfinite(offset[3 * h + i])) return who + "non-finite offset";
        if (link[h] < 0) {
            if (!rot) return who + "a world hull needs rot";
            for (int i = 0; i < 9; i++)
                if (!std::isfinite(rot[9 * h + i])) return who + "non-finite rotation";
        }
        const double *V = verts + 3 * (size_t)vbeg[h], *Pl = planes + 4 * (size_t)fbeg[h];
        const int32_t *E = edges + 4 * (size_t)ebeg[h];
        for (long i = 0; i < 3 * nv; i++)
            if (!std::isfinite(V[i])) return who + "non-finite vertex";
        double dm = 0.0;
        for (long i = 0; i < nv; i++)
            for (long j = i + 1; j < nv; j++) {
                const double a = V[3 * i] - V[3 * j], b = V[3 * i + 1] - V[3 * j + 1], c = V[3 * i + 2] - V[3 * j + 2];
                dm = std::max(dm, std::sqrt(a * a + b * b + c * c));
            }
        if (!(dm > 0.0)) return who + "all vertices coincide";
        if (diam) diam[h] = dm;
        for (long f = 0; f < nf; f++) {
            const double *p = Pl + 4 * f;
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3])) return who + "non-finite plane";
            if (std::fabs(std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) - 1.0) > 1e-9) return who + "the normal of face " + S(f) + " is not unit to 1e-9";
            for (long i = 0; i < nv; i++)
                if (p[0] * V[3 * i] + p[1] * V[3 * i + 1] + p[2] * V[3 * i + 2] - p[3] > 1e-9 * dm)
                    return who + "vertex " + S(i) + " lies outside face " + S(f) + " by more than 1e-9 x the diameter";
        }
        for (long e = 0; e < ne; e++) {
            const int32_t *q = E + 4 * e;
            if (q[0] < 0 || q[0] >= nv || q[1] < 0 || q[1] >= nv || q[0] == q[1] || q[2] < 0 || q[2] >= nf || q[3] < 0 || q[3] >= nf)
                return who + "edge " + S(e) + ": vertex or face index out of range";
            if (q[2] == q[3]) return who + "edge " + S(e) + ": its two faces are the same";
        }
    }
    for (int k = 0; k < npairs; k++) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || a >= nhulls || b < 0 || b >= nhulls || a == b) return "hull pair " + S(k) + ": hull index out of range, or a hull paired with itself";
        if (link[a] < 0 && link[b] < 0) return "hull pair " + S(k) + ": two world hulls";
    }
    return "";
}

#if defined(__HIPCC__)
#define FBR_HULL_BATCH 16  // pairs whose 64 distances a wave stages in the LDS (8.3 KB a wave), as for the boxes

struct DevHulls {
    DevBoxes fr;          // the view fbr_box_frames_kernel takes: steps, slots, cen = the offsets; half is not read; npairs = 0
    int nhulls, npairs;
    const int *tab;       // [nhulls][8]: robot-hull number or -1 - (world-hull number) | vbeg | nv | fbeg | nf | ebeg | ne | 0, by the caller's number
    const double *diam;   // [nhulls]
    const double *world;  // [nworld][12] R | centre of the world hulls
    const double *verts;  // [][3]
    const double *planes; // [][4]
    const int *edges;     // [][4] end vertices and faces, relative to the hull's own tables
    const int2 *pairs;    // [npairs] the caller's hull numbers
    const int *col;       // [npairs] the column of pval / pidx a pair writes, or null: its own number (a set split by fbr_model_set_hull_meshes)
    int ldp;              // the columns of pval / pidx: npairs, or all pairs of a split set
};

#if defined(FBR_KERNELS_COLLISION)
typedef FbrHullT<fbr_cdouble_ptr, fbr_cint_ptr> FbrDevHull;

// the frame and the tables of hull h (wave-uniform) for this lane's sample
__device__ __forceinline__ void fbr_hull_fetch(const DevHulls &hs, int h, const double *f, double *R, double *c, FbrDevHull *H)
{
    const fbr_cint_ptr tb = (fbr_cint_ptr)(unsigned long)(hs.tab + 8 * (long)h);
    const int code = FBR_UNI(tb[0]);
    H->nv = FBR_UNI(tb[2]);
    H->nf = FBR_UNI(tb[4]);
    H->ne = FBR_UNI(tb[6]);
    H->verts = (fbr_cdouble_ptr)(unsigned long)(hs.verts + 3 * (long)FBR_UNI(tb[1]));
    H->planes = (fbr_cdouble_ptr)(unsigned long)(hs.planes + 4 * (long)FBR_UNI(tb[3]));
    H->edges = (fbr_cint_ptr)(unsigned long)(hs.edges + 4 * (long)FBR_UNI(tb[5]));
    H->diam = ((fbr_cdouble_ptr)(unsigned long)hs.diam)[h];
    if (code >= 0) {
        for (int i = 0; i < 9; i++) R[i] = f[((long)code * 12 + i) * 64];
        for (int i = 0; i < 3; i++) c[i] = f[((long)code * 12 + 9 + i) * 64];
    } else {
        const fbr_cdouble_ptr w = (fbr_cdouble_ptr)(unsigned long)(hs.world + 12 * (long)(-1 - code));
        for (int i = 0; i < 9; i++) R[i] = w[i];
        for (int i = 0; i < 3; i++) c[i] = w[9 + i];
    }
}

// work items (block, batch of FBR_HULL_BATCH pairs), one wave each; pval / pidx [nb][npairs] as for fbr_box_pairs_kernel
// (The decode and the scan tail are fbr_pair_item and fbr_pair_scan_store of fbr_capsule.h written out: on the helpers this kernel
// measured 1 to 2 % slower on an MI355X -- DESIGN.md, "collision layout".)
__global__ __launch_bounds__(64) void fbr_hull_pairs_kernel(DevHulls hs, DevCapTiles tl, long blk0, long nb, const double *__restrict__ fr,
                                                            double *__restrict__ pval, long *__restrict__ pidx)
{
    __shared__ double sd[FBR_HULL_BATCH * 65];
    const int lane = threadIdx.x;
    const long nbatch = (hs.npairs + FBR_HULL_BATCH - 1) / FBR_HULL_BATCH, items = nb * nbatch;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long b = it / nbatch;
        const int k0 = (int)(it - b * nbatch) * FBR_HULL_BATCH, cnt = min(FBR_HULL_BATCH, hs.npairs - k0);
        const long blk = blk0 + b, c = blk / tl.tiles, i0 = (blk - c * tl.tiles) << 6;
        const int valid = (int)min(64L, tl.Tc - i0);
        // lanes behind the last checked sample repeat it: they take its path through the loops below and are never scanned
        const double *f = fr + b * (long)hs.fr.nrob * 12 * 64 + min(lane, valid - 1);
        int cura = 0;
        bool have = false;
        double RA[9], cA[3];
        FbrDevHull HA = {0, 0, 0, nullptr, nullptr, nullptr, 0.0};
        for (int i = 0; i < 9; i++) RA[i] = 0.0;
        for (int i = 0; i < 3; i++) cA[i] = 0.0;
        __syncthreads();  // (the item before has been scanned)
#pragma unroll 1
        for (int j = 0; j < cnt; j++) {
            const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(hs.pairs + k0 + j);
            const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
            if (!have || ia != cura) {  // (pair lists come sorted by their first hull: its frame stays in registers)
                fbr_hull_fetch(hs, ia, f, RA, cA, &HA);
                cura = ia;
                have = true;
            }
            double RB[9], cB[3];
            FbrDevHull HB;
            fbr_hull_fetch(hs, ib, f, RB, cB, &HB);
            sd[j * 65 + lane] = fbr_hull_distance(RA, cA, HA, RB, cB, HB, (int *)nullptr);
        }
        __syncthreads();
        if (lane < cnt) {
            double best = FBR_CAPSULE_NONE;
            int ibest = -1;
            for (int r = 0; r < valid; r++) {
                const double a = sd[lane * 65 + r];
                if (fbr_capsule_take(a, best)) best = a, ibest = r;
            }
            const int col = hs.col ? hs.col[k0 + lane] : k0 + lane;
            pval[b * hs.ldp + col] = best;
            pidx[b * hs.ldp + col] = ibest < 0 ? -1 : (i0 + ibest) * tl.step;
        }
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
