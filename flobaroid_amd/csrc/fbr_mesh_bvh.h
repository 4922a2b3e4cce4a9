// fbr_mesh_bvh.h -- triangle meshes of up to FBR_MAX_LARGE_MESH_TRIANGLES triangles on hulls of the set (fbr_model_set_large_hull_meshes):
// the brute-force double loop of fbr_mesh.h behind a bounding-volume hierarchy.  KUKA LWR4 has visual meshes only, of 1098 to 4434
// triangles: a pair is 1e7 triangle pairs a sample, and collisionMode "full" runs on it only through a tree.
//
// The tree (host, at set time, HIP-free: tests/emul/mesh_bvh_emul.cpp runs the same text).  Per mesh a binary tree by median splits: the
// triangles of a node are sorted by their centroid along the longest axis of the centroids' bounding box (stable, ties by the caller's
// number: the builder is deterministic) and cut in two halves; a node of at most FBR_MESH_BVH_LEAF triangles is a leaf.  The triangles are
// reordered so that every node owns a contiguous range [first, first + count); the per-triangle aux records of fbr_mesh.h are kept, so a
// leaf pair is evaluated with the triangle-level culling of fbr_mesh_range_oriented.  Halving bounds the depth by
// ceil(log2(8192 / FBR_MESH_BVH_LEAF)) = 10; a tree deeper than FBR_MESH_BVH_MAX_DEPTH is refused, which bounds the stack below by
// construction.
//
// The volume: a sphere per node, on both sides -- the middle of the bounding box of the node's triangle vertices, the largest distance of
// one of them from it, inflated by 4 eps as the spheres of fbr_mesh.h are.  A sphere needs no rotation: its centre goes through the lane's
// relative pose (nine multiplications), and everything is measured in the axes of hull A.  A hull without a mesh is one node, its sphere
// of the table sph.
//
// The traversal (fbr_mesh_bvh_distance) is the wave's, not the lane's: a stack of node pairs (a, b) in the LDS, popped by all 64 lanes
// together.  Every lane forms its own bound |c_a - (C c_b + t)| - r_a - r_b from its own pose; a lane is live when its pose is finite and
// its best is not 0.0 yet, and wants the pair when bound - slack < best.  A pair no lane wants is dropped for the wave (one ballot).  Two
// leaves: fbr_mesh_range_oriented on the two ranges, lanes that do not want the pair switched off.  Otherwise the node with the larger
// radius (a leaf never) is split, and of its two children the one that is nearer for most live lanes is visited first (a vote: ballot and
// popcount, no data crosses lanes); a child no lane wants is not pushed.  Consecutive lanes are consecutive samples of one candidate, so
// the lanes' wishes nearly coincide.  The stack holds FBR_MESH_BVH_STACK pairs: a pop takes one and pushes at most two that lie one level
// deeper in one of the trees, so it never holds more than depth A + depth B + 2 <= 2 FBR_MESH_BVH_MAX_DEPTH + 2; should a push ever not
// fit, the pair's two whole ranges are evaluated in place (every node carries its range), which is the same minimum.
//
// Why the bits are those of the brute force (fbr_mesh_distance_oriented<false> on the same pose).  The result is a minimum over triangle
// pairs of what fbr_hull_gjk returns for (q, T_A, X) in the same orientation, and a strict minimum of the same values does not depend on
// the order they are visited in.  A pair of nodes is skipped only when, for the lane, (bound - slack) >= best.  A node's sphere holds the
// vertices of its triangles, hence the triangles, so the true sphere bound is at most the true distance of every triangle pair below the
// two nodes.  The computed bound: the centre of b through the pose carries 3 roundings of products and sums of magnitude <= scale each way,
// the difference, the norm and the two subtractions a few more -- at most 8 eps scale above the true bound, the budget the header of
// fbr_mesh.h gives the triangle spheres (node centres lie in the same bounding boxes, radii are no larger than the hull's diameter).  A
// computed distance is at least the true one - 16 eps scale.  With slack = FBR_MESH_CULL_K eps scale = 64 eps scale a skipped evaluation
// would have returned more than best + 40 eps scale: it could not have won.  The 4 eps inflation covers the rounding of the radius itself.
// A lane switched off in a leaf pair skipped it under the same inequality.  So no skip changes a bit, for any order and any leaf size.
#pragma once
#include "fbr_mesh.h"

#define FBR_MESH_BVH_LEAF 8        // triangles of a leaf at most
#define FBR_MESH_BVH_MAX_DEPTH 30  // of one tree (the root has depth 0)
#define FBR_MESH_BVH_STACK 64      // node pairs: >= 2 FBR_MESH_BVH_MAX_DEPTH + 2

struct FbrMeshBvh {              // the tree of one mesh
    std::vector<int32_t> node;   // [N][4] left child | right child (-1 | -1: a leaf) | first triangle | count, the root first
    std::vector<double> vol;     // [N][4] sphere centre | radius
    std::vector<int32_t> depth;  // [N]
    std::vector<int32_t> order;  // [nt] the caller's number of the triangle at a place
    int max_depth = 0;
};

// the sphere of the triangles [first, first + count) of tris [][9]
inline void fbr_mesh_bvh_sphere(const double *tris, long first, long count, double *vol)
{
    const double *v = tris + 9 * first;
    fbr_mesh_point_sphere(3 * count, v, 0, v, vol);
}

// Builds the tree of the nt >= 1 triangles tris [nt][9].  Returns "" or what is wrong.
inline std::string fbr_mesh_bvh_build(long nt, const double *tris, FbrMeshBvh &out)
{
    out = FbrMeshBvh();
    if (nt < 1) return "mesh tree: no triangle";
    std::vector<double> cen((size_t)nt * 3);
    for (long t = 0; t < nt; t++)
        for (int k = 0; k < 3; k++) cen[3 * t + k] = (tris[9 * t + k] + tris[9 * t + 3 + k] + tris[9 * t + 6 + k]) / 3.0;
    out.order.resize((size_t)nt);
    for (long t = 0; t < nt; t++) out.order[t] = (int32_t)t;
    struct Todo {
        int node;
        long first, count;
    };
    std::vector<Todo> todo;
    out.node.assign(4, -1);
    out.depth.assign(1, 0);
    todo.push_back({0, 0, nt});
    while (!todo.empty()) {
        const Todo w = todo.back();
        todo.pop_back();
        out.node[4 * (size_t)w.node + 2] = (int32_t)w.first, out.node[4 * (size_t)w.node + 3] = (int32_t)w.count;
        if (w.count <= FBR_MESH_BVH_LEAF) continue;
        int32_t *o = out.order.data() + w.first;
        double lo[3], hi[3];
        for (int k = 0; k < 3; k++) lo[k] = hi[k] = cen[3 * (size_t)o[0] + k];
        for (long i = 1; i < w.count; i++)
            for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], cen[3 * (size_t)o[i] + k]), hi[k] = std::max(hi[k], cen[3 * (size_t)o[i] + k]);
        int ax = 0;
        for (int k = 1; k < 3; k++)
            if (hi[k] - lo[k] > hi[ax] - lo[ax]) ax = k;
        std::stable_sort(o, o + w.count, [&](int32_t a, int32_t b) {
            const double x = cen[3 * (size_t)a + ax], y = cen[3 * (size_t)b + ax];
            return x < y || (x == y && a < b);
        });
        const long half = w.count / 2;
        const int d = out.depth[w.node] + 1;
        if (d > FBR_MESH_BVH_MAX_DEPTH) return "mesh tree: deeper than " + std::to_string(FBR_MESH_BVH_MAX_DEPTH) + " levels, more than the traversal's stack holds";
        const int l = (int)out.depth.size(), r = l + 1;
        out.node[4 * (size_t)w.node] = l, out.node[4 * (size_t)w.node + 1] = r;
        out.node.insert(out.node.end(), 8, -1);
        out.depth.push_back(d), out.depth.push_back(d);
        out.max_depth = std::max(out.max_depth, d);
        todo.push_back({r, w.first + half, w.count - half});
        todo.push_back({l, w.first, half});
    }
    // the spheres, over the reordered triangles
    std::vector<double> sorted((size_t)nt * 9);
    for (long t = 0; t < nt; t++) std::copy(tris + 9 * (size_t)out.order[t], tris + 9 * (size_t)out.order[t] + 9, sorted.data() + 9 * t);
    const size_t N = out.depth.size();
    out.vol.resize(N * 4);
    for (size_t n = 0; n < N; n++) fbr_mesh_bvh_sphere(sorted.data(), out.node[4 * n + 2], out.node[4 * n + 3], out.vol.data() + 4 * n);
    return "";
}

struct FbrMeshBvhStats {  // (host only: tests/emul/mesh_bvh_emul.cpp)
    long node_pairs, leaf_pairs, tri_pairs;  // popped and wanted | of them two leaves | triangle pairs of those
    int max_stack;
    FbrMeshStats tri;  // the evaluations inside the leaf pairs
};

// lanes of c [NL] that are set: on the device the wave's (NL = 1, one lane a thread), on the host the packet's
template <int NL>
FBR_HD int fbr_mesh_bvh_count(const bool *c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_popcountll(__builtin_amdgcn_ballot_w64(c[0]));
#else
    int n = 0;
    for (int l = 0; l < NL; l++) n += c[l] ? 1 : 0;
    return n;
#endif
}

// this lane's sphere bound of (ca | ra) in the axes of A against (cb | rb) in the axes of B; hb [3]: the centre of b in the axes of A
template <class DP>
FBR_HD double fbr_mesh_bvh_bound(const FbrHullRel &q, DP ca, DP cb, double *hb)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    hb[0] = (q.C00 * cb[0] + q.C01 * cb[1] + q.C02 * cb[2]) + q.t0;
    hb[1] = (q.C10 * cb[0] + q.C11 * cb[1] + q.C12 * cb[2]) + q.t1;
    hb[2] = (q.C20 * cb[0] + q.C21 * cb[1] + q.C22 * cb[2]) + q.t2;
    const double x = ca[0] - hb[0], y = ca[1] - hb[1], z = ca[2] - hb[2];
    return sqrt(x * x + y * y + z * z) - ca[3] - cb[3];
}

// Distance of the mesh MA with the tree (nodeA, volA), in the axes of hull A, to B -- the mesh MB with its tree when MB.nt >= 1, else the
// solid hull B, one node with the sphere sphB -- for NL lanes at once: the device calls it with NL = 1 from every lane of a wave (the
// votes are ballots), the host with the poses of a whole packet, nl <= NL of them.  q [NL]: B relative to A; stk [2 FBR_MESH_BVH_STACK]: the
// wave's stack; out [NL]: what fbr_mesh_distance_oriented returns for the pose.
template <int NL, class DP, class IP>
FBR_HD void fbr_mesh_bvh_distance(int nl, const FbrHullRel *q, const FbrHullT<DP, IP> &A, const FbrMeshT<DP> &MA, IP nodeA, DP volA,
                                  const FbrHullT<DP, IP> &B, const FbrMeshT<DP> &MB, IP nodeB, DP volB, DP sphB, int *stk, double *out,
                                  FbrMeshBvhStats *stats)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double best[NL], slack[NL], hb[NL][3], hc[NL][3];
    bool dead[NL], live[NL], want[NL], want1[NL], near0[NL];
    for (int l = 0; l < NL; l++) {
        const FbrHullRel &ql = q[l < nl ? l : 0];
        const double nan0 = ql.chk - ql.chk;
        dead[l] = !(nan0 == 0.0) || l >= nl;
        best[l] = FBR_CAPSULE_NONE;
        slack[l] = fbr_mesh_slack(ql, A, B);
    }
    int sp = 1;
    stk[0] = 0, stk[1] = MB.nt > 0 ? 0 : -1;
#pragma unroll 1
    while (sp > 0) {
        sp--;
        const int a = FBR_UNI(stk[2 * sp]), b = FBR_UNI(stk[2 * sp + 1]);
        const IP na = nodeA + 4 * a;
        const DP ca = volA + 4 * a, cb = b < 0 ? sphB : volB + 4 * b;
        const int al = na[0], ar = na[1], af = na[2], an = na[3];
        int bl = -1, br = -1, bf = 0, bn = 0;
        if (b >= 0) {
            const IP nb = nodeB + 4 * b;
            bl = nb[0], br = nb[1], bf = nb[2], bn = nb[3];
        }
        for (int l = 0; l < NL; l++) {
            live[l] = !dead[l] && best[l] != 0.0;
            want[l] = live[l] && fbr_mesh_bvh_bound(q[l], ca, cb, hb[l]) - slack[l] < best[l];
        }
        if (fbr_mesh_bvh_count<NL>(want) == 0) continue;
        if (stats) stats->node_pairs++;
        const bool leaves = al < 0 && bl < 0;
        if (leaves || sp + 2 > FBR_MESH_BVH_STACK) {  // (the second: never, by the depth check of the builder)
            const FbrMeshT<DP> RA = {an, MA.tris + 9 * af, MA.aux + 5 * af};
            const FbrMeshT<DP> RB = {bn, MB.tris + 9 * bf, MB.aux + 5 * bf};
            if (stats) stats->leaf_pairs++, stats->tri_pairs += (long)an * (bn > 0 ? bn : 1);
            for (int l = 0; l < NL; l++)
                fbr_mesh_range_oriented<true>(q[l], A, RA, B, RB, hb[l][0], hb[l][1], hb[l][2], cb[3], slack[l], !want[l], &best[l],
                                              stats ? &stats->tri : (FbrMeshStats *)nullptr);
            continue;
        }
        // split the node of the larger sphere (a leaf never); its children against the other node
        const bool splitA = al >= 0 && (bl < 0 || ca[3] >= cb[3]);
        const int c0 = splitA ? al : bl, c1 = splitA ? ar : br;
        const DP v0 = (splitA ? volA : volB) + 4 * c0, v1 = (splitA ? volA : volB) + 4 * c1;
        for (int l = 0; l < NL; l++) {
            want[l] = want1[l] = near0[l] = false;
            if (!live[l]) continue;
            const double b0 = splitA ? fbr_mesh_bvh_bound(q[l], v0, cb, hc[l]) : fbr_mesh_bvh_bound(q[l], ca, v0, hc[l]);
            const double b1 = splitA ? fbr_mesh_bvh_bound(q[l], v1, cb, hc[l]) : fbr_mesh_bvh_bound(q[l], ca, v1, hc[l]);
            want[l] = live[l] && b0 - slack[l] < best[l];
            want1[l] = live[l] && b1 - slack[l] < best[l];
            near0[l] = live[l] && b0 <= b1;
        }
        const bool w0 = fbr_mesh_bvh_count<NL>(want) != 0, w1 = fbr_mesh_bvh_count<NL>(want1) != 0;
        const bool first0 = 2 * fbr_mesh_bvh_count<NL>(near0) >= fbr_mesh_bvh_count<NL>(live);
        // the child visited first is pushed last
        for (int k = 0; k < 2; k++) {
            const bool zero = (k == 1) == first0;  // k = 0: the farther child
            if (zero ? w0 : w1) {
                stk[2 * sp] = splitA ? (zero ? c0 : c1) : a;
                stk[2 * sp + 1] = splitA ? b : (zero ? c0 : c1);
                sp++;
            }
        }
        if (stats) stats->max_stack = sp > stats->max_stack ? sp : stats->max_stack;
    }
    for (int l = 0; l < NL; l++)
        if (l < nl) out[l] = dead[l] ? q[l].chk - q[l].chk : best[l];
}

// ---- what fbr_model_set_large_hull_meshes builds of its meshes (HIP-free): the triangles in tree order with their aux records, and the node
// tables of all trees one after the other, nbeg [nmesh + 1] the first node of a mesh's.  Returns "" or what is wrong (with the mesh's number).
struct FbrMeshBvhSet {
    std::vector<double> tris, aux, vol;
    std::vector<int32_t> node, nbeg;
    int max_depth = 0;
};

inline std::string fbr_mesh_bvh_set(int nmesh, const int32_t *tbeg, const double *tris, FbrMeshBvhSet &out)
{
    out = FbrMeshBvhSet();
    const size_t NT = (size_t)tbeg[nmesh];
    out.tris.resize(NT * 9), out.aux.resize(NT * 5);
    out.nbeg.assign(1, 0);
    for (int i = 0; i < nmesh; i++) {
        FbrMeshBvh tree;
        const long n = (long)tbeg[i + 1] - tbeg[i];
        const std::string bad = fbr_mesh_bvh_build(n, tris + 9 * (size_t)tbeg[i], tree);
        if (!bad.empty()) return "mesh " + std::to_string(i) + ": " + bad;
        for (long t = 0; t < n; t++) {
            const double *src = tris + 9 * ((size_t)tbeg[i] + (size_t)tree.order[t]);
            double *dst = out.tris.data() + 9 * ((size_t)tbeg[i] + (size_t)t);
            std::copy(src, src + 9, dst);
            fbr_mesh_triangle_aux(dst, out.aux.data() + 5 * ((size_t)tbeg[i] + (size_t)t));
        }
        out.node.insert(out.node.end(), tree.node.begin(), tree.node.end());
        out.vol.insert(out.vol.end(), tree.vol.begin(), tree.vol.end());
        out.nbeg.push_back((int32_t)(out.node.size() / 4));
        out.max_depth = std::max(out.max_depth, tree.max_depth);
    }
    return "";
}

#if defined(__HIPCC__)
struct DevMeshBvh {
    const int *nbeg;    // [nhulls] the first node of the tree of the hull's mesh (no mesh: 0, never read)
    const int *node;    // [][4]
    const double *vol;  // [][4]
};

#if defined(FBR_KERNELS_COLLISION)
// work items (block, mesh pair), one wave each: the scaffolding of fbr_mesh_pairs_kernel with batches of one pair (a pair is 1e3 to 1e5
// triangle pairs' work after the tree); ms: the tables of fbr_model_set_large_hull_meshes, the triangles in tree order
__global__ __launch_bounds__(64) void fbr_mesh_bvh_pairs_kernel(DevHulls hs, DevMeshes ms, DevMeshBvh bv, DevCapTiles tl, long blk0, long nb,
                                                                const double *__restrict__ fr, double *__restrict__ pval, long *__restrict__ pidx)
{
    __shared__ double sd[65];
    __shared__ int stk[2 * FBR_MESH_BVH_STACK];
    const int lane = threadIdx.x;
    const long nbatch = ms.npairs, items = nb * nbatch;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const FbrPairItem w = fbr_pair_item(it, nbatch, 1, ms.npairs, tl, blk0);
        // lanes behind the last checked sample repeat it, as in fbr_hull_pairs_kernel
        const double *f = fr + w.b * (long)hs.fr.nrob * 12 * 64 + min(lane, w.valid - 1);
        __syncthreads();  // (the item before has been scanned)
        const fbr_cint_ptr pr = (fbr_cint_ptr)(unsigned long)(ms.pairs + w.k0);
        const int ia = FBR_UNI(pr[0]), ib = FBR_UNI(pr[1]);
        double RA[9], cA[3], RB[9], cB[3];
        FbrDevHull HA, HB;
        fbr_hull_fetch(hs, ia, f, RA, cA, &HA);
        fbr_hull_fetch(hs, ib, f, RB, cB, &HB);
        const fbr_cint_ptr ma = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ia), mb = (fbr_cint_ptr)(unsigned long)(ms.mtab + 2 * (long)ib);
        const long ta0 = FBR_UNI(ma[0]), tb0 = FBR_UNI(mb[0]);
        const FbrMeshT<fbr_cdouble_ptr> MA = {FBR_UNI(ma[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * ta0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * ta0)};
        const FbrMeshT<fbr_cdouble_ptr> MB = {FBR_UNI(mb[1]), (fbr_cdouble_ptr)(unsigned long)(ms.tris + 9 * tb0), (fbr_cdouble_ptr)(unsigned long)(ms.aux + 5 * tb0)};
        const fbr_cint_ptr nbeg = (fbr_cint_ptr)(unsigned long)bv.nbeg;
        const long na0 = FBR_UNI(nbeg[ia]), nb0 = FBR_UNI(nbeg[ib]);
        FbrHullRel q;
        fbr_hull_relative(RA, cA, RB, cB, &q);
        double d;
        fbr_mesh_bvh_distance<1>(1, &q, HA, MA, (fbr_cint_ptr)(unsigned long)(bv.node + 4 * na0), (fbr_cdouble_ptr)(unsigned long)(bv.vol + 4 * na0), HB, MB,
                                 (fbr_cint_ptr)(unsigned long)(bv.node + 4 * nb0), (fbr_cdouble_ptr)(unsigned long)(bv.vol + 4 * nb0),
                                 (fbr_cdouble_ptr)(unsigned long)(ms.sph + 4 * (long)ib), stk, &d, (FbrMeshBvhStats *)nullptr);
        sd[lane] = d;
        __syncthreads();
        fbr_pair_scan_store(sd, w, lane, tl, hs.ldp, [&](int k) { return ms.col[k]; }, pval, pidx);
    }
}
#endif  // FBR_KERNELS_COLLISION
#endif  // __HIPCC__
