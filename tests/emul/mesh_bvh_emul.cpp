// mesh_bvh_emul.cpp -- the HIP-free text of csrc/fbr_mesh_bvh.h on the CPU (TEST ONLY, built by tests/test_meshes_large.py with g++
// -ffp-contract=off): the tree builder, the checks of fbr_model_set_large_hull_meshes, and the traversal walked as a wave walks it, over
// packets of up to 64 consecutive poses at once, beside the brute force of csrc/fbr_mesh.h with its culling off on the same poses.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_mesh_bvh.h"

typedef FbrHullT<const double *, const int32_t *> Hull;
typedef FbrMeshT<const double *> Mesh;

static int message(const std::string &e, char *msg, int len)
{
    if (msg && len > 0) {
        strncpy(msg, e.c_str(), len - 1);
        msg[len - 1] = 0;
    }
    return e.empty() ? 0 : -1;
}

extern "C" {

int bvh_leaf(void) { return FBR_MESH_BVH_LEAF; }
int bvh_max_depth(void) { return FBR_MESH_BVH_MAX_DEPTH; }
int bvh_stack(void) { return FBR_MESH_BVH_STACK; }

// the tree of tris [nt][9]: node [cap][4], vol [cap][4], depth [cap], order [nt]; returns the number of nodes (cap >= 2 nt holds any
// tree), or -1 and the message
int bvh_build(long nt, const double *tris, int cap, int32_t *node, double *vol, int32_t *depth, int32_t *order, char *msg, int len)
{
    FbrMeshBvh t;
    const std::string e = fbr_mesh_bvh_build(nt, tris, t);
    if (message(e, msg, len)) return -1;
    const int N = (int)t.depth.size();
    if (N > cap) return message("bvh_build: cap too small", msg, len);
    std::copy(t.node.begin(), t.node.end(), node);
    std::copy(t.vol.begin(), t.vol.end(), vol);
    std::copy(t.depth.begin(), t.depth.end(), depth);
    std::copy(t.order.begin(), t.order.end(), order);
    return N;
}

// 0 when fbr_model_set_large_hull_meshes would accept the meshes on this hull set, else -1 and the message in msg [len]
int bvh_validate(int nhulls, const int32_t *link, const int32_t *fbeg, const double *planes, const double *diam, int npairs, const int32_t *pairs,
                 int nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris, char *msg, int len)
{
    std::string e = fbr_mesh_validate(nhulls, link, fbeg, planes, diam, npairs, pairs, FBR_MAX_LARGE_MESH_TRIANGLES, std::numeric_limits<long>::max(),
                                      nmesh, hull, tbeg, tris);
    if (e.empty() && nmesh > 0) {
        FbrMeshBvhSet set;
        e = fbr_mesh_bvh_set(nmesh, tbeg, tris, set);
        if (!e.empty()) e = "hull meshes: " + e;
    }
    return message(e, msg, len);
}

// dist [S][npairs] from the frames fr [S][nhulls][12] (R | centre), as tests/emul/mesh_emul.cpp's mesh_pairs takes them.  A pair with a mesh
// on either side: the meshed hull first (both meshed: the caller's order); tree == 0: fbr_mesh_distance_oriented<false>, the brute force
// without culling, pose by pose, on the caller's triangle order; tree != 0: fbr_mesh_bvh_distance over packets of `packet` (<= 64)
// consecutive samples on the trees and the triangle order fbr_mesh_bvh_set gives.  The other pairs: fbr_hull_distance.
// stats [8] (may be null), of the mesh pairs: node pairs wanted | leaf pairs | triangle pairs of those | GJK evaluations | the highest
// stack | the most GJK iterations | the deepest tree | all triangle pairs (the brute force's work).
void bvh_pairs(long S, int nhulls, const double *fr, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes,
               const int32_t *ebeg, const int32_t *edges, const double *diam, const int32_t *mtab, const double *tris, long ntris, int npairs,
               const int32_t *pairs, int tree, int packet, double *dist, int64_t *stats)
{
    // the meshes in table order, as the setter takes them
    std::vector<int32_t> mh, tbeg(1, 0);
    std::vector<double> packed;
    for (int h = 0; h < nhulls; h++)
        if (mtab[2 * h + 1] > 0) {
            mh.push_back(h);
            packed.insert(packed.end(), tris + 9 * (size_t)mtab[2 * h], tris + 9 * ((size_t)mtab[2 * h] + (size_t)mtab[2 * h + 1]));
            tbeg.push_back(tbeg.back() + mtab[2 * h + 1]);
        }
    (void)ntris;
    const int nmesh = (int)mh.size();
    FbrMeshBvhSet set;
    std::vector<double> aux0(packed.size() / 9 * 5 + 5);
    if (nmesh > 0) {
        const std::string e = fbr_mesh_bvh_set(nmesh, tbeg.data(), packed.data(), set);
        if (!e.empty()) {
            for (long i = 0; i < S * npairs; i++) dist[i] = std::nan("");
            return;
        }
    }
    for (size_t t = 0; t < packed.size() / 9; t++) fbr_mesh_triangle_aux(packed.data() + 9 * t, aux0.data() + 5 * t);
    std::vector<int> mof((size_t)nhulls, -1);
    for (int i = 0; i < nmesh; i++) mof[mh[i]] = i;
    std::vector<double> sph((size_t)std::max(nhulls, 1) * 4);
    for (int h = 0; h < nhulls; h++)
        fbr_mesh_point_sphere(vbeg[h + 1] - vbeg[h], verts + 3 * (size_t)vbeg[h], 3L * mtab[2 * h + 1], tris + 9 * (size_t)mtab[2 * h], sph.data() + 4 * (size_t)h);
    auto view = [&](int h) {
        return Hull{vbeg[h + 1] - vbeg[h], fbeg[h + 1] - fbeg[h], ebeg[h + 1] - ebeg[h], verts + 3 * (size_t)vbeg[h], planes + 4 * (size_t)fbeg[h],
                    edges + 4 * (size_t)ebeg[h], diam[h]};
    };
    auto mesh = [&](int h, bool sorted) {
        if (mof[h] < 0) return Mesh{0, packed.data(), aux0.data()};
        const size_t t0 = (size_t)tbeg[mof[h]];
        return Mesh{tbeg[mof[h] + 1] - tbeg[mof[h]], (sorted ? set.tris.data() : packed.data()) + 9 * t0, (sorted ? set.aux.data() : aux0.data()) + 5 * t0};
    };
    FbrMeshBvhStats bs = {0, 0, 0, 0, {0, 0, 0}};
    FbrMeshStats ms = {0, 0, 0};
    long all = 0;
    int stk[2 * FBR_MESH_BVH_STACK];
    if (packet < 1 || packet > 64) packet = 64;
    for (int k = 0; k < npairs; k++) {
        int a = pairs[2 * k], b = pairs[2 * k + 1];
        if (mof[a] < 0 && mof[b] < 0) {
            for (long s = 0; s < S; s++) {
                const double *f = fr + (size_t)s * nhulls * 12;
                dist[(size_t)s * npairs + k] = fbr_hull_distance(f + 12 * a, f + 12 * a + 9, view(a), f + 12 * b, f + 12 * b + 9, view(b), (int *)nullptr);
            }
            continue;
        }
        if (mof[a] < 0) std::swap(a, b);
        const Hull A = view(a), B = view(b);
        all += S * (long)mesh(a, false).nt * std::max(mesh(b, false).nt, 1);
        for (long s0 = 0; s0 < S; s0 += packet) {
            const int nl = (int)std::min<long>(packet, S - s0);
            FbrHullRel q[64];
            double out[64];
            for (int l = 0; l < nl; l++) {
                const double *f = fr + (size_t)(s0 + l) * nhulls * 12;
                fbr_hull_relative(f + 12 * a, f + 12 * a + 9, f + 12 * b, f + 12 * b + 9, &q[l]);
            }
            if (tree) {
                const int32_t *na = set.node.data() + 4 * (size_t)set.nbeg[mof[a]], *nb = mof[b] < 0 ? set.node.data() : set.node.data() + 4 * (size_t)set.nbeg[mof[b]];
                const double *va = set.vol.data() + 4 * (size_t)set.nbeg[mof[a]], *vb = mof[b] < 0 ? set.vol.data() : set.vol.data() + 4 * (size_t)set.nbeg[mof[b]];
                fbr_mesh_bvh_distance<64>(nl, q, A, mesh(a, true), na, va, B, mesh(b, true), nb, vb, (const double *)sph.data() + 4 * b, stk, out, &bs);
            } else {
                for (int l = 0; l < nl; l++)
                    out[l] = fbr_mesh_distance_oriented<false>(q[l], A, mesh(a, false), B, mesh(b, false), (const double *)sph.data() + 4 * b, &ms);
            }
            for (int l = 0; l < nl; l++) dist[(size_t)(s0 + l) * npairs + k] = out[l];
        }
    }
    if (stats) {
        stats[0] = bs.node_pairs, stats[1] = bs.leaf_pairs, stats[2] = bs.tri_pairs, stats[3] = tree ? bs.tri.evals : ms.evals, stats[4] = bs.max_stack;
        stats[5] = tree ? bs.tri.max_iter : ms.max_iter, stats[6] = set.max_depth, stats[7] = all;
    }
}
}
