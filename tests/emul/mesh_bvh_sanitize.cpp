// mesh_bvh_sanitize.cpp -- a stand-alone program (TEST ONLY, built by tests/test_meshes_large.py with g++ -fsanitize=address,undefined and
// run on the CPU): the HIP-free text of csrc/fbr_mesh_bvh.h -- the builder, the set builder and the traversal over packets of 64, 3 and 1
// poses -- on seeded soups of 1, 8, 9, 17, 65 and 257 triangles against each other and against a box, checked against the brute force
// of csrc/fbr_mesh.h bit for bit.  Prints "ok" and returns 0; the sanitizers abort on an out-of-bounds access, an overflow or a bad shift.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_mesh_bvh.h"

typedef FbrHullT<const double *, const int32_t *> Hull;
typedef FbrMeshT<const double *> Mesh;

int main()
{
    std::mt19937_64 gen(7);
    std::normal_distribution<double> nd(0.0, 1.0);
    // a box of half extent 0.5 that holds nothing of the soups' culling: the hull tables of both sides (the traversal reads diam and, for a
    // solid B, the vertices)
    const double bv[24] = {-.5, -.5, -.5, -.5, -.5, .5, -.5, .5, -.5, -.5, .5, .5, .5, -.5, -.5, .5, -.5, .5, .5, .5, -.5, .5, .5, .5};
    const Hull box = {8, 0, 0, bv, nullptr, nullptr, std::sqrt(3.0)};
    const double sphB[4] = {0.0, 0.0, 0.0, std::sqrt(0.75) * (1.0 + 4.0 * FBR_MESH_EPS)};
    const int sizes[6] = {1, 8, 9, 17, 65, 257};
    long checked = 0;
    for (int ia = 0; ia < 6; ia++)
        for (int ib = -1; ib < 6; ib += 2) {  // -1: the solid box
            const int na = sizes[ia], nb = ib < 0 ? 0 : sizes[ib];
            std::vector<double> tris((size_t)(na + nb) * 9);
            for (int t = 0; t < na + nb; t++) {
                double c[3] = {0.3 * nd(gen), 0.3 * nd(gen), 0.3 * nd(gen)};
                for (int k = 0; k < 9; k++) tris[9 * (size_t)t + k] = c[k % 3] + 0.05 * nd(gen);
            }
            const int32_t tbeg[3] = {0, na, na + nb};
            FbrMeshBvhSet set;
            const std::string e = fbr_mesh_bvh_set(ib < 0 ? 1 : 2, tbeg, tris.data(), set);
            if (!e.empty()) return printf("set: %s\n", e.c_str()), 1;
            std::vector<double> aux((size_t)(na + nb) * 5);
            for (int t = 0; t < na + nb; t++) fbr_mesh_triangle_aux(tris.data() + 9 * (size_t)t, aux.data() + 5 * (size_t)t);
            const Mesh MA = {na, set.tris.data(), set.aux.data()}, MB = {nb, set.tris.data() + 9 * (size_t)na, set.aux.data() + 5 * (size_t)na};
            const Mesh MA0 = {na, tris.data(), aux.data()}, MB0 = {nb, tris.data() + 9 * (size_t)na, aux.data() + 5 * (size_t)na};
            const int32_t *nA = set.node.data(), *nB = ib < 0 ? set.node.data() : set.node.data() + 4 * (size_t)set.nbeg[1];
            const double *vA = set.vol.data(), *vB = ib < 0 ? set.vol.data() : set.vol.data() + 4 * (size_t)set.nbeg[1];
            for (int nl : {64, 3, 1}) {
                FbrHullRel q[64];
                for (int l = 0; l < nl; l++) {
                    const double a = 0.02 * l + nd(gen), RA[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, cA[3] = {0, 0, 0};
                    const double RB[9] = {std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a), 0, 0, 0, 1}, cB[3] = {1.2 + 0.01 * l, 0.3 * nd(gen), 0.0};
                    fbr_hull_relative(RA, cA, RB, cB, &q[l]);
                }
                if (nl == 64) q[5].t1 = q[5].chk = std::nan("");  // a dead lane
                int stk[2 * FBR_MESH_BVH_STACK];
                double out[64];
                FbrMeshBvhStats st = {0, 0, 0, 0, {0, 0, 0}};
                fbr_mesh_bvh_distance<64>(nl, q, box, MA, nA, vA, box, MB, nB, vB, sphB, stk, out, &st);
                for (int l = 0; l < nl; l++) {
                    const double want = fbr_mesh_distance_oriented<false>(q[l], box, MA0, box, MB0, sphB, (FbrMeshStats *)nullptr);
                    if (std::memcmp(&want, &out[l], sizeof(double)) != 0 && !(std::isnan(want) && std::isnan(out[l])))
                        return printf("mismatch: %d x %d triangles, lane %d of %d: %.17g against %.17g\n", na, nb, l, nl, out[l], want), 1;
                    checked++;
                }
            }
        }
    printf("ok %ld\n", checked);
    return 0;
}
