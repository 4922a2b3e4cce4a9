// mesh_emul.cpp -- the HIP-free text of csrc/fbr_mesh.h on the CPU (TEST ONLY, built by tests/test_meshes.py with g++ -ffp-contract=off): the
// mesh distance the pairs kernel calls, with the culling switched on or off, on frames the caller supplies (tests/emul/hull_emul.cpp
// walks the robot), and the checks of fbr_model_set_hull_meshes.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_mesh.h"

typedef FbrHullT<const double *, const int32_t *> Hull;
typedef FbrMeshT<const double *> Mesh;

extern "C" {

// dist [S][npairs] from the frames fr [S][nhulls][12] (R | centre).  mtab [nhulls][2]: first triangle | count (0: no mesh) in tris [][9].  A
// pair with a mesh on either side goes to fbr_mesh_distance (cull != 0: with the sphere culling), the others to fbr_hull_distance.
// stats [3] (may be null): GJK evaluations, evaluations skipped (by the culling, or because the best was 0.0 already), the most GJK iterations -- of the mesh pairs.
void mesh_pairs(long S, int nhulls, const double *fr, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes,
                const int32_t *ebeg, const int32_t *edges, const double *diam, const int32_t *mtab, const double *tris, long ntris, int npairs,
                const int32_t *pairs, int cull, double *dist, int64_t *stats)
{
    std::vector<double> aux((size_t)std::max(ntris, 1L) * 5), sph((size_t)std::max(nhulls, 1) * 4);
    for (long t = 0; t < ntris; t++) fbr_mesh_triangle_aux(tris + 9 * t, aux.data() + 5 * t);
    for (int h = 0; h < nhulls; h++) fbr_mesh_point_sphere(vbeg[h + 1] - vbeg[h], verts + 3 * (size_t)vbeg[h], 3L * mtab[2 * h + 1], tris + 9 * (size_t)mtab[2 * h], sph.data() + 4 * (size_t)h);
    auto view = [&](int h) {
        return Hull{vbeg[h + 1] - vbeg[h], fbeg[h + 1] - fbeg[h], ebeg[h + 1] - ebeg[h], verts + 3 * (size_t)vbeg[h], planes + 4 * (size_t)fbeg[h],
                    edges + 4 * (size_t)ebeg[h], diam[h]};
    };
    auto mesh = [&](int h) { return Mesh{mtab[2 * h + 1], tris + 9 * (size_t)mtab[2 * h], aux.data() + 5 * (size_t)mtab[2 * h]}; };
    FbrMeshStats st = {0, 0, 0};
    for (long s = 0; s < S; s++) {
        const double *f = fr + (size_t)s * nhulls * 12;
        for (int k = 0; k < npairs; k++) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            double d;
            if (mtab[2 * a + 1] == 0 && mtab[2 * b + 1] == 0)
                d = fbr_hull_distance(f + 12 * a, f + 12 * a + 9, view(a), f + 12 * b, f + 12 * b + 9, view(b), (int *)nullptr);
            else if (cull)
                d = fbr_mesh_distance<true>(f + 12 * a, f + 12 * a + 9, view(a), mesh(a), (const double *)sph.data() + 4 * a, f + 12 * b, f + 12 * b + 9,
                                            view(b), mesh(b), (const double *)sph.data() + 4 * b, &st);
            else
                d = fbr_mesh_distance<false>(f + 12 * a, f + 12 * a + 9, view(a), mesh(a), (const double *)sph.data() + 4 * a, f + 12 * b, f + 12 * b + 9,
                                             view(b), mesh(b), (const double *)sph.data() + 4 * b, &st);
            dist[(size_t)s * npairs + k] = d;
        }
    }
    if (stats) stats[0] = st.evals, stats[1] = st.culled, stats[2] = st.max_iter;
}

// 0 when fbr_model_set_hull_meshes would accept the meshes on this hull set, else -1 and the message in msg [len]
int mesh_validate(int nhulls, const int32_t *link, const int32_t *fbeg, const double *planes, const double *diam, int npairs, const int32_t *pairs,
                  int nmesh, const int32_t *hull, const int32_t *tbeg, const double *tris, char *msg, int len)
{
    const std::string e = fbr_mesh_validate(nhulls, link, fbeg, planes, diam, npairs, pairs, FBR_MAX_MESH_TRIANGLES, FBR_MAX_MESH_PAIR_WORK, nmesh, hull,
                                            tbeg, tris);
    if (msg && len > 0) {
        strncpy(msg, e.c_str(), len - 1);
        msg[len - 1] = 0;
    }
    return e.empty() ? 0 : -1;
}
}
