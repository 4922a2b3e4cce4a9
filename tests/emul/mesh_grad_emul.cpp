// mesh_grad_emul.cpp -- the HIP-free text of csrc/fbr_mesh_grad.h on the CPU (TEST ONLY, built by tests/test_mesh_gradient.py with
// g++ -ffp-contract=off).  Two routes over the library's own step program and ancestor masks:
//   0  the single pass, the emulation of record: fbr_rigidgrad_item with fbr_mesh_distance as its functor;
//   1  the device's stages: fbr_meshgrad_frames_item records the relative poses, fbr_mesh_distance_oriented measures each, the slot table
//      of fbr_meshgrad_slots and fbr_meshgrad_quotients make the row.
// A pair without a mesh goes through fbr_hullgrad_item on either route, as on the device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_mesh_grad.h"

typedef FbrHullT<const double *, const int32_t *> Hull;
typedef FbrMeshT<const double *> Mesh;

extern "C" {

// One hull pair per configuration, as hullgrad_eval of hull_grad_emul.cpp; mtab [nhulls][2]: first triangle | count (0: no mesh) in
// tris [ntris][9].  route: see above; cull != 0: with the sphere culling.  nslots [M] (may be null): the stencil points of the item (0: a
// pair without a mesh).  Returns -4 when the recorded poses do not number what fbr_meshgrad_slots says.
int meshgrad_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
                  const int32_t *jtype, int floating, int nhulls, const int32_t *link, const double *offset, const double *rot, int cmode,
                  const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges,
                  const int32_t *mtab, const double *tris, long ntris, double eps, long M, const int32_t *pairs, const double *q, const double *rpy,
                  const double *bpos, int route, int cull, double *dist, double *grad, int32_t *nslots)
{
    std::vector<double> diam(std::max(nhulls, 1));
    if (!fbr_hull_validate(L, FBR_MAX_HULLS, FBR_MAX_HULL_PAIRS, FBR_MAX_HULL_VERTICES, nhulls, link, offset, rot, vbeg, verts, fbeg, planes, ebeg, edges, 0,
                           nullptr, diam.data())
             .empty())
        return -3;
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    try {
        hm.build(L, n, parent, dof, restR, restp, axis, floating, g, 0, 1, 0, 0.0, nullptr, jtype);
    } catch (...) {
        return -1;
    }
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    std::vector<int> stepof, anc;
    fbr_capgrad_ancestors(hm, prog, stepof, anc);
    const int W = fbr_capgrad_words(prog.nsteps);
    std::vector<double> slots((size_t)std::max(prog.nslots, 1) * 12);
    std::vector<double> aux((size_t)std::max(ntris, 1L) * 5), sph((size_t)std::max(nhulls, 1) * 4);
    for (long t = 0; t < ntris; t++) fbr_mesh_triangle_aux(tris + 9 * t, aux.data() + 5 * t);
    for (int h = 0; h < nhulls; h++)
        fbr_mesh_point_sphere(vbeg[h + 1] - vbeg[h], verts + 3 * (size_t)vbeg[h], 3L * mtab[2 * h + 1], tris + 9 * (size_t)mtab[2 * h], sph.data() + 4 * (size_t)h);
    auto view = [&](int h) {
        return Hull{vbeg[h + 1] - vbeg[h], fbeg[h + 1] - fbeg[h], ebeg[h + 1] - ebeg[h], verts + 3 * (size_t)vbeg[h], planes + 4 * (size_t)fbeg[h],
                    edges + 4 * (size_t)ebeg[h], diam[h]};
    };
    auto mesh = [&](int h) { return Mesh{mtab[2 * h + 1], tris + 9 * (size_t)mtab[2 * h], aux.data() + 5 * (size_t)mtab[2 * h]}; };
    std::fill(grad, grad + (size_t)M * n, 0.0);
    double se, omc;
    fbr_boxgrad_trig(eps, &se, &omc);
    for (long i = 0; i < M; i++) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= nhulls || b < 0 || b >= nhulls || (link[a] < 0 && link[b] < 0)) return -2;
        const int ka = link[a] < 0 ? -1 : stepof[link[a]], kb = link[b] < 0 ? -1 : stepof[link[b]];
        double x[2][12];
        for (int j = 0; j < 2; j++) {
            const int c = j ? b : a;
            for (int t = 0; t < 12; t++) x[j][t] = 0.0;
            if (link[c] < 0) {
                for (int t = 0; t < 9; t++) x[j][t] = rot[9 * c + t];
                for (int t = 0; t < 3; t++) x[j][9 + t] = offset[3 * c + t];
            } else {
                for (int t = 0; t < 3; t++) x[j][t] = offset[3 * c + t];
            }
        }
        const Hull HA = view(a), HB = view(b);
        const Mesh MA = mesh(a), MB = mesh(b);
        const double *sA = sph.data() + 4 * (size_t)a, *sB = sph.data() + 4 * (size_t)b;
        const int kam = std::max(ka, 0), kbm = std::max(kb, 0), keep = (ka < 0 ? 0 : 1) | (kb < 0 ? 0 : 2);
        auto mask = [&](int k) { return fbr_capgrad_mask(anc.data(), W, kam, kbm, k) & keep; };
        auto qf = [&](int d) { return q[i * n + d]; };
        auto basef = [&](double *e3, double *b3) {
            for (int j = 0; j < 3; j++) {
                e3[j] = rpy ? rpy[i * 3 + j] : 0.0;
                b3[j] = bpos ? bpos[i * 3 + j] : 0.0;
            }
        };
        auto save = [&](int s, int j, double v) { slots[(size_t)s * 12 + j] = v; };
        auto load = [&](int s, int j) { return slots[(size_t)s * 12 + j]; };
        auto consts = [&](int l, double *rR, double *rp, double *ax) {
            for (int j = 0; j < 9; j++) rR[j] = hm.restR[9 * l + j];
            for (int j = 0; j < 3; j++) {
                rp[j] = hm.restp[3 * l + j];
                ax[j] = hm.axis[3 * l + j];
            }
        };
        auto gst = [&](int d, double v) { grad[i * n + d] = v; };
        const bool fl = floating && rpy != nullptr;
        if (nslots) nslots[i] = 0;
        if (MA.nt == 0 && MB.nt == 0) {
            dist[i] = fbr_hullgrad_item(ka, kb, cmode, x[0], HA, x[1], HB, eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load, consts, gst);
            continue;
        }
        auto oriented = [&](const FbrHullRel &r) {  // (the meshed hull first, as DevMeshes.pairs has it)
            if (MA.nt > 0)
                return cull ? fbr_mesh_distance_oriented<true>(r, HA, MA, HB, MB, sB, (FbrMeshStats *)nullptr)
                            : fbr_mesh_distance_oriented<false>(r, HA, MA, HB, MB, sB, (FbrMeshStats *)nullptr);
            return cull ? fbr_mesh_distance_oriented<true>(r, HB, MB, HA, MA, sA, (FbrMeshStats *)nullptr)
                        : fbr_mesh_distance_oriented<false>(r, HB, MB, HA, MA, sA, (FbrMeshStats *)nullptr);
        };
        if (route == 0) {
            dist[i] = fbr_rigidgrad_item(ka, kb, cmode, x[0], x[1], eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load, consts, gst,
                                         [&](const double *X, const double *Y) {
                                             return cull ? fbr_mesh_distance<true>(X, X + 9, HA, MA, sA, Y, Y + 9, HB, MB, sB, (FbrMeshStats *)nullptr)
                                                         : fbr_mesh_distance<false>(X, X + 9, HA, MA, sA, Y, Y + 9, HB, MB, sB, (FbrMeshStats *)nullptr);
                                         });
            continue;
        }
        std::vector<FbrHullRel> rel;
        std::vector<int> joint;
        fbr_meshgrad_slots(ka, kb, cmode, prog.steps.data(), anc.data(), W, joint);
        const int S = fbr_meshgrad_frames_item(ka, kb, cmode, x[0], x[1], MA.nt == 0, eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load,
                                               consts, [&](int s, const FbrHullRel &r) {
                                                   if ((int)rel.size() == s) rel.push_back(r);
                                               });
        if (S != (int)joint.size() || S != (int)rel.size()) return -4;
        if (nslots) nslots[i] = S;
        std::vector<double> dv((size_t)S);
        for (int s = 0; s < S; s++) dv[s] = oriented(rel[s]);
        dist[i] = fbr_meshgrad_quotients(
            S, [&](int s) { return joint[s]; }, [&](int s) { return dv[s]; }, eps, gst);
    }
    return 0;
}
}
