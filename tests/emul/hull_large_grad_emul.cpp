// hull_large_grad_emul.cpp -- the HIP-free text of csrc/fbr_hull_large_grad.h on the CPU (TEST ONLY, built by
// tests/test_hull_large_gradient.py with g++ -ffp-contract=off).  Two routes over the library's own step program and ancestor masks:
//   0  the single pass, the emulation of record: fbr_rigidgrad_item with fbr_hull_large_distance as its functor;
//   1  the device's stages (fbr_hull_large_grad_item): fbr_meshgrad_frames_item records the relative poses, fbr_hull_large_entry measures
//      each (GJK, then the wave's facet pass), the slot table of fbr_meshgrad_slots and fbr_meshgrad_quotients make the row.
// A pair of two hulls of at most FBR_MAX_HULL_VERTICES vertices goes through fbr_hullgrad_item on either route, as on the device, unless
// `all` is set (option hull_large_all).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_hull_large_grad.h"

typedef FbrHullT<const double *, const int32_t *> Hull;

extern "C" {

// One hull pair per configuration, as hullgrad_eval of hull_grad_emul.cpp.  nslots [M] (may be null): the stencil points of the item (0: a
// pair that went through fbr_hullgrad_item); facet (may be null): the stencil entries of route 1 that entered the facet pass.  Returns -4
// when the recorded poses do not number what fbr_meshgrad_slots says.
int hulllgrad_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
                   const int32_t *jtype, int floating, int nhulls, const int32_t *link, const double *offset, const double *rot, int cmode,
                   const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges,
                   double eps, long M, const int32_t *pairs, const double *q, const double *rpy, const double *bpos, int route, int all, double *dist,
                   double *grad, int32_t *nslots, long *facet)
{
    std::vector<double> diam(std::max(nhulls, 1));
    if (!fbr_hull_validate(L, FBR_MAX_HULLS, FBR_MAX_HULL_PAIRS, FBR_MAX_LARGE_HULL_VERTICES, nhulls, link, offset, rot, vbeg, verts, fbeg, planes, ebeg,
                           edges, 0, nullptr, diam.data())
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
    auto view = [&](int h) {
        return Hull{vbeg[h + 1] - vbeg[h], fbeg[h + 1] - fbeg[h], ebeg[h + 1] - ebeg[h], verts + 3 * (size_t)vbeg[h], planes + 4 * (size_t)fbeg[h],
                    edges + 4 * (size_t)ebeg[h], diam[h]};
    };
    std::fill(grad, grad + (size_t)M * n, 0.0);
    if (facet) *facet = 0;
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
        if (!all && HA.nv <= FBR_MAX_HULL_VERTICES && HB.nv <= FBR_MAX_HULL_VERTICES) {
            dist[i] = fbr_hullgrad_item(ka, kb, cmode, x[0], HA, x[1], HB, eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load, consts, gst);
            continue;
        }
        if (route == 0) {
            dist[i] = fbr_rigidgrad_item(ka, kb, cmode, x[0], x[1], eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load, consts, gst,
                                         [&](const double *X, const double *Y) { return fbr_hull_large_distance(X, X + 9, HA, Y, Y + 9, HB, (int *)nullptr); });
            continue;
        }
        int S = 0;
        dist[i] = fbr_hull_large_grad_item(ka, kb, cmode, x[0], HA, x[1], HB, eps, se, omc, prog.steps.data(), anc.data(), W, fl, mask, qf, basef, save, load,
                                           consts, gst, &S, facet);
        if (S < 0) return -4;
        if (nslots) nslots[i] = S;
    }
    return 0;
}

// fbr_hull_large_grad_width on sbeg [npairs + 1]
int hulllgrad_width(const int32_t *sbeg, int npairs, long C, long want) { return fbr_hull_large_grad_width(sbeg, npairs, C, want); }
}
