// hull_emul.cpp -- the HIP-free text of csrc/fbr_hull.h on the CPU (TEST ONLY, built by tests/test_hulls.py with g++ -ffp-contract=off): the
// hull distance the pairs kernel calls, the frames of the robot hulls from the positions-only lane walk (the step program and the slot order
// the library builds for the boxes), and the checks of fbr_model_set_hulls.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_hull.h"

typedef FbrHullT<const double *, const int32_t *> Hull;

static Hull view(int h, const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges,
                 const double *diam)
{
    return Hull{vbeg[h + 1] - vbeg[h], fbeg[h + 1] - fbeg[h], ebeg[h + 1] - ebeg[h], verts + 3 * (size_t)vbeg[h], planes + 4 * (size_t)fbeg[h],
                edges + 4 * (size_t)ebeg[h], diam[h]};
}

extern "C" {

// dist [N], iters [N] of N poses of ONE pair of hulls (tables of two hulls: 0 is A, 1 is B): R [N][9], c [N][3]
void hull_distance(long N, const double *RA, const double *cA, const double *RB, const double *cB, const int32_t *vbeg, const double *verts,
                   const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges, const double *diam, double *dist, int32_t *iters)
{
    const Hull A = view(0, vbeg, verts, fbeg, planes, ebeg, edges, diam), B = view(1, vbeg, verts, fbeg, planes, ebeg, edges, diam);
    for (long i = 0; i < N; i++) {
        int it = 0;
        dist[i] = fbr_hull_distance(RA + 9 * i, cA + 3 * i, A, RB + 9 * i, cB + 3 * i, B, &it);
        iters[i] = it;
    }
}

// 0 when fbr_model_set_hulls would accept the set on a model of L links, else -1 and the message in msg [len]
int hull_validate(int L, int nhulls, const int32_t *link, const double *offset, const double *rot, const int32_t *vbeg, const double *verts,
                  const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges, int npairs, const int32_t *pairs, char *msg, int len)
{
    const std::string e = fbr_hull_validate(L, FBR_MAX_HULLS, FBR_MAX_HULL_PAIRS, FBR_MAX_HULL_VERTICES, nhulls, link, offset, rot, vbeg, verts, fbeg,
                                            planes, ebeg, edges, npairs, pairs, nullptr);
    if (msg && len > 0) {
        strncpy(msg, e.c_str(), len - 1);
        msg[len - 1] = 0;
    }
    return e.empty() ? 0 : -1;
}

// Frames fr [S][nhulls][12] (R | centre) of every hull, dist [S][npairs] and iters [S][npairs] of every sample.  link -1: a world hull (rot,
// offset in the world).  jtype NULL: every DOF revolute; rpy NULL or not floating: identity base.
int hull_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
              const int32_t *jtype, int floating, int nhulls, const int32_t *link, const double *offset, const double *rot, int mode,
              const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges,
              int npairs, const int32_t *pairs, long S, const double *q, const double *rpy, const double *bpos, double *fr, double *dist, int32_t *iters)
{
    std::vector<double> diam(std::max(nhulls, 1));
    if (!fbr_hull_validate(L, FBR_MAX_HULLS, FBR_MAX_HULL_PAIRS, FBR_MAX_HULL_VERTICES, nhulls, link, offset, rot, vbeg, verts, fbeg, planes, ebeg, edges,
                           npairs, pairs, diam.data()).empty())
        return -2;
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    try {
        hm.build(L, n, parent, dof, restR, restp, axis, floating, g, 0, 1, 0, 0.0, nullptr, jtype);
    } catch (...) {
        return -1;
    }
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    std::vector<int> stepof(L, 0), beg(prog.nsteps + 1, 0), hid;
    for (int k = 0; k < prog.nsteps; k++) stepof[prog.steps[(size_t)k * FBR_KINID_STEP]] = k;
    for (int c = 0; c < nhulls; c++)
        if (link[c] >= 0) beg[stepof[link[c]] + 1]++;
    for (int k = 0; k < prog.nsteps; k++) beg[k + 1] += beg[k];
    hid.assign(beg[prog.nsteps] + 1, 0);
    std::vector<int> fill(beg.begin(), beg.end() - 1);
    for (int c = 0; c < nhulls; c++)
        if (link[c] >= 0) hid[fill[stepof[link[c]]]++] = c;
    std::vector<double> slots((size_t)std::max(prog.nslots, 1) * 12);
    for (long s = 0; s < S; s++) {
        double *f = fr + (size_t)s * nhulls * 12;
        for (int c = 0; c < nhulls; c++)
            if (link[c] < 0) {
                for (int i = 0; i < 9; i++) f[12 * c + i] = rot[9 * c + i];
                for (int i = 0; i < 3; i++) f[12 * c + 9 + i] = offset[3 * c + i];
            }
        auto qf = [&](int d) { return q[s * n + d]; };
        auto basef = [&](double *e3, double *b3) {
            for (int i = 0; i < 3; i++) {
                e3[i] = rpy ? rpy[s * 3 + i] : 0.0;
                b3[i] = bpos ? bpos[s * 3 + i] : 0.0;
            }
        };
        auto save = [&](int b, int i, double v) { slots[(size_t)b * 12 + i] = v; };
        auto load = [&](int b, int i) { return slots[(size_t)b * 12 + i]; };
        auto consts = [&](int l, double *rR, double *rp, double *ax) {
            for (int i = 0; i < 9; i++) rR[i] = hm.restR[9 * l + i];
            for (int i = 0; i < 3; i++) {
                rp[i] = hm.restp[3 * l + i];
                ax[i] = hm.axis[3 * l + i];
            }
        };
        auto box = [&](int bs, const double *R, const double *p) {
            const int id = hid[bs];
            for (int i = 0; i < 9; i++) f[12 * id + i] = R[i];
            fbr_box_centre(mode, R, p, offset + 3 * id, f + 12 * id + 9);
        };
        fbr_capsule_lane(prog.nsteps, prog.steps.data(), beg.data(), floating && rpy != nullptr, qf, basef, save, load, consts, box);
        for (int k = 0; k < npairs; k++) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            int it = 0;
            dist[(size_t)s * npairs + k] = fbr_hull_distance(f + 12 * a, f + 12 * a + 9, view(a, vbeg, verts, fbeg, planes, ebeg, edges, diam.data()), f + 12 * b,
                                                             f + 12 * b + 9, view(b, vbeg, verts, fbeg, planes, ebeg, edges, diam.data()), &it);
            if (iters) iters[(size_t)s * npairs + k] = it;
        }
    }
    return 0;
}
}
