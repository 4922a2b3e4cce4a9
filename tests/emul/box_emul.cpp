// box_emul.cpp -- the HIP-free text of csrc/fbr_box.h on the CPU (TEST ONLY, built by tests/test_boxes.py with g++ -ffp-contract=off): the box
// distance the pairs kernel calls, and the frames of the robot boxes from the positions-only lane walk on the step program and the box
// order the library builds (fbr_kinid_build; robot boxes sorted by the step of their link).
#include <cmath>
#include <cstring>
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_box.h"

extern "C" {

// dist [N] of N box pairs: R [N][9], c [N][3], h [N][3] each
void box_distance(long N, const double *RA, const double *cA, const double *hA, const double *RB, const double *cB, const double *hB, double *dist)
{
    for (long i = 0; i < N; i++) dist[i] = fbr_box_distance(RA + 9 * i, cA + 3 * i, hA + 3 * i, RB + 9 * i, cB + 3 * i, hB + 3 * i);
}

// Frames fr [S][nboxes][12] (R | centre) of every box and dist [S][npairs] of every sample.  link -1: a world box (rot, center in the world).
// jtype NULL: every DOF revolute; rpy NULL or not floating: identity base.
int box_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
             const int32_t *jtype, int floating, int nboxes, const int32_t *link, const double *half, const double *center, const double *rot,
             int cmode, int npairs, const int32_t *pairs, long S, const double *q, const double *rpy, const double *bpos, double *fr, double *dist)
{
    FbrHostModel hm;
    const double g[3] = {0, 0, -9.81};
    try {
        hm.build(L, n, parent, dof, restR, restp, axis, floating, g, 0, 1, 0, 0.0, nullptr, jtype);
    } catch (...) {
        return -1;
    }
    FbrKinIdProgram prog;
    fbr_kinid_build(hm, prog);
    std::vector<int> stepof(L, 0), boxbeg(prog.nsteps + 1, 0), boxid;
    for (int k = 0; k < prog.nsteps; k++) stepof[prog.steps[(size_t)k * FBR_KINID_STEP]] = k;
    for (int c = 0; c < nboxes; c++)
        if (link[c] >= 0) boxbeg[stepof[link[c]] + 1]++;
    for (int k = 0; k < prog.nsteps; k++) boxbeg[k + 1] += boxbeg[k];
    boxid.assign(boxbeg[prog.nsteps] + 1, 0);
    std::vector<int> fill(boxbeg.begin(), boxbeg.end() - 1);
    for (int c = 0; c < nboxes; c++)
        if (link[c] >= 0) boxid[fill[stepof[link[c]]]++] = c;
    std::vector<double> slots((size_t)std::max(prog.nslots, 1) * 12);
    for (long s = 0; s < S; s++) {
        double *f = fr + (size_t)s * nboxes * 12;
        for (int c = 0; c < nboxes; c++)
            if (link[c] < 0) {
                for (int i = 0; i < 9; i++) f[12 * c + i] = rot[9 * c + i];
                for (int i = 0; i < 3; i++) f[12 * c + 9 + i] = center[3 * c + i];
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
            const int id = boxid[bs];
            for (int i = 0; i < 9; i++) f[12 * id + i] = R[i];
            fbr_box_centre(cmode, R, p, center + 3 * id, f + 12 * id + 9);
        };
        fbr_capsule_lane(prog.nsteps, prog.steps.data(), boxbeg.data(), floating && rpy != nullptr, qf, basef, save, load, consts, box);
        for (int k = 0; k < npairs; k++) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            dist[(size_t)s * npairs + k] = fbr_box_distance(f + 12 * a, f + 12 * a + 9, half + 3 * a, f + 12 * b, f + 12 * b + 9, half + 3 * b);
        }
    }
    return 0;
}
}
