// capsule_emul.cpp -- the HIP-free text of csrc/fbr_capsule.h on the CPU (TEST ONLY, built by tests/test_capsules.py with g++ -ffp-contract=off):
// the segment routine the pairs kernel calls and the positions-only lane walk of the points kernel, on the step program and the capsule
// order the library builds (fbr_kinid_build; capsules sorted by the step of their link).
#include <cmath>
#include <cstring>
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_capsule.h"

extern "C" {

// out3 = (distance, s, t) of the segments a0 a1 and b0 b1
void cap_segment(const double *a0, const double *a1, const double *b0, const double *b1, double *out3)
{
    out3[0] = fbr_segment_distance(a0, a1, b0, b1, out3 + 1, out3 + 2);
}

// World endpoints ep [S][ncaps][6] of the capsules and, when pairs != NULL, dist [S][npairs] / st [S][npairs][2] (the distance minus the
// radii and the closest-point parameters) of every sample.  jtype NULL: every DOF revolute; rpy NULL or not floating: identity base.
int cap_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
             const int32_t *jtype, int floating, int ncaps, const int32_t *link, const double *seg, const double *radius, int npairs,
             const int32_t *pairs, long S, const double *q, const double *rpy, const double *bpos, double *ep, double *dist, double *st)
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
    std::vector<int> stepof(L, 0), capbeg(prog.nsteps + 1, 0), capid(ncaps);
    for (int k = 0; k < prog.nsteps; k++) stepof[prog.steps[(size_t)k * FBR_KINID_STEP]] = k;
    for (int c = 0; c < ncaps; c++) capbeg[stepof[link[c]] + 1]++;
    for (int k = 0; k < prog.nsteps; k++) capbeg[k + 1] += capbeg[k];
    std::vector<int> fill(capbeg.begin(), capbeg.end() - 1);
    for (int c = 0; c < ncaps; c++) capid[fill[stepof[link[c]]]++] = c;
    std::vector<double> slots((size_t)std::max(prog.nslots, 1) * 12);
    for (long s = 0; s < S; s++) {
        double *e = ep + (size_t)s * ncaps * 6;
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
        auto cap = [&](int cs, const double *R, const double *p) {
            const int id = capid[cs];
            fbr_capsule_point(R, p, seg + 6 * id, e + 6 * id);
            fbr_capsule_point(R, p, seg + 6 * id + 3, e + 6 * id + 3);
        };
        fbr_capsule_lane(prog.nsteps, prog.steps.data(), capbeg.data(), floating && rpy != nullptr, qf, basef, save, load, consts, cap);
        if (!pairs) continue;
        for (int k = 0; k < npairs; k++) {
            const int a = pairs[2 * k], b = pairs[2 * k + 1];
            double sv, tv;
            dist[(size_t)s * npairs + k] = fbr_segment_distance(e + 6 * a, e + 6 * a + 3, e + 6 * b, e + 6 * b + 3, &sv, &tv) - radius[a] - radius[b];
            st[((size_t)s * npairs + k) * 2] = sv;
            st[((size_t)s * npairs + k) * 2 + 1] = tv;
        }
    }
    return 0;
}

// the candidate minimum of the kernels' comparison rule over rows 0, step, 2 step, ... of dist [T][npairs]
void cap_minimum(long T, long step, int npairs, const double *dist, double *val, long *idx)
{
    for (int k = 0; k < npairs; k++) {
        double best = FBR_CAPSULE_NONE;
        long ib = -1;
        for (long t = 0; t < T; t += step)
            if (fbr_capsule_take(dist[(size_t)t * npairs + k], best)) best = dist[(size_t)t * npairs + k], ib = t;
        val[k] = best;
        idx[k] = ib;
    }
}
}
