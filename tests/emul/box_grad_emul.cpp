// box_grad_emul.cpp -- the HIP-free text of csrc/fbr_box_grad.h on the CPU (TEST ONLY, built by tests/test_box_gradient.py with
// g++ -ffp-contract=off): the masked walk and the item routine of fbr_box_grad_kernel, on the step program and the ancestor masks the
// library builds (fbr_kinid_build, fbr_capgrad_ancestors).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../flobaroid_amd/csrc/fbr_box_grad.h"

extern "C" {

// One box pair per configuration: boxes as for fbr_model_set_boxes (link -1: a world box with rot), pairs [M][2] box indices, q [M][n],
// rpy / bpos [M][3] or NULL -> dist [M], grad [M][n] (zeroed here; the routine stores the path joints only).
int boxgrad_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
                 const int32_t *jtype, int floating, int nboxes, const int32_t *link, const double *half, const double *center, const double *rot,
                 int cmode, double eps, long M, const int32_t *pairs, const double *q, const double *rpy, const double *bpos, double *dist, double *grad)
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
    std::vector<int> stepof, anc;
    fbr_capgrad_ancestors(hm, prog, stepof, anc);
    const int W = fbr_capgrad_words(prog.nsteps);
    std::vector<double> slots((size_t)std::max(prog.nslots, 1) * 12);
    std::fill(grad, grad + (size_t)M * n, 0.0);
    double se, omc;
    fbr_boxgrad_trig(eps, &se, &omc);
    for (long i = 0; i < M; i++) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= nboxes || b < 0 || b >= nboxes || (link[a] < 0 && link[b] < 0)) return -2;
        const int ka = link[a] < 0 ? -1 : stepof[link[a]], kb = link[b] < 0 ? -1 : stepof[link[b]];
        double x[2][12];
        for (int j = 0; j < 2; j++) {
            const int c = j ? b : a;
            for (int t = 0; t < 12; t++) x[j][t] = 0.0;
            if (link[c] < 0) {
                for (int t = 0; t < 9; t++) x[j][t] = rot[9 * c + t];
                for (int t = 0; t < 3; t++) x[j][9 + t] = center[3 * c + t];
            } else {
                for (int t = 0; t < 3; t++) x[j][t] = center[3 * c + t];
            }
        }
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
        dist[i] = fbr_boxgrad_item(ka, kb, cmode, x[0], half + 3 * a, x[1], half + 3 * b, eps, se, omc, prog.steps.data(), floating && rpy != nullptr,
                                   mask, qf, basef, save, load, consts, gst);
    }
    return 0;
}
}
