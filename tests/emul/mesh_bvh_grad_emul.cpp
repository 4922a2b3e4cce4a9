// mesh_bvh_grad_emul.cpp -- the HIP-free text of csrc/fbr_mesh_bvh_grad.h on the CPU (TEST ONLY, built by tests/test_mesh_large_gradient.py
// with g++ -ffp-contract=off; tests/emul/mesh_bvh_grad_sanitize.cpp includes this file).  Routes over the library's own step program,
// ancestor masks, trees and triangle order:
//   0  the single pass, the emulation of record: fbr_rigidgrad_item with the brute-force fbr_mesh_distance (no culling, the caller's
//      triangle order) as its functor;
//   1  the restatement of the device's stages, fbr_mesh_bvh_grad_item: recorded poses, one walk through the trees per pose, the quotients;
//   2, 3  the stages as the device's waves run them: the recorded poses of all candidates of a pair flattened candidate-major (2) or
//      slot-major (3) by fbr_mesh_bvh_grad_entry, cut into packets of 64 consecutive entries, each packet one fbr_mesh_bvh_distance<64>.
// Only pairs with a mesh on either side are served (-5 otherwise): the others have emulations of their own.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/fbr.h"
#include "../../flobaroid_amd/csrc/fbr_mesh_bvh_grad.h"

typedef FbrHullT<const double *, const int32_t *> Hull;
typedef FbrMeshT<const double *> Mesh;
typedef FbrMeshBvhMember<const double *, const int32_t *> Member;

extern "C" {

int meshbvhgrad_leaf(void) { return FBR_MESH_BVH_LEAF; }
int meshbvhgrad_default_order(void) { return FBR_MESH_GRAD_ORDER_DEFAULT; }

// entry e -> (s, c) and back, as the kernel maps them; returns the entry fbr_mesh_bvh_grad_entry_of gives for the (s, c) of e
long meshbvhgrad_entry(int order, long e, int S, long C, int32_t *s, int64_t *c)
{
    int ss;
    long cc;
    fbr_mesh_bvh_grad_entry(order, e, S, C, &ss, &cc);
    *s = ss, *c = cc;
    return fbr_mesh_bvh_grad_entry_of(order, ss, cc, S, C);
}

// tile t of a pair with E entries as the kernel cuts it: returns its entries (0: behind the last), *e0 its first
int meshbvhgrad_tile(long t, long E, int64_t *e0)
{
    long f;
    const int n = fbr_mesh_bvh_grad_tile(t, E, &f);
    *e0 = f;
    return n;
}

// One hull pair per item, M = C x K items, item c K + k: pair k of candidate c (routes 2 and 3 need pairs [c K + k] the same for every c;
// routes 0 and 1 take any M items with K = 1 or not).  Arguments as meshgrad_eval of mesh_grad_emul.cpp; hulls of up to
// FBR_MAX_LARGE_HULL_VERTICES vertices.  nslots [M] (may be null): the stencil points of the item (route 0: 0).  stats [6] (may be null),
// summed over the call: node pairs wanted | leaf pairs | triangle pairs of those | GJK evaluations | packets (routes 2, 3) or walks (1) |
// the highest stack.  stencil [M][cap] (may be null; routes 2 and 3): the stencil values of the item, the centre first, those beyond cap left
// out.  Returns -4 when the recorded poses do not number what fbr_meshgrad_slots says, -6 on a tree the setter refuses.
int meshbvhgrad_eval(int L, int n, const int32_t *parent, const int32_t *dof, const double *restR, const double *restp, const double *axis,
                     const int32_t *jtype, int floating, int nhulls, const int32_t *link, const double *offset, const double *rot, int cmode,
                     const int32_t *vbeg, const double *verts, const int32_t *fbeg, const double *planes, const int32_t *ebeg, const int32_t *edges,
                     const int32_t *mtab, const double *tris, long ntris, double eps, long C, long K, const int32_t *pairs, const double *q,
                     const double *rpy, const double *bpos, int route, double *dist, double *grad, int32_t *nslots, int64_t *stats, int cap, double *stencil)
{
    const long M = C * K;
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
    // the meshes in table order, as the setter takes them; aux0: of the caller's order (the brute force)
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
    if (nmesh > 0 && !fbr_mesh_bvh_set(nmesh, tbeg.data(), packed.data(), set).empty()) return -6;
    std::vector<double> aux0(packed.size() / 9 * 5 + 5);
    for (size_t t = 0; t < packed.size() / 9; t++) fbr_mesh_triangle_aux(packed.data() + 9 * t, aux0.data() + 5 * t);
    std::vector<int> mof((size_t)std::max(nhulls, 1), -1);
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
    auto member = [&](int h) {
        const size_t n0 = mof[h] < 0 ? 0 : (size_t)set.nbeg[mof[h]];
        return Member{view(h), mesh(h, true), set.node.data() + 4 * n0, set.vol.data() + 4 * n0, (const double *)sph.data() + 4 * (size_t)h};
    };
    std::fill(grad, grad + (size_t)M * n, 0.0);
    double se, omc;
    fbr_boxgrad_trig(eps, &se, &omc);
    FbrMeshBvhStats bs = {0, 0, 0, 0, {0, 0, 0}};
    long walks = 0;
    const bool fl = floating && rpy != nullptr;
    // the lambdas of item i, handed to `body`
    auto with_item = [&](long i, auto body) -> int {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= nhulls || b < 0 || b >= nhulls || (link[a] < 0 && link[b] < 0)) return -2;
        if (mof[a] < 0 && mof[b] < 0) return -5;
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
        return body(a, b, ka, kb, x[0], x[1], mask, qf, basef, save, load, consts);
    };
    if (route == 0 || route == 1) {
        for (long i = 0; i < M; i++) {
            auto gst = [&](int d, double v) { grad[i * n + d] = v; };
            if (nslots) nslots[i] = 0;
            const int rc = with_item(i, [&](int a, int b, int ka, int kb, const double *xa, const double *xb, auto mask, auto qf, auto basef, auto save,
                                            auto load, auto consts) {
                if (route == 0) {
                    const Hull HA = view(a), HB = view(b);
                    const Mesh MA = mesh(a, false), MB = mesh(b, false);
                    const double *sA = sph.data() + 4 * (size_t)a, *sB = sph.data() + 4 * (size_t)b;
                    dist[i] = fbr_rigidgrad_item(ka, kb, cmode, xa, xb, eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load, consts, gst,
                                                 [&](const double *X, const double *Y) {
                                                     return fbr_mesh_distance<false>(X, X + 9, HA, MA, sA, Y, Y + 9, HB, MB, sB, (FbrMeshStats *)nullptr);
                                                 });
                    return 0;
                }
                int S = 0;
                dist[i] = fbr_mesh_bvh_grad_item(ka, kb, cmode, xa, member(a), xb, member(b), eps, se, omc, prog.steps.data(), anc.data(), W, fl, mask, qf,
                                                 basef, save, load, consts, gst, &S, &bs);
                if (S < 0) return -4;
                walks += S;
                if (nslots) nslots[i] = S;
                return 0;
            });
            if (rc) return rc;
        }
    } else {
        const int order = route == 2 ? FBR_MESH_GRAD_CANDIDATE_MAJOR : FBR_MESH_GRAD_SLOT_MAJOR;
        int stk[2 * FBR_MESH_BVH_STACK];
        for (long k = 0; k < K; k++) {
            // stage A of every candidate of the pair
            std::vector<std::vector<FbrHullRel>> rel((size_t)C);
            std::vector<int> joint;
            int S = -1, a0 = 0, b0 = 0;
            for (long c = 0; c < C; c++) {
                const long i = c * K + k;
                const int rc = with_item(i, [&](int a, int b, int ka, int kb, const double *xa, const double *xb, auto mask, auto qf, auto basef, auto save,
                                                auto load, auto consts) {
                    if (c == 0) a0 = a, b0 = b, fbr_meshgrad_slots(ka, kb, cmode, prog.steps.data(), anc.data(), W, joint);
                    if (a != a0 || b != b0) return -7;
                    std::vector<FbrHullRel> &r = rel[(size_t)c];
                    const int Sc = fbr_meshgrad_frames_item(ka, kb, cmode, xa, xb, mof[a] < 0, eps, se, omc, prog.steps.data(), fl, mask, qf, basef, save, load,
                                                            consts, [&](int s, const FbrHullRel &p) {
                                                                if ((int)r.size() == s) r.push_back(p);
                                                            });
                    if (Sc != (int)joint.size() || Sc != (int)r.size()) return -4;
                    S = Sc;
                    return 0;
                });
                if (rc) return rc;
            }
            // stage B over packets of 64 consecutive entries
            const Member A = member(mof[a0] < 0 ? b0 : a0), B = member(mof[a0] < 0 ? a0 : b0);
            const long E = (long)S * C;
            std::vector<double> dv((size_t)E);  // [s][c]
            for (long t = 0;; t++) {
                long e0;
                const int nl = fbr_mesh_bvh_grad_tile(t, E, &e0);
                if (nl == 0) break;
                FbrHullRel pq[64];
                double out[64];
                int es[64];
                long ec[64];
                for (int l = 0; l < nl; l++) {
                    fbr_mesh_bvh_grad_entry(order, e0 + l, S, C, &es[l], &ec[l]);
                    pq[l] = rel[(size_t)ec[l]][(size_t)es[l]];
                }
                fbr_mesh_bvh_distance<64>(nl, pq, A.hull, A.mesh, A.node, A.vol, B.hull, B.mesh, B.node, B.vol, B.sph, stk, out, &bs);
                walks++;
                for (int l = 0; l < nl; l++) dv[(size_t)es[l] * C + ec[l]] = out[l];
            }
            // stage C
            for (long c = 0; c < C; c++) {
                const long i = c * K + k;
                if (nslots) nslots[i] = S;
                for (int sp = 0; stencil && sp < S && sp < cap; sp++) stencil[(size_t)i * cap + sp] = dv[(size_t)sp * C + c];
                dist[i] = fbr_meshgrad_quotients(
                    S, [&](int s) { return joint[s]; }, [&](int s) { return dv[(size_t)s * C + c]; }, eps, [&](int d, double v) { grad[i * n + d] = v; });
            }
        }
    }
    if (stats) {
        stats[0] = bs.node_pairs, stats[1] = bs.leaf_pairs, stats[2] = bs.tri_pairs, stats[3] = bs.tri.evals, stats[4] = walks, stats[5] = bs.max_stack;
    }
    return 0;
}
}
